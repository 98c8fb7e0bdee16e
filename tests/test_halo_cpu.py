"""The vector halo without a GPU: the planner's per-peer sizes and interior / boundary counts (pdh_check_halo) against a derivation from
the face list and the owners alone on every world of tests/halo_cases.py, the coverage those worlds claim, the refusals of the planner,
and the NumPy reference of CG (tests/pcg_ref.py) on the worlds tests/test_gpu_dist_solve.py solves on: the reference alone meets the
bounds the GPU test applies."""
import numpy as np
import pytest
import scipy.sparse as sp

import exchange_cases as xc
import halo_cases as hc
import polydeal_amd as pa
from pcg_ref import pcg, preconditioner
from polydeal_amd import _capi


@pytest.fixture(autouse=True)
def _halo_abi():
    """every test here is about pdh_check_halo: a library without it fails them all at this call"""
    assert pa.load_library().pdh_check_halo(None, 0, 0, 1, None, None, None, None) == _capi.PDH_EINVAL


def test_expected_halo_on_a_hand_worked_world():
    """four polytopes 0 - 1 - 2 - 3 in a row plus the face (3, 0), dofs 20, 0, 30, 10 (n = 10), owners 1, 0, 1, 0: rank 0 owns the dofs
    0 .. 19 (polytopes 1, 3), rank 1 the dofs 20 .. 39 (polytopes 0, 2); every polytope has a neighbour of the other rank"""
    faces = [(0, 1), (2, 1), (2, 3), (3, 0)]
    exp = hc.expected_halo(faces, [20, 0, 30, 10], np.array([1, 0, 1, 0]), 10, 2)
    assert exp["send"] == {(0, 1): [1, 3], (1, 0): [0, 2]}
    assert exp["interior"] == [[], []] and exp["boundary"] == [[1, 3], [0, 2]]
    assert hc.send_matrix(exp).tolist() == [[0, 20], [20, 0]]
    assert hc.send_dofs(exp, 0).tolist() == list(range(0, 20)) and hc.ghost_dofs(exp, 0).tolist() == list(range(20, 40))
    # a chain 0 - 1 - 2 on one rank each but the middle one twice: 0 | 1, 2 | 3
    exp = hc.expected_halo([(0, 1), (1, 2), (2, 3)], [0, 10, 20, 30], np.array([0, 1, 1, 2]), 10, 3)
    assert exp["send"] == {(0, 1): [0], (1, 0): [1], (1, 2): [2], (2, 1): [3]} and exp["interior"] == [[], [], []]


@pytest.mark.parametrize("name", hc.NAMES)
def test_planner_sizes_equal_the_independent_derivation(name):
    w = hc.world(name)
    part, exp = w.part, w.expected()
    W = part.world
    send = hc.send_matrix(exp)
    assert np.all(np.diag(send) == 0)
    for r, (prob, (r0, r1)) in enumerate(part.problems()):
        sc, rc, info = _capi.check_halo(prob, r0, r1, part.splits)
        assert sc == send[r].tolist(), (r, sc, send[r])
        assert rc == send[:, r].tolist(), (r, rc, send[:, r])  # the receive matrix is the transpose of the send matrix
        assert info == {"n_owned_rows": r1 - r0, "n_ghost_rows": int(send[:, r].sum()), "n_interior": len(exp["interior"][r]),
                        "n_boundary": len(exp["boundary"][r])}, (r, info)
        assert info["n_interior"] + info["n_boundary"] == (r1 - r0) // part.n


def test_worlds_cover_the_descriptions():
    kinds = {}
    for name in hc.NAMES:
        prob = hc.world(name).part.problems()[0][0]
        kinds[name] = (int(prob.c.local), bool(prob.c.col_offset), bool(getattr(prob, "cartesian", None)), int(prob.c.diag_first))
    assert kinds["mirror_col_offset"] == (1, True, False, 0) and kinds["cartesian"][2] and kinds["cartesian"][0] == 1
    assert any(k[0] == 0 for k in kinds.values()) and any(k[0] == 1 and not k[2] for k in kinds.values())
    assert {k[3] for k in kinds.values()} == {0, 1}
    assert hc.world("dgq4").part.n == 125


def test_slab_worlds_have_the_interior_polytopes_they_were_chosen_for():
    for name, want in hc.SLAB_INTERIOR.items():
        w = hc.world(name)
        got = [len(v) for v in w.expected()["interior"]]
        assert got == want, (name, got)
        assert list(w.part.owner) == hc.slab_owner(w.part.kw["bbox"], w.part.world)
    pin = hc.world("slab_pinwheel_dgp1")
    cov = hc.coverage(pin.expected(), pin.part.owner)
    assert cov["sent_to_two_peers"] == 8 and cov["silent_pairs"] == [(2, 0)], cov
    # the interleaved worlds have no interior polytope at all, but for the quadrants of silent_pair: one each
    for name in xc.ALL_CASES:
        got = [len(v) for v in hc.world(name).expected()["interior"]]
        if name == "silent_pair":
            assert got == [1, 1, 1, 1]
        elif name == "one_rank":
            assert got == [16]
        else:
            assert not any(got), (name, got)


def test_coverage_conditions():
    cov = {name: hc.coverage(hc.world(name).expected(), hc.world(name).part.owner) for name in hc.NAMES}
    for name, c in cov.items():
        print(name, c)
    assert any(c["sent_to_two_peers"] for c in cov.values())
    assert any(c["silent_pairs"] and c["zero_inside"] for c in cov.values())
    assert any(0 in c["interior"] and len(c["interior"]) > 1 for c in cov.values())  # a rank with no interior polytope
    assert any(max(c["interior"]) >= 2 and len(c["interior"]) > 1 for c in cov.values())  # a rank with several
    assert any(c["single_polytope_rank"] for name, c in cov.items() if hc.world(name).part.world > 1)
    one = hc.world("one_rank")
    assert one.part.world == 1 and not one.expected()["send"] and hc.send_matrix(one.expected()).tolist() == [[0]]
    per = hc.world("rank_per_polytope")
    assert per.part.world == per.part.kw["n_agg"] and all(len(v) == 1 for v in per.expected()["boundary"])


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _refused(prob, r0, r1, splits, code, fragment):
    with pytest.raises(pa.PdhError) as e:
        _capi.check_halo(prob, r0, r1, splits)
    assert e.value.code == code and fragment in str(e.value), str(e.value)


def test_planner_refusals():
    part = hc.world("dist3d_dgq1").part
    n, W, splits = part.n, part.world, list(part.splits)
    prob, (r0, r1) = part.problems()[1]
    assert _capi.check_halo(prob, r0, r1, splits)[2]["n_owned_rows"] == r1 - r0
    E = _capi.PDH_EINVAL
    swapped = list(splits)
    swapped[1], swapped[2] = swapped[2], swapped[1]
    _refused(prob, r0, r1, swapped, E, "not ascending")
    # no range is the owned one: the splits of another partition of the same rows
    moved = list(splits)
    moved[1] -= n
    _refused(prob, r0, r1, moved, E, "no range of row_splits is the owned range")
    # a split inside a ghost polytope (the owned range itself stays a range): the first polytope of rank 3 is a ghost of rank 1
    exp = hc.world("dist3d_dgq1").expected()
    off = np.asarray(part.kw["dof_offset"])
    assert splits[3] in off[exp["send"][(3, 1)]] and (0, 1) in exp["send"]
    cut = list(splits)
    cut[3] += 1
    _refused(prob, r0, r1, cut, E, "cut the polytope")
    # a ghost block in no range: the last rank, then the first, is left out
    _refused(prob, r0, r1, splits[:-1], E, "lies in no range")
    _refused(prob, r0, r1, splits[1:], E, "lies in no range")
    # the same through a rank-local description
    loc = pa.Problem(**xc.local_description(part.kw, r0, r1))
    assert _capi.check_halo(loc, r0, r1, splits)[:2] == _capi.check_halo(prob, r0, r1, splits)[:2]
    _refused(loc, r0, r1, cut, E, "cut the polytope")
    # a misaligned range is refused before the halo is planned
    _refused(prob, r0 + 1, r1, splits, E, "whole polytopes")
    lib = pa.load_library()
    assert lib.pdh_check_halo(prob.c, r0, r1, W, None, None, None, None) == E


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference of CG on the worlds the GPU test solves on
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hc.CG_WORLDS)
def test_reference_cg_meets_the_bounds_of_the_gpu_test(name):
    w = hc.world(name)
    A, b, n = w.dense(), hc.rhs(name), w.part.n
    assert np.allclose(A, A.T, rtol=0, atol=1e-12 * np.max(np.abs(A)))
    ref = np.linalg.solve(A, b)
    for kind in hc.cg_kinds(name):
        x, it, res = pcg(A, b, preconditioner(sp.csr_matrix(A), n, kind))
        assert res <= 1e-13 * np.linalg.norm(b), (kind, it, res)
        assert np.linalg.norm(x - ref) <= 1e-9 * np.linalg.norm(ref), (kind, it)
        assert 0 < it < 20000


def test_cg_worlds_are_the_ones_asked_for():
    assert sum(n.startswith("slab_") for n in hc.CG_WORLDS) >= 1
    assert {"rank_per_polytope", "single_polytope", "mirror_col_offset", "dgq4", "cartesian"} <= set(hc.CG_WORLDS)
    assert hc.cg_kinds("dgq4") == ("jacobi",) and len(hc.CG_WORLDS) >= 6
