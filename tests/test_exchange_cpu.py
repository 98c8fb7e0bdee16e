"""The ghost-block exchange without a GPU: the planner's per-peer sizes (pdh_check_exchange) against a count from the face list and the
owners alone for every world of tests/exchange_cases.py, the coverage those worlds claim - traffic in both directions, M22 sums from
several peers, M21 blocks on either side of the diagonal block -, and the refusals of the planner."""
import ctypes as C

import numpy as np
import pytest

import exchange_cases as xc
import polydeal_amd as pa
from flatten_oracle import flatten
from oracle import polydeal_oracle as po
from polydeal_amd import _capi

ALL = list(xc.ALL_CASES) + [xc.MIRROR_CASE]


def _check_exchange(prob, r0, r1, world):
    lib = pa.load_library()
    sc, rc = (C.c_int64 * world)(), (C.c_int64 * world)()
    code = lib.pdh_check_exchange(C.byref(prob.c), r0, r1, world, sc, rc)
    return code, list(sc), list(rc), (lib.pdh_last_error(None) or b"").decode()


def test_expected_exchange_on_a_hand_worked_world():
    """four polytopes 0 - 1 - 2 - 3 in a row plus the face (3, 0), dofs 20, 0, 30, 10 (n = 10), owners 0, 1, 0, 1"""
    faces = [(0, 1), (2, 1), (2, 3), (3, 0)]
    exp = xc.expected_exchange(faces, [20, 0, 30, 10], np.array([0, 1, 0, 1]), 10, 2)
    # 0 -> 1: cut faces by (side-0 dof, side-1 dof): (20, 0) = (0, 1); (30, 0) = (2, 1); (30, 10) = (2, 3); M22 of the dofs 0 and 10
    assert exp[(0, 1)] == [("m21", 0, 1), ("m21", 2, 1), ("m21", 2, 3), ("m22", 1, [0, 2]), ("m22", 3, [2])]
    assert exp[(1, 0)] == [("m21", 3, 0), ("m22", 0, [3])]
    assert xc.expected_sizes(exp, 10, 2).tolist() == [[0, 500], [200, 0]]


@pytest.mark.parametrize("cid", ALL)
def test_planner_sizes_equal_the_independent_count(cid):
    part = xc.world(cid)
    W = part.world
    send = xc.expected_sizes(part.expected(), part.n, W)
    assert np.all(np.diag(send) == 0)
    assert part.kw["n_agg"] <= 64 and part.n <= 64
    dropped = 0
    for r, (prob, (r0, r1)) in enumerate(part.problems()):
        code, sc, rc, msg = _check_exchange(prob, r0, r1, W)
        assert code == 0, (r, msg)
        assert sc == send[r].tolist(), (r, sc, send[r])
        assert rc == send[:, r].tolist(), (r, rc, send[:, r])  # the receive matrix is the transpose of the send matrix
        assert prob.c.local == (1 if part.local == "drop" or cid == xc.MIRROR_CASE else 0)
        if part.local == "drop":  # the rank-local description packs to the counts of the global one restricted to the range
            dropped += part.kw["n_agg"] - prob.c.n_agg
            assert prob.check(r0, r1) == pa.Problem(**part.kw).check(r0, r1)
    assert (dropped > 0) == (part.local == "drop")


def test_two_worlds_run_through_rank_local_descriptions():
    assert sum(c[7] == "drop" for c in xc.CASES.values()) >= 2 and xc.world(xc.MIRROR_CASE).problems()[0][0].c.local == 1


@pytest.mark.parametrize("cid", list(xc.CASES))
def test_renumbering_is_interleaved_and_shuffled(cid):
    """every rank owns one contiguous row range; consecutive polytopes fall to different ranks and the order inside a rank is not the
    polytope order (a monotone numbering is what the suite had before)"""
    part = xc.world(cid)
    off, owner = np.asarray(part.kw["dof_offset"], dtype=np.int64), part.owner
    assert sorted(off.tolist()) == list(range(0, part.kw["n_rows"], part.n))
    for r in range(part.world):
        r0, r1 = part.rows(r)
        assert np.array_equal((off >= r0) & (off < r1), owner == r)
    assert np.any(np.diff(owner) < 0)
    assert any(np.any(np.diff(off[owner == r]) < 0) for r in range(part.world))
    assert np.array_equal(np.sort(part.old_to_new), np.arange(part.kw["n_rows"]))


def test_cases_cover_what_the_suite_never_ran():
    cov = {cid: xc.coverage(xc.world(cid)) for cid in xc.CASES}
    for cid, c in cov.items():
        print(cid, c)
    assert any(c["both_directions"] for c in cov.values())
    assert any(c["m22_from_two_peers"] for c in cov.values()) and any(c["two_faces_from_one_peer"] for c in cov.values())
    assert any(c["rank0_receives"] for c in cov.values()) and any(c["last_rank_sends"] for c in cov.values())
    assert any(c["m21_left"] for c in cov.values()) and any(c["m21_right"] for c in cov.values())
    # (in fact every case meets every condition that its number of ranks allows)
    for cid, c in cov.items():
        assert c["both_directions"] and c["rank0_receives"] and c["last_rank_sends"] and c["m21_left"] and c["m21_right"], cid
        if xc.world(cid).world >= 3:
            assert c["m22_from_two_peers"] >= 1 and c["two_faces_from_one_peer"], cid


def test_cases_cover_elements_meshes_variants_and_layouts():
    cases = list(xc.CASES.values())
    fes = {(xc.element(cid).dim, c[1], c[2], xc.element(cid).n_dofs_per_cell) for cid, c in xc.CASES.items()}
    assert fes == {(2, "dgp", 1, 3), (2, "dgq", 1, 4), (2, "dgq", 7, 64), (3, "dgp", 1, 4), (3, "dgp", 3, 20), (3, "dgq", 1, 8),
                   (3, "dgq", 2, 27), (3, "dgq", 3, 64)}
    assert {c[0] for c in cases} >= {"dist2d", "dist3d", "pinwheel", "grown6", "t3"}
    assert {(c[3], c[4]) for c in cases} == {(v, d) for v in ("poisson", "dr", "adm") for d in (True, False)}
    assert {c[5] for c in cases} == {2, 3, 4}


def test_meshes_are_what_the_cases_say():
    ah = xc.handler("pinwheel_dgp1")[0]
    nbrs = [len(b) - 1 for b in xc.coupled_polytopes(*(flatten(ah, xc.handler("pinwheel_dgp1")[1])[k] for k in ("dof_offset", "rowptr", "colind")),
                                                     4)]
    assert min(nbrs) == 3 and max(nbrs) == 13 and ah.n_agglomerates == 30  # (rows of 4 to 14 blocks)
    # grown agglomerates: a polytope smaller than its bounding box (a staircase), in 3-D and on the unstructured 2-D mesh
    for cid in ("grown6_dgp3", "t3_dgp1"):
        ah = xc.handler(cid)[0]
        fill = [ah.volume_jxw_sum(P) / np.prod(ah.bboxes[P][1] - ah.bboxes[P][0]) for P in range(ah.n_agglomerates)]
        assert min(fill) < 0.6, (cid, min(fill))
    # no interior face of the t3 mesh is axis-aligned
    kw = xc.world("t3_dgp1").kw
    interior = np.repeat(np.asarray(kw["face_out"]) >= 0, np.diff(kw["fq_ptr"]))
    assert interior.sum() > 100 and np.all(np.max(np.abs(np.asarray(kw["fq_n"])), axis=0)[interior] < 1.0 - 1e-6)


def test_edge_worlds():
    one = xc.world("one_rank")
    assert one.world == 1 and not one.expected()
    per = xc.world("rank_per_polytope")
    assert per.world == per.kw["n_agg"] <= 8
    silent = xc.coverage(xc.world("silent_pair"))
    assert silent["silent_pairs"] and silent["zero_inside"]
    assert xc.coverage(xc.world("single_polytope"))["single_polytope_rank"]
    assert int(np.sum(xc.world("single_polytope").owner == 2)) == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _refused(kw, r0, r1, world, code, fragment):
    got, _, _, msg = _check_exchange(pa.Problem(**kw), r0, r1, world)
    assert got == code and fragment in msg, (got, msg)


def test_planner_refusals():
    part = xc.world("dist3d_dgq1")
    kw, (r0, r1), W = part.kw, part.rows(1), part.world
    assert _check_exchange(pa.Problem(**kw), r0, r1, W)[0] == 0
    E = _capi.PDH_EINVAL
    _refused(dict(kw, agg_rank=None), r0, r1, W, E, "needs agg_rank")
    rank = np.array(kw["agg_rank"])
    off = np.asarray(kw["dof_offset"])
    outside = np.nonzero(rank != 1)[0]
    neg = rank.copy()
    neg[outside[0]] = -1
    _refused(dict(kw, agg_rank=neg), r0, r1, W, E, "agg_rank must be non-negative")
    mixed = rank.copy()
    mixed[np.nonzero(rank == 1)[0][-1]] = 3
    _refused(dict(kw, agg_rank=mixed), r0, r1, W, E, "owned polytopes carry different ranks")
    stray = rank.copy()
    stray[outside[-1]] = 1
    assert not r0 <= off[outside[-1]] < r1
    _refused(dict(kw, agg_rank=stray), r0, r1, W, E, "outside the owned row range carries the owner's rank")
    _refused(kw, r0, r1, W - 1, E, "n_ranks is smaller than the number of ranks in agg_rank")
    # ... and the same through the rank-local description
    loc = xc.local_description(kw, r0, r1)
    assert _check_exchange(pa.Problem(**loc), r0, r1, W)[0] == 0
    _refused(dict(loc, agg_rank=None), r0, r1, W, E, "needs agg_rank")
    # a misaligned range is refused before the exchange is planned
    got, _, _, msg = _check_exchange(pa.Problem(**kw), r0 + 1, r1, W)
    assert got == E and "whole polytopes" in msg


def test_more_than_64_dofs_per_polytope_are_refused():
    part = xc.dgq4_world()
    assert part.n == 125
    prob = pa.Problem(**part.kw)
    assert prob.check(*part.rows(0))[5] == 125  # owner-computes-rows takes it
    code, _, _, msg = _check_exchange(prob, *part.rows(0), 2)
    assert code == _capi.PDH_EUNSUPPORTED and "more than 64 dofs per polytope" in msg and "no ghost-block exchange" in msg
