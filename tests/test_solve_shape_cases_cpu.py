"""The cases of tests/solve_shape_cases.py without a GPU: every case has the property it is listed for (from the host mirror's flattened
arrays), and the NumPy yardsticks pass, on oracle-assembled matrices, the conditions the device test (tests/test_gpu_solve_shapes.py)
relies on - CG converges, the three-step iterate is finite, the recorded float64-versus-long-double spreads hold - so that the device is
only compared on cases whose yardstick stands.  The pattern of tests/test_chebyshev_cpu.py."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import cheb_ref as cr
import solve_shape_cases as sc
from pcg_ref import diag_blocks, pcg, preconditioner


@pytest.mark.parametrize("cid", list(sc.CASES))
@pytest.mark.parametrize("diag_first", [True, False])
def test_every_case_has_the_property_it_is_listed_for(cid, diag_first):
    ah, fe, flat = sc.mirror_flat(cid, diag_first)
    arr = flat.arrays()
    rows = sc.check_property(cid, ah, fe, arr)
    c = sc.CASES[cid]
    n = c["n"]
    assert len(arr["colind"]) == rows.sum() and ah.n_dofs == n * c["n_agg"]
    if c["agg"][0] == "big":  # the explicit cell lists assume lexicographic cells: polytope 0 is the box they name
        lo, r, h = c["agg"][1], c["agg"][2], 1.0 / c["cells"]
        blo, bhi = ah.bbox(0)
        assert np.allclose(blo, lo * h, atol=1e-14) and np.allclose(bhi, (lo + r) * h, atol=1e-14)
        o = int(ah.dof_indices(0)[0])  # (dofs are numbered in the order of the master cells, not of the polytopes)
        own = np.zeros(len(rows), dtype=bool)
        own[o:o + n] = True
        assert np.all(rows[own] == c["row_max"]) and rows[~own].max() < c["row_max"]
        assert c["row_max"] == (1 + 2 * c["dim"] * r ** (c["dim"] - 1) // (2 if lo == 0 else 1)) * n
    if cid == "dgq4_3x3x3":
        assert sorted(set(rows // n)) == [4, 5, 6, 7]
    if cid == "dgq3_big_among_singles":
        assert sorted(set(rows // n)) == [4, 5, 6, 7, 13]
    if cid.startswith("slots"):
        assert (c["n_agg"] % 256 != 0) == (cid == "slots_289") and c["n_agg"] > 256


def test_the_case_lists_cover_the_table():
    assert set(sc.VMULT_IDS) == set(sc.CASES) - {"lds_cap_out"}
    assert set(sc.CG3_IDS) == {"dgq4_3x3x3", "dgp6", "dgp7", "dgq5", "dgq6", "dgq7", "dgq3_big_among_singles", "dgq3_grown"}
    assert all(sc.CASES[k]["n"] > 64 or sc.CASES[k]["row_max"] > 512 for k in sc.CG3_IDS)
    assert [sc.CASES[k]["n"] for k in ("dgp6", "dgp7", "dgq5", "dgq6", "dgq7")] == [84, 120, 216, 343, 512]
    for k in sc.CG3_IDS:
        assert ("block_jacobi" in sc.kinds_of(k)) == (sc.CASES[k]["n"] <= 64)


@pytest.mark.parametrize("cid", sc.CG3_IDS)
def test_three_step_iterate_of_the_host_loop_is_finite(cid):
    """what the device's iterate after max_iter = 3 is compared with: three steps taken, finite, not converged; the oracle's pattern has
    the mirror's row lengths"""
    A, n = sc.oracle_system(cid)
    ah, fe, flat = sc.mirror_flat(cid, False)
    assert np.array_equal(np.sort(np.diff(A.indptr)), np.sort(np.diff(np.asarray(flat.arrays()["rowptr"], dtype=np.int64))))
    b = sc.rhs(A.shape[0])
    for kind in sc.kinds_of(cid):
        x3, it3, res3 = pcg(A, b, preconditioner(A, n, kind), max_iter=3)
        assert it3 == 3 and np.all(np.isfinite(x3)) and np.isfinite(res3), (cid, kind)
        assert res3 > 1e-13 * np.linalg.norm(b) and np.linalg.norm(x3) > 0


@pytest.mark.parametrize("cid", sc.SLOT_IDS)
def test_many_slot_cases_converge_and_their_estimate_spread_is_recorded(cid):
    A, n = sc.oracle_system(cid)
    b = sc.rhs(A.shape[0])
    ref = spla.spsolve(A.tocsc(), b)
    for kind in ("none", "jacobi", "block_jacobi"):
        x, it, res = pcg(A, b, preconditioner(A, n, kind))
        assert np.linalg.norm(x - ref) <= 1e-9 * np.linalg.norm(ref) and res <= 1e-13 * np.linalg.norm(b), (cid, kind, it, res)
    for kind in ("jacobi", "block_jacobi"):
        assert cr.estimate(A, n, kind)[1] == 20
    if cid == "slots_289":  # (the long-double run of the other one multiplies a dense 4096 x 4096 matrix: `python tests/solve_shape_cases.py`)
        for kind in ("jacobi", "block_jacobi"):
            assert sc.estimate_spread(cid, kind) <= sc.SLOT_EST_SPREAD


@pytest.mark.parametrize("cid", sc.CHEB_IDS)
def test_chebyshev_yardstick_on_the_shape_cases(cid):
    """the estimate takes its 20 steps, 1.2 est gives a positive symmetric operator of every degree, and on the worst recorded case
    the spread of an application is the recorded one"""
    A, n = sc.oracle_system(cid)
    b, x0 = sc.vectors(A.shape[0])
    for kind in sc.cheb_kinds(cid):
        est, steps = cr.estimate(A, n, kind)
        assert steps == 20 and est > 0
        lo, hi = cr.bounds(est)
        for m in sc.CHEB_DEGREES:
            Mb, Mx = cr.apply(A, n, kind, lo, hi, m, b), cr.apply(A, n, kind, lo, hi, m, x0)
            assert np.all(np.isfinite(Mb)) and np.all(np.isfinite(cr.apply(A, n, kind, lo, hi, m, b, x0)))
            assert b @ Mb > 0 and abs(x0 @ Mb - b @ Mx) <= 1e-12 * np.linalg.norm(x0) * np.linalg.norm(Mb), (cid, kind, m)
    if cid == "dgp6":
        assert sc.z_spread(cid, "jacobi") <= sc.SHAPE_Z_SPREAD


@pytest.mark.parametrize("iid", list(sc.INVERSE_CASES))
def test_block_inverse_spread_is_the_recorded_one(iid):
    """the diagonal blocks are positive definite and numpy.linalg.inv stays within the recorded spread of the long-double inverse; on
    the anisotropic meshes block-Jacobi CG reaches the direct solution within the bounds the device test uses"""
    A, n = sc.inverse_oracle_system(iid)
    blocks = diag_blocks(A, n)
    assert n <= 64 and np.linalg.eigvalsh(blocks).min() > 0
    spread, blk = sc.inverse_spread(iid)
    print(iid, "spread %.3e (block %d), recorded %.3e" % (spread, blk, sc.INVERSE_SPREAD[iid]))
    assert spread <= sc.INVERSE_SPREAD[iid]
    if iid in sc.ANISO_CG_IDS:
        b = sc.rhs(A.shape[0])
        ref = spla.spsolve(A.tocsc(), b)
        x, it, res = pcg(A, b, preconditioner(A, n, "block_jacobi"))
        dx = float(np.linalg.norm(x - ref) / np.linalg.norm(ref))
        print(iid, "cond_2(A) = %.3e, %d iterations, |x - spsolve| / |spsolve| = %.3e" % (np.linalg.cond(A.toarray()), it, dx))
        assert dx <= 1e-9 and res <= 1e-13 * np.linalg.norm(b)


def test_tolerances_come_from_the_recorded_spreads():
    assert sc.SLOT_EST_TOL == max(100 * sc.SLOT_EST_SPREAD, 1e-13) and sc.SHAPE_Z_TOL == max(100 * sc.SHAPE_Z_SPREAD, 1e-13)
    assert set(sc.INVERSE_TOL) == set(sc.INVERSE_SPREAD) == set(sc.INVERSE_CASES)
    for k, v in sc.INVERSE_SPREAD.items():
        assert 0 < v and sc.INVERSE_TOL[k] == max(100 * v, 1e-13)
