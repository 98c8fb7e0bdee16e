"""The Galerkin product without a GPU: the host planner (pdh_galerkin_plan through ctypes) against a brute-force plan on the oracle's
patterns, every refusal with its message, the block pattern of P^T A P against the assembled coarse pattern, the float64 yardstick
against its long-double form, and V-cycle PCG on the Galerkin hierarchy with the NumPy restatements.  Cases: tests/galerkin_cases.py."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import galerkin_cases as gc
import galerkin_ref as gr
import pcg_ref
import vcycle_cases as vc
import vcycle_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _capi():
    from polydeal_amd import _capi
    return _capi


def _level(lists, off, n_rows, **kw):
    return _capi().GalerkinLevel(blk_ptr=lists[0], blk_dof=lists[1], dof_offset=off, n_rows=n_rows, **kw)


def _pair_lists(case, l, keys=(None, None)):
    """((fine lists, coarse lists), desc) of level pair l of a case from the oracle's patterns; keys: the order of the blocks per level"""
    n = gc.SHAPES[case][0]
    mats, d = gc.oracle_matrices(case), gc.descriptions(case)[l]
    return (gc.level_lists(mats[l + 1], d.fine_dof_offset, n, keys[0]), gc.level_lists(mats[l], d.coarse_dof_offset, n, keys[1])), d


def _check_plan(lists, d):
    E = _capi()
    fine, coarse = lists
    ptr, slot, pos = E.galerkin_plan(d, _level(fine, d.fine_dof_offset, d.n_fine_rows), _level(coarse, d.coarse_dof_offset, d.n_coarse_rows))
    ref = gr.brute_force_plan(d.parent, fine, d.fine_dof_offset, coarse, d.coarse_dof_offset)
    assert len(ptr) == len(ref) + 1 and ptr[0] == 0 and ptr[-1] == len(slot) == int(fine[0][-1])
    got = [list(zip(slot[ptr[b]:ptr[b + 1]].tolist(), pos[ptr[b]:ptr[b + 1]].tolist())) for b in range(len(ref))]
    assert got == ref
    # every fine block exactly once, in ascending (slot, position) inside every coarse block
    every = sorted(e for blk in got for e in blk)
    assert every == [(F, t) for F in range(d.n_fine) for t in range(int(fine[0][F + 1] - fine[0][F]))]
    assert all(blk == sorted(blk) and len(blk) > 0 for blk in got)


@pytest.mark.parametrize("case", gc.ALL, ids=gc.case_id)
def test_planner_against_the_brute_force_plan(case):
    gc.check_shape(case)
    for l in range(len(gc.descriptions(case))):
        _check_plan(*_pair_lists(case, l))


@pytest.mark.parametrize("case", [gc.CASES[0], gc.CASES[3]], ids=gc.case_id)
def test_planner_with_blocks_ordered_by_col_offset(case):
    """pdh_problem.col_offset orders the blocks of a row by another numbering than dof_offset: the plan follows the block lists"""
    l = len(gc.descriptions(case)) - 1
    d = gc.descriptions(case)[l]
    rng = np.random.default_rng(3)
    keys = (rng.permutation(d.n_fine), rng.permutation(d.n_coarse))
    lists, d = _pair_lists(case, l, keys)
    plain, _ = _pair_lists(case, l)
    assert not np.array_equal(lists[0][1], plain[0][1]) and not np.array_equal(lists[1][1], plain[1][1])
    _check_plan(lists, d)


def _refused(code, *words, d, fine, coarse):
    E = _capi()
    with pytest.raises(E.PdhError) as e:
        E.galerkin_plan(d, fine, coarse)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_planner_refusals():
    E = _capi()
    case = gc.CASES[0]
    (fine, coarse), d = _pair_lists(case, 1)
    n = d.n
    F = lambda lists=fine, off=d.fine_dof_offset, rows=d.n_fine_rows, **kw: _level(lists, off, rows, **kw)
    Cl = lambda lists=coarse, off=d.coarse_dof_offset, rows=d.n_coarse_rows, **kw: _level(lists, off, rows, **kw)
    E.galerkin_plan(d, F(), Cl())
    # PDH_EINVAL: the parents of a coupled fine pair are no block of the coarse pattern (a coarse row list with one block taken out)
    ptr, dof = coarse
    cut_ptr = ptr.copy()
    cut_ptr[1:] -= 1
    _refused(E.PDH_EINVAL, "not nested", "face-neighbour", d=d, fine=F(), coarse=Cl(lists=(cut_ptr, np.delete(dof, 1))))
    # ... a coarse block that receives nothing (one block too many: polytope 0 coupled to the farthest one)
    far = int(d.coarse_dof_offset[d.n_coarse - 1])
    assert far not in dof[ptr[0]:ptr[1]].tolist()
    add_ptr = ptr.copy()
    add_ptr[1:] += 1
    _refused(E.PDH_EINVAL, "receives no contribution", "coarse polytope 0", d=d, fine=F(),
             coarse=Cl(lists=(add_ptr, np.insert(dof, ptr[1], far))))
    # ... row counts, polytope counts and dof offsets that differ from the transfer's
    _refused(E.PDH_EINVAL, "fine level has %d rows" % (d.n_fine_rows + n), d=d, fine=F(rows=d.n_fine_rows + n), coarse=Cl())
    _refused(E.PDH_EINVAL, "coarse level has %d rows" % (d.n_coarse_rows + n), d=d, fine=F(), coarse=Cl(rows=d.n_coarse_rows + n))
    swapped = np.array(d.coarse_dof_offset).copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    _refused(E.PDH_EINVAL, "dof offset of coarse polytope 0", d=d, fine=F(), coarse=Cl(off=swapped))
    _refused(E.PDH_EINVAL, "polytopes", d=d, fine=Cl(), coarse=Cl())
    # ... a block dof that is not the first dof of a polytope
    bad = fine[1].copy()
    bad[2] += 1
    _refused(E.PDH_EINVAL, "not the first dof of a polytope", "fine polytope 0", d=d, fine=F(lists=(fine[0], bad)), coarse=Cl())
    # PDH_EUNSUPPORTED: rank-local and ghost contexts, two devices
    _refused(E.PDH_EUNSUPPORTED, "all rows", "fine level", d=d, fine=F(n_rows_owned=d.n_fine_rows - n), coarse=Cl())
    _refused(E.PDH_EUNSUPPORTED, "PDH_EXCHANGE_GHOST", "coarse level", d=d, fine=F(), coarse=Cl(exchange_mode=1))
    _refused(E.PDH_EUNSUPPORTED, "device 0", "device 1", d=d, fine=F(), coarse=Cl(device=1))
    # ... more than 64 dofs per polytope: 3-D FE_DGQ(4), which the transfers accept
    import transfer_cases as tc

    big = tc.build(("pair",) + tc.PAIRS[5]).desc
    assert big.n == 125
    big.check()
    _refused(E.PDH_EUNSUPPORTED, "at most 64 dofs", "125", "transfers accept", d=big, fine=F(), coarse=Cl())
    # the description itself is checked first, NULL outputs are refused
    lib = E.load_library()
    import ctypes as C
    assert lib.pdh_galerkin_plan(None, C.byref(F().c), C.byref(Cl().c), None, None, None) == E.PDH_EINVAL
    assert lib.pdh_galerkin_plan(C.byref(d.c), C.byref(F().c), C.byref(Cl().c), None, None, None) == E.PDH_EINVAL
    assert b"required" in lib.pdh_last_error(None)


@pytest.mark.parametrize("case", gc.ALL, ids=gc.case_id)
def test_pattern_and_rounding_of_the_yardstick(case):
    """On every level pair, A the oracle's assembled fine matrix: the block pattern of P^T A P (threshold 1e-12 max|entry|) is the
    assembled coarse level's, and the float64 yardstick stays within 1e-13 (|P|^T |A| |P|)_ij of its long-double form - the bound the
    device is held to is one the reference arithmetic itself keeps."""
    n = gc.SHAPES[case][0]
    mats, Ps, descs = gc.oracle_matrices(case), gc.injections(case), gc.descriptions(case)
    for l, (P, d) in enumerate(zip(Ps, descs)):
        A = mats[l + 1]
        G64, Gld, Gabs = gr.product(P, A), gr.product_longdouble(P, A, d), gr.abs_product(P, A)
        got = gr.block_pattern(G64, n, 1e-12 * np.max(np.abs(G64)))
        want = gr.block_pattern(gr.dense(mats[l]), n, 0.0)
        assert got == want, (l, len(got), len(want))
        assert len(want) == gc.SHAPES[case][2][l]
        err = np.abs(G64.astype(gr.LD) - Gld)
        worst = float(np.max(err / np.where(Gabs > 0, Gabs, 1.0)))
        print("%s pair %d: max |G64 - Gld| / (|P|^T |A| |P|) = %.3e; max|G - assembled| / max|assembled| = %.2f" %
              (gc.case_id(case), l, worst, np.max(np.abs(G64 - gr.dense(mats[l]))) / np.max(np.abs(gr.dense(mats[l])))))
        assert np.all(err <= gr.TOL * Gabs)
        assert np.max(np.abs(G64 - G64.T)) <= 1e-13 * np.max(np.abs(G64))


@pytest.mark.parametrize("case", gc.ALL, ids=gc.case_id)
def test_the_factors_of_the_product_against_the_oracle_injection(case):
    """pdh_galerkin_matrices_1d: the Kronecker products of the 1-D factors the device applies have the zeros of the oracle's injection
    - exact where a fine support point is a coarse one - and, both products formed in long double on the oracle's fine matrix, give
    P^T A P within 1e-13 (|P|^T |A| |P|)_ij of the oracle injection's, entry by entry: the difference of the two injections alone
    leaves the device its bound.  The transfer's own factors (pdh_transfer_matrices_1d) differ from these by 64 ulp at most, in rows
    that are unit vectors to rounding."""
    import transfer_cases as tc

    mats, Ps, descs = gc.oracle_matrices(case), gc.injections(case), gc.descriptions(case)
    for l, (P, d) in enumerate(zip(Ps, descs)):
        P = np.asarray(P)
        B, Bt = d.galerkin_matrices_1d(), d.matrices_1d()
        moved = B != Bt
        assert np.max(np.abs(B - Bt)) <= 64 * 2.220446049250313e-16
        rows = moved.any(axis=-1)
        assert np.all(np.sort(B[rows], axis=-1)[:, :-1] == 0.0) and np.all(B[rows].max(axis=-1) == 1.0)
        Pg = tc.dense_from_blocks(d, tc.kron_blocks(B))
        assert np.array_equal(Pg == 0, P == 0)
        A = mats[l + 1]
        err = np.abs(gr.product_longdouble(Pg, A, d) - gr.product_longdouble(P, A, d))
        Gabs = gr.abs_product(P, A)
        print("%s pair %d: %d rows of the 1-D factors made exact; max|P_dev - P_oracle| = %.3e; worst ratio to the bound %.3e" %
              (gc.case_id(case), l, int(rows.sum()), np.max(np.abs(Pg - P)), float(np.max(err[Gabs > 0] / Gabs[Gabs > 0])) / gr.TOL))
        assert np.all(err <= gr.TOL * Gabs)


def test_the_long_double_product_is_one():
    """the block-wise long-double product against numpy's own dense long-double matmul on the smallest case, entry by entry"""
    case = gc.CASES[0]
    P, A, d = gc.injections(case)[1], gr.dense(gc.oracle_matrices(case)[2]), gc.descriptions(case)[1]
    slow = P.astype(gr.LD).T @ (A.astype(gr.LD) @ P.astype(gr.LD))
    assert np.all(np.abs(gr.product_longdouble(P, A, d) - slow) <= 64 * float(np.finfo(gr.LD).eps) * gr.abs_product(P, A))


@pytest.fixture(scope="module")
def galerkin_hierarchy():
    cache = {}

    def get(case):
        """vcycle_ref.Hierarchy whose coarse matrices are the float64 yardstick chained from the oracle's finest matrix, on the pattern
        of the assembled levels (what the device stores)"""
        if case not in cache:
            mats, Ps = gc.oracle_matrices(case), gc.injections(case)
            n = (case[3] + 1) ** case[0]
            chain = gr.chain(Ps, mats[-1])
            lv = [sp.csr_matrix(np.where(gr.dense(m) != 0, g, 0.0)) for m, g in zip(mats[:-1], chain[:-1])] + [mats[-1]]
            kind = vc.inner_kind(n)
            cache[case] = vr.Hierarchy(lv, n, Ps, vr.smoother_bounds(lv, n, kind), vc.DEGREE, kind)
        return cache[case]
    return get


@pytest.mark.parametrize("case", gc.PCG_CASES, ids=gc.case_id)
def test_pcg_on_the_galerkin_hierarchy(case, galerkin_hierarchy):
    """V-cycle PCG converges to rel_tol 1e-13 on the Galerkin hierarchy, in the recorded number of iterations - about as many as on the
    re-assembled one"""
    H = galerkin_hierarchy(case)
    A = H.mats[-1]
    b = gc.rhs(A.shape[0])
    x, it, res = pcg_ref.pcg(A, b, vr.preconditioner(H), rel_tol=1e-13)
    _, it_asm, _ = pcg_ref.pcg(A, b, vr.preconditioner(vc.oracle_hierarchy(case)), rel_tol=1e-13)
    print("%s: PCG iterations to 1e-13: Galerkin %d, re-assembled %d" % (gc.case_id(case), it, it_asm))
    assert np.linalg.norm(b - A @ x) <= 1e-12 * np.linalg.norm(b)
    assert (it, it_asm) == gc.PCG_COUNTS[case]
    assert abs(it - it_asm) <= 10


@pytest.mark.parametrize("case", gc.PCG_CASES[:3], ids=gc.case_id)
def test_the_galerkin_cycle_is_symmetric(case, galerkin_hierarchy):
    """u^T M v = v^T M u for the applied cycle M (from zero), within 1e-12 |u| |M v| (the check of test_vcycle_cpu.py)"""
    H = galerkin_hierarchy(case)
    rng = np.random.default_rng(5)
    N = H.mats[-1].shape[0]
    for _ in range(3):
        u, v = rng.standard_normal(N), rng.standard_normal(N)
        Mv, Mu = vr.cycle(H, v), vr.cycle(H, u)
        a, b = float(u @ Mv), float(v @ Mu)
        assert abs(a - b) <= 1e-12 * float(np.linalg.norm(u) * np.linalg.norm(Mv))


def test_the_galerkin_cycle_is_positive(galerkin_hierarchy):
    """dense eigenvalues of the applied cycle on the 256-row case; the Galerkin level matrices themselves are positive definite"""
    H = galerkin_hierarchy(gc.CASES[0])
    N = H.mats[-1].shape[0]
    assert N == 256
    M = np.stack([vr.cycle(H, e) for e in np.eye(N)], axis=1)
    assert np.max(np.abs(M - M.T)) <= 1e-12 * np.max(np.abs(M))
    assert np.linalg.eigvalsh((M + M.T) / 2)[0] > 0
    for m in H.mats[:-1]:
        D = gr.dense(m)
        assert np.linalg.eigvalsh((D + D.T) / 2)[0] > 0


def test_header_and_ctypes_agree_on_the_level_struct():
    E = _capi()
    hdr = open(os.path.join(ROOT, "include", "polydeal_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    text = re.search(r"typedef struct pdh_galerkin_level\s*\{(.*?)\}", body, re.S).group(1)
    fields = []
    for t, names in re.findall(r"(?:const\s+)?(\w+)\s+([\w\s,\*]+);", text):
        fields += [(nm.strip().lstrip("*"), "ptr" if "*" in nm else t) for nm in names.split(",")]
    got = [(f[0], "ptr" if f[1] is E.C.c_void_p else "int32_t") for f in E.pdh_galerkin_level._fields_]
    assert got == fields
    for sym in ("pdh_galerkin_plan", "pdh_galerkin_device"):
        assert sym in E.EXPORTS and re.search(r"\b%s\s*\(" % sym, body), sym
    if os.path.exists(E.LIB_PATH):
        lib = E.load_library()
        assert lib.pdh_galerkin_device.argtypes == [E.pdh_transfer_p, E.pdh_ctx_p]
