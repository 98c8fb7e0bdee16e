"""The Galerkin product on the device (csrc/pdh_galerkin.hip; C ABI: pdh_galerkin_device): every entry of P^T A P against the long-double
yardstick (tests/galerkin_ref.py) applied to the fine values as read back, in all four layout combinations; the same bits twice; the
variational identity A_c x = P^T (A_f (P x)) composed of device calls alone; chained levels; the state rules and refusals; and
levels.multigrid_hierarchy(coarse_operators="galerkin") end to end.  Cases and shapes: tests/galerkin_cases.py."""
import hashlib

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import galerkin_cases as gc
import galerkin_ref as gr
import pcg_ref
import vcycle_cases as vc
import vcycle_ref as vr
from test_gpu_solve import _Device, _global_matrix

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
LAYOUT_IDS = {True: "dealii", False: "ascending"}


def _pa():
    import polydeal_amd as pa
    return pa


def _variant(fe):
    return _pa().SipVariant.poisson_example(fe)


class _Levels:
    """One context per level of a case (coarse to fine) with its problem resident - layouts[l]: diagonal first or ascending - and the
    transfers between them; nothing assembled yet."""

    def __init__(self, case, layouts=None):
        pa = _pa()
        from polydeal_amd.levels import level_transfer

        self.mirror, _ = gc.handlers(case)
        dim, p = gc.dim_degree(case)
        self.fe = pa.FE_DGQ(dim, p)
        self.n = self.fe.n_dofs_per_cell
        self.layouts = layouts or [True] * len(self.mirror)
        self.ctxs, self.flats, self.transfers = [], [], []
        try:
            for l, ah in enumerate(self.mirror):
                ctx = pa.Context(0)
                self.ctxs.append(ctx)
                self.flats.append(ah.flatten(_variant(self.fe), self.layouts[l], True))
                ctx.set_problem(self.flats[l])
                if l > 0:
                    self.transfers.append(level_transfer(ctx, self.mirror[l - 1], ah))
        except Exception:
            self.close()
            raise

    def matrix(self, l):
        """level l as it stands in HBM: scipy CSR"""
        return _global_matrix(self.ctxs[l], self.flats[l].arrays(), self.mirror[l].n_dofs)

    def close(self):
        for t in self.transfers:
            t.close()
        for c in self.ctxs:
            c.close()


_YARDSTICK = {}


def _yardstick(key, P, A, desc):
    """(long-double P^T A P, |P|^T |A| |P|) of a fine matrix as read back, computed once per (case, pair, fine values)"""
    D = gr.dense(A)
    key = key + (hashlib.sha1(np.ascontiguousarray(D).tobytes()).hexdigest(),)
    if key not in _YARDSTICK:
        _YARDSTICK[key] = (gr.product_longdouble(P, A, desc), gr.abs_product(P, A))
    return _YARDSTICK[key]


def _check_entries(what, G, ref, bound):
    """|G - ref|_ij <= bound_ij everywhere; the worst ratio is printed first"""
    err = np.abs(G.astype(gr.LD) - ref)
    large = bound > 1e-20 * np.max(bound)
    ratio = float(np.max(err[large] / bound[large]))
    beyond = err > bound
    print("%s: max |G_dev - G_ref|_ij / bound_ij = %.3e where the bound is above 1e-20 of its largest; %d of %d entries beyond their bound, "
          "by at most %.3e (largest bound %.3e)" % (what, ratio, int(beyond.sum()), beyond.size,
                                                   float(np.max(err[beyond])) if beyond.any() else 0.0, float(np.max(bound))))
    assert np.all(np.isfinite(G))
    assert not beyond.any(), (what, ratio, int(beyond.sum()))


PARITY = [(c, f, k) for c in gc.LAYOUT_CASES for f in (True, False) for k in (True, False)] + \
         [(c, True, True) for c in gc.ALL if c not in gc.LAYOUT_CASES]


def _table_injections(case):
    """[P_l] from the 1-D matrices the device applies (pdh_galerkin_matrices_1d), by the Kronecker formula"""
    import transfer_cases as tc

    return [tc.dense_from_blocks(d, tc.kron_blocks(d.galerkin_matrices_1d())) for d in gc.descriptions(case)]


def _parity(case, fine_df, coarse_df, Ps, tag):
    rows = gc.check_shape(case)
    descs = gc.descriptions(case)
    for l in range(len(descs)):
        layouts = [coarse_df] * len(rows)
        layouts[l + 1] = fine_df
        L = _Levels(case, layouts)
        try:
            fine, coarse, t = L.ctxs[l + 1], L.ctxs[l], L.transfers[l]
            fine.assemble_device()
            A = L.matrix(l + 1)
            coarse.poison_values()
            t.galerkin_device(coarse)
            v1 = coarse.values()
            G = L.matrix(l).toarray()
            ref, Gabs = _yardstick((case, l, tag), Ps[l], A, descs[l])
            _check_entries("%s pair %d (%s injection)" % (gc.case_id(case), l, tag), G, ref, gr.TOL * Gabs)
            # nothing outside the coarse pattern is lost: the yardstick is zero there to the same bound
            mask = np.zeros(G.shape, dtype=bool)
            M = L.matrix(l).tocoo()
            mask[M.row, M.col] = True
            assert np.all(np.abs(ref[~mask]) <= gr.TOL * Gabs[~mask])
            coarse.poison_values()
            t.galerkin_device(coarse)
            assert np.array_equal(coarse.values(), v1)
            assert np.array_equal(L.matrix(l + 1).toarray(), A.toarray())  # the fine values are only read
        finally:
            L.close()


def _parity_ids(params):
    return ["%s-%s_to_%s" % (gc.case_id(c), LAYOUT_IDS[f], LAYOUT_IDS[k]) for c, f, k in params]


@pytest.mark.parametrize("case,fine_df,coarse_df", PARITY, ids=_parity_ids(PARITY))
def test_entrywise_parity_and_the_same_bits_twice(case, fine_df, coarse_df):
    """Every level pair of the case on its own: the fine level assembled on the device and read back, pdh_galerkin_device into the
    (poisoned) coarse values, every entry within 1e-13 (|P|^T |A| |P|)_ij of the long-double yardstick - P the oracle's dense injection -
    on the fine values read back; a second call gives the same bits.  Level l is in the fine layout when it is the fine side of a
    pair, else in the coarse one.

    Measured: the largest ratio to the bound is 0.004 at n = 9 and 27, 0.017 on the distorted grid, 0.022 for FE_DGQ(3) and 0.046 for FE_DGQ(7) at n = 64.  A third of the
    entries of a coarse block of FE_DGQ(3) and FE_DGQ(7) have a sum of absolute products of exactly zero, or 1e-29: the oracle's
    injection is exactly zero where a fine support point is a coarse one, and the bound there admits nothing but a zero.  The product
    meets it because it applies 1-D factors that are exact in those places (pdh_galerkin_matrices_1d); with the transfer's rounded
    factors, which hold up to 1.1e-19 and 1.3e-17 there, 43008 of 262144 and 25088 of 65536 entries lay beyond it."""
    _parity(case, fine_df, coarse_df, gc.injections(case), "oracle")


TABLE_PARITY = [p for p in PARITY if gc.SHAPES[p[0]][0] == 64] + [(gc.CASES[3], True, False)]


@pytest.mark.parametrize("case,fine_df,coarse_df", TABLE_PARITY, ids=_parity_ids(TABLE_PARITY))
def test_entrywise_parity_with_the_factors_the_product_applies(case, fine_df, coarse_df):
    """The same check with P the Kronecker products of the 1-D matrices the kernel is given (pdh_galerkin_matrices_1d), which differ
    from the oracle's injection by its rounding (up to 8.9e-16 for FE_DGQ(3), 3.3e-15 for FE_DGQ(7)): every entry within 1e-13 of ITS
    sum of absolute products, on the n = 64 elements in every layout."""
    Ps = _table_injections(case)
    for P, P_oracle in zip(Ps, gc.injections(case)):
        assert np.max(np.abs(P - np.asarray(P_oracle))) <= 1e-14
    _parity(case, fine_df, coarse_df, Ps, "device")


def test_permuted_numbering_and_dof_offsets():
    """the n = 9 pair with the dof ranges of both levels shuffled (ascending layout, as pdh_problem.dof_offset allows): blocks ordered by
    the shuffled offsets on both sides"""
    pa = _pa()
    from polydeal_amd._capi import TransferDesc, Transfer
    from test_gpu_vcycle import _permuted_problem

    case = gc.PERMUTED_BASE
    gc.check_shape(case)
    mirror, _ = gc.handlers(case)
    fe = pa.FE_DGQ(case[0], case[3])
    d0, P0 = gc.descriptions(case)[0], gc.injections(case)[0]
    (prob_c, m_c), (prob_f, m_f) = _permuted_problem(mirror[0], fe), _permuted_problem(mirror[1], fe)
    n = fe.n_dofs_per_cell
    desc = TransferDesc(dim=d0.dim, degree=d0.degree, fine_bbox=d0.fine_bbox, coarse_bbox=d0.coarse_bbox,
                        fine_dof_offset=m_f[np.asarray(d0.fine_dof_offset)], coarse_dof_offset=m_c[np.asarray(d0.coarse_dof_offset)],
                        parent=d0.parent)
    assert np.any(desc.fine_dof_offset != d0.fine_dof_offset) and np.any(desc.coarse_dof_offset != d0.coarse_dof_offset)
    P = np.zeros_like(P0)
    P[np.ix_(m_f, m_c)] = P0
    fine, coarse = pa.Context(0), pa.Context(0)
    t = None
    try:
        fine.set_problem(prob_f)
        coarse.set_problem(prob_c)
        fine.assemble_device()
        A = _global_matrix(fine, prob_f.arrays, mirror[1].n_dofs)
        t = Transfer(fine, desc)
        coarse.poison_values()
        t.galerkin_device(coarse)
        G = _global_matrix(coarse, prob_c.arrays, mirror[0].n_dofs).toarray()
        _check_entries("permuted", G, gr.product_longdouble(P, A, desc), gr.TOL * gr.abs_product(P, A))
        assert n == 9
    finally:
        if t is not None:
            t.close()
        fine.close()
        coarse.close()


@pytest.mark.parametrize("case", [gc.CASES[1], gc.CASES[3], gc.CASES[4], gc.CASES[5]], ids=gc.case_id)
def test_variational_identity_on_the_device(case):
    """For a random coarse x on the finest pair: A_c x by pdh_vmult_device on the coarse context against P^T (A_f (P x)) by
    pdh_prolongate_device, pdh_vmult_device, pdh_restrict_device - no host arithmetic between the calls.  Every row within 1e-13 of its
    sum of absolute products (|P|^T |A_f| |P| |x|)_i, formed on the host from the values read back."""
    gc.check_shape(case)
    L, dev = _Levels(case), _Device()
    try:
        l = len(L.transfers) - 1
        fine, coarse, t = L.ctxs[l + 1], L.ctxs[l], L.transfers[l]
        fine.assemble_device()
        t.galerkin_device(coarse)
        Nc, Nf = L.mirror[l].n_dofs, L.mirror[l + 1].n_dofs
        x = np.random.default_rng(13).standard_normal(Nc)
        d_x, d_y, d_px, d_apx, d_z = dev.put(x), dev.put(np.full(Nc, np.nan)), dev.put(np.full(Nf, np.nan)), dev.put(np.full(Nf, np.nan)), \
            dev.put(np.full(Nc, np.nan))
        coarse.vmult_device(d_x, d_y)
        coarse.synchronize()
        t.prolongate_device(d_x, d_px)
        fine.vmult_device(d_px, d_apx)
        t.restrict_device(d_apx, d_z)
        fine.synchronize()
        y, z = dev.get(d_y, Nc), dev.get(d_z, Nc)
        P = np.abs(np.asarray(gc.injections(case)[l]))
        bound = gr.TOL * (P.T @ (abs(L.matrix(l + 1)) @ (P @ np.abs(x))))
        ratio = float(np.max(np.abs(y - z) / bound))
        print("%s: max |A_c x - P^T A_f P x|_i / (1e-13 sum of absolute products) = %.3e" % (gc.case_id(case), ratio))
        assert np.all(np.isfinite(y)) and np.all(np.abs(y - z) <= bound)
    finally:
        L.close()
        dev.free()


def test_chained_levels():
    """The four-level case: the finest level assembled, every level below it the Galerkin product of the level above.  Against the
    yardstick chained the same way (long-double products, rounded to double between the levels); the bound of a level is 1e-13 of its
    own sum of absolute products plus the bound of the level above carried through |P|^T . |P| - the product is linear in the fine
    matrix."""
    case = gc.CASES[1]
    rows = gc.check_shape(case)
    assert len(rows) == 4 and rows[0] == 9
    Ps, descs = gc.injections(case), gc.descriptions(case)
    L = _Levels(case)
    try:
        L.ctxs[-1].assemble_device()
        for l in range(len(rows) - 1, 0, -1):
            L.ctxs[l - 1].poison_values()
            L.transfers[l - 1].galerkin_device(L.ctxs[l - 1])
        ref = gr.chain(Ps, L.matrix(len(rows) - 1), descs)
        bound = np.zeros(ref[-1].shape)
        for l in range(len(rows) - 2, -1, -1):
            aP = np.abs(np.asarray(Ps[l]))
            bound = gr.TOL * gr.abs_product(Ps[l], ref[l + 1]) + aP.T @ (bound @ aP)
            _check_entries("chained level %d" % l, L.matrix(l).toarray(), ref[l].astype(gr.LD), bound)
    finally:
        L.close()


def test_state_rules_and_refusals():
    pa = _pa()
    E = pa._capi
    from polydeal_amd._capi import Multigrid
    from polydeal_amd.levels import level_transfer

    case = gc.CASES[0]
    mirror, _ = gc.handlers(case)
    fe = pa.FE_DGQ(case[0], case[3])
    var = _variant(fe)
    ctxs = [pa.Context(0) for _ in mirror]
    c0, c1, c2 = ctxs
    ts, mg, dev = [], None, _Device()
    try:
        lib = c0.lib
        ts = [level_transfer(c1, mirror[0], mirror[1]), level_transfer(c2, mirror[1], mirror[2])]
        assert lib.pdh_galerkin_device(None, c0.h) == E.PDH_EINVAL
        assert lib.pdh_galerkin_device(ts[0].h, None) == E.PDH_EINVAL
        # PDH_ESTATE: no fine problem, no fine values, no coarse problem - reported on the fine context
        for expect in ("before pdh_set_problem on the fine context", "never assembled", "before pdh_set_problem on the coarse context"):
            with pytest.raises(pa.PdhError) as e:
                ts[0].galerkin_device(c0)
            assert e.value.code == E.PDH_ESTATE and expect in str(e.value), str(e.value)
            if "fine context" in expect:
                c1.set_problem(mirror[1].flatten(var, True, True))
            elif "never" in expect:
                c1.assemble_device()
        flats = [ah.flatten(var, True, True) for ah in mirror]
        for c, f in zip(ctxs, flats):
            c.set_problem(f)
        for c in ctxs:
            c.assemble_device()
        assembled0 = c0.values()
        # a preconditioner set up on the coarse context before the call is stale after it
        c0.setup_direct()
        ts[0].galerkin_device(c0)
        d = dev.put(np.zeros(mirror[0].n_dofs))
        with pytest.raises(pa.PdhError) as e:
            c0.precondition_device(d, d)
        assert e.value.code == E.PDH_ESTATE and "values changed" in str(e.value)
        galerkin0 = c0.values()
        assert not np.array_equal(galerkin0, assembled0)
        # everything that reads the values works on them: the product, every set-up, CG
        A0 = _global_matrix(c0, flats[0].arrays(), mirror[0].n_dofs)
        x = np.random.default_rng(3).standard_normal(mirror[0].n_dofs)
        assert np.max(np.abs(c0.vmult(x) - A0 @ x)) <= 1e-13 * np.max(abs(A0) @ np.abs(x))
        c0.setup_preconditioner("block_jacobi")
        c0.setup_chebyshev("block_jacobi", degree=3)
        c0.setup_direct()
        xs, cg = c0.solve_cg(x)
        assert cg["iterations"] <= 2 and np.max(np.abs(A0 @ xs - x)) <= 1e-9 * np.max(np.abs(x))
        # a pdh_mg that holds the coarse context turns stale, naming the level
        c1.setup_chebyshev("block_jacobi", degree=3)
        c2.setup_chebyshev("block_jacobi", degree=3)
        mg = Multigrid(ctxs, ts)
        N = mirror[2].n_dofs
        d_b, d_x = dev.put(gc.rhs(N)), dev.put(np.zeros(N))
        mg.vcycle_device(d_b, d_x, True)
        c2.synchronize()
        ts[0].galerkin_device(c0)
        with pytest.raises(pa.PdhError) as e:
            mg.vcycle_device(d_b, d_x, True)
        assert e.value.code == E.PDH_ESTATE and "values of level 0 of 3" in str(e.value), str(e.value)
        mg.close()
        mg = None
        # the same product again gives the same values; pdh_assemble_device afterwards restores the assembled ones
        assert np.array_equal(c0.values(), galerkin0)
        c0.assemble_device()
        assert np.array_equal(c0.values(), assembled0)
        # the plan follows a new problem on either context: the coarse level in the other layout
        c0.set_problem(mirror[0].flatten(var, False, True))
        ts[0].galerkin_device(c0)
        B0 = _global_matrix(c0, mirror[0].flatten(var, False, True).arrays(), mirror[0].n_dofs)
        assert np.array_equal(B0.toarray(), A0.toarray())
        # a transfer whose levels are not the contexts': row counts differ
        with pytest.raises(pa.PdhError) as e:
            ts[1].galerkin_device(c0)
        assert e.value.code == E.PDH_EINVAL and "coarse level" in str(e.value)
        # a rank-local coarse context
        from polydeal_amd.partition import row_range

        split = row_range(mirror[0].n_agglomerates, fe.n_dofs_per_cell, 1, 2)[0]
        c0.set_problem(mirror[0].flatten(var, True, True), 0, split)
        with pytest.raises(pa.PdhError) as e:
            ts[0].galerkin_device(c0)
        assert e.value.code == E.PDH_EUNSUPPORTED and "all rows" in str(e.value), str(e.value)
    finally:
        if mg is not None:
            mg.close()
        for t in ts:
            t.close()
        for c in ctxs:
            c.close()
        dev.free()


def test_more_than_64_dofs_per_polytope_is_refused():
    pa = _pa()
    from polydeal_amd.levels import level_transfer

    case = vc.CASES[5]
    mirror, _ = vc.handlers(*case)
    fe = pa.FE_DGQ(case[0], case[3])
    assert fe.n_dofs_per_cell == 125
    ctxs, t = [pa.Context(0), pa.Context(0)], None
    try:
        for c, ah in zip(ctxs, mirror):
            c.set_problem(ah.flatten(_variant(fe), True, True))
        ctxs[1].assemble_device()
        t = level_transfer(ctxs[1], mirror[0], mirror[1])
        with pytest.raises(pa.PdhError) as e:
            t.galerkin_device(ctxs[0])
        assert e.value.code == pa._capi.PDH_EUNSUPPORTED and "at most 64 dofs" in str(e.value) and "125" in str(e.value)
    finally:
        if t is not None:
            t.close()
        for c in ctxs:
            c.close()


def _rel(x, ref):
    return float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("case", [vc.HIERARCHY_CASE, gc.CASES[4]], ids=vc.case_id)
def test_multigrid_hierarchy_with_galerkin_operators(case):
    """levels.multigrid_hierarchy(coarse_operators="galerkin"): the coarse matrices read back are the yardstick's, three V-cycles lie
    within vcycle_cases.CYCLE_TOL + 10 cond_2(A_0) 2.2e-16 of vcycle_ref on the matrices read back with the device's smoother bounds, CG
    takes the restatement's number of iterations and meets spsolve at 1e-9; float32 smoothers take the same number +- 1."""
    pa = _pa()
    from polydeal_amd.levels import multigrid_hierarchy

    mirror, _ = vc.handlers(*case)
    vc.check_shape(case, mirror)
    fe = pa.FE_DGQ(case[0], case[3])
    var, n = _variant(fe), fe.n_dofs_per_cell
    Ps = vc.injections(case)
    N = mirror[-1].n_dofs
    b = vc.rhs(N)
    dev = _Device()
    hier = multigrid_hierarchy(mirror, fe, var, diag_first=True, degree=vc.DEGREE, coarse_operators="galerkin")
    try:
        mats = [_global_matrix(c, ah.flatten(var, True, True).arrays(), ah.n_dofs) for c, ah in zip(hier.contexts, mirror)]
        for l in range(len(Ps)):
            # (entry by entry: the parity tests; here, that every level holds the product of the level above - the oracle's injection and
            # the transfer's differ by a few ulp, so against the largest sum of absolute products)
            ref = gr.product(Ps[l], mats[l + 1])
            assert np.max(np.abs(mats[l].toarray() - ref)) <= 10 * gr.TOL * np.max(gr.abs_product(Ps[l], mats[l + 1]))
        assert hier.info[0]["n_rows"] == mirror[0].n_dofs and [i["degree"] for i in hier.info[1:]] == [vc.DEGREE] * (len(mirror) - 1)
        bounds = [(i.get("lambda_lo"), i.get("lambda_hi")) for i in hier.info]
        H = vr.Hierarchy(mats, n, Ps, bounds, vc.DEGREE, vc.inner_kind(n))
        tol = vc.CYCLE_TOL + 10.0 * float(np.linalg.cond(mats[0].toarray())) * EPS
        d_b, d_x = dev.put(b), dev.put(np.full(N, np.nan))
        x_ref = None
        for cyc in range(3):
            hier.vcycle_device(d_b, d_x, zero_initial_guess=(cyc == 0))
            hier.finest.synchronize()
            x_ref = vr.cycle(H, b, x_ref)
            err = _rel(dev.get(d_x, N), x_ref)
            print("%s: Galerkin hierarchy, cycle %d: %.3e (bound %.3e)" % (vc.case_id(case), cyc + 1, err, tol))
            assert err <= tol
        x, cg = hier.solve_cg(b)
        x_sp = spla.spsolve(mats[-1].tocsc(), b)
        _, it_ref, _ = pcg_ref.pcg(mats[-1], b, vr.preconditioner(H), rel_tol=1e-13)
        print("%s: Galerkin hierarchy: CG iterations %d (restatement %d)" % (vc.case_id(case), cg["iterations"], it_ref))
        assert np.max(np.abs(x - x_sp)) <= 1e-9 * np.max(np.abs(x_sp))
        assert cg["iterations"] == it_ref
    finally:
        hier.close()
        dev.free()
    h32 = multigrid_hierarchy(mirror, fe, var, diag_first=True, degree=vc.DEGREE, coarse_operators="galerkin", smoother_precision="f32")
    try:
        assert [c.smoother_precision for c in h32.contexts] == ["f64"] + ["f32"] * (len(mirror) - 1)
        x32, cg32 = h32.solve_cg(b)
        print("%s: Galerkin hierarchy, float32 smoothers: CG iterations %d" % (vc.case_id(case), cg32["iterations"]))
        assert abs(cg32["iterations"] - cg["iterations"]) <= 1
        assert np.max(np.abs(x32 - x_sp)) <= 1e-9 * np.max(np.abs(x_sp))
    finally:
        h32.close()


def test_assembled_operators_are_the_default_bit_for_bit():
    pa = _pa()
    from polydeal_amd.levels import multigrid_hierarchy

    case = vc.HIERARCHY_CASE
    mirror, _ = vc.handlers(*case)
    fe = pa.FE_DGQ(case[0], case[3])
    b = vc.rhs(mirror[-1].n_dofs)
    got = []
    for kw in ({}, {"coarse_operators": "assembled"}):
        hier = multigrid_hierarchy(mirror, fe, _variant(fe), degree=vc.DEGREE, **kw)
        try:
            x, cg = hier.solve_cg(b)
            got.append((x, cg, [c.values() for c in hier.contexts]))
        finally:
            hier.close()
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1]
    assert all(np.array_equal(u, v) for u, v in zip(got[0][2], got[1][2]))
    with pytest.raises(ValueError):
        multigrid_hierarchy(mirror, fe, _variant(fe), coarse_operators="petrov")
