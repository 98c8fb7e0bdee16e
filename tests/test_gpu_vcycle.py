"""The dense direct solve (csrc/pdh_dense.hip, pdh_setup_direct) and the multigrid V-cycle (csrc/pdh_capi_mg.cpp) on the device: the explicit
inverse against the long-double inverse of the matrix read back, the cycle and V-cycle-preconditioned CG against their NumPy restatement
(tests/vcycle_ref.py) on the matrices read back with the device's own smoother bounds, reproducibility, the state and argument errors,
and levels.multigrid_hierarchy end to end.  Hierarchies, sizes and bounds: tests/vcycle_cases.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import pcg_ref
import vcycle_cases as vc
import vcycle_ref as vr
from exchange_cases import block_pattern, coupled_polytopes, row_map
from test_gpu_solve import _Device, _global_matrix

pytestmark = pytest.mark.gpu

EPS = 2.2e-16


def _pa():
    import polydeal_amd as pa
    return pa


def _variant(fe):
    return _pa().SipVariant.poisson_example(fe)


# ---------------------------------------------------------------------------------------------------------------------------------
# direct solve
# ---------------------------------------------------------------------------------------------------------------------------------
def _resident(ctx, ah, fe, diag_first):
    """the level assembled on the device and read back: scipy CSR"""
    flat = ah.flatten(_variant(fe), diag_first, True)
    ctx.set_problem(flat)
    ctx.assemble()
    return _global_matrix(ctx, flat.arrays(), ah.n_dofs)


def _columns_of_G(ctx, dev, N, cols):
    """G[:, cols] through one pdh_precondition_device per unit vector"""
    E = np.zeros((len(cols), N))
    E[np.arange(len(cols)), cols] = 1.0
    d_e, d_z = dev.put(E), dev.put(np.full((len(cols), N), np.nan))
    for k in range(len(cols)):
        ctx.precondition_device(d_e + 8 * N * k, d_z + 8 * N * k)
    ctx.synchronize()
    return dev.get(d_z, len(cols) * N).reshape(len(cols), N).T


def _check_direct(ctx, dev, A, N):
    info = ctx.setup_direct()
    assert info["n_rows"] == N and 0.0 < info["pivot_min"] <= info["pivot_max"] < np.inf, info
    cols = vc.direct_columns(N)
    G = _columns_of_G(ctx, dev, N, cols)
    ref = vr.inverse_longdouble(A.toarray(), cols)
    scale = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(G.astype(np.longdouble) - ref))) / scale
    print("%d rows: max|G - G_longdouble| / max|G| = %.3e (bound %.3e), pivots %.3e .. %.3e" %
          (N, err, vc.INVERSE_TOL[N], info["pivot_min"], info["pivot_max"]))
    sub = G[cols, :]
    assert np.array_equal(sub, sub.T), "G is not exactly symmetric"
    assert err <= vc.INVERSE_TOL[N], (N, err)
    # repeats, and the in-place call, give the bits of the out-of-place call
    r = vc.rhs(N)
    d_r, d_z, d_w = dev.put(r), dev.put(np.full(N, np.nan)), dev.put(r)
    ctx.precondition_device(d_r, d_z)
    ctx.synchronize()
    z = dev.get(d_z, N)
    ctx.precondition_device(d_r, d_z)
    ctx.precondition_device(d_w, d_w)
    ctx.synchronize()
    assert np.array_equal(dev.get(d_z, N), z) and np.array_equal(dev.get(d_w, N), z)
    assert np.array_equal(dev.get(d_r, N), r)
    # CG preconditioned with the inverse
    x, cg = ctx.solve_cg(r)
    x_ref = spla.spsolve(A.tocsc(), r)
    print("%d rows: CG with PDH_PREC_DIRECT: %d iterations" % (N, cg["iterations"]))
    assert cg["iterations"] <= 2
    assert np.max(np.abs(x - x_ref)) <= 1e-9 * np.max(np.abs(x_ref))
    x2, cg2 = ctx.solve_cg(r)
    assert np.array_equal(x2, x) and cg2 == cg
    return info


# every size in the deal.II layout; the ascending one at 125 rows (one polytope, rows of two pieces) and 576 rows (many polytopes)
DIRECT_PARAMS = [(s, True) for s in vc.DIRECT_SIZES] + [(vc.DIRECT_SIZES[2], False), (vc.DIRECT_SIZES[3], False)]


@pytest.mark.parametrize("size,diag_first", DIRECT_PARAMS, ids=lambda v: vc.size_id(v) if isinstance(v, tuple) else ("dealii" if v else "ascending"))
def test_direct_solve_against_the_long_double_inverse(size, diag_first):
    pa = _pa()
    ah, fe = vc.direct_handler(size)
    ctx, dev = pa.Context(0), _Device()
    try:
        A = _resident(ctx, ah, fe, diag_first)
        _check_direct(ctx, dev, A, size[1])
        # stale values
        ctx.assemble_device()
        d = dev.put(np.zeros(size[1]))
        with pytest.raises(pa.PdhError) as e:
            ctx.precondition_device(d, d)
        assert e.value.code == pa._capi.PDH_ESTATE and "values changed" in str(e.value)
        with pytest.raises(pa.PdhError) as e:
            ctx.solve_cg(np.ones(size[1]))
        assert e.value.code == pa._capi.PDH_ESTATE
    finally:
        ctx.close()
        dev.free()


def _permuted_problem(ah, fe):
    """the problem of a handler with the polytopes' dof ranges shuffled (fixed seed): dof_offset permuted, rowptr and colind rebuilt in the
    new row order, ascending layout"""
    pa = _pa()
    flat = ah.flatten(_variant(fe), False, True)
    kw = {k: (None if v is None else np.array(v)) for k, v in flat.arrays().items()}
    c = flat.c
    n, n_agg = fe.n_dofs_per_cell, c.n_agg
    off = kw["dof_offset"].astype(np.int64)
    new_off = n * np.random.default_rng(5).permutation(n_agg)
    assert np.any(new_off != off)
    new_rp, new_ci = block_pattern(coupled_polytopes(off, kw["rowptr"], kw["colind"], n), new_off, n, False)
    kw.update(dof_offset=new_off.astype(np.int32), rowptr=new_rp, colind=new_ci)
    kw.update(dim=c.dim, degree=c.degree, basis=c.basis, n_agg=c.n_agg, n_faces=c.n_faces, n_rows=c.n_rows, diag_first=0,
              reaction_c=c.reaction_c)
    prob = pa.Problem(**kw)
    prob.check()
    return prob, row_map(off, new_off, n)


def test_direct_solve_with_permuted_dof_offsets():
    """8 x 8 polytopes of 9 dofs whose dof ranges are shuffled: the gather honours dof_offset - the inverse of the matrix read back, and
    the matrix itself is the unpermuted one's rows and columns moved"""
    pa = _pa()
    size = vc.DIRECT_SIZES[3]
    ah, fe = vc.direct_handler(size)
    N = size[1]
    prob, m = _permuted_problem(ah, fe)
    ctx, dev = pa.Context(0), _Device()
    try:
        A0 = _resident(ctx, ah, fe, False)
        ctx.set_problem(prob)
        ctx.assemble()
        A = _global_matrix(ctx, prob.arrays, N)
        assert np.max(np.abs(A.toarray()[np.ix_(m, m)] - A0.toarray())) <= 1e-13 * np.max(np.abs(A0.toarray()))
        _check_direct(ctx, dev, A, N)
    finally:
        ctx.close()
        dev.free()


def test_direct_solve_refusals():
    pa = _pa()
    E = pa._capi
    ah, fe = vc.direct_handler(vc.DIRECT_REFUSED)
    ctx, dev = pa.Context(0), _Device()
    try:
        assert ctx.lib.pdh_setup_direct(ctx.h, None) == E.PDH_ESTATE  # no resident problem
        assert ctx.lib.pdh_setup_direct(None, None) == E.PDH_EINVAL
        _resident(ctx, ah, fe, True)
        with pytest.raises(pa.PdhError) as e:
            ctx.setup_direct()
        assert e.value.code == E.PDH_EUNSUPPORTED and "1600 rows" in str(e.value) and "1024" in str(e.value)
        # ... and the context then serves a smaller problem
        small = vc.DIRECT_SIZES[0]
        ah2, fe2 = vc.direct_handler(small)
        A = _resident(ctx, ah2, fe2, True)
        _check_direct(ctx, dev, A, small[1])
        # pdh_setup_preconditioner does not take the kind
        with pytest.raises(pa.PdhError) as e:
            ctx.setup_preconditioner(E.PDH_PREC_DIRECT)
        assert e.value.code == E.PDH_EINVAL
        # a row-range context and a ghost context: 8 x 8 polytopes of 9 dofs cut in two
        from polydeal_amd.partition import row_range

        ah3, fe3 = vc.direct_handler(vc.DIRECT_SIZES[3])
        var, N3 = _variant(fe3), ah3.n_dofs
        splits = [row_range(ah3.n_agglomerates, fe3.n_dofs_per_cell, r, 2)[0] for r in range(2)] + [N3]
        ctx.set_problem(ah3.flatten(var, True, True), 0, splits[1])
        ctx.assemble()
        with pytest.raises(pa.PdhError) as e:
            ctx.setup_direct()
        assert e.value.code == E.PDH_EUNSUPPORTED and "all rows" in str(e.value)
        ctx.set_exchange_mode("ghost")
        ctx.set_problem(ah3.flatten_local(var, 0, splits[1], True, True, row_splits=splits), 0, splits[1])
        ctx.assemble()
        with pytest.raises(pa.PdhError) as e:
            ctx.setup_direct()
        assert e.value.code == E.PDH_EUNSUPPORTED and "EXCHANGE_GHOST" in str(e.value)
    finally:
        ctx.close()
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# V-cycle
# ---------------------------------------------------------------------------------------------------------------------------------
class _Levels:
    """One context per level of a case (coarse to fine), assembled on the device (ascending layout) and read back; Chebyshev(degree)
    on every level above the coarsest, the direct solve (or Chebyshev) on the coarsest; the transfers.  No Multigrid yet: attach()."""

    def __init__(self, case, degree=vc.DEGREE, coarse="direct", diag_first=False):
        pa = _pa()
        from polydeal_amd.levels import level_transfer

        self.case, self.degree = case, degree
        self.mirror, _ = vc.handlers(*case)
        vc.check_shape(case, self.mirror)
        fe = pa.FE_DGQ(case[0], case[3])
        self.n = fe.n_dofs_per_cell
        self.kind = vc.inner_kind(self.n)
        self.ctxs, self.transfers, self.mats, self.infos, self.mg = [], [], [], [], None
        try:
            for l, ah in enumerate(self.mirror):
                ctx = pa.Context(0)
                self.ctxs.append(ctx)
                self.mats.append(_resident(ctx, ah, fe, diag_first))
                if l == 0 and coarse == "direct":
                    self.infos.append(ctx.setup_direct())
                else:
                    self.infos.append(ctx.setup_chebyshev(self.kind, degree=degree))
                if l > 0:
                    self.transfers.append(level_transfer(ctx, self.mirror[l - 1], ah))
        except Exception:
            self.close()
            raise
        bounds = [(i.get("lambda_lo"), i.get("lambda_hi")) for i in self.infos]
        self.H = vr.Hierarchy(self.mats, self.n, vc.injections(case), bounds, degree, self.kind, coarse)
        self.N = self.mats[-1].shape[0]
        self.finest = self.ctxs[-1]
        self.tol = vc.CYCLE_TOL + 10.0 * float(np.linalg.cond(self.mats[0].toarray())) * EPS

    def attach(self):
        from polydeal_amd._capi import Multigrid

        self.mg = Multigrid(self.ctxs, self.transfers)
        return self.mg

    def close(self):
        if self.mg is not None:
            self.mg.close()
        for t in self.transfers:
            t.close()
        for c in self.ctxs:
            c.close()


def _rel(x, ref):
    return float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("case", vc.CASES, ids=vc.case_id)
def test_vcycle_and_cg_against_the_numpy_restatement(case):
    """One cycle from zero through pdh_precondition_device and through pdh_mg_vcycle_device, a cycle from a non-zero x, three consecutive
    cycles, all within the case bound + 10 cond_2(A_0) 2.2e-16 of vcycle_ref on the matrices read back, relative to |x|_inf; the same
    bits twice.  Then CG on the finest context: against spsolve (1e-9), iterations within one of pcg_ref's with vcycle_ref and strictly
    fewer than the device's own Chebyshev(3) CG on the same matrix; two runs give the same bits."""
    L = _Levels(case)
    dev = _Device()
    try:
        N, H, A = L.N, L.H, L.mats[-1]
        b = vc.rhs(N)
        _, cheb_cg = L.finest.solve_cg(b)  # Chebyshev(3) is the finest context's preconditioner until the mg is attached
        mg = L.attach()
        d_b, d_z, d_x = dev.put(b), dev.put(np.full(N, np.nan)), dev.put(np.full(N, np.nan))
        ref1 = vr.cycle(H, b)
        L.finest.precondition_device(d_b, d_z)
        L.finest.synchronize()
        z = dev.get(d_z, N)
        print("%s: precondition_device: %.3e (bound %.3e)" % (vc.case_id(case), _rel(z, ref1), L.tol))
        assert _rel(z, ref1) <= L.tol
        # in place
        d_w = dev.put(b)
        L.finest.precondition_device(d_w, d_w)
        L.finest.synchronize()
        assert np.array_equal(dev.get(d_w, N), z)
        # three consecutive cycles on x; the first from zero gives the bits of precondition_device
        x_ref = None
        for cyc in range(3):
            mg.vcycle_device(d_b, d_x, zero_initial_guess=(cyc == 0))
            L.finest.synchronize()
            x = dev.get(d_x, N)
            x_ref = vr.cycle(H, b, x_ref)
            print("%s: cycle %d: %.3e" % (vc.case_id(case), cyc + 1, _rel(x, x_ref)))
            assert _rel(x, x_ref) <= L.tol, (cyc, _rel(x, x_ref), L.tol)
            if cyc == 0:
                assert np.array_equal(x, z)
        # from a non-zero x, twice
        x0 = np.random.default_rng(7).standard_normal(N)
        ref = vr.cycle(H, b, x0)
        got = []
        for _ in range(2):
            d_y = dev.put(x0)
            mg.vcycle_device(d_b, d_y, zero_initial_guess=False)
            L.finest.synchronize()
            got.append(dev.get(d_y, N))
        assert np.array_equal(got[0], got[1])
        assert _rel(got[0], ref) <= L.tol, (_rel(got[0], ref), L.tol)
        assert np.array_equal(dev.get(d_b, N), b)
        # CG
        x, cg = L.finest.solve_cg(b)
        x_sp = spla.spsolve(A.tocsc(), b)
        assert np.max(np.abs(x - x_sp)) <= 1e-9 * np.max(np.abs(x_sp))
        _, it_ref, _ = pcg_ref.pcg(A, b, vr.preconditioner(H), rel_tol=1e-13)
        print("%s: CG iterations: V-cycle %d (restatement %d), Chebyshev(%d) %d" % (vc.case_id(case), cg["iterations"], it_ref, L.degree,
                                                                                 cheb_cg["iterations"]))
        assert abs(cg["iterations"] - it_ref) <= 1
        assert cg["iterations"] < cheb_cg["iterations"]
        x2, cg2 = L.finest.solve_cg(b)
        assert np.array_equal(x2, x) and cg2 == cg
    finally:
        L.close()
        dev.free()


def test_vcycle_with_a_chebyshev_coarsest_level():
    L = _Levels(vc.CASES[0], coarse="chebyshev")
    dev = _Device()
    try:
        assert L.infos[0]["degree"] == vc.DEGREE
        L.attach()
        b = vc.rhs(L.N)
        d_b, d_z = dev.put(b), dev.put(np.full(L.N, np.nan))
        L.finest.precondition_device(d_b, d_z)
        L.finest.synchronize()
        z, ref = dev.get(d_z, L.N), vr.cycle(L.H, b)
        print("Chebyshev coarsest level: %.3e (bound %.3e)" % (_rel(z, ref), vc.CYCLE_TOL))
        assert _rel(z, ref) <= vc.CYCLE_TOL  # (no coarse inverse: the case bound alone)
        assert _rel(z, vr.cycle(_Levels_direct_reference(L), b)) > 1e-6  # ... and it is not the direct coarse solve
    finally:
        L.close()
        dev.free()


def _Levels_direct_reference(L):
    return vr.Hierarchy(L.mats, L.n, L.H.Ps, L.H.bounds, L.degree, L.kind, "direct")


def test_vcycle_on_a_callers_stream():
    """pdh_set_stream on the finest context: every level's launches follow it (the other contexts keep their own streams, idle)"""
    L = _Levels(vc.CASES[2])
    dev = _Device()
    hip = dev.hip
    stream = C.c_void_p()
    try:
        mg = L.attach()
        b = vc.rhs(L.N)
        d_b, d_x = dev.put(b), dev.put(np.full(L.N, np.nan))
        mg.vcycle_device(d_b, d_x, True)
        L.finest.synchronize()
        x_own = dev.get(d_x, L.N)
        hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        hip.hipStreamDestroy.argtypes = [C.c_void_p]
        assert hip.hipStreamCreate(C.byref(stream)) == 0
        L.finest.set_stream(stream.value)
        assert L.finest.lib.pdh_stream(L.finest.h) == stream.value
        d_y = dev.put(np.full(L.N, np.nan))
        mg.vcycle_device(d_b, d_y, True)
        assert hip.hipStreamSynchronize(stream) == 0  # the caller's stream alone
        assert np.array_equal(dev.get(d_y, L.N), x_own)
        x, cg = L.finest.solve_cg(b)
        L.finest.set_stream(None)
        x2, cg2 = L.finest.solve_cg(b)
        assert np.array_equal(x, x2) and cg == cg2
    finally:
        L.close()
        if stream.value:
            hip.hipStreamDestroy(stream)
        dev.free()


def test_state_and_argument_errors():
    pa = _pa()
    E = pa._capi
    from polydeal_amd._capi import Multigrid
    from polydeal_amd.levels import level_transfer

    L = _Levels(vc.CASES[0])  # 16 / 64 / 256
    dev = _Device()
    extra = []
    try:
        c0, c1, c2 = L.ctxs
        t01, t12 = L.transfers
        lib = c2.lib

        def refused(levels, transfers, code, *fragments):
            with pytest.raises(pa.PdhError) as e:
                Multigrid(levels, transfers).close()
            assert e.value.code == code, str(e.value)
            for f in fragments:
                assert f in str(e.value), (f, str(e.value))
        # level counts
        refused([c2], [], E.PDH_EINVAL, "1 levels")
        h = C.c_void_p()
        lv = (C.c_void_p * 17)(*([c0.h.value, c1.h.value] + [c2.h.value] * 15))
        tr = (C.c_void_p * 16)(*([t01.h.value] * 16))
        assert lib.pdh_mg_create(17, lv, tr, C.byref(h)) == E.PDH_EINVAL and not h.value
        assert "17 levels" in lib.pdh_last_error(c2.h).decode()
        assert lib.pdh_mg_create(3, None, tr, C.byref(h)) == E.PDH_EINVAL
        assert lib.pdh_mg_create(3, lv, tr, None) == E.PDH_EINVAL
        # a level without Chebyshev: the middle one with block Jacobi, the coarsest with nothing
        c1.setup_preconditioner("block_jacobi")
        refused(L.ctxs, L.transfers, E.PDH_ESTATE, "level 1 of 3", "PDH_PREC_CHEBYSHEV")
        c1.setup_chebyshev(L.kind, degree=L.degree)
        c0.setup_preconditioner("none")
        refused(L.ctxs, L.transfers, E.PDH_ESTATE, "level 0 of 3", "coarsest")
        c0.setup_direct()
        # stale values on a level at create
        c1.assemble_device()
        refused(L.ctxs, L.transfers, E.PDH_ESTATE, "level 1 of 3", "not current")
        c1.setup_chebyshev(L.kind, degree=L.degree)
        # a transfer on the wrong context, of the wrong size, missing
        t_wrong = level_transfer(c1, L.mirror[1], L.mirror[2])  # the fine pair's, created on the middle context
        extra.append(t_wrong)
        refused(L.ctxs, [t01, t_wrong], E.PDH_EINVAL, "transfer 1", "finer level")
        t_size = level_transfer(c2, L.mirror[0], L.mirror[2])  # level 0 <-> 2, on the finest context
        extra.append(t_size)
        refused(L.ctxs, [t01, t_size], E.PDH_EINVAL, "transfer 1", "rows")
        tr3 = (C.c_void_p * 2)(t01.h.value, None)
        lv3 = (C.c_void_p * 3)(c0.h.value, c1.h.value, c2.h.value)
        assert lib.pdh_mg_create(3, lv3, tr3, C.byref(h)) == E.PDH_EINVAL and "transfer 1" in lib.pdh_last_error(c2.h).decode()
        # the same context twice
        refused([c0, c2, c2], L.transfers, E.PDH_EINVAL, "level 2 of 3", "too")
        # a good one; NULL and overlapping vectors
        mg = L.attach()
        N = L.N
        d_b, d_x = dev.put(vc.rhs(N)), dev.put(np.zeros(N))
        assert lib.pdh_mg_vcycle_device(None, C.c_void_p(d_b), C.c_void_p(d_x), 1) == E.PDH_EINVAL
        assert lib.pdh_mg_vcycle_device(mg.h, None, C.c_void_p(d_x), 1) == E.PDH_EINVAL
        assert lib.pdh_mg_vcycle_device(mg.h, C.c_void_p(d_b), C.c_void_p(d_b + 8 * (N - 1)), 1) == E.PDH_EINVAL
        assert "overlap" in lib.pdh_last_error(c2.h).decode()
        mg.vcycle_device(d_b, d_x, True)
        c2.synchronize()
        # values changed on the middle level: every mg entry and CG on the finest context say which
        c1.assemble_device()
        for call in (lambda: mg.vcycle_device(d_b, d_x, True), lambda: c2.precondition_device(d_b, d_x), lambda: c2.solve_cg(np.ones(N))):
            with pytest.raises(pa.PdhError) as e:
                call()
            assert e.value.code == E.PDH_ESTATE and "values of level 1 of 3" in str(e.value), str(e.value)
        # the smoother of the middle level set up again (same values): a change too; a new mg serves
        c1.setup_chebyshev(L.kind, degree=L.degree)
        with pytest.raises(pa.PdhError) as e:
            mg.vcycle_device(d_b, d_x, True)
        assert e.value.code == E.PDH_ESTATE and "level 1 of 3" in str(e.value)
        mg.close()
        L.mg = None
        # the mg destroyed, then CG asked: the context fell back to PDH_PREC_NONE and says so
        with pytest.raises(pa.PdhError) as e:
            c2.solve_cg(np.ones(N))
        assert e.value.code == E.PDH_ESTATE and "destroyed" in str(e.value) and "PDH_PREC_NONE" in str(e.value)
        with pytest.raises(pa.PdhError) as e:
            c2.precondition_device(d_b, d_x)
        assert e.value.code == E.PDH_ESTATE and "destroyed" in str(e.value)
        c2.setup_chebyshev(L.kind, degree=L.degree)
        mg = L.attach()
        mg.vcycle_device(d_b, d_x, True)
        # the preconditioner replaced on the finest context: the mg is detached, the context uses the new one
        c2.setup_preconditioner("block_jacobi")
        with pytest.raises(pa.PdhError) as e:
            mg.vcycle_device(d_b, d_x, True)
        assert e.value.code == E.PDH_ESTATE and "detached" in str(e.value) and "level 2 of 3" in str(e.value)
        x, cg = c2.solve_cg(vc.rhs(N))
        assert cg["iterations"] > 30  # (block Jacobi, not the cycle)
    finally:
        for t in extra:
            t.close()
        L.close()
        dev.free()


def test_mixed_devices_are_refused():
    hip, count = C.CDLL("libamdhip64.so"), C.c_int(0)
    if hip.hipGetDeviceCount(C.byref(count)) != 0 or count.value < 2:
        pytest.skip("one device: two contexts cannot differ in theirs")
    pa = _pa()
    from polydeal_amd._capi import Multigrid
    from polydeal_amd.levels import level_transfer

    case = vc.CASES[0]
    mirror, _ = vc.handlers(*case)
    fe = pa.FE_DGQ(case[0], case[3])
    ctxs, ts = [pa.Context(1), pa.Context(0), pa.Context(0)], []
    try:
        for l, (ctx, ah) in enumerate(zip(ctxs, mirror)):
            _resident(ctx, ah, fe, False)
            ctx.setup_direct() if l == 0 else ctx.setup_chebyshev("block_jacobi", degree=3)
            if l:
                ts.append(level_transfer(ctx, mirror[l - 1], ah))
        with pytest.raises(pa.PdhError) as e:
            Multigrid(ctxs, ts)
        assert e.value.code == pa._capi.PDH_EINVAL and "level 0 of 3" in str(e.value) and "device" in str(e.value)
    finally:
        for t in ts:
            t.close()
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# levels.multigrid_hierarchy
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diag_first", [True, False], ids=["dealii", "ascending"])
def test_multigrid_hierarchy_end_to_end(diag_first):
    pa = _pa()
    from polydeal_amd.levels import multigrid_hierarchy

    case = vc.HIERARCHY_CASE
    mirror, _ = vc.handlers(*case)
    assert vc.check_shape(case, mirror) == (27, 216, 1728)
    fe = pa.FE_DGQ(case[0], case[3])
    hier = multigrid_hierarchy(mirror, fe, _variant(fe), diag_first=diag_first, degree=vc.DEGREE)
    try:
        assert hier.info[0]["n_rows"] == 27 and [i["degree"] for i in hier.info[1:]] == [vc.DEGREE] * 2
        N = mirror[-1].n_dofs
        A = _global_matrix(hier.finest, mirror[-1].flatten(_variant(fe), diag_first, True).arrays(), N)
        b = vc.rhs(N)
        x, cg = hier.solve_cg(b)
        x_sp = spla.spsolve(A.tocsc(), b)
        print("multigrid_hierarchy (diag_first=%d): %d iterations" % (diag_first, cg["iterations"]))
        assert np.max(np.abs(x - x_sp)) <= 1e-9 * np.max(np.abs(x_sp))
        hier.finest.setup_preconditioner("block_jacobi")  # detaches the mg
        _, bj = hier.finest.solve_cg(b)
        assert cg["iterations"] < bj["iterations"]
    finally:
        hier.close()
