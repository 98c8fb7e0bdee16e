"""What the driver units (csrc/pdh_capi*.cpp over pdh_ctx.h) owe each other: the answers before a problem is set, that nothing of a
dropped problem survives a failed pdh_set_problem, and that the context's shared device buffers do not cross between entry points.
Every failure here is an argument or state error answered on the host."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _pa():
    import polydeal_amd as pa
    return pa


def _handler():
    """2-D, 4 x 4 cells in blocks of 2, FE_DGQ(1): four polytopes of four dofs"""
    pa = _pa()
    ah = pa.AgglomerationHandler(pa.BackgroundGrid.hyper_cube_refined(2, 0.0, 1.0, 2))
    ah.define_block_agglomerates(2)
    fe = pa.FE_DGQ(2, 1)
    ah.initialize_fe_values(2, 2)
    ah.distribute_agglomerated_dofs(fe)
    return ah, fe


def _called_before(name):
    return name + " called before pdh_set_problem"


_NONE = "no problem resident"
_NO_GHOST = "no problem resident in PDH_EXCHANGE_GHOST mode"
# the text each entry point that needs a problem gives before pdh_set_problem (transcribed from the driver's source before it was split
# into units: the *_device variants name their host-pointer sibling, some entry points answer a NULL context in the same words)
NO_PROBLEM_ANSWERS = {
    "pdh_terms_merge_stats": _called_before("pdh_terms_merge_stats"),
    "pdh_algorithm_in_use": _NONE, "pdh_rows_kernel_in_use": _NONE,
    "pdh_assemble_device": _called_before("pdh_assemble_device"), "pdh_assemble": _called_before("pdh_assemble_device"),
    "pdh_exchange_layout": _NONE, "pdh_exchange_get_send": _NO_GHOST, "pdh_exchange_apply": _NO_GHOST,
    "pdh_debug_rows_stamps": "no row-kernel problem resident",
    "pdh_copy_values": _NONE, "pdh_values_checksum": _NONE, "pdh_device_values": _NONE, "pdh_kernel_work": _NONE,
    "pdh_problem_stats": _NONE,
    "pdh_assemble_rhs": _called_before("pdh_assemble_rhs"), "pdh_assemble_rhs_device": _called_before("pdh_assemble_rhs"),
    "pdh_evaluate": _called_before("pdh_evaluate"), "pdh_evaluate_device": _called_before("pdh_evaluate"),
    "pdh_global_error": _called_before("pdh_global_error"), "pdh_global_error_device": _called_before("pdh_global_error"),
    "pdh_vmult": _called_before("pdh_vmult"), "pdh_vmult_device": _called_before("pdh_vmult"),
    "pdh_setup_preconditioner": _called_before("pdh_setup_preconditioner"),
    "pdh_precondition_device": _called_before("pdh_precondition_device"),
    "pdh_solve_cg": _called_before("pdh_solve_cg"), "pdh_solve_cg_device": _called_before("pdh_solve_cg"),
    "pdh_setup_chebyshev": _called_before("pdh_setup_chebyshev"),
    "pdh_chebyshev_step_device": _called_before("pdh_chebyshev_step_device"),
}


def _call(ctx, name, room):
    """the entry point on the context with every pointer valid (host memory: a state error comes before any of it is read)"""
    fn = getattr(ctx.lib, name)
    args = [ctx.h]
    for t in fn.argtypes[1:]:
        if t is C.c_void_p:
            args.append(C.addressof(room))
        elif hasattr(t, "contents"):
            args.append(C.cast(room, t))
        else:
            args.append(0)
    rc = fn(*args)
    return rc, ctx.lib.pdh_last_error(ctx.h).decode()


def _state_error(ctx, fn, *args):
    from polydeal_amd import _capi
    rc = fn(ctx.h, *args)
    assert rc == _capi.PDH_ESTATE, (fn.__name__, rc, ctx.lib.pdh_last_error(ctx.h))


def test_driver_contract():
    pa = _pa()
    from polydeal_amd import _capi
    ah, fe = _handler()
    var = pa.SipVariant.poisson_example(fe)
    flat = ah.flatten(var, True, True)
    arr = flat.arrays()
    N, nA = ah.n_dofs, ah.n_agglomerates
    assert (N, nA) == (16, 4)
    rng = np.random.default_rng(7)
    f_vol, g_bdry = rng.standard_normal(int(arr["vq_ptr"][-1])), rng.standard_normal(int(arr["fq_ptr"][-1]))
    x, b = rng.standard_normal(N), rng.standard_normal(N)

    def products(c):
        return c.assemble(), c.assemble_rhs(f_vol, g_bdry), c.vmult(x)

    fresh = pa.Context(0)
    ctx = pa.Context(0)
    try:
        fresh.set_problem(flat)
        want = products(fresh)
        want_sum = fresh.checksum()

        # (a) before any problem
        ctx.lib.pdh_debug_rows_stamps.argtypes = [C.c_void_p, C.c_void_p]
        room = (C.c_double * 64)()
        for name, text in sorted(NO_PROBLEM_ANSWERS.items()):
            assert _call(ctx, name, room) == (_capi.PDH_ESTATE, text), name

        # (b) a failed pdh_set_problem leaves nothing of the problem before it
        splits = [0, N // 2, N]
        loc = ah.flatten_local(var, 0, splits[1], True, True, row_splits=splits)
        ctx.set_exchange_mode("ghost")
        ctx.set_problem(loc, 0, splits[1])
        ctx.assemble()
        assert sum(map(sum, ctx.exchange_layout(2))) > 0
        loc.c.n_rows += 1
        with pytest.raises(pa.PdhError) as e:
            ctx.set_problem(loc, 0, splits[1])
        loc.c.n_rows -= 1
        assert e.value.code == _capi.PDH_EINVAL
        cnt, y8, rhs8 = (C.c_int64 * 2)(), np.zeros(N // 2), np.zeros(N // 2)
        _state_error(ctx, ctx.lib.pdh_exchange_layout, 2, cnt, cnt)
        _state_error(ctx, ctx.lib.pdh_vmult, x.ctypes.data, y8.ctypes.data)
        _state_error(ctx, ctx.lib.pdh_assemble_rhs, None, None, rhs8.ctypes.data)
        ctx.set_exchange_mode("none")
        ctx.set_problem(flat)
        _state_error(ctx, ctx.lib.pdh_exchange_get_send, C.addressof(room))
        for got, ref in zip(products(ctx), want):
            assert np.array_equal(got, ref)

        # (c) the shared buffers: staging copies (solve, estimate, evaluate, shape values), the solver's vectors (CG, estimate,
        # Chebyshev chain), the checksum's own
        x_none, info_none = ctx.solve_cg(b)
        cheb = ctx.setup_chebyshev("jacobi", 3, 20.0, 8)
        assert cheb["cg_iterations"] >= 1
        bbox = np.asarray(arr["bbox"], dtype=np.float64).reshape(nA, 4)
        pts = np.ascontiguousarray(((bbox[:, :2] + bbox[:, 2:]) / 2).T)
        u = ctx.evaluate(x_none, np.arange(nA + 1), pts)
        assert np.all(np.isfinite(u))
        shape = ctx.shape_values(3, 2, _capi.PDH_BASIS_AGGLODGP, [0.0, 0.0, 0.0, 1.0, 2.0, 3.0], [0, 2], [[0.25, 0.5], [1.0, 0.5], [2.0, 1.5]])
        assert shape.shape == (2, 10) and np.all(np.isfinite(shape))
        assert ctx.checksum() == want_sum
        x_cheb, info_cheb = ctx.solve_cg(b)
        ctx.setup_preconditioner("none")
        x_again, info_again = ctx.solve_cg(b)
        assert np.array_equal(x_again, x_none) and info_again == info_none
        # ... and the Chebyshev-preconditioned solve equals that of a context that did nothing else
        assert fresh.setup_chebyshev("jacobi", 3, 20.0, 8) == cheb
        x_ref, info_ref = fresh.solve_cg(b)
        assert np.array_equal(x_cheb, x_ref) and info_cheb == info_ref
    finally:
        ctx.close()
        fresh.close()
