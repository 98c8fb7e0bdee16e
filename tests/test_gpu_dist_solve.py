"""Solving over several ranks (csrc/pdh_dist.hip, pdh_capi_dist.cpp, polydeal_amd/distributed.py) on the worlds of tests/halo_cases.py:
W contexts on device 0 play the ranks, the transport is the lock-step driver's device-to-device copies.

The wire format of the halo: with the global dof number in every owned entry, every entry of every send segment and of every ghost tail
is the dof tests/halo_cases.py::expected_halo puts there.  The product on local vectors against pdh_vmult_device, to the bit, whole and
in its interior and boundary halves.  CG by reverse communication with every rank-local preconditioner against the dense solve and
tests/pcg_ref.py under the bounds of tests/test_gpu_solve.py::test_cg_against_spsolve_and_the_host_loop; the request sequence; the
refusals and state errors; examples/diffusion_reaction --device-solve; two gloo processes through polydeal_amd.distributed.TorchRank."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import halo_cases as hc
from device_buffers import Device
from pcg_ref import pcg, preconditioner

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pa():
    import polydeal_amd as pa
    return pa


@pytest.fixture(autouse=True)
def _dist_abi():
    """every test here is about the entry points of solving over the ranks: a library without them fails them all at these calls"""
    pa = _pa()
    lib = pa.load_library()
    assert lib.pdh_halo_setup(None, 1, None, None, None, None) == pa._capi.PDH_EINVAL
    assert lib.pdh_dcg_resume(None, None, None) == pa._capi.PDH_EINVAL


class Ranks:
    """the contexts of a world with their halos set up"""

    def __init__(self, w, assemble=True):
        pa = _pa()
        self.w, self.part, self.W, self.n, self.dev = w, w.part, w.part.world, w.part.n, Device()
        self.exp = w.expected()
        self.ctxs, self.probs, self.lay = [], [], []
        try:
            for prob, (r0, r1) in self.part.problems():
                c = pa.Context(0)
                self.ctxs.append(c)
                self.probs.append(prob)
                c.set_problem(prob, r0, r1)
                if assemble:
                    c.assemble_device()
                self.lay.append(c.halo_setup(self.part.splits))
        except Exception:
            self.close()
            raise

    def close(self):
        for c in self.ctxs:
            c.close()
        self.dev.free()

    def local_vector(self, r, x):
        """rank r's local vector of the global vector x"""
        r0, r1 = self.part.rows(r)
        return np.concatenate([x[r0:r1], x[hc.ghost_dofs(self.exp, r)]])

    def interior_rows(self, r):
        """mask over rank r's rows: those of its interior polytopes"""
        r0, r1 = self.part.rows(r)
        mask = np.zeros(r1 - r0, dtype=bool)
        for P in self.exp["interior"][r]:
            mask[self.exp["off"][P] - r0:self.exp["off"][P] - r0 + self.n] = True
        return mask


# ---------------------------------------------------------------------------------------------------------------------------------
# the wire format
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hc.NAMES)
def test_wire_format(name):
    w = hc.world(name)
    R = Ranks(w, assemble=False)
    try:
        send_m = hc.send_matrix(R.exp)
        d_v, d_send, sends = [], [], []
        for r, c in enumerate(R.ctxs):
            r0, r1 = R.part.rows(r)
            sc, rc, info = R.lay[r]
            assert sc == send_m[r].tolist() and rc == send_m[:, r].tolist() and info["n_owned_rows"] == r1 - r0
            assert info["n_ghost_rows"] == sum(rc) and info["n_interior"] == len(R.exp["interior"][r])
            v = np.concatenate([np.arange(r0, r1, dtype=np.float64), np.full(sum(rc), np.nan)])
            d_v.append(R.dev.put(v))
            d_send.append(R.dev.fill(sum(sc), np.nan))
            c.halo_pack(d_v[r], d_send[r])
            c.synchronize()
            sends.append(R.dev.get(d_send[r], sum(sc)))
            assert np.array_equal(sends[r], hc.send_dofs(R.exp, r).astype(np.float64)), r
            assert np.array_equal(R.dev.get(d_v[r], len(v))[:r1 - r0], v[:r1 - r0])  # (the pack reads only)
        # the lock-step move: segment d of s's send buffer becomes segment s of d's tail
        for s in range(R.W):
            so = hc.xc.segment_offsets(R.lay[s][0])
            for d in range(R.W):
                ro = hc.xc.segment_offsets(R.lay[d][1])
                R.dev.write(d_v[d], sends[s][so[d]:so[d + 1]], offset=R.part.rows(d)[1] - R.part.rows(d)[0] + ro[s])
        for r in range(R.W):
            r0, r1 = R.part.rows(r)
            tail = R.dev.get(d_v[r], r1 - r0 + sum(R.lay[r][1]))[r1 - r0:]
            assert np.array_equal(tail, hc.ghost_dofs(R.exp, r).astype(np.float64)), r
    finally:
        R.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the product
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hc.NAMES)
def test_product_on_local_vectors(name):
    w = hc.world(name)
    A = w.dense().astype(np.longdouble)
    N = A.shape[0]
    x = np.random.default_rng(1).standard_normal(N)
    ref = A @ x.astype(np.longdouble)
    bound = 1e-13 * (np.abs(A) @ np.abs(x).astype(np.longdouble))
    R = Ranks(w)
    try:
        d_x = R.dev.put(x)
        ys = []
        for r, c in enumerate(R.ctxs):
            r0, r1 = R.part.rows(r)
            m, inner = r1 - r0, R.interior_rows(r)
            d_ref = R.dev.fill(m, np.nan)
            c.vmult_device(d_x, d_ref)
            c.synchronize()
            y_ref = R.dev.get(d_ref, m)
            v = R.local_vector(r, x)
            d_v, d_y = R.dev.put(v), R.dev.fill(m, np.nan)
            c.vmult_local(d_v, d_y, "all")
            c.synchronize()
            assert R.dev.get(d_y, m).tobytes() == y_ref.tobytes(), (r, "all")
            # interior alone: the boundary rows are not touched; then the boundary rows: the same bits
            R.dev.write(d_y, np.full(m, np.nan))
            c.vmult_local(d_v, d_y, "interior")
            c.synchronize()
            y = R.dev.get(d_y, m)
            assert np.all(np.isnan(y[~inner])) and y[inner].tobytes() == y_ref[inner].tobytes(), (r, "interior")
            c.vmult_local(d_v, d_y, "boundary")
            c.synchronize()
            assert R.dev.get(d_y, m).tobytes() == y_ref.tobytes(), (r, "interior, boundary")
            # boundary alone leaves the interior rows
            R.dev.write(d_y, np.full(m, np.nan))
            c.vmult_local(d_v, d_y, "boundary")
            c.synchronize()
            y = R.dev.get(d_y, m)
            assert np.all(np.isnan(y[inner])) and y[~inner].tobytes() == y_ref[~inner].tobytes(), (r, "boundary")
            # the interior rows need no ghost value: a NaN tail does not reach them
            v_nan = v.copy()
            v_nan[m:] = np.nan
            d_vn = R.dev.put(v_nan)
            R.dev.write(d_y, np.full(m, np.nan))
            c.vmult_local(d_vn, d_y, "interior")
            c.synchronize()
            y = R.dev.get(d_y, m)
            assert np.all(np.isfinite(y[inner])) and y[inner].tobytes() == y_ref[inner].tobytes(), (r, "NaN tail")
            ys.append(y_ref)
        err = np.abs(np.concatenate(ys).astype(np.longdouble) - ref)
        print("%s: worst |y - y_ref| / sum|a||x| = %.3e, interior polytopes %s" % (
            name, float(np.max(err / np.maximum(bound * 1e13, 1e-300))), [len(v) for v in R.exp["interior"]]))
        assert np.all(err <= bound), (int(np.sum(err > bound)), float(np.max(err / bound)))
    finally:
        R.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# conjugate gradients
# ---------------------------------------------------------------------------------------------------------------------------------
def _expected_trace(iterations):
    from polydeal_amd._capi import PDH_DCG_ALLREDUCE as AR, PDH_DCG_DONE as DONE, PDH_DCG_HALO_BEGIN as HB, PDH_DCG_HALO_END as HE
    return [(HB, 0), (HE, 0), (AR, 3)] + [(HB, 0), (HE, 0), (AR, 1), (AR, 2)] * iterations + [(DONE, 0)]


CG_RUNS = [(name, kind) for name in hc.CG_WORLDS for kind in hc.cg_kinds(name)]


@pytest.mark.parametrize("name,kind", CG_RUNS, ids=["%s-%s" % r for r in CG_RUNS])
def test_cg_over_the_ranks(name, kind):
    pa = _pa()
    from polydeal_amd.distributed import solve_cg_lockstep

    w = hc.world(name)
    A, b, n = w.dense(), hc.rhs(name), w.part.n
    ref = np.linalg.solve(A, b)
    _, it_ref, _ = pcg(A, b, preconditioner(sp.csr_matrix(A), n, kind))
    R = Ranks(w)
    try:
        splits = R.part.splits
        b_parts = [b[splits[r]:splits[r + 1]] for r in range(R.W)]
        for c in R.ctxs:
            c.setup_preconditioner(kind)
        trace = []
        x_parts, info = solve_cg_lockstep(R.ctxs, splits, b_parts, trace=trace)  # (the driver asserts that all ranks report the same info)
        x = np.concatenate(x_parts)
        print("%s %s: %d iterations (reference %d), residual %.3e, |x - x_ref| / |x_ref| = %.3e" % (
            name, kind, info["iterations"], it_ref, info["residual"], np.linalg.norm(x - ref) / np.linalg.norm(ref)))
        assert np.linalg.norm(x - ref) <= 1e-9 * np.linalg.norm(ref), info
        assert abs(info["iterations"] - it_ref) <= 1, (info, it_ref)
        assert info["residual"] <= 1e-13 * np.linalg.norm(b) and info["residual0"] == pytest.approx(np.linalg.norm(b), rel=1e-13)
        assert trace == _expected_trace(info["iterations"])
        # again: the same bits
        x2_parts, info2 = solve_cg_lockstep(R.ctxs, splits, b_parts)
        assert info2 == info and np.concatenate(x2_parts).tobytes() == x.tobytes()
        # max_iter: every rank answers PDH_ENOCONV with the same count
        with pytest.raises(pa.PdhError) as e:
            solve_cg_lockstep(R.ctxs, splits, b_parts, max_iter=3)
        assert e.value.code == pa._capi.PDH_ENOCONV and [i["iterations"] for i in e.value.infos] == [3] * R.W
        assert len({i["residual"] for i in e.value.infos}) == 1 and e.value.info["residual"] > 1e-13 * np.linalg.norm(b)
        x3, _, _ = pcg(A, b, preconditioner(sp.csr_matrix(A), n, kind), max_iter=3)
        assert np.linalg.norm(np.concatenate(e.value.x_parts) - x3) <= 1e-10 * np.linalg.norm(x3)
        if R.W == 1:
            # one rank: zero counts, and the iterates of pdh_solve_cg_device
            assert R.lay[0][:2] == ([0], [0]) and R.lay[0][2]["n_ghost_rows"] == 0
            d_b, d_x = R.dev.put(b), R.dev.put(np.zeros(len(b)))
            assert R.ctxs[0].solve_cg_device(d_b, d_x) == info
            assert R.dev.get(d_x, len(b)).tobytes() == x.tobytes()
    finally:
        R.close()


def test_exact_initial_guess_and_zero_rhs_take_no_iteration():
    from polydeal_amd.distributed import solve_cg_lockstep

    w = hc.world("slab_pinwheel_dgp1")
    R = Ranks(w)
    try:
        splits, N = R.part.splits, w.dense().shape[0]
        xs = np.random.default_rng(9).standard_normal(N)
        parts = lambda v: [v[splits[r]:splits[r + 1]] for r in range(R.W)]
        b = np.concatenate([c.vmult(xs) for c in R.ctxs])  # b = A x* by the same arithmetic: r = 0 exactly
        trace = []
        x_parts, info = solve_cg_lockstep(R.ctxs, splits, parts(b), parts(xs), trace=trace)
        assert info["iterations"] == 0 and info["residual"] == 0.0 and np.array_equal(np.concatenate(x_parts), xs)
        assert trace == _expected_trace(0)
        x_parts, info = solve_cg_lockstep(R.ctxs, splits, parts(np.zeros(N)))
        assert info["iterations"] == 0 and not np.any(np.concatenate(x_parts))
    finally:
        R.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals and state errors
# ---------------------------------------------------------------------------------------------------------------------------------
def _refused(ctx, rc, code, fragment):
    msg = ctx.lib.pdh_last_error(ctx.h).decode()
    assert rc == code and fragment in msg, (rc, msg)


def test_state_errors():
    pa = _pa()
    E = pa._capi
    w = hc.world("slab_dist2d_dgq1")
    part = w.part
    prob, (r0, r1) = part.problems()[0]
    m = r1 - r0
    ctx, dev = pa.Context(0), Device()
    req, res = E.pdh_dcg_request(), E.pdh_cg_result()
    ctl = E.pdh_cg_control(100, 1e-13, 0.0)
    try:
        d_b, d_x, d_v = dev.fill(m, 1.0), dev.fill(m, 0.0), dev.fill(2 * part.kw["n_rows"], 1.0)
        begin = lambda: ctx.lib.pdh_dcg_begin(ctx.h, C.byref(ctl), C.c_void_p(d_b), C.c_void_p(d_x), C.byref(req))
        resume = lambda: ctx.lib.pdh_dcg_resume(ctx.h, C.byref(req), C.byref(res))
        _refused(ctx, begin(), E.PDH_ESTATE, "before pdh_set_problem")
        # the ghost-block variant has no vector halo
        ctx.set_exchange_mode("ghost")
        ctx.set_problem(prob, r0, r1)
        with pytest.raises(pa.PdhError) as e:
            ctx.halo_setup(part.splits)
        assert e.value.code == E.PDH_EUNSUPPORTED and "PDH_EXCHANGE_GHOST" in str(e.value)
        ctx.set_exchange_mode("none")
        ctx.set_problem(prob, r0, r1)
        ctx.assemble_device()
        # before the halo is set up
        _refused(ctx, begin(), E.PDH_ESTATE, "halo is not set up")
        _refused(ctx, ctx.lib.pdh_halo_pack_device(ctx.h, C.c_void_p(d_v), C.c_void_p(d_b)), E.PDH_ESTATE, "halo is not set up")
        _refused(ctx, ctx.lib.pdh_vmult_local_device(ctx.h, C.c_void_p(d_v), C.c_void_p(d_b), 0), E.PDH_ESTATE, "halo is not set up")
        _refused(ctx, resume(), E.PDH_ESTATE, "no run is open")
        # the planner's refusals reach the context
        with pytest.raises(pa.PdhError) as e:
            ctx.halo_setup([0, part.splits[1] - part.n, part.kw["n_rows"]])
        assert e.value.code == E.PDH_EINVAL and "no range of row_splits is the owned range" in str(e.value)
        _refused(ctx, begin(), E.PDH_ESTATE, "halo is not set up")
        ctx.halo_setup(part.splits)
        _refused(ctx, ctx.lib.pdh_vmult_local_device(ctx.h, C.c_void_p(d_v), C.c_void_p(d_b), 3), E.PDH_EINVAL, "which must be")
        _refused(ctx, ctx.lib.pdh_vmult_local_device(ctx.h, C.c_void_p(d_v), C.c_void_p(d_v + 8), 0), E.PDH_EINVAL, "overlap")
        _refused(ctx, ctx.lib.pdh_dcg_begin(ctx.h, C.byref(ctl), C.c_void_p(d_b), C.c_void_p(d_b), C.byref(req)), E.PDH_EINVAL, "b and x overlap")
        # a preconditioner older than the values
        ctx.setup_preconditioner("jacobi")
        ctx.assemble_device()
        _refused(ctx, begin(), E.PDH_ESTATE, "values changed")
        ctx.setup_preconditioner("jacobi")
        # one run at a time
        assert begin() == 0 and req.kind == E.PDH_DCG_HALO_BEGIN
        _refused(ctx, begin(), E.PDH_ESTATE, "a run is open")
        with pytest.raises(pa.PdhError) as e:
            ctx.halo_setup(part.splits)
        assert e.value.code == E.PDH_ESTATE
        # the preconditioner changes during the run: the run is closed
        ctx.setup_preconditioner("block_jacobi")
        _refused(ctx, resume(), E.PDH_ESTATE, "preconditioner changed during the run")
        _refused(ctx, resume(), E.PDH_ESTATE, "no run is open")
        # ... the values
        assert begin() == 0
        assert resume() == 0 and req.kind == E.PDH_DCG_HALO_END
        ctx.assemble_device()
        _refused(ctx, resume(), E.PDH_ESTATE, "values changed during the run")
        _refused(ctx, resume(), E.PDH_ESTATE, "no run is open")
        # a new problem takes the halo and the run with it
        ctx.setup_preconditioner("jacobi")
        assert begin() == 0
        ctx.set_problem(prob, r0, r1)
        _refused(ctx, resume(), E.PDH_ESTATE, "no run is open")
        _refused(ctx, begin(), E.PDH_ESTATE, "halo is not set up")
    finally:
        ctx.close()
        dev.free()


def test_preconditioners_that_are_not_rank_local_are_refused():
    """Chebyshev (also with the float32 smoother and the matrix-free operator), the direct solve and the V-cycle: PDH_EUNSUPPORTED naming
    the kind.  They need a context that owns all rows, so the world has one rank."""
    pa = _pa()
    E = pa._capi
    import ptransfer_cases as pc
    from polydeal_amd.levels import p_multigrid_hierarchy

    grid = pa.BackgroundGrid.hyper_cube_refined(3, 0.0, 1.0, 2)
    ah = pa.AgglomerationHandler(grid)
    ah.define_block_agglomerates(2)
    fe = pa.FE_DGQ(3, 2)
    ah.initialize_fe_values(3, 3)
    ah.distribute_agglomerated_dofs(fe)
    N = ah.n_dofs
    ctx, dev = pa.Context(0), Device()
    hier = None
    try:
        ctx.set_problem(ah.flatten(pa.SipVariant.poisson_example(fe), False, True))
        ctx.assemble_device()
        ctx.halo_setup([0, N])
        d_b, d_x = dev.fill(N, 1.0), dev.fill(N, 0.0)

        def refused(c, fragment):
            with pytest.raises(pa.PdhError) as e:
                c.dcg_begin(d_b, d_x)
            assert e.value.code == E.PDH_EUNSUPPORTED and fragment in str(e.value), str(e.value)
        ctx.setup_chebyshev()
        refused(ctx, "PDH_PREC_CHEBYSHEV is not")
        ctx.set_smoother_precision("f32")
        refused(ctx, "PDH_PREC_CHEBYSHEV with the float32 smoother")
        ctx.setup_chebyshev()
        ctx.setup_matrix_free()
        ctx.set_smoother_operator("matrix_free")
        refused(ctx, "PDH_PREC_CHEBYSHEV with the matrix-free smoother operator")
        ctx.setup_direct()
        refused(ctx, "PDH_PREC_DIRECT")
        ctx.setup_preconditioner("jacobi")  # (the context still serves)
        assert ctx.dcg_begin(d_b, d_x)["kind"] == E.PDH_DCG_HALO_BEGIN
        # the V-cycle
        name = sorted(pc.HIERARCHIES)[0]
        mirror, _ = pc.handlers(name)
        hier = p_multigrid_hierarchy(mirror, lambda f: pa.SipVariant.poisson_example(f), diag_first=False, degree=pc.DEGREE)
        Nf = mirror[-1].n_dofs
        hier.finest.halo_setup([0, Nf])
        d_b, d_x = dev.fill(Nf, 1.0), dev.fill(Nf, 0.0)
        refused(hier.finest, "PDH_PREC_MULTIGRID")
    finally:
        if hier is not None:
            hier.close()
        ctx.close()
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# the example and two processes
# ---------------------------------------------------------------------------------------------------------------------------------
def _norms(out):
    """the L2 and H1 error norms of every degree, as printed"""
    l2 = [float(v) for v in re.findall(r"^L2 error \(exponential solution\): (\S+)$", out, re.M)]
    h1 = [float(v) for v in re.findall(r"^Semi H1 error \(exponential solution\): (\S+)$", out, re.M)]
    assert len(l2) == len(h1) == 4, out
    return l2 + h1


def test_example_device_solve_matches_the_host_solver():
    exe = os.path.join(ROOT, "examples", "diffusion_reaction")
    assert os.path.exists(exe), "examples/diffusion_reaction is not built"
    host = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert host.returncode == 0, host.stdout + host.stderr
    devs = subprocess.run([exe, "--device-solve"], capture_output=True, text=True, timeout=600)
    assert devs.returncode == 0, devs.stdout + devs.stderr
    # (degree 4 has 125 dofs per polytope, beyond the device's block Jacobi: the example keeps the host solver there and says so)
    assert len(re.findall(r"^device solve: \d+ iterations on 4 ranks$", devs.stdout, re.M)) == 3, devs.stdout
    for a, b in zip(_norms(host.stdout), _norms(devs.stdout)):
        assert abs(a - b) <= 1e-8 * abs(a), (host.stdout, devs.stdout)


def test_two_processes_over_gloo():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29537", os.path.join(ROOT, "tests", "_dist_solve_worker.py")],
        env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "DIST_SOLVE_OK world=2" in out.stdout
