"""The ghost-block exchange (PDH_EXCHANGE_GHOST, csrc/pdh_exchange.hip and the planner's plan_exchange) on the worlds of
tests/exchange_cases.py: W contexts on device 0 play the ranks, the transport is a copy through the host.  Interleaved ownership makes ranks
exchange in both directions, puts M21 blocks on either side of the diagonal block and sends a polytope M22 sums from several peers.

Checked per world and algorithm: the rows after a step against the oracle (tests/parity.py) and against PDH_EXCHANGE_NONE; the wire format -
every block of every send buffer where tests/exchange_cases.py::expected_exchange says it is, against the oracle's block; what
pdh_exchange_apply touches; that a step is repeatable to the bit; the edge worlds and refusals; vmult and a stale preconditioner after the
apply.

In a buffer an M21 block is plain [row of Q][column of P].  An M22 block has the layout of the receiver's diagonal block: plain in the
ascending layout, in the diagonal-first layout every row carries its diagonal entry in front (decode_m22)."""
import ctypes as C

import numpy as np
import pytest

import exchange_cases as xc
from device_buffers import Device
from parity import FLOOR, TOL, assert_parity_ah

pytestmark = pytest.mark.gpu

RUNS = [(cid, alg) for cid in list(xc.ALL_CASES) for alg in xc.algorithms(xc.element(cid))] + \
    [(xc.MIRROR_CASE, alg) for alg in ("auto", "moment", "direct")]


def _pa():
    import polydeal_amd as pa
    return pa


def decode_m22(raw, diag_first):
    """[row][column] of an M22 block as it travels"""
    if not diag_first:
        return raw
    n = raw.shape[0]
    out = np.empty_like(raw)
    for R in range(n):
        out[R, R] = raw[R, 0]
        out[R, :R] = raw[R, 1:R + 1]
        out[R, R + 1:] = raw[R, R + 1:]
    return out


class Ranks:
    """the contexts of a world, their buffers and the positions of blocks in their values"""

    def __init__(self, part, alg, mode="ghost"):
        pa = _pa()
        self.part, self.W, self.n, self.dev = part, part.world, part.n, Device()
        self.off = np.asarray(part.kw["dof_offset"], dtype=np.int64)
        self.rp, self.ci = np.asarray(part.kw["rowptr"], dtype=np.int64), np.asarray(part.kw["colind"], dtype=np.int64)
        self.ctxs, self.probs = [], []
        try:
            for prob, (r0, r1) in part.problems():
                c = pa.Context(0)
                self.ctxs.append(c)
                self.probs.append(prob)  # (the description outlives the set-up: nothing but the test needs it, the arrays are cheap)
                c.set_algorithm(alg)
                c.set_exchange_mode(mode)
                c.set_problem(prob, r0, r1)
            if mode == "ghost":
                self.lay = [c.exchange_layout(self.W) for c in self.ctxs]
                self.d_send = [self.dev.fill(sum(l[0]), 0.0) for l in self.lay]
                self.d_recv = [self.dev.fill(sum(l[1]), np.nan) for l in self.lay]
        except Exception:
            self.close()
            raise

    def close(self):
        for c in self.ctxs:
            c.close()
        self.dev.free()

    def positions(self, r, Q, P):
        """[n][n] positions in rank r's values of A[rows of Q, columns of P] ([row][column])"""
        n, r0 = self.n, self.part.rows(r)[0]
        assert self.part.owner[Q] == r
        out = np.empty((n, n), dtype=np.int64)
        for i in range(n):
            row = self.off[Q] + i
            seg = self.ci[self.rp[row]:self.rp[row + 1]]
            at = np.nonzero((seg >= self.off[P]) & (seg < self.off[P] + n))[0]
            assert len(at) == n
            out[i, seg[at] - self.off[P]] = self.rp[row] - self.rp[r0] + at
        return out

    def assemble_and_send(self):
        """assembly and pdh_exchange_get_send on every rank: (send buffers, values before the apply) on the host"""
        for r, c in enumerate(self.ctxs):
            c.assemble_device()
            c.exchange_get_send(self.d_send[r])
            c.synchronize()
        return [self.dev.get(self.d_send[r], sum(self.lay[r][0])) for r in range(self.W)], [c.values() for c in self.ctxs]

    def transport(self, sends):
        """segment (s -> d) of s's send buffer becomes segment (from s) of d's receive buffer; the receive buffers on the host"""
        for r in range(self.W):
            self.dev.write(self.d_recv[r], np.full(max(sum(self.lay[r][1]), 1), np.nan))
        for s in range(self.W):
            so = xc.segment_offsets(self.lay[s][0])
            for d in range(self.W):
                ro = xc.segment_offsets(self.lay[d][1])
                self.dev.write(self.d_recv[d], sends[s][so[d]:so[d + 1]], offset=ro[s])
        return [self.dev.get(self.d_recv[r], sum(self.lay[r][1])) for r in range(self.W)]

    def apply(self):
        for r, c in enumerate(self.ctxs):
            c.exchange_apply(self.d_recv[r])
        return [c.values() for c in self.ctxs]


def _block_bound(ref_block, scale):
    return TOL * max(float(np.max(np.abs(ref_block))), FLOOR * scale)


def _check_algorithm(ctxs, alg):
    used = {c.algorithm_in_use() for c in ctxs}
    assert all(c.rows_kernel_in_use() == "none" for c in ctxs)  # the row kernels do not serve the exchange variant
    if alg != "auto":
        assert used == {alg}, (alg, used)
    assert used <= {"direct", "moment", "mixed"}, used
    return used


@pytest.mark.parametrize("cid,alg", RUNS, ids=lambda v: str(v))
def test_exchange_step(cid, alg):
    """parity after the step, the wire format, what the apply touches, and the step again"""
    part = xc.world(cid)
    oah, ref = xc.reference(cid)
    A = xc.oracle_dense(cid)
    scale = float(np.max(np.abs(ref)))
    diag_first, n, W = bool(part.kw["diag_first"]), part.n, part.world
    exp = part.expected()
    want = xc.expected_sizes(exp, n, W)
    rows_of = lambda P: slice(int(part.kw["dof_offset"][P]), int(part.kw["dof_offset"][P]) + n)

    # owner-computes-rows on the same descriptions
    own = Ranks(part, alg, "none")
    try:
        own_values = [c.assemble() for c in own.ctxs]
    finally:
        own.close()

    R = Ranks(part, alg)
    try:
        used = _check_algorithm(R.ctxs, alg)
        for r in range(W):
            assert R.lay[r][0] == want[r].tolist() and R.lay[r][1] == want[:, r].tolist(), (r, R.lay[r])
        sends, before = R.assemble_and_send()

        # -- the wire format: every block where the independent order puts it -------------------------------------------------------------
        worst21 = worst22 = 0.0
        m22_sum, touched = {}, [np.zeros(v.shape, dtype=bool) for v in before]
        m21_mask = [np.zeros(v.shape, dtype=bool) for v in before]
        for s in range(W):
            assert np.all(np.isfinite(sends[s])), "rank %d: non-finite values in the send buffer" % s
            so = xc.segment_offsets(R.lay[s][0])
            for d in range(W):
                seg = sends[s][so[d]:so[d + 1]].reshape(-1, n, n)
                blocks = exp.get((s, d), [])
                assert len(blocks) == len(seg)
                for raw, b in zip(seg, blocks):
                    if b[0] == "m21":
                        _, P, Q = b
                        want_block = A[rows_of(Q), rows_of(P)]
                        err = float(np.max(np.abs(raw - want_block)))
                        bound = _block_bound(want_block, scale)
                        assert err <= bound, "M21 of face (%d, %d), rank %d -> %d: err %.3e, bound %.3e" % (P, Q, s, d, err, bound)
                        worst21 = max(worst21, err / bound)
                        pos = R.positions(d, Q, P)
                        m21_mask[d][pos] = True
                        touched[d][pos] = True
                    else:
                        Q = b[1]
                        m22_sum[Q] = m22_sum.get(Q, 0.0) + decode_m22(raw, diag_first)
                        touched[d][R.positions(d, Q, Q)] = True
        for Q, add in m22_sum.items():
            d = int(part.owner[Q])
            want_block = A[rows_of(Q), rows_of(Q)]
            got_block = before[d][R.positions(d, Q, Q)] + add
            err = float(np.max(np.abs(got_block - want_block)))
            bound = _block_bound(want_block, scale)
            assert err <= bound, "diagonal block of %d + its received M22 sums: err %.3e, bound %.3e" % (Q, err, bound)
            worst22 = max(worst22, err / bound)

        # -- the transport: the layouts tile ---------------------------------------------------------------------------------------------
        recvs = R.transport(sends)
        for r in range(W):
            assert recvs[r].size == want[:, r].sum() and not np.any(np.isnan(recvs[r])), "rank %d: the receive buffer is not tiled" % r

        # -- what the apply touches ------------------------------------------------------------------------------------------------------
        after = R.apply()
        for r in range(W):
            same = before[r] == after[r]
            assert np.all(same[~touched[r]]), "rank %d: pdh_exchange_apply changed %d values outside its destination blocks" % (
                r, int(np.sum(~same[~touched[r]])))
            assert before[r][~touched[r]].tobytes() == after[r][~touched[r]].tobytes()
            assert np.all(np.isfinite(after[r]))

        # -- parity after the step -------------------------------------------------------------------------------------------------------
        got = xc.to_oracle_order(part, oah, after)
        rel = assert_parity_ah(got, ref, oah, diag_first, what="ghost exchange %s %s" % (cid, alg))
        none_rel = max((float(np.max(np.abs(a - o))) for a, o in zip(after, own_values)), default=0.0) / scale
        assert none_rel <= 1e-13, none_rel
        print("%s %s: algorithm %s, parity %.3e of max|A|, M21 on the wire %.3e and diagonal + M22 %.3e of the per-block bound, "
              "against PDH_EXCHANGE_NONE %.3e of max|A|" % (cid, alg, "/".join(sorted(used)), rel, worst21, worst22, none_rel))

        # -- the step again: the same bits (assembly resets the M22 targets and the send region) ------------------------------------------
        sends2, before2 = R.assemble_and_send()
        for r in range(W):
            assert sends2[r].tobytes() == sends[r].tobytes(), r
            # (nothing but the apply writes where the M21 blocks go: there the values of the first apply still stand)
            assert before2[r][~m21_mask[r]].tobytes() == before[r][~m21_mask[r]].tobytes(), r
        R.transport(sends2)
        after2 = R.apply()
        for r in range(W):
            assert after2[r].tobytes() == after[r].tobytes(), r

        # -- ... and again with other values where the M21 blocks go: they are stored, not added to ---------------------------------------
        sends3, before3 = R.assemble_and_send()
        for r, c in enumerate(R.ctxs):
            if m21_mask[r].any():
                v = before3[r].copy()
                v[m21_mask[r]] = 1.0e300
                ptr, count = c.device_values()
                assert count == v.size
                R.dev.write(ptr, v)
        R.transport(sends3)
        after3 = R.apply()
        for r in range(W):
            assert after3[r].tobytes() == after[r].tobytes(), r
    finally:
        R.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# edge worlds and refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_one_rank_exchanges_nothing():
    pa = _pa()
    part = xc.world("one_rank")
    prob, (r0, r1) = part.problems()[0]
    plain = pa.Context(0)
    ctx = pa.Context(0)
    try:
        plain.set_problem(prob, r0, r1)
        want = plain.assemble()
        ctx.set_exchange_mode("ghost")
        ctx.set_problem(prob, r0, r1)
        assert ctx.exchange_layout(1) == ([0], [0])
        assert ctx.exchange_layout(3) == ([0, 0, 0], [0, 0, 0])
        ctx.assemble_device()
        ctx.exchange_get_send(0)
        ctx.exchange_apply(0)
        assert ctx.algorithm_in_use() == plain.algorithm_in_use()
        assert ctx.values().tobytes() == want.tobytes()
    finally:
        ctx.close()
        plain.close()


def test_exchange_argument_and_state_errors():
    pa = _pa()
    E = pa._capi
    part = xc.world("dist3d_dgq1")
    (prob, (r0, r1)) = part.problems()[1]
    ctx, dev = pa.Context(0), Device()
    cnt = (C.c_int64 * 8)()

    def refused(rc, code, fragment):
        msg = ctx.lib.pdh_last_error(ctx.h).decode()
        assert rc == code and fragment in msg, (rc, msg)
    try:
        ctx.set_exchange_mode("ghost")
        ctx.set_problem(prob, r0, r1)
        sc, rc_ = ctx.exchange_layout(part.world)
        assert sum(sc) > 0 and sum(rc_) > 0
        ctx.assemble_device()
        room = dev.fill(max(sum(sc), sum(rc_)), 0.0)
        refused(ctx.lib.pdh_exchange_get_send(ctx.h, None), E.PDH_EINVAL, "d_send is NULL")
        refused(ctx.lib.pdh_exchange_apply(ctx.h, None), E.PDH_EINVAL, "d_recv is NULL")
        refused(ctx.lib.pdh_exchange_layout(ctx.h, part.world - 1, cnt, cnt), E.PDH_EINVAL, "n_ranks is smaller")
        refused(ctx.lib.pdh_exchange_layout(ctx.h, part.world, None, cnt), E.PDH_EINVAL, "an output is NULL")
        ctx.exchange_get_send(room)  # (the context still serves)
        ctx.synchronize()
        # the same problem without the ghost mode: every exchange call is a state error
        ctx.set_exchange_mode("none")
        ctx.set_problem(prob, r0, r1)
        ctx.assemble_device()
        refused(ctx.lib.pdh_exchange_layout(ctx.h, part.world, cnt, cnt), E.PDH_ESTATE, "not set in PDH_EXCHANGE_GHOST mode")
        refused(ctx.lib.pdh_exchange_get_send(ctx.h, C.c_void_p(room)), E.PDH_ESTATE, "no problem resident in PDH_EXCHANGE_GHOST mode")
        refused(ctx.lib.pdh_exchange_apply(ctx.h, C.c_void_p(room)), E.PDH_ESTATE, "no problem resident in PDH_EXCHANGE_GHOST mode")
        # more than 64 dofs per polytope: refused at set-up, and nothing is resident afterwards
        ctx.set_exchange_mode("ghost")
        big = xc.dgq4_world()
        with pytest.raises(pa.PdhError) as e:
            ctx.set_problem(pa.Problem(**big.kw), *big.rows(0))
        assert e.value.code == E.PDH_EUNSUPPORTED and "more than 64 dofs per polytope" in str(e.value)
        refused(ctx.lib.pdh_exchange_layout(ctx.h, 2, cnt, cnt), E.PDH_ESTATE, "no problem resident")
        ctx.set_exchange_mode("none")
        ctx.set_problem(pa.Problem(**big.kw), *big.rows(0))  # owner-computes-rows takes it
    finally:
        ctx.close()
        dev.free()


def test_cartesian_description_is_refused_in_ghost_mode():
    pa = _pa()
    from polydeal_amd.partition import row_range

    grid = pa.BackgroundGrid.subdivided_hyper_cube(3, 4, 0.0, 1.0)
    ah = pa.AgglomerationHandler(grid)
    ah.define_block_agglomerates(2)
    fe = pa.FE_DGQ(3, 2)
    ah.initialize_fe_values(3, 3)
    ah.distribute_agglomerated_dofs(fe)
    var = pa.SipVariant.poisson_example(fe)
    splits = [row_range(ah.n_agglomerates, fe.n_dofs_per_cell, r, 2)[0] for r in range(2)] + [ah.n_dofs]
    cf = ah.flatten_cartesian(var, True, False, 0, splits[1], splits)
    assert cf.cartesian
    ctx = pa.Context(0)
    try:
        ctx.set_exchange_mode("ghost")
        with pytest.raises(pa.PdhError) as e:
            ctx.set_problem(cf, 0, splits[1])
        assert e.value.code == pa._capi.PDH_EUNSUPPORTED and "cartesian description runs owner-computes-rows only" in str(e.value)
        ctx.set_exchange_mode("none")
        ctx.set_problem(cf, 0, splits[1])
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# downstream of the apply
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["dist3d_dgq1", xc.MIRROR_CASE])
def test_vmult_and_stale_preconditioner_after_apply(cid):
    """y = A x from the ranks' rows after the apply against the oracle's product in long double, per row within 1e-13 of sum_j |A_ij x_j|
    (the bound of tests/test_gpu_solve.py::test_vmult_parity); a preconditioner set up before the apply is stale after it, on a rank
    that receives nothing too"""
    pa = _pa()
    part = xc.world(cid)
    A = xc.oracle_dense(cid).astype(np.longdouble)
    N = A.shape[0]
    x = np.random.default_rng(1).standard_normal(N)
    ref = A @ x.astype(np.longdouble)
    bound = 1e-13 * (np.abs(A) @ np.abs(x).astype(np.longdouble))
    R = Ranks(part, "auto")
    try:
        receives = [sum(l[1]) > 0 for l in R.lay]
        if cid == xc.MIRROR_CASE:
            assert not receives[0]  # every cut face of the first rank is its own
        sends, _ = R.assemble_and_send()
        for c in R.ctxs:
            c.setup_preconditioner("jacobi")
        d_r = R.dev.fill(N, 1.0)
        d_z = R.dev.fill(N, 0.0)
        for c in R.ctxs:
            c.precondition_device(d_r, d_z)  # (in date before the apply)
            c.synchronize()
        R.transport(sends)
        R.apply()
        for r, c in enumerate(R.ctxs):
            rc = c.lib.pdh_precondition_device(c.h, C.c_void_p(d_r), C.c_void_p(d_z))
            msg = c.lib.pdh_last_error(c.h).decode()
            assert rc == pa._capi.PDH_ESTATE and "values changed" in msg, (r, receives[r], rc, msg)
        y = np.concatenate([c.vmult(x) for c in R.ctxs])
        err = np.abs(y.astype(np.longdouble) - ref)
        print("%s: vmult after the apply, worst |y - y_ref| / sum|a||x| = %.3e" % (cid, float(np.max(err / np.maximum(bound * 1e13, 1e-300)))))
        assert np.all(err <= bound), (int(np.sum(err > bound)), float(np.max(err / bound)))
        for c in R.ctxs:
            c.setup_preconditioner("jacobi")
            c.precondition_device(d_r, d_z)
            c.synchronize()
    finally:
        R.close()
