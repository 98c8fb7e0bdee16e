"""Drivers of CG over several ranks (include/polydeal_hip.h: pdh_dcg_*).  The C ABI hands out requests - move a halo, sum a few scalars -
and calls no transport; the two drivers here carry the requests out:

``solve_cg_lockstep``  W contexts of ONE process play the ranks in lock-step: halo moves are device-to-device copies, the all-reduce adds
                       in rank order on the host.  For tests, examples and tools/solve_bench.py --distributed; one device playing W
                       ranks shows neither overlap nor interconnect.
``TorchRank``          one rank of a ``torch.distributed`` group: ``all_to_all_single`` with the halo's split sizes and ``all_reduce``;
                       under a backend that moves host memory only (gloo) both stage through the host, as bench.py's rehearsal does.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import PDH_DCG_ALLREDUCE, PDH_DCG_DONE, PDH_DCG_HALO_BEGIN, PDH_DCG_HALO_END, PdhError

_D2H, _H2D, _D2D = 2, 1, 3


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def _copy(hip, dst, src, n_doubles, kind):
    if n_doubles and hip.hipMemcpy(C.c_void_p(dst), C.c_void_p(src), 8 * int(n_doubles), kind) != 0:
        raise PdhError(_capi.PDH_EDEVICE, "hipMemcpy failed")


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def solve_cg_lockstep(ctxs, row_splits, b_parts, x0_parts=None, rel_tol=1e-13, abs_tol=0.0, max_iter=None, trace=None):
    """solve_cg_lockstep_device for host arrays: b_parts[r] (and x0_parts[r], default zero) are rank r's rows.  Returns (x_parts, info);
    PDH_ENOCONV raises PdhError carrying .x_parts (the last iterates) and .info."""
    hip, W, bufs = _hip(), len(ctxs), []
    try:
        d_b, d_x, xs = [], [], []
        for r in range(W):
            b = np.ascontiguousarray(b_parts[r], dtype=np.float64)
            x = np.zeros(len(b)) if x0_parts is None else np.array(x0_parts[r], dtype=np.float64, copy=True)
            if x.shape != b.shape or len(b) != int(row_splits[r + 1]) - int(row_splits[r]):
                raise ValueError("b_parts[%d] and x0_parts[%d] must hold the rows of rank %d" % (r, r, r))
            for a, lst in ((b, d_b), (x, d_x)):
                ptr = C.c_void_p()
                if hip.hipMalloc(C.byref(ptr), max(a.nbytes, 8)) != 0:
                    raise PdhError(_capi.PDH_EDEVICE, "solve_cg_lockstep: out of device memory")
                bufs.append(ptr)
                _copy(hip, ptr.value, a.ctypes.data, len(a), _H2D)
                lst.append(ptr.value)
            xs.append(x)

        def fetch():
            for r in range(W):
                ctxs[r].synchronize()
                _copy(hip, xs[r].ctypes.data, d_x[r], len(xs[r]), _D2H)
            return xs
        try:
            info = solve_cg_lockstep_device(ctxs, row_splits, d_b, d_x, rel_tol, abs_tol, max_iter, trace=trace)
        except PdhError as e:
            if e.code == _capi.PDH_ENOCONV:
                e.x_parts = fetch()
            raise
        return fetch(), info
    finally:
        for ptr in bufs:
            hip.hipFree(ptr)


def solve_cg_lockstep_device(ctxs, row_splits, d_b, d_x, rel_tol=1e-13, abs_tol=0.0, max_iter=None, layouts=None, trace=None):
    """Preconditioned CG on the rows of W contexts of this process (rank r = ctxs[r], rows row_splits[r] .. row_splits[r + 1], each with
    its problem resident, its values assembled and its preconditioner set up).  d_b[r], d_x[r]: device pointers (ints) of rank r's
    right-hand side and of its initial guess / solution, [owned rows] each.  layouts: what halo_setup returned per rank (None: set the
    halos up here).  trace: a list that receives the kind of every round of requests.  Returns the info of rank 0 - every rank reports
    the same iteration count and residual, which is asserted; PDH_ENOCONV raises PdhError with .info after every rank has answered."""
    W = len(ctxs)
    if layouts is None:
        layouts = [c.halo_setup(row_splits) for c in ctxs]
    hip = _hip()
    send_at = [_offsets(l[0]) for l in layouts]
    recv_at = [_offsets(l[1]) for l in layouts]
    reqs = [c.dcg_begin(d_b[r], d_x[r], rel_tol, abs_tol, max_iter) for r, c in enumerate(ctxs)]
    infos, errors = [None] * W, [None] * W
    while True:
        kinds = {q["kind"] for q in reqs}
        if len(kinds) != 1:
            raise PdhError(_capi.PDH_ESTATE, "the ranks are out of step: requests %s" % sorted(kinds))
        kind = kinds.pop()
        if trace is not None:
            trace.append((kind, reqs[0]["n_scalars"]))
        if kind == PDH_DCG_DONE:
            break
        if kind == PDH_DCG_HALO_BEGIN:  # a synchronous transport: everything moves here
            for c in ctxs:
                c.synchronize()
            for s in range(W):
                for d in range(W):
                    _copy(hip, reqs[d]["d_recv"] + 8 * int(recv_at[d][s]), reqs[s]["d_send"] + 8 * int(send_at[s][d]), layouts[s][0][d], _D2D)
        elif kind == PDH_DCG_ALLREDUCE:
            m = reqs[0]["n_scalars"]
            parts = np.empty((W, m))
            for r, c in enumerate(ctxs):
                c.synchronize()
                _copy(hip, parts[r].ctypes.data, reqs[r]["d_scalars"], m, _D2H)
            total = parts[0].copy()
            for r in range(1, W):  # rank order: the same bits for every rank
                total += parts[r]
            for r in range(W):
                _copy(hip, reqs[r]["d_scalars"], total.ctypes.data, m, _H2D)
        elif kind != PDH_DCG_HALO_END:
            raise PdhError(_capi.PDH_ESTATE, "unknown request %d" % kind)
        for r, c in enumerate(ctxs):
            try:
                reqs[r], infos[r] = c.dcg_resume()
            except PdhError as e:
                if e.code != _capi.PDH_ENOCONV:
                    raise
                errors[r], infos[r], reqs[r] = e, e.info, {"kind": PDH_DCG_DONE, "n_scalars": 0}
    if any(i != infos[0] for i in infos) or (any(errors) and not all(errors)):
        raise PdhError(_capi.PDH_ESTATE, "the ranks disagree about the end of the run: %s" % infos)
    if errors[0] is not None:
        errors[0].infos = infos
        raise errors[0]
    return infos[0]


class TorchRank:
    """One rank of a torch.distributed group driving its context through a CG run.  The group must be initialised; rank r of the group
    owns the rows row_splits[r] .. row_splits[r + 1].  With a backend that moves device memory (nccl, i.e. RCCL) the collectives work on
    tensors that alias the library's buffers; otherwise (gloo) every move is staged through the host.  Only the staged path has run: the
    tests drive two gloo processes on one device, there is no multi-GPU node."""

    def __init__(self, ctx, row_splits, group=None):
        import torch
        import torch.distributed as dist

        self.torch, self.dist, self.ctx, self.group = torch, dist, ctx, group
        self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        if len(row_splits) != self.world + 1:
            raise ValueError("row_splits must have world + 1 entries")
        self.send_count, self.recv_count, self.info = ctx.halo_setup(row_splits)
        self.on_device = dist.get_backend(group) == "nccl"
        self.hip = _hip()
        if self.on_device:  # order the collectives with the library's kernels on one stream
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)

    def _view(self, ptr, n):
        """a CUDA tensor over n doubles of device memory at ptr"""
        class _Cai:
            __cuda_array_interface__ = {"shape": (max(int(n), 1),), "typestr": "<f8", "data": (int(ptr), False), "version": 2}
        return self.torch.as_tensor(_Cai(), device="cuda")[:int(n)]

    def _halo(self, req):
        torch, dist = self.torch, self.dist
        ns, nr = sum(self.send_count), sum(self.recv_count)
        if self.on_device:
            dist.all_to_all_single(self._view(req["d_recv"], nr), self._view(req["d_send"], ns), self.recv_count, self.send_count,
                                   group=self.group)
            return
        self.ctx.synchronize()
        send, recv = torch.empty(ns, dtype=torch.float64), torch.empty(nr, dtype=torch.float64)
        _copy(self.hip, send.data_ptr(), req["d_send"], ns, _D2H)
        dist.all_to_all_single(recv, send, self.recv_count, self.send_count, group=self.group)
        _copy(self.hip, req["d_recv"], recv.data_ptr(), nr, _H2D)

    def _allreduce(self, req):
        torch, dist, m = self.torch, self.dist, req["n_scalars"]
        if self.on_device:
            dist.all_reduce(self._view(req["d_scalars"], m), group=self.group)
            return
        self.ctx.synchronize()
        t = torch.empty(m, dtype=torch.float64)
        _copy(self.hip, t.data_ptr(), req["d_scalars"], m, _D2H)
        dist.all_reduce(t, group=self.group)  # (every rank receives the same bits from one reduction)
        _copy(self.hip, req["d_scalars"], t.data_ptr(), m, _H2D)

    def solve_cg_torch(self, d_b, d_x, rel_tol=1e-13, abs_tol=0.0, max_iter=None):
        """CG on this rank's rows: d_b, d_x [owned rows] device pointers (ints), x0 in, solution out.  Returns the info
        {iterations, residual0, residual}, the same on every rank; PDH_ENOCONV raises PdhError with .info on every rank."""
        req, info = self.ctx.dcg_begin(d_b, d_x, rel_tol, abs_tol, max_iter), None
        while req["kind"] != PDH_DCG_DONE:
            if req["kind"] == PDH_DCG_HALO_BEGIN:
                self._halo(req)
            elif req["kind"] == PDH_DCG_ALLREDUCE:
                self._allreduce(req)
            req, info = self.ctx.dcg_resume()
        return info
