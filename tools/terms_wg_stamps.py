#!/usr/bin/env python3
"""Step timing of the FE_DGQ(3) workgroup kernel (pdh_terms_wg.h) from in-kernel cycle-counter stamps (library built with
-DPDHT_STAMP):  python tools/terms_wg_stamps.py build/tstamp/libpolydeal_hip.so [cells] [grown]
Per polytope: the first and the last writer wave (start of the step, last store issued, barrier left) and the first and the last
builder wave (requests of the next polytope issued, tables of this one done, barrier left)."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench  # noqa: E402
import polydeal_amd as pa  # noqa: E402

os.environ["PDH_TERMS_DGQ3"] = "1"
lib_path = os.path.abspath(sys.argv[1])
cells = int(sys.argv[2]) if len(sys.argv) > 2 else 64
grown = len(sys.argv) > 3 and sys.argv[3] == "grown"
grid, ah, fe = bench.build_handler(pa, 3, cells, 2, "dgq", 3, 4, grown=grown)
flat = ah.flatten(pa.SipVariant.poisson_example(fe), True, False)
ctx = pa.Context(0, lib_path=lib_path)
ctx.set_problem(flat)
assert ctx.rows_kernel_in_use() == "terms"
for _ in range(3):
    ctx.assemble_device()
ctx.synchronize()
n = ctx.stats()["n_owned_agg"]
out = np.zeros((n, 16), dtype=np.int64)
ctx.lib.pdh_debug_rows_stamps.argtypes = [C.c_void_p, C.c_void_p]
assert ctx.lib.pdh_debug_rows_stamps(ctx.h, out.ctypes.data) == 0
st = out[:, :12].reshape(n, 4, 3).astype(np.float64)
print("FE_DGQ(3) %s, %d polytopes, writer waves %s" % ("grown" if grown else "blocks", n, os.environ.get("PDH_TERMS_WG_WAVES", "8")))
for w, nm in ((0, "first writer"), (1, "last writer ")):
    step, busy, wait = st[:, w, 2] - st[:, w, 0], st[:, w, 1] - st[:, w, 0], st[:, w, 2] - st[:, w, 1]
    print("%s: step %8.0f cycles (median %8.0f) = tables to last store issued %8.0f + wait at the barrier %8.0f (%4.1f %% of a step)"
          % (nm, step.mean(), np.median(step), busy.mean(), wait.mean(), 100 * wait.mean() / step.mean()))
for w, nm in ((2, "first builder"), (3, "last builder ")):
    ok = st[:, w, 0] > 0
    busy, idle = (st[:, w, 1] - st[:, w, 0])[ok], (st[:, w, 2] - st[:, w, 1])[ok]
    print("%s: requests issued to tables done %8.0f cycles (median %8.0f), idle at the barrier %8.0f (%4.1f %%)"
          % (nm, busy.mean(), np.median(busy), idle.mean(), 100 * idle.mean() / (busy.mean() + idle.mean())))
