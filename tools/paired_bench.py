#!/usr/bin/env python3
"""Paired timing of the store policies of k_terms_wg's writers (pdh_terms_wg.h) on ONE resident problem.
    make -C polydeal_amd/csrc variants          (a -DPDHT_VARIANTS library in build/variants/)
    python tools/paired_bench.py [--lib build/variants/libpolydeal_hip.so] [--contexts 4] [--rounds 9]
Two builds in two contexts cannot resolve a few percent: the kernel's time is a property of where the allocator put the 7 GB of
values (+-5-9 % between contexts, profiles/r03_placement_spread.txt).  Here every context holds the headline problem once, and
pdh_debug_terms_wg_variant re-resolves its row launch between the variants, which therefore write the SAME allocation; the variants
run in interleaved rounds, their order rotating from round to round.  The baseline (nt stores left in flight, the library's policy
until sc1|nt drained stores - "sc1nt/drain", what the library now ships - were chosen with this tool) runs twice per round, as "base"
and "self": base - self is the spread the baseline shows against itself on that context, the yardstick for
every other difference.  Prints, per context and variant, the median kernel time (HIP events of the library, --steps launches each)
and the paired differences to the baseline; then compares the matrices of all variants at --check-cells (the sums and their order do
not depend on the store policy: they must be bit-identical)."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench  # noqa: E402
import polydeal_amd as pa  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name: (order, aux, drain) of pdh_debug_terms_wg_variant; "base" and "self" are the same kernel
# ("nt/drain" and "sc1nt/fly" were measured with these two and taken out of the source again: profiles/r14_paired_variants.txt)
VARIANTS = {"base": (0, 2, 0), "self": (0, 2, 0), "sc1nt/drain": (0, 18, 1)}


def set_variant(ctx, name):
    order, aux, drain = VARIANTS[name]
    ctx._chk(ctx.lib.pdh_debug_terms_wg_variant(ctx.h, order, aux, drain))


def make_context(lib, flat):
    c = pa.Context(0, lib_path=lib)
    c.lib.pdh_debug_terms_wg_variant.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    c.lib.pdh_debug_terms_wg_variant.restype = C.c_int
    c.set_problem(flat)
    assert c.rows_kernel_in_use() == "terms", c.rows_kernel_in_use()
    c.set_overlap(False)  # (kernel times of kernels that have the device to themselves)
    return c


def problem(cells, grown):
    grid, ah, fe = bench.build_handler(pa, 3, cells, 2, "dgq", 3, 4, grown=grown)
    return ah.flatten(pa.SipVariant.poisson_example(fe), True, False), (grid, ah, fe)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=os.path.join(ROOT, "build", "variants", "libpolydeal_hip.so"))
    ap.add_argument("--contexts", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20, help="timed launches per variant and round (3: a round's mean moves by +-3 %)")
    ap.add_argument("--cells", type=int, default=64, help="cells per direction of the timed problem (64: the headline problem)")
    ap.add_argument("--check-cells", type=int, default=32, help="cells per direction of the problem whose matrices are compared (0: none)")
    ap.add_argument("--grown", action="store_true", help="irregular agglomerates grown over the cell graph")
    a = ap.parse_args()
    lib = os.path.abspath(a.lib)
    names = list(VARIANTS)

    if a.check_cells > 0:
        flat, keep = problem(a.check_cells, a.grown)
        c = make_context(lib, flat)
        mats = {}
        for name in names:
            set_variant(c, name)
            mats[name] = c.assemble().copy()
        same = {name: bool(np.array_equal(mats["base"], mats[name])) for name in names}
        print("matrices at --cells %d, np.array_equal with the baseline: %s" % (a.check_cells, " ".join("%s=%s" % kv for kv in same.items())))
        c.close()
        del mats, flat, keep
        if not all(same.values()):
            return 1

    flat, keep = problem(a.cells, a.grown)
    ctxs = [make_context(lib, flat) for _ in range(a.contexts)]
    for c in ctxs:
        for name in names:  # (every variant launched once before anything is timed)
            set_variant(c, name)
            c.assemble_device()
        c.synchronize()
    t = [{name: [] for name in names} for _ in ctxs]
    for r in range(a.rounds):
        for k, c in enumerate(ctxs):
            for i in range(len(names)):
                name = names[(i + r + k) % len(names)]
                set_variant(c, name)
                c.assemble_device()  # (not timed: the first launch on a context another one has just left is slower)
                c.set_profiling(True)
                for _ in range(a.steps):
                    c.assemble_device()
                (kd, _), _ = c.kernel_times_ms()
                c.set_profiling(False)
                t[k][name].append(kd)
    print("kernel time, ms: median over %d rounds of %d launches | paired difference to base per round: median [min, max]" % (a.rounds, a.steps))
    verdict = {name: [] for name in names if name != "base"}
    for k in range(len(ctxs)):
        base = t[k]["base"]
        print("context %d: base %.4f" % (k, statistics.median(base)))
        spread = None
        for name in names[1:]:
            d = [x - b for x, b in zip(t[k][name], base)]
            med = statistics.median(d)
            if name == "self":
                spread = max(abs(x) for x in d)
            print("    %-12s %.4f   %+.4f [%+.4f, %+.4f]  (%+.2f %%)" % (name, statistics.median(t[k][name]), med, min(d), max(d), 100.0 * med / statistics.median(base)))
            verdict[name].append((statistics.median(t[k][name]) < statistics.median(base), med, spread))
    print("a variant replaces the baseline only if it is faster on every context AND its median paired difference exceeds three times the")
    print("largest |base - self| of that context:")
    for name in names[2:]:
        faster = all(f for f, _, _ in verdict[name])
        beyond = all(-m > 3.0 * s for _, m, s in verdict[name])
        print("    %-12s faster on every context: %s; beyond 3 x self-spread on every context: %s" % (name, faster, beyond))
    for c in ctxs:
        c.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
