"""Timing of the solver kernels on the resident matrix (csrc/pdh_solve.hip): pdh_vmult_device, the block-inverse set-up and one
block-Jacobi CG iteration on the headline problem (3-D FE_DGQ(3), 64^3 cells in 32 768 polytopes of 2^3, both row layouts) and on
FE_AggloDGP(3) of the same mesh; then a full headline solve.  bench.py is not involved.

Times are HIP events on the library's stream (the context runs on torch's current stream), median of --reps launches after a warm-up.
Rates are over the bytes the kernel must read: the values (vmult), the values + the inverse blocks (one CG iteration), and the fraction
of the 8 TB/s HBM figure.  One CG iteration = (time of a solve with max_iter = k + m - time with max_iter = k) / m, host stop test
included.  Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def event_times_ms(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def handler(pa, cells, basis):
    grid = pa.BackgroundGrid.hyper_cube_refined(3, 0.0, 1.0, cells.bit_length() - 1)
    ah = pa.AgglomerationHandler(grid)
    ah.define_block_agglomerates(2)
    fe = (pa.FE_DGQ if basis == "dgq" else pa.FE_AggloDGP)(3, 3)
    ah.initialize_fe_values(4, 4)
    ah.distribute_agglomerated_dofs(fe)
    return ah, fe


def cg_iteration_ms(pa, ctx, torch, d_b, d_x, k, m, reps):
    """wall time of one CG iteration: solves capped at k and k + m iterations (PDH_ENOCONV expected), x reset before each"""
    def solve(cap):
        d_x.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            ctx.solve_cg_device(d_b.data_ptr(), d_x.data_ptr(), rel_tol=0.0, max_iter=cap)
        except pa.PdhError as e:
            if e.code != pa.PDH_ENOCONV:
                raise
        return time.perf_counter() - t0
    solve(k)
    diffs = [(solve(k + m) - solve(k)) / m * 1e3 for _ in range(reps)]
    return median(diffs)


def run_case(pa, torch, ctx, cells, basis, diag_first, reps):
    t0 = time.time()
    ah, fe = handler(pa, cells, basis)
    flat = ah.flatten(pa.SipVariant.poisson_example(fe), diag_first, False)
    ctx.set_problem(flat)
    ctx.assemble_device()
    ctx.synchronize()
    N, n = ah.n_dofs, fe.n_dofs_per_cell
    st = ctx.stats()
    val_bytes = 8.0 * st["n_values"]
    inv_bytes = 8.0 * st["n_owned_agg"] * n * n
    x = torch.rand(N, dtype=torch.float64, device="cuda")
    y = torch.empty(N, dtype=torch.float64, device="cuda")
    vm = event_times_ms(torch, lambda: ctx.vmult_device(x.data_ptr(), y.data_ptr()), reps)
    su = event_times_ms(torch, lambda: ctx.setup_preconditioner("block_jacobi"), max(3, reps // 3))
    it_ms = cg_iteration_ms(pa, ctx, torch, y, x, 2, 20, max(3, reps // 3))
    t_vm = median(vm) * 1e-3
    rec = {
        "element": "FE_DGQ(3)" if basis == "dgq" else "FE_AggloDGP(3)", "layout": "diag_first" if diag_first else "ascending",
        "n_dofs": N, "dofs_per_polytope": n, "polytopes": st["n_owned_agg"], "n_values": st["n_values"],
        "algorithm": ctx.algorithm_in_use(), "row_kernel": ctx.rows_kernel_in_use(),
        "vmult_ms_median": median(vm), "vmult_ms_min": min(vm), "vmult_TBps": val_bytes / t_vm / 1e12,
        "vmult_fraction_of_8TBps": val_bytes / t_vm / HBM_PEAK,
        "block_inverse_setup_ms_median": median(su), "block_inverse_bytes_written": inv_bytes,
        "cg_iteration_ms_median": it_ms, "cg_iteration_minus_vmult_ms": it_ms - median(vm),
        "cg_iteration_TBps_values_plus_inverse": (val_bytes + inv_bytes) / (it_ms * 1e-3) / 1e12,
        "cg_iteration_fraction_of_8TBps": (val_bytes + inv_bytes) / (it_ms * 1e-3) / HBM_PEAK,
        "launches": len(vm), "case_wall_s": time.time() - t0,
    }
    return rec, ah


def full_solve(pa, torch, ctx, N, reps_unused=None):
    """block-Jacobi CG on the resident headline matrix, b = A x* for a random x*, rel_tol 1e-13, x0 = 0"""
    gen = torch.Generator(device="cuda").manual_seed(1)
    xs = torch.rand(N, dtype=torch.float64, device="cuda", generator=gen)
    b = torch.empty(N, dtype=torch.float64, device="cuda")
    x = torch.zeros(N, dtype=torch.float64, device="cuda")
    ctx.vmult_device(xs.data_ptr(), b.data_ptr())
    ctx.setup_preconditioner("block_jacobi")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = ctx.solve_cg_device(b.data_ptr(), x.data_ptr(), rel_tol=1e-13)
    wall = time.perf_counter() - t0
    err = float(torch.linalg.norm(x - xs) / torch.linalg.norm(xs))
    return {"what": "block-Jacobi CG, b = A x* (x* random), x0 = 0, rel_tol 1e-13", "iterations": info["iterations"],
            "wall_s": wall, "ms_per_iteration": wall / max(info["iterations"], 1) * 1e3, "residual0": info["residual0"],
            "residual": info["residual"], "rel_error_vs_x_star": err}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cells", type=int, default=64, help="cells per axis (power of two); 64 = the headline problem")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-solve", action="store_true", help="skip the full headline solve")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import polydeal_amd as pa
    ctx = pa.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"tool": "tools/solve_bench.py", "version": pa.load_library().pdh_version().decode(),
           "device": torch.cuda.get_device_name(0), "cases": []}
    for basis, diag_first in (("dgq", True), ("dgq", False), ("dgp", True)):
        rec, ah = run_case(pa, torch, ctx, args.cells, basis, diag_first, args.reps)
        out["cases"].append(rec)
        print(json.dumps(rec), flush=True)
        if basis == "dgq" and diag_first and not args.no_solve:
            out["full_solve"] = full_solve(pa, torch, ctx, ah.n_dofs)
            print(json.dumps(out["full_solve"]), flush=True)
        del ah
    ctx.close()
    doc = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
