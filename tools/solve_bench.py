"""Timing of the solver kernels on the resident matrix (csrc/pdh_solve.hip): pdh_vmult_device, the block-inverse set-up and one
block-Jacobi CG iteration on the headline problem (3-D FE_DGQ(3), 64^3 cells in 32 768 polytopes of 2^3, both row layouts) and on
FE_AggloDGP(3) of the same mesh; then a full headline solve.  bench.py is not involved.

Times are HIP events on the library's stream (the context runs on torch's current stream), median of --reps launches after a warm-up.
Rates are over the bytes the kernel must read: the values (vmult), the values + the inverse blocks (one CG iteration), and the fraction
of the 8 TB/s HBM figure.  One CG iteration = (time of a solve with max_iter = k + m - time with max_iter = k) / m, host stop test
included.

Chebyshev section (--chebyshev; pdh_setup_chebyshev), in the same process and on the same resident matrices as the figures above, so
that the two can be compared: k_cheb_update alone (a degree-1 application from a zero start is exactly one launch of it), one degree-5
application (4 k_vmult + 5 updates, HIP events), the set-up with the inner build and the eigenvalue estimate apart, and full solves of
b = A x* with block Jacobi and with Chebyshev of degree 2, 3 and 5: iterations, products with A and seconds.  The condition checked
(field cheb5_within_bound): a degree-m application takes no longer than m x 1.10 block-Jacobi CG iterations measured here.
Prints one JSON document (and writes it to --out)."""
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


def chebyshev_case(pa, torch, ctx, N, rec, reps, solves):
    """the Chebyshev figures of the resident matrix; rec: the record of run_case (its CG iteration is the yardstick)"""
    x = torch.rand(N, dtype=torch.float64, device="cuda")
    z = torch.empty(N, dtype=torch.float64, device="cuda")
    out = {"element": rec["element"], "layout": rec["layout"]}
    inner = event_times_ms(torch, lambda: ctx.setup_preconditioner("block_jacobi"), max(3, reps // 3))
    t = []
    for _ in range(max(3, reps // 3) + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = ctx.setup_chebyshev("block_jacobi", degree=5)
        t.append((time.perf_counter() - t0) * 1e3)
    out.update(setup_inner_ms_median=median(inner), setup_total_ms_median=median(t[1:]), setup_estimate_ms=median(t[1:]) - median(inner),
               estimate=info["estimate"], estimate_cg_steps=info["cg_iterations"])
    est = info["estimate"]
    for m in (1, 5):
        ctx.setup_chebyshev("block_jacobi", degree=m, max_eigenvalue=est)
        tm = event_times_ms(torch, lambda: ctx.precondition_device(x.data_ptr(), z.data_ptr()), reps)
        out["cheb_update_ms_median" if m == 1 else "cheb5_application_ms_median"] = median(tm)
        out["cheb_update_ms_min" if m == 1 else "cheb5_application_ms_min"] = min(tm)
    out["cg_iteration_ms_median"] = rec["cg_iteration_ms_median"]
    out["vmult_ms_median"] = rec["vmult_ms_median"]
    out["cheb5_bound_ms"] = 5 * 1.10 * rec["cg_iteration_ms_median"]
    out["cheb5_over_cg_iteration"] = out["cheb5_application_ms_median"] / rec["cg_iteration_ms_median"]
    out["cheb5_within_bound"] = bool(out["cheb5_application_ms_median"] <= out["cheb5_bound_ms"])
    if solves:
        gen = torch.Generator(device="cuda").manual_seed(1)
        xs = torch.rand(N, dtype=torch.float64, device="cuda", generator=gen)
        b = torch.empty(N, dtype=torch.float64, device="cuda")
        ctx.vmult_device(xs.data_ptr(), b.data_ptr())
        out["solves"] = []
        for m in (0, 2, 3, 5):
            if m:
                ctx.setup_chebyshev("block_jacobi", degree=m, max_eigenvalue=est)
            else:
                ctx.setup_preconditioner("block_jacobi")
            sol = torch.zeros(N, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            si = ctx.solve_cg_device(b.data_ptr(), sol.data_ptr(), rel_tol=1e-13)
            wall = time.perf_counter() - t0
            its = si["iterations"]
            out["solves"].append({"preconditioner": "Chebyshev(%d) over block Jacobi" % m if m else "block Jacobi", "iterations": its,
                                  "products_with_A": 1 + its * max(m, 1), "wall_s": wall, "residual": si["residual"],
                                  "rel_error_vs_x_star": float(torch.linalg.norm(sol - xs) / torch.linalg.norm(xs))})
    return out


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
    ap.add_argument("--chebyshev", action="store_true", help="add the Chebyshev section (FE_DGQ(3) diag_first and FE_AggloDGP(3))")
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
        if args.chebyshev and diag_first:
            ch = chebyshev_case(pa, torch, ctx, ah.n_dofs, rec, args.reps, not args.no_solve)
            out.setdefault("chebyshev", []).append(ch)
            print(json.dumps(ch), flush=True)
        del ah
    ctx.close()
    doc = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
