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

Transfer section (--transfer, alone: nothing of the above runs; pdh_transfer_create), written to profiles/r08_transfer.json unless --out
says otherwise: the headline level pair (64^3 cells, FE_DGQ(3), polytopes of 2^3 under polytopes of 4^3) and the FE_DGQ(2) pair of the same
mesh, each level assembled in a context of its own.  prolongate, restrict and residual by HIP events, one two_grid_cycle_device
(Chebyshev(3) over block Jacobi, block-Jacobi CG to 1e-13 on the coarse level) by wall time since it synchronises inside; the bytes
each call must move (vectors + 1-D tables + index arrays; residual: the values + three vectors) and the resulting GB/s.  The one
condition (field transfer_pair_under_cheb_update): prolongate + restrict together take less than one k_cheb_update on the fine level,
measured in the same process.

V-cycle section (--vcycle, alone; pdh_setup_direct, pdh_mg_create), written to profiles/r09_vcycle.json unless --out says otherwise: the
hierarchy of the headline mesh (64^3 cells, FE_DGQ(3), polytopes of 32^3, 16^3, 8^3, 4^3 and 2^3 cells: 8 .. 32 768 polytopes, a coarsest
level of 512 rows) built by levels.multigrid_hierarchy, every level resident in a context of its own.  (a) pdh_setup_direct on the
coarsest level (wall time, it synchronises) and k_dense_symv alone (HIP events); (b) one V-cycle at smoother degree 3 and the same
launches restricted to the finest level (pre-smoothing from zero, residual, post-smoothing), both by HIP events in the same process -
their difference is what the coarser levels cost; (c) the solve b = A x*, rel_tol 1e-13, with block Jacobi and with the V-cycle at
smoother degrees 2, 3 and 5: iterations, products with the finest A, seconds.  No condition is checked: the table is the result.

Galerkin section (--vcycle --galerkin, alone; pdh_galerkin_device), written to profiles/r11_galerkin.json unless --out says otherwise, on
the hierarchy of the V-cycle section, ONE process, HIP events, medians of --reps: k_galerkin per level pair and summed, k_vmult of the finest
matrix (the yardstick: it reads the same bytes once), wall time of the whole Galerkin set-up - first call with the plans, and later calls -
against assembling the coarser levels, and the headline V-cycle solve on the Galerkin and on the assembled hierarchy, alternating twice each.

Single-precision smoother section (--vcycle --smoother-f32, or --chebyshev --smoother-f32, alone; pdh_set_smoother_precision), written to
profiles/r10_smoother_f32.json unless --out says otherwise (the --chebyshev form writes only where --out says).  Everything in ONE process,
the F64 path measured there being the yardstick: k_vmult against k_vmult_f32 on the finest matrix, alternating, in ms and in TB/s of the
bytes each must move (values, the gathered x, the index arrays, y); the shadow's bytes and its set-up time next to the block-inverse
set-up; one V-cycle with either precision; and the solve b = A x*, rel_tol 1e-13, F64 and F32 alternating, twice each.  Two conditions
(fields f32_solve_faster_beyond_spread, f32_vmult_faster_beyond_spread): the F32 solve and the F32 product are faster than the F64 ones by
more than the spread between the two F64 repeats.

Matrix-free section (--vcycle --matrix-free, alone, combinable with --smoother-f32; pdh_setup_matrix_free, pdh_set_smoother_operator), written
to profiles/r12_matrix_free.json unless --out says otherwise, on the hierarchy of the V-cycle section, ONE process, HIP events, medians of
--reps, the stored path measured there being the yardstick: per level whether the tables are granted, their bytes and the wall time of
the set-up; k_vmult, k_vmult_f32 and k_mf_vmult on the finest level, alternating twice each; one V-cycle and the solve b = A x*, rel_tol
1e-13, with the stored and the matrix-free smoother operator alternating twice each (and once each over F32 inverses with
--smoother-f32); the stored and the matrix-free product on FE_AggloDGP(3) and on grown agglomerates of the same cells.  Conditions (fields
mf_faster_than_stored_beyond_spread, same_iterations_within_one, matrix_free_solve_not_slower); mf_faster_than_f32 is recorded either way.

p-multigrid section (--p-vcycle, alone; pdh_ptransfer_create, levels.p_multigrid_hierarchy), written to profiles/r13_p_multigrid.json
unless --out says otherwise, ONE process, HIP events, medians of --reps: (a) prolongate + restrict of the p-pairs FE_DGQ 2 -> 3 and
FE_AggloDGP 2 -> 3 on the headline polytopes next to one k_cheb_update of their fine level (field transfer_pair_under_cheb_update, the
condition of the transfer section; the h-pair of profiles/r08_transfer.json is recorded beside it); (b) the headline solve with the
h-hierarchy of FE_DGQ(3) and with "FE_DGQ(1) on polytopes of 32^3 .. 2^3 cells, then FE_DGQ(2) and FE_DGQ(3) on the 2^3 polytopes":
iterations, ms per cycle, seconds, bytes of the level matrices; (c) FE_DGQ(3) on grown agglomerates of about 2^3 cells, which have no
nested hierarchy: block-Jacobi CG against the p-V-cycle over the degrees 1 -> 2 -> 3 with a Chebyshev coarsest level.  (b) and (c) are
reports: no condition is checked.
Distributed section (--distributed W, alone; pdh_halo_setup, pdh_dcg_*), written to profiles/r15_distributed_cg.json unless --out says
otherwise: the headline problem split by partition.balanced_row_splits into W rank-local contexts on ONE device, solved in lock-step
(polydeal_amd/distributed.py).  Per iteration the halo pack, the interior and the boundary product, the fused update and the whole step,
as wall times between stream synchronisations summed over the ranks (one device runs them one after the other); with W = 1 next to
pdh_solve_cg_device on the same problem in the same process.  A report: no time is a condition.  One device playing W ranks shows neither
the overlap of the interior product with the halo move nor an interconnect - there is no multi-GPU node to measure them on.
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


def transfer_case(pa, torch, cells, p, reps):
    """one level pair: fine polytopes of 2^3 cells under coarse ones of 4^3, each level resident in its own context"""
    from polydeal_amd.handler import transfer_description
    from polydeal_amd._capi import Transfer
    from polydeal_amd.levels import two_grid_cycle_device

    t0 = time.time()
    grid = pa.BackgroundGrid.hyper_cube_refined(3, 0.0, 1.0, cells.bit_length() - 1)
    fe = pa.FE_DGQ(3, p)
    levels, ctxs = [], []
    for block in (4, 2):
        ah = pa.AgglomerationHandler(grid)
        ah.define_block_agglomerates(block)
        ah.initialize_fe_values(p + 1, p + 1)
        ah.distribute_agglomerated_dofs(fe)
        ctx = pa.Context(0)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_problem(ah.flatten(pa.SipVariant.poisson_example(fe), False, False))
        ctx.assemble_device()
        levels.append(ah)
        ctxs.append(ctx)
    (coarse, fine), (ctx_c, ctx_f) = levels, ctxs
    desc = transfer_description(coarse, fine)
    tr = Transfer(ctx_f, desc)
    Nf, Nc, n = fine.n_dofs, coarse.n_dofs, fe.n_dofs_per_cell
    vec = lambda N: torch.rand(N, dtype=torch.float64, device="cuda")
    xc, rf, xf, bf, yc = vec(Nc), vec(Nf), vec(Nf), vec(Nf), vec(Nc)
    ctx_f.synchronize()
    pro = event_times_ms(torch, lambda: tr.prolongate_device(xc.data_ptr(), xf.data_ptr()), reps)
    res = event_times_ms(torch, lambda: tr.restrict_device(rf.data_ptr(), yc.data_ptr()), reps)
    rsd = event_times_ms(torch, lambda: ctx_f.residual_device(bf.data_ptr(), xf.data_ptr(), rf.data_ptr()), reps)
    est = ctx_f.setup_chebyshev("block_jacobi", degree=1)["estimate"]
    upd = event_times_ms(torch, lambda: ctx_f.precondition_device(bf.data_ptr(), xf.data_ptr()), reps)  # one k_cheb_update
    ctx_f.setup_chebyshev("block_jacobi", degree=3, max_eigenvalue=est)
    ctx_c.setup_preconditioner("block_jacobi")
    b, x, r = vec(Nf), torch.zeros(Nf, dtype=torch.float64, device="cuda"), torch.empty(Nf, dtype=torch.float64, device="cuda")
    rc, ec = torch.empty(Nc, dtype=torch.float64, device="cuda"), torch.empty(Nc, dtype=torch.float64, device="cuda")
    cyc, coarse_its = [], []
    for _ in range(max(3, reps // 3) + 1):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        info = two_grid_cycle_device(ctx_f, ctx_c, tr, b.data_ptr(), x.data_ptr(), r.data_ptr(), rc.data_ptr(), ec.data_ptr())
        torch.cuda.synchronize()
        cyc.append((time.perf_counter() - w0) * 1e3)
        coarse_its.append(info["iterations"])
    tab_bytes = 8.0 * desc.n_fine * 3 * (p + 1) ** 2
    idx_bytes = 4.0 * (3 * desc.n_fine + 2 * desc.n_coarse + 1)  # parent, child_idx, fine_off; child_ptr, coarse_off
    vec_bytes = 8.0 * (Nf + Nc)
    moved = vec_bytes + tab_bytes + idx_bytes
    res_bytes = 8.0 * (ctx_f.stats()["n_values"] + 3 * Nf)
    upd_bytes = 8.0 * (desc.n_fine * n * n + 4 * Nf)  # the inverse blocks; b in, r, d, x out
    rec = {
        "element": "FE_DGQ(%d)" % p, "cells_per_axis": cells, "fine_polytopes": desc.n_fine, "coarse_polytopes": desc.n_coarse,
        "fine_dofs": Nf, "coarse_dofs": Nc, "dofs_per_polytope": n,
        "prolongate_ms_median": median(pro), "prolongate_ms_min": min(pro), "restrict_ms_median": median(res), "restrict_ms_min": min(res),
        "transfer_bytes": moved, "transfer_table_bytes": tab_bytes,
        "prolongate_GBps": moved / (median(pro) * 1e-3) / 1e9, "restrict_GBps": moved / (median(res) * 1e-3) / 1e9,
        "residual_ms_median": median(rsd), "residual_bytes": res_bytes, "residual_GBps": res_bytes / (median(rsd) * 1e-3) / 1e9,
        "cheb_update_ms_median": median(upd), "cheb_update_bytes": upd_bytes, "cheb_update_GBps": upd_bytes / (median(upd) * 1e-3) / 1e9,
        "transfer_pair_ms": median(pro) + median(res),
        "transfer_pair_under_cheb_update": bool(median(pro) + median(res) < median(upd)),
        "two_grid_cycle_wall_ms_median": median(cyc[1:]), "two_grid_coarse_cg_iterations": coarse_its[1:],
        "launches": len(pro), "case_wall_s": time.time() - t0,
    }
    tr.close()
    ctx_f.close()
    ctx_c.close()
    return rec


def vcycle_case(pa, torch, cells, reps):
    """the V-cycle figures: see the module docstring"""
    from polydeal_amd._capi import Multigrid
    from polydeal_amd.levels import block_hierarchy, multigrid_hierarchy

    t0 = time.time()
    grid = pa.BackgroundGrid.hyper_cube_refined(3, 0.0, 1.0, cells.bit_length() - 1)
    fe = pa.FE_DGQ(3, 3)
    blocks = [b for b in (32, 16, 8, 4, 2) if 2 * b <= cells]
    handlers = block_hierarchy(grid, fe, blocks)
    print("handlers of %d levels: %.1f s" % (len(blocks), time.time() - t0), flush=True)
    hier = multigrid_hierarchy(handlers, fe, pa.SipVariant.poisson_example(fe), diag_first=True, degree=3)
    print("hierarchy resident: %.1f s" % (time.time() - t0), flush=True)
    stream = torch.cuda.current_stream().cuda_stream
    for c in hier.contexts:
        c.set_stream(stream)
    fin, coarse = hier.finest, hier.contexts[0]
    N, Nc = handlers[-1].n_dofs, handlers[0].n_dofs
    vec = lambda n: torch.rand(n, dtype=torch.float64, device="cuda")
    values = [c.stats()["n_values"] for c in hier.contexts]
    est = [i.get("estimate") for i in hier.info]
    out = {"element": "FE_DGQ(3)", "cells_per_axis": cells, "blocks": blocks, "polytopes": [h.n_agglomerates for h in handlers],
           "rows": [h.n_dofs for h in handlers], "n_values": values, "level_matrix_bytes": 8.0 * sum(values),
           "coarser_levels_over_finest_bytes": sum(values[:-1]) / values[-1]}
    # (a) the direct solve of the coarsest level
    hier.mg.close()
    hier.mg = None
    t = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        info = coarse.setup_direct()
        t.append((time.perf_counter() - w0) * 1e3)
    rc, zc = vec(Nc), vec(Nc)
    sy = event_times_ms(torch, lambda: coarse.precondition_device(rc.data_ptr(), zc.data_ptr()), reps)
    out.update(direct_rows=Nc, direct_setup_wall_ms_median=median(t[1:]), direct_setup_wall_ms_min=min(t[1:]), direct_pivot_min=info["pivot_min"],
               direct_pivot_max=info["pivot_max"], dense_symv_ms_median=median(sy), dense_symv_ms_min=min(sy),
               dense_symv_GBps=8.0 * Nc * Nc / (median(sy) * 1e-3) / 1e9)
    # (b) one cycle at degree 3 against its finest-level launches alone (the finest context still has Chebyshev(3): the mg is closed)
    b, x, r = vec(N), vec(N), vec(N)

    def finest_only():
        fin.chebyshev_step_device(b.data_ptr(), x.data_ptr(), True)
        fin.residual_device(b.data_ptr(), x.data_ptr(), r.data_ptr())
        fin.chebyshev_step_device(b.data_ptr(), x.data_ptr(), False)
    fin.setup_chebyshev("block_jacobi", degree=3, max_eigenvalue=est[-1])
    fo = event_times_ms(torch, finest_only, reps)
    mg = Multigrid(hier.contexts, hier.transfers)
    cy = event_times_ms(torch, lambda: mg.vcycle_device(b.data_ptr(), x.data_ptr(), True), reps)
    out.update(vcycle3_ms_median=median(cy), vcycle3_ms_min=min(cy), finest_level_only_ms_median=median(fo), finest_level_only_ms_min=min(fo),
               coarser_levels_ms=median(cy) - median(fo), coarser_levels_over_finest_time=(median(cy) - median(fo)) / median(fo))
    # (c) the solves
    gen = torch.Generator(device="cuda").manual_seed(1)
    xs = torch.rand(N, dtype=torch.float64, device="cuda", generator=gen)
    rhs = torch.empty(N, dtype=torch.float64, device="cuda")
    fin.vmult_device(xs.data_ptr(), rhs.data_ptr())
    out["solves"] = []
    for m in (0, 2, 3, 5):
        if mg is not None:
            mg.close()
            mg = None
        if m:
            for c, e in zip(hier.contexts[1:], est[1:]):
                c.setup_chebyshev("block_jacobi", degree=m, max_eigenvalue=e)
            mg = Multigrid(hier.contexts, hier.transfers)
        else:
            fin.setup_preconditioner("block_jacobi")
        sol = torch.zeros(N, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        si = fin.solve_cg_device(rhs.data_ptr(), sol.data_ptr(), rel_tol=1e-13)
        wall = time.perf_counter() - w0
        its = si["iterations"]
        out["solves"].append({"preconditioner": "V-cycle, Chebyshev(%d) over block Jacobi, direct coarse solve" % m if m else "block Jacobi",
                              "iterations": its, "products_with_finest_A": 1 + (its + 1) * 2 * m + its if m else 1 + its, "wall_s": wall,
                              "ms_per_iteration": wall / max(its, 1) * 1e3, "residual": si["residual"],
                              "rel_error_vs_x_star": float(torch.linalg.norm(sol - xs) / torch.linalg.norm(xs))})
        print(json.dumps(out["solves"][-1]), flush=True)
    bj = out["solves"][0]["wall_s"]
    for srec in out["solves"]:
        srec["wall_over_block_jacobi"] = srec["wall_s"] / bj
    out["case_wall_s"] = time.time() - t0
    hier.mg = mg
    hier.close()
    return out


def galerkin_case(pa, torch, cells, reps):
    """the Galerkin figures: see the module docstring"""
    from polydeal_amd._capi import Multigrid
    from polydeal_amd.levels import block_hierarchy, multigrid_hierarchy

    t0 = time.time()
    grid = pa.BackgroundGrid.hyper_cube_refined(3, 0.0, 1.0, cells.bit_length() - 1)
    fe = pa.FE_DGQ(3, 3)
    blocks = [b for b in (32, 16, 8, 4, 2) if 2 * b <= cells]
    handlers = block_hierarchy(grid, fe, blocks)
    w0 = time.perf_counter()
    hier = multigrid_hierarchy(handlers, fe, pa.SipVariant.poisson_example(fe), diag_first=True, degree=3)
    set_up_wall = time.perf_counter() - w0
    stream = torch.cuda.current_stream().cuda_stream
    for c in hier.contexts:
        c.set_stream(stream)
    ctxs, trs, fin = hier.contexts, hier.transfers, hier.finest
    hier.mg.close()
    hier.mg = None
    N = handlers[-1].n_dofs
    values = [c.stats()["n_values"] for c in ctxs]
    out = {"element": "FE_DGQ(3)", "cells_per_axis": cells, "blocks": blocks, "polytopes": [h.n_agglomerates for h in handlers],
           "rows": [h.n_dofs for h in handlers], "n_values": values, "assembled_hierarchy_set_up_wall_s": set_up_wall,
           "note": "the coarse contexts go through pdh_set_problem like any other: their assembly set-up (points, tables, launches) is "
                   "paid inside assembled_hierarchy_set_up_wall_s and is not used by the Galerkin product"}

    def wall_ms(fn):
        torch.cuda.synchronize()
        w = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - w) * 1e3

    def galerkin_all():
        for l in range(len(ctxs) - 1, 0, -1):
            trs[l - 1].galerkin_device(ctxs[l - 1])

    def assemble_coarser():
        for c in ctxs[:-1]:
            c.assemble_device()
    # (a) wall time of the set-up: the first round builds the plans, the later ones find them on the transfers
    first = wall_ms(galerkin_all)
    later = [wall_ms(galerkin_all) for _ in range(reps)]
    asm = [wall_ms(assemble_coarser) for _ in range(reps + 1)][1:]
    out.update(galerkin_set_up_wall_ms_first_call_with_plans=first, galerkin_set_up_wall_ms_median=median(later),
               assemble_coarser_levels_wall_ms_median=median(asm))
    # (b) the kernel per pair (events round the call: one kernel on the stream) and k_vmult of the finest matrix in the same process
    x, y = torch.rand(N, dtype=torch.float64, device="cuda"), torch.empty(N, dtype=torch.float64, device="cuda")
    vm = event_times_ms(torch, lambda: fin.vmult_device(x.data_ptr(), y.data_ptr()), reps)
    galerkin_all()  # every level holds the product of the level above, as in the set-up
    pairs = []
    for l in range(len(ctxs) - 1, 0, -1):
        t = event_times_ms(torch, lambda: trs[l - 1].galerkin_device(ctxs[l - 1]), reps)
        pairs.append({"fine_polytopes": handlers[l].n_agglomerates, "coarse_polytopes": handlers[l - 1].n_agglomerates,
                      "fine_bytes": 8.0 * values[l], "k_galerkin_ms_median": median(t), "k_galerkin_ms_min": min(t),
                      "fine_read_TBps": 8.0 * values[l] / (median(t) * 1e-3) / 1e12})
    vm2 = event_times_ms(torch, lambda: fin.vmult_device(x.data_ptr(), y.data_ptr()), reps)
    k_vm = median(vm + vm2)
    out.update(pairs=pairs, k_vmult_finest_ms_median=k_vm, k_galerkin_finest_pair_ms_median=pairs[0]["k_galerkin_ms_median"],
               k_galerkin_all_pairs_ms=sum(p["k_galerkin_ms_median"] for p in pairs),
               k_galerkin_finest_pair_over_k_vmult=pairs[0]["k_galerkin_ms_median"] / k_vm, expected_ratio_at_most=4.0)
    # (c) the headline V-cycle solve, Galerkin against assembled hierarchy, alternating twice each
    gen = torch.Generator(device="cuda").manual_seed(1)
    xs = torch.rand(N, dtype=torch.float64, device="cuda", generator=gen)
    rhs = torch.empty(N, dtype=torch.float64, device="cuda")
    fin.vmult_device(xs.data_ptr(), rhs.data_ptr())
    out["solves"] = []
    for kind in ("galerkin", "assembled", "galerkin", "assembled"):
        galerkin_all() if kind == "galerkin" else assemble_coarser()
        for l, c in enumerate(ctxs):
            c.setup_direct() if l == 0 else c.setup_chebyshev("block_jacobi", degree=3)
        mg = Multigrid(ctxs, trs)
        sol = torch.zeros(N, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        w = time.perf_counter()
        si = fin.solve_cg_device(rhs.data_ptr(), sol.data_ptr(), rel_tol=1e-13)
        wall = time.perf_counter() - w
        its = si["iterations"]
        out["solves"].append({"coarse_operators": kind, "iterations": its, "products_with_finest_A": 1 + (its + 1) * 2 * 3 + its,
                              "wall_s": wall, "residual": si["residual"],
                              "rel_error_vs_x_star": float(torch.linalg.norm(sol - xs) / torch.linalg.norm(xs))})
        print(json.dumps(out["solves"][-1]), flush=True)
        mg.close()
    out["case_wall_s"] = time.time() - t0
    hier.close()
    return out


def vmult_bytes(st, n, N, f32):
    """what one product must move: the values, the x gathered per slot (row_len doubles), blk_dof per block and the per-slot arrays
    (row_base, row_len, diag_L, own_row, blk_ptr; the shadow adds its base), and y"""
    nv, slots = st["n_values"], st["n_owned_agg"]
    per_slot = 8 + 4 + 4 + 4 + 8 + (8 if f32 else 0)
    return (4.0 if f32 else 8.0) * nv + 8.0 * nv / n + 4.0 * nv / (n * n) + per_slot * slots + 8.0 * N


def smoother_f32_case(pa, torch, cells, reps, vcycle):
    """the single-precision smoother figures: see the module docstring"""
    from polydeal_amd._capi import Multigrid
    from polydeal_amd.levels import block_hierarchy, multigrid_hierarchy

    t0 = time.time()
    grid = pa.BackgroundGrid.hyper_cube_refined(3, 0.0, 1.0, cells.bit_length() - 1)
    fe = pa.FE_DGQ(3, 3)
    n = fe.n_dofs_per_cell
    degree = 3 if vcycle else 5
    stream = torch.cuda.current_stream().cuda_stream
    if vcycle:  # the hierarchy of the V-cycle section
        handlers = block_hierarchy(grid, fe, [b for b in (32, 16, 8, 4, 2) if 2 * b <= cells])
        hier = multigrid_hierarchy(handlers, fe, pa.SipVariant.poisson_example(fe), diag_first=True, degree=degree)
        contexts, transfers, info, first_mg = hier.contexts, hier.transfers, hier.info, hier.mg
        hier.mg = None
        N = handlers[-1].n_dofs
    else:  # the headline level alone, Chebyshev(5) over block Jacobi as its preconditioner
        ah, _ = handler(pa, cells, "dgq")
        ctx = pa.Context(0)
        ctx.set_problem(ah.flatten(pa.SipVariant.poisson_example(fe), True, False))
        ctx.assemble_device()
        contexts, transfers, info, first_mg = [ctx], [], [ctx.setup_chebyshev("block_jacobi", degree=degree)], None
        N = ah.n_dofs
    for c in contexts:
        c.set_stream(stream)
    fin = contexts[-1]
    est = [i.get("estimate") for i in info]
    stats = [c.stats() for c in contexts]
    out = {"element": "FE_DGQ(3)", "cells_per_axis": cells, "preconditioner": "V-cycle" if vcycle else "Chebyshev", "smoother_degree": degree,
           "rows": [c.n_rows for c in contexts], "n_values_finest": stats[-1]["n_values"]}
    smooth = list(range(1, len(contexts))) if vcycle else [0]
    state = {"mg": first_mg}

    def remake(prec):
        """every smoother level set up again with its own estimate (F64), then `prec`; the V-cycle attached again"""
        if state["mg"] is not None:
            state["mg"].close()
            state["mg"] = None
        for l in smooth:
            contexts[l].setup_chebyshev("block_jacobi", degree=degree, max_eigenvalue=est[l])
            if prec == "f32":
                contexts[l].set_smoother_precision("f32")
        if vcycle:
            state["mg"] = Multigrid(contexts, transfers)
    try:
        # the shadow: bytes and set-up time (the first call allocates; the later ones convert only), next to the block-inverse set-up
        if state["mg"] is not None:
            state["mg"].close()
            state["mg"] = None
        inv = event_times_ms(torch, lambda: fin.setup_preconditioner("block_jacobi"), reps)
        fin.setup_chebyshev("block_jacobi", degree=degree, max_eigenvalue=est[-1])
        t = []
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            fin.set_smoother_precision("f32")
            torch.cuda.synchronize()
            t.append((time.perf_counter() - w0) * 1e3)
        sh_rows = [4.0 * st["n_values"] for st in stats]  # (n = 64: every row length is even, no pad entries)
        sh_inv = [4.0 * st["n_owned_agg"] * n * n for st in stats]
        lv = smooth
        out.update(shadow_rows_bytes_finest=sh_rows[-1], shadow_inverse_bytes_finest=sh_inv[-1],
                   shadow_bytes_all_smoother_levels=sum(sh_rows[l] + sh_inv[l] for l in lv),
                   shadow_setup_first_wall_ms=t[0], shadow_setup_wall_ms_median=median(t[1:]), shadow_setup_wall_ms_min=min(t[1:]),
                   shadow_setup_GBps=(12.0 * stats[-1]["n_values"] + 12.0 * stats[-1]["n_owned_agg"] * n * n) / (median(t[1:]) * 1e-3) / 1e9,
                   block_inverse_setup_ms_median=median(inv))
        # the two products, alternating (F32 is in force on the finest context; pdh_vmult_device keeps reading the doubles)
        x = torch.rand(N, dtype=torch.float64, device="cuda")
        y = torch.empty(N, dtype=torch.float64, device="cuda")
        f64 = lambda: fin.vmult_device(x.data_ptr(), y.data_ptr())
        f32 = lambda: fin.smoother_vmult_device(x.data_ptr(), y.data_ptr())
        vm = {"f64": [], "f32": []}
        for _ in range(2):
            vm["f64"].append(event_times_ms(torch, f64, reps))
            vm["f32"].append(event_times_ms(torch, f32, reps))
        b64, b32 = vmult_bytes(stats[-1], n, N, False), vmult_bytes(stats[-1], n, N, True)
        m64, m32 = [median(v) for v in vm["f64"]], [median(v) for v in vm["f32"]]
        spread = abs(m64[0] - m64[1])
        out.update(vmult_ms_medians=m64, vmult_f32_ms_medians=m32, vmult_ms_min=min(map(min, vm["f64"])), vmult_f32_ms_min=min(map(min, vm["f32"])),
                   vmult_bytes=b64, vmult_f32_bytes=b32, vmult_TBps=b64 / (median(m64) * 1e-3) / 1e12,
                   vmult_f32_TBps=b32 / (median(m32) * 1e-3) / 1e12, vmult_spread_ms=spread, vmult_f32_speedup=median(m64) / median(m32),
                   f32_vmult_faster_beyond_spread=bool(min(m64) - max(m32) > spread))
        print(json.dumps({k: out[k] for k in ("vmult_ms_medians", "vmult_f32_ms_medians", "vmult_TBps", "vmult_f32_TBps")}), flush=True)
        # one application of the preconditioner with either precision
        r, z = torch.rand(N, dtype=torch.float64, device="cuda"), torch.empty(N, dtype=torch.float64, device="cuda")
        for prec in ("f64", "f32"):
            remake(prec)
            ap = event_times_ms(torch, lambda: fin.precondition_device(r.data_ptr(), z.data_ptr()), reps)
            out["application_%s_ms_median" % prec], out["application_%s_ms_min" % prec] = median(ap), min(ap)
        # the solves, alternating
        gen = torch.Generator(device="cuda").manual_seed(1)
        xs = torch.rand(N, dtype=torch.float64, device="cuda", generator=gen)
        rhs = torch.empty(N, dtype=torch.float64, device="cuda")
        fin.vmult_device(xs.data_ptr(), rhs.data_ptr())
        out["solves"] = []
        per_it = 2 * degree if vcycle else degree - 1  # products of one application with the smoother's matrix
        for prec in ("f64", "f32", "f64", "f32"):
            remake(prec)
            sol = torch.zeros(N, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            si = fin.solve_cg_device(rhs.data_ptr(), sol.data_ptr(), rel_tol=1e-13)
            wall = time.perf_counter() - w0
            its = si["iterations"]
            res = torch.empty(N, dtype=torch.float64, device="cuda")
            fin.residual_device(rhs.data_ptr(), sol.data_ptr(), res.data_ptr())
            out["solves"].append({"smoother_precision": prec, "iterations": its, "products_with_A_double": 1 + its,
                                  "products_with_the_smoother_matrix": (its + 1) * per_it, "wall_s": wall,
                                  "ms_per_iteration": wall / max(its, 1) * 1e3, "residual": si["residual"],
                                  "true_relative_residual": float(torch.linalg.norm(res) / torch.linalg.norm(rhs)),
                                  "rel_error_vs_x_star": float(torch.linalg.norm(sol - xs) / torch.linalg.norm(xs))})
            print(json.dumps(out["solves"][-1]), flush=True)
        w64 = [s_["wall_s"] for s_ in out["solves"] if s_["smoother_precision"] == "f64"]
        w32 = [s_["wall_s"] for s_ in out["solves"] if s_["smoother_precision"] == "f32"]
        out.update(solve_f64_wall_s=w64, solve_f32_wall_s=w32, solve_f64_spread_s=abs(w64[0] - w64[1]),
                   solve_f32_speedup=median(w64) / median(w32),
                   f32_solve_faster_beyond_spread=bool(min(w64) - max(w32) > abs(w64[0] - w64[1])))
    finally:
        if state["mg"] is not None:
            state["mg"].close()
        for t_ in transfers:
            t_.close()
        for c in contexts:
            c.close()
    out["case_wall_s"] = time.time() - t0
    return out


def matrix_free_case(pa, torch, cells, reps, with_f32):
    """the matrix-free smoother-operator figures: see the module docstring"""
    from polydeal_amd._capi import Multigrid
    from polydeal_amd.levels import block_hierarchy, multigrid_hierarchy

    t0 = time.time()
    grid = pa.BackgroundGrid.hyper_cube_refined(3, 0.0, 1.0, cells.bit_length() - 1)
    fe = pa.FE_DGQ(3, 3)
    n, degree = fe.n_dofs_per_cell, 3
    stream = torch.cuda.current_stream().cuda_stream
    handlers = block_hierarchy(grid, fe, [b for b in (32, 16, 8, 4, 2) if 2 * b <= cells])
    hier = multigrid_hierarchy(handlers, fe, pa.SipVariant.poisson_example(fe), diag_first=True, degree=degree)
    contexts, transfers, info = hier.contexts, hier.transfers, hier.info
    state = {"mg": hier.mg}
    hier.mg = None
    N = handlers[-1].n_dofs
    for c in contexts:
        c.set_stream(stream)
    fin = contexts[-1]
    est = [i.get("estimate") for i in info]
    stats = [c.stats() for c in contexts]
    smooth = list(range(1, len(contexts)))
    out = {"element": "FE_DGQ(3)", "cells_per_axis": cells, "preconditioner": "V-cycle", "smoother_degree": degree,
           "rows": [c.n_rows for c in contexts], "n_values_finest": stats[-1]["n_values"], "levels": []}

    def remake(mode):
        """every smoother level set up again with its own estimate, then the mode: operator and precision; the V-cycle attached again"""
        if state["mg"] is not None:
            state["mg"].close()
            state["mg"] = None
        for l in smooth:
            contexts[l].setup_chebyshev("block_jacobi", degree=degree, max_eigenvalue=est[l])
            if mode.endswith("f32"):
                contexts[l].set_smoother_precision("f32")
            if mode.startswith("matrix_free") and granted[l]:
                contexts[l].set_smoother_operator("matrix_free")
        state["mg"] = Multigrid(contexts, transfers)
    try:
        # the tables: which levels are granted, their bytes, the wall time of the set-up (it synchronises)
        granted = [False] * len(contexts)
        for l in smooth:
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            try:
                mf = contexts[l].setup_matrix_free()
                granted[l] = True
            except pa.PdhError as e:
                if e.code != pa._capi.PDH_EUNSUPPORTED:
                    raise
                mf = {"refused": str(e)}
            torch.cuda.synchronize()
            out["levels"].append(dict(mf, level=l, rows=contexts[l].n_rows, values_bytes=8.0 * stats[l]["n_values"],
                                      setup_matrix_free_wall_ms=(time.perf_counter() - w0) * 1e3))
        out["granted_levels"] = [l for l in smooth if granted[l]]
        # the three products on the finest level, alternating, twice each (F32 is in force for the shadow's product only)
        if state["mg"] is not None:
            state["mg"].close()
            state["mg"] = None
        fin.setup_chebyshev("block_jacobi", degree=degree, max_eigenvalue=est[-1])
        fin.set_smoother_precision("f32")
        x = torch.rand(N, dtype=torch.float64, device="cuda")
        y = torch.empty(N, dtype=torch.float64, device="cuda")
        prods = {"k_vmult": lambda: fin.vmult_device(x.data_ptr(), y.data_ptr()),
                 "k_vmult_f32": lambda: fin.smoother_vmult_device(x.data_ptr(), y.data_ptr()),
                 "k_mf_vmult": lambda: fin.matrix_free_vmult_device(x.data_ptr(), y.data_ptr())}
        tm = {k: [] for k in prods}
        for _ in range(2):
            for k, fn in prods.items():
                tm[k].append(event_times_ms(torch, fn, reps))
        med = {k: [median(v) for v in tm[k]] for k in prods}
        spread = max(abs(med[k][0] - med[k][1]) for k in ("k_vmult", "k_mf_vmult"))
        tb = out["levels"][-1].get("table_bytes", 0)
        out["products_finest"] = {
            "ms_medians": med, "ms_min": {k: min(map(min, tm[k])) for k in prods}, "spread_ms": spread,
            "bytes": {"k_vmult": vmult_bytes(stats[-1], n, N, False), "k_vmult_f32": vmult_bytes(stats[-1], n, N, True),
                      "k_mf_vmult": tb + 8.0 * stats[-1]["n_values"] / n + 8.0 * N},
            "mf_over_stored": median(med["k_mf_vmult"]) / median(med["k_vmult"]),
            "mf_over_f32": median(med["k_mf_vmult"]) / median(med["k_vmult_f32"]),
            "mf_faster_than_stored_beyond_spread": bool(min(med["k_vmult"]) - max(med["k_mf_vmult"]) > spread),
            "mf_faster_than_f32": bool(max(med["k_mf_vmult"]) < min(med["k_vmult_f32"]))}
        print(json.dumps(out["products_finest"]), flush=True)
        # one V-cycle and the headline solve in every mode, stored and matrix-free alternating twice
        modes = ["stored", "matrix_free", "stored", "matrix_free"] + (["stored+f32", "matrix_free+f32"] if with_f32 else [])
        r, z = torch.rand(N, dtype=torch.float64, device="cuda"), torch.empty(N, dtype=torch.float64, device="cuda")
        gen = torch.Generator(device="cuda").manual_seed(1)
        xs = torch.rand(N, dtype=torch.float64, device="cuda", generator=gen)
        rhs = torch.empty(N, dtype=torch.float64, device="cuda")
        fin.vmult_device(xs.data_ptr(), rhs.data_ptr())
        out["solves"] = []
        for mode in modes:
            remake(mode)
            ap = event_times_ms(torch, lambda: fin.precondition_device(r.data_ptr(), z.data_ptr()), reps)
            sol = torch.zeros(N, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            si = fin.solve_cg_device(rhs.data_ptr(), sol.data_ptr(), rel_tol=1e-13)
            wall = time.perf_counter() - w0
            its = si["iterations"]
            res = torch.empty(N, dtype=torch.float64, device="cuda")
            fin.residual_device(rhs.data_ptr(), sol.data_ptr(), res.data_ptr())
            kind = "k_mf_vmult" if mode.startswith("matrix_free") else ("k_vmult_f32" if mode.endswith("f32") else "k_vmult")
            out["solves"].append({"mode": mode, "vcycle_ms_median": median(ap), "vcycle_ms_min": min(ap), "iterations": its,
                                  "products_finest": {"k_vmult (CG)": 1 + its, kind + " (smoother, residual)": (its + 1) * 2 * degree},
                                  "wall_s": wall, "residual": si["residual"],
                                  "true_relative_residual": float(torch.linalg.norm(res) / torch.linalg.norm(rhs)),
                                  "rel_error_vs_x_star": float(torch.linalg.norm(sol - xs) / torch.linalg.norm(xs))})
            print(json.dumps(out["solves"][-1]), flush=True)
        ws = [s_["wall_s"] for s_ in out["solves"] if s_["mode"] == "stored"]
        wm = [s_["wall_s"] for s_ in out["solves"] if s_["mode"] == "matrix_free"]
        its_s = [s_["iterations"] for s_ in out["solves"] if s_["mode"] == "stored"]
        its_m = [s_["iterations"] for s_ in out["solves"] if s_["mode"] == "matrix_free"]
        out.update(solve_stored_wall_s=ws, solve_matrix_free_wall_s=wm, solve_stored_spread_s=abs(ws[0] - ws[1]),
                   solve_matrix_free_speedup=median(ws) / median(wm),
                   same_iterations_within_one=bool(abs(its_s[0] - its_m[0]) <= 1 and abs(its_s[1] - its_m[1]) <= 1),
                   matrix_free_solve_not_slower=bool(median(wm) <= median(ws)))
    finally:
        if state["mg"] is not None:
            state["mg"].close()
        for t_ in transfers:
            t_.close()
        for c in contexts:
            c.close()
    # the same products on FE_AggloDGP(3) and on grown agglomerates of the bench cells (FE_DGQ(3)), a context each
    out["other_products"] = []
    for name in ("FE_AggloDGP(3), polytopes of 2^3", "FE_DGQ(3), grown agglomerates of 8 cells"):
        if name.startswith("FE_AggloDGP"):
            ah, fe2 = handler(pa, cells, "dgp")
        else:
            fe2 = pa.FE_DGQ(3, 3)
            ah = pa.AgglomerationHandler(grid)
            ah.define_grown_agglomerates(8, seed=cells)
            ah.initialize_fe_values(4, 4)
            ah.distribute_agglomerated_dofs(fe2)
        ctx = pa.Context(0)
        try:
            ctx.set_stream(stream)
            ctx.set_problem(ah.flatten(pa.SipVariant.poisson_example(fe2), True, False))
            rec = {"what": name, "rows": ah.n_dofs, "polytopes": ah.n_agglomerates, "rows_kernel": ctx.rows_kernel_in_use()}
            try:
                rec.update(ctx.setup_matrix_free())
            except pa.PdhError as e:
                if e.code != pa._capi.PDH_EUNSUPPORTED:
                    raise
                rec["refused"] = str(e)
            else:
                ctx.assemble_device()
                x = torch.rand(ah.n_dofs, dtype=torch.float64, device="cuda")
                y = torch.empty(ah.n_dofs, dtype=torch.float64, device="cuda")
                st = ctx.stats()
                a, b = [], []
                for _ in range(2):
                    a.append(median(event_times_ms(torch, lambda: ctx.vmult_device(x.data_ptr(), y.data_ptr()), reps)))
                    b.append(median(event_times_ms(torch, lambda: ctx.matrix_free_vmult_device(x.data_ptr(), y.data_ptr()), reps)))
                rec.update(values_bytes=8.0 * st["n_values"], k_vmult_ms_medians=a, k_mf_vmult_ms_medians=b, mf_over_stored=median(b) / median(a))
            out["other_products"].append(rec)
            print(json.dumps(rec), flush=True)
        finally:
            ctx.close()
    out["case_wall_s"] = time.time() - t0
    return out


def p_vcycle_case(pa, torch, cells, reps):
    """the p-multigrid figures (profiles/r13_p_multigrid.json), one process:
    (a) the prolongate + restrict pair of FE_DGQ 2 -> 3 and of FE_AggloDGP 2 -> 3 on the headline polytopes (2^3 cells) next to one
        k_cheb_update of the fine level, the condition the h-transfers are held to in profiles/r08_transfer.json;
    (b) the headline solve with the h-hierarchy of FE_DGQ(3) against the hierarchy "FE_DGQ(1) on polytopes of 32^3 .. 2^3 cells, then
        FE_DGQ(2) and FE_DGQ(3) on the 2^3 polytopes": iterations, ms per cycle, seconds per solve, bytes of the level matrices;
    (c) grown agglomerates of about 2^3 cells with FE_DGQ(3) (bench.py's dgq3_grown: no nested hierarchy exists): block-Jacobi CG against
        the p-V-cycle over the degrees 1 -> 2 -> 3 with a Chebyshev coarsest level."""
    from polydeal_amd._capi import PTransferDesc, Transfer
    from polydeal_amd.levels import block_hierarchy, multigrid_hierarchy, p_multigrid_hierarchy

    t0 = time.time()
    stream = torch.cuda.current_stream().cuda_stream
    grid = pa.BackgroundGrid.hyper_cube_refined(3, 0.0, 1.0, cells.bit_length() - 1)
    vec = lambda n: torch.rand(n, dtype=torch.float64, device="cuda")
    variant = pa.SipVariant.poisson_example
    out = {"cells_per_axis": cells, "pairs": []}

    def one_level(fe, block=2, grown=False):
        ah = pa.AgglomerationHandler(grid)
        if grown:
            ah.define_grown_agglomerates(block ** 3, seed=1)
        else:
            ah.define_block_agglomerates(block)
        ah.initialize_fe_values(fe.degree + 1, fe.degree + 1)
        ah.distribute_agglomerated_dofs(fe)
        return ah

    # (a)
    for mk, name in ((pa.FE_DGQ, "FE_DGQ"), (pa.FE_AggloDGP, "FE_AggloDGP")):
        fe_c, fe_f = mk(3, 2), mk(3, 3)
        ah = one_level(fe_f)
        ctx = pa.Context(0)
        ctx.set_stream(stream)
        ctx.set_problem(ah.flatten(variant(fe_f), False, False))
        ctx.assemble_device()
        nA, n_f, n_c = ah.n_agglomerates, fe_f.n_dofs_per_cell, fe_c.n_dofs_per_cell
        desc = PTransferDesc(dim=3, fine_degree=3, coarse_degree=2, basis=fe_f.basis, fine_dof_offset=[P * n_f for P in range(nA)],
                             coarse_dof_offset=[P * n_c for P in range(nA)])  # (the numbering of distribute_agglomerated_dofs)
        tr = Transfer(ctx, desc)
        Nf, Nc = desc.n_fine_rows, desc.n_coarse_rows
        xc, rf, xf, bf, yc = vec(Nc), vec(Nf), vec(Nf), vec(Nf), vec(Nc)
        ctx.synchronize()
        pro = event_times_ms(torch, lambda: tr.prolongate_device(xc.data_ptr(), xf.data_ptr()), reps)
        res = event_times_ms(torch, lambda: tr.restrict_device(rf.data_ptr(), yc.data_ptr()), reps)
        ctx.setup_chebyshev("block_jacobi", degree=1)
        upd = event_times_ms(torch, lambda: ctx.precondition_device(bf.data_ptr(), xf.data_ptr()), reps)  # one k_cheb_update
        moved = 8.0 * (Nf + Nc) + 8.0 * nA
        rec = {"pair": "%s 2 -> 3" % name, "polytopes": nA, "fine_dofs": Nf, "coarse_dofs": Nc, "fine_dofs_per_polytope": n_f,
               "prolongate_ms_median": median(pro), "prolongate_ms_min": min(pro), "restrict_ms_median": median(res),
               "restrict_ms_min": min(res), "transfer_bytes": moved, "prolongate_GBps": moved / (median(pro) * 1e-3) / 1e9,
               "restrict_GBps": moved / (median(res) * 1e-3) / 1e9, "cheb_update_ms_median": median(upd),
               "transfer_pair_ms": median(pro) + median(res), "h_pair_ms_at_FE_DGQ3_r08": 0.087,
               "transfer_pair_under_cheb_update": bool(median(pro) + median(res) < median(upd))}
        out["pairs"].append(rec)
        print(json.dumps(rec), flush=True)
        tr.close()
        ctx.close()
        del ah

    def solve(hier, label, handlers):
        for c in hier.contexts:
            c.set_stream(stream)
        fin, N = hier.finest, handlers[-1].n_dofs
        values = [c.stats()["n_values"] for c in hier.contexts]
        b, x = vec(N), vec(N)
        cy = event_times_ms(torch, lambda: hier.vcycle_device(b.data_ptr(), x.data_ptr(), True), reps)
        xs = torch.rand(N, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        rhs, sol = torch.empty(N, dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.float64, device="cuda")
        fin.vmult_device(xs.data_ptr(), rhs.data_ptr())
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        si = hier.solve_cg_device(rhs.data_ptr(), sol.data_ptr(), rel_tol=1e-13)
        wall = time.perf_counter() - w0
        rec = {"hierarchy": label, "rows": [h.n_dofs for h in handlers], "polytopes": [h.n_agglomerates for h in handlers],
               "coarsest": "direct" if "pivot_min" in hier.info[0] else "one Chebyshev(3) application", "iterations": si["iterations"],
               "vcycle_ms_median": median(cy), "vcycle_ms_min": min(cy), "solve_wall_s": wall, "residual": si["residual"],
               "rel_error_vs_x_star": float(torch.linalg.norm(sol - xs) / torch.linalg.norm(xs)), "level_matrix_bytes": 8.0 * sum(values),
               "coarser_levels_over_finest_bytes": sum(values[:-1]) / values[-1]}
        print(json.dumps(rec), flush=True)
        return rec, rhs, xs

    # (b)
    fe3 = pa.FE_DGQ(3, 3)
    blocks = [b for b in (32, 16, 8, 4, 2) if 2 * b <= cells]
    handlers = block_hierarchy(grid, fe3, blocks)
    hier = multigrid_hierarchy(handlers, fe3, variant(fe3), diag_first=True, degree=3)
    out["headline"] = [solve(hier, "h: FE_DGQ(3) on polytopes of %s cells per axis" % blocks, handlers)[0]]
    hier.close()
    fine3 = handlers[-1]
    del handlers, hier
    handlers = block_hierarchy(grid, pa.FE_DGQ(3, 1), blocks) + [one_level(pa.FE_DGQ(3, 2)), fine3]
    hier = p_multigrid_hierarchy(handlers, variant, diag_first=True, degree=3)
    out["headline"].append(solve(hier, "p-then-h: FE_DGQ(1) on polytopes of %s cells per axis, then FE_DGQ(2), FE_DGQ(3) on 2" % blocks, handlers)[0])
    hier.close()
    del handlers, hier, fine3
    # (c)
    handlers = [one_level(pa.FE_DGQ(3, q), grown=True) for q in (1, 2, 3)]
    hier = p_multigrid_hierarchy(handlers, variant, diag_first=True, degree=3)
    rec, rhs, xs = solve(hier, "p: FE_DGQ 1 -> 2 -> 3 on grown agglomerates of about 2^3 cells", handlers)
    fin, N = hier.finest, handlers[-1].n_dofs
    fin.setup_preconditioner("block_jacobi")  # detaches the mg
    sol = torch.zeros(N, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    si = fin.solve_cg_device(rhs.data_ptr(), sol.data_ptr(), rel_tol=1e-13)
    wall = time.perf_counter() - w0
    bj = {"preconditioner": "block Jacobi", "iterations": si["iterations"], "solve_wall_s": wall, "residual": si["residual"],
          "rel_error_vs_x_star": float(torch.linalg.norm(sol - xs) / torch.linalg.norm(xs))}
    print(json.dumps(bj), flush=True)
    out["dgq3_grown"] = {"p_vcycle": rec, "block_jacobi": bj, "wall_over_block_jacobi": rec["solve_wall_s"] / wall}
    hier.close()
    out["case_wall_s"] = time.time() - t0
    return out


def distributed_case(pa, torch, cells, W, reps):
    """CG over W rank-local contexts of the headline problem on one device (see the module docstring)"""
    import ctypes as C

    from polydeal_amd import _capi
    from polydeal_amd.distributed import _copy, _hip, _offsets, solve_cg_lockstep_device
    from polydeal_amd.partition import balanced_row_splits

    ah, fe = handler(pa, cells, "dgq")
    var = pa.SipVariant.poisson_example(fe)
    n, N = fe.n_dofs_per_cell, ah.n_dofs
    splits = [int(v) for v in balanced_row_splits(ah.blocks_per_row(), n, W)]
    ctxs, lay = [], []
    t0 = time.time()
    for r in range(W):
        c = pa.Context(0)
        ctxs.append(c)
        c.set_problem(ah.flatten_local(var, splits[r], splits[r + 1], True, False, row_splits=splits), splits[r], splits[r + 1])
        c.assemble_device()
        c.setup_preconditioner("block_jacobi")
        lay.append(c.halo_setup(splits))
        c.synchronize()
    setup_s = time.time() - t0
    gen = torch.Generator(device="cuda").manual_seed(1)
    b = [torch.rand(splits[r + 1] - splits[r], dtype=torch.float64, device="cuda", generator=gen) for r in range(W)]
    x = [torch.zeros_like(v) for v in b]
    d_b, d_x = [v.data_ptr() for v in b], [v.data_ptr() for v in x]

    def capped(cap):
        for v in x:
            v.zero_()
        torch.cuda.synchronize()
        t = time.perf_counter()
        try:
            solve_cg_lockstep_device(ctxs, splits, d_b, d_x, rel_tol=0.0, max_iter=cap, layouts=lay)
        except pa.PdhError as e:
            if e.code != pa.PDH_ENOCONV:
                raise
        return time.perf_counter() - t
    k, m = 2, 20
    capped(k)
    step_ms = median([(capped(k + m) - capped(k)) / m * 1e3 for _ in range(max(3, reps // 3))])

    # the phases of an iteration: the lock-step loop again with a synchronisation after every piece
    hip = _hip()
    send_at, recv_at = [_offsets(l[0]) for l in lay], [_offsets(l[1]) for l in lay]
    phases = {"halo_copy": [], "interior": [], "boundary": [], "allreduce_host": [], "update": [], "direction_readback_and_pack": []}

    def timed(key, fn):
        t = time.perf_counter()
        fn()
        for c in ctxs:
            c.synchronize()
        phases[key].append((time.perf_counter() - t) * 1e3)

    def resume_all(reqs):
        done = False
        for r, c in enumerate(ctxs):
            try:
                reqs[r] = c.dcg_resume()[0]
            except pa.PdhError as e:
                if e.code != pa.PDH_ENOCONV:
                    raise
                done = True
        return done
    for v in x:
        v.zero_()
    torch.cuda.synchronize()
    reqs = [c.dcg_begin(d_b[r], d_x[r], 0.0, 0.0, k + m) for r, c in enumerate(ctxs)]
    stage, done = 0, False
    while not done:
        kind = reqs[0]["kind"]
        if kind == _capi.PDH_DCG_HALO_BEGIN:
            # (the pack was queued by the call that asked for the move and is timed with it; on its own: `standalone` below)
            def move():
                for s_ in range(W):
                    for d_ in range(W):
                        _copy(hip, reqs[d_]["d_recv"] + 8 * int(recv_at[d_][s_]), reqs[s_]["d_send"] + 8 * int(send_at[s_][d_]), lay[s_][0][d_], 3)
            timed("halo_copy", move)
            timed("interior", lambda: resume_all(reqs))
        elif kind == _capi.PDH_DCG_HALO_END:
            timed("boundary", lambda: resume_all(reqs))
        elif kind == _capi.PDH_DCG_ALLREDUCE:
            m_ = reqs[0]["n_scalars"]

            def reduce_():
                import numpy as np
                parts = np.empty((W, m_))
                for r in range(W):
                    _copy(hip, parts[r].ctypes.data, reqs[r]["d_scalars"], m_, 2)
                total = parts[0].copy()
                for r in range(1, W):
                    total += parts[r]
                for r in range(W):
                    _copy(hip, reqs[r]["d_scalars"], total.ctypes.data, m_, 1)
            timed("allreduce_host", reduce_)
            flag = []
            timed("update" if m_ == 1 else "direction_readback_and_pack", lambda: flag.append(resume_all(reqs)))
            done = flag[0]
        else:
            break
    # (the first halo / products / reduction belong to the start)
    # the three kernels of this unit on their own, all ranks one after the other
    v = [torch.rand(l[2]["n_owned_rows"] + l[2]["n_ghost_rows"], dtype=torch.float64, device="cuda", generator=gen) for l in lay]
    snd = [torch.empty(max(sum(l[0]), 1), dtype=torch.float64, device="cuda") for l in lay]
    standalone = {}
    for key, fn in (("pack", lambda r: ctxs[r].halo_pack(v[r].data_ptr(), snd[r].data_ptr())),
                    ("interior", lambda r: ctxs[r].vmult_local(v[r].data_ptr(), x[r].data_ptr(), "interior")),
                    ("boundary", lambda r: ctxs[r].vmult_local(v[r].data_ptr(), x[r].data_ptr(), "boundary")),
                    ("all", lambda r: ctxs[r].vmult_local(v[r].data_ptr(), x[r].data_ptr(), "all"))):
        ts = []
        torch.cuda.synchronize()
        for _ in range(reps + 1):
            t = time.perf_counter()
            for r in range(W):
                fn(r)
            for c in ctxs:
                c.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        standalone[key] = median(ts[1:])
    per_iter = {key: median(v[1:]) if len(v) > 1 else None for key, v in phases.items()}
    out = {"what": "FE_DGQ(3), %d^3 cells, polytopes of 2^3 cells: block-Jacobi CG over %d rank-local contexts on one device, lock-step" % (cells, W),
           "caveat": "one device plays all ranks one after the other: no overlap of the interior product with the halo move and no "
                     "interconnect (xGMI) is measured, there is no multi-GPU node; the times are wall times between stream synchronisations, "
                     "summed over the ranks, launch and host latencies included.  A report, no time is a pass condition.",
           "world": W, "n_dofs": N, "row_splits": splits, "setup_s_all_ranks": setup_s,
           "halo": [{"send_doubles": int(sum(l[0])), "recv_doubles": int(sum(l[1])), "interior_polytopes": l[2]["n_interior"],
                     "boundary_polytopes": l[2]["n_boundary"]} for l in lay],
           "whole_step_ms_median": step_ms, "phase_ms_median": per_iter, "standalone_kernel_ms_median": standalone}
    if W == 1:
        cg_ms = cg_iteration_ms(pa, ctxs[0], torch, b[0], x[0], k, m, max(3, reps // 3))
        out["pdh_solve_cg_device_iteration_ms_median_same_problem"] = cg_ms
        out["whole_step_over_pdh_solve_cg_device"] = step_ms / cg_ms
        out["parent_commit_cg_iteration_ms"] = {"source": "profiles/r06_solve_bench.json, FE_DGQ(3) diag_first (the tool's default mode)", "value": None}
        try:
            with open(os.path.join(ROOT, "profiles", "r06_solve_bench.json")) as f:
                out["parent_commit_cg_iteration_ms"]["value"] = json.load(f)["cases"][0]["cg_iteration_ms_median"]
        except (OSError, KeyError, IndexError, ValueError):
            pass
    for c in ctxs:
        c.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cells", type=int, default=64, help="cells per axis (power of two); 64 = the headline problem")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-solve", action="store_true", help="skip the full headline solve")
    ap.add_argument("--chebyshev", action="store_true", help="add the Chebyshev section (FE_DGQ(3) diag_first and FE_AggloDGP(3))")
    ap.add_argument("--transfer", action="store_true", help="the level-transfer section alone (default --out: profiles/r08_transfer.json)")
    ap.add_argument("--vcycle", action="store_true", help="the V-cycle section alone (default --out: profiles/r09_vcycle.json)")
    ap.add_argument("--smoother-f32", action="store_true",
                    help="with --vcycle or --chebyshev: the single-precision smoother section alone (--vcycle: default --out profiles/r10_smoother_f32.json)")
    ap.add_argument("--matrix-free", action="store_true",
                    help="with --vcycle: the matrix-free smoother-operator section alone, with --smoother-f32 also over F32 inverses "
                         "(default --out: profiles/r12_matrix_free.json)")
    ap.add_argument("--galerkin", action="store_true",
                    help="with --vcycle: the Galerkin-product section alone (default --out: profiles/r11_galerkin.json)")
    ap.add_argument("--p-vcycle", action="store_true",
                    help="the p-multigrid section alone: p-transfer pairs, the headline solve over a p-then-h hierarchy, dgq3_grown "
                         "(default --out: profiles/r13_p_multigrid.json)")
    ap.add_argument("--distributed", type=int, default=0, metavar="W",
                    help="the distributed-CG section alone: the headline problem over W rank-local contexts on one device; several "
                         "runs append to the same file (default --out: profiles/r15_distributed_cg.json)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import polydeal_amd as pa
    if args.distributed:
        path = args.out or os.path.join(ROOT, "profiles", "r15_distributed_cg.json")
        out = {"tool": "tools/solve_bench.py --distributed W", "version": pa.load_library().pdh_version().decode(),
               "device": torch.cuda.get_device_name(0), "runs": []}
        if os.path.exists(path):  # runs of other W under the same build are kept
            with open(path) as f:
                old = json.load(f)
            if old.get("version") == out["version"]:
                out["runs"] = [r for r in old.get("runs", []) if r.get("world") != args.distributed]
        out["runs"].append(distributed_case(pa, torch, args.cells, args.distributed, args.reps))
        out["runs"].sort(key=lambda r: r["world"])
        doc = json.dumps(out, indent=1)
        with open(path, "w") as f:
            f.write(doc + "\n")
        print(doc)
        return
    if args.p_vcycle:
        out = {"tool": "tools/solve_bench.py --p-vcycle", "version": pa.load_library().pdh_version().decode(),
               "device": torch.cuda.get_device_name(0)}
        out.update(p_vcycle_case(pa, torch, args.cells, args.reps))
        doc = json.dumps(out, indent=1)
        with open(args.out or os.path.join(ROOT, "profiles", "r13_p_multigrid.json"), "w") as f:
            f.write(doc + "\n")
        print(doc)
        return
    if args.matrix_free:
        if not args.vcycle or args.galerkin:
            ap.error("--matrix-free goes with --vcycle (and --smoother-f32)")
        out = {"tool": "tools/solve_bench.py --vcycle --matrix-free" + (" --smoother-f32" if args.smoother_f32 else ""),
               "version": pa.load_library().pdh_version().decode(), "device": torch.cuda.get_device_name(0)}
        out.update(matrix_free_case(pa, torch, args.cells, args.reps, args.smoother_f32))
        doc = json.dumps(out, indent=1)
        with open(args.out or os.path.join(ROOT, "profiles", "r12_matrix_free.json"), "w") as f:
            f.write(doc + "\n")
        print(doc)
        return
    if args.galerkin:
        if not args.vcycle or args.smoother_f32:
            ap.error("--galerkin goes with --vcycle alone")
        out = {"tool": "tools/solve_bench.py --vcycle --galerkin", "version": pa.load_library().pdh_version().decode(),
               "device": torch.cuda.get_device_name(0)}
        out.update(galerkin_case(pa, torch, args.cells, args.reps))
        doc = json.dumps(out, indent=1)
        with open(args.out or os.path.join(ROOT, "profiles", "r11_galerkin.json"), "w") as f:
            f.write(doc + "\n")
        print(doc)
        return
    if args.smoother_f32:
        if not (args.vcycle or args.chebyshev):
            ap.error("--smoother-f32 goes with --vcycle or --chebyshev")
        out = {"tool": "tools/solve_bench.py --%s --smoother-f32" % ("vcycle" if args.vcycle else "chebyshev"),
               "version": pa.load_library().pdh_version().decode(), "device": torch.cuda.get_device_name(0)}
        out.update(smoother_f32_case(pa, torch, args.cells, args.reps, args.vcycle))
        doc = json.dumps(out, indent=1)
        path = args.out or (os.path.join(ROOT, "profiles", "r10_smoother_f32.json") if args.vcycle else None)
        if path:
            with open(path, "w") as f:
                f.write(doc + "\n")
        print(doc)
        return
    if args.vcycle:
        out = {"tool": "tools/solve_bench.py --vcycle", "version": pa.load_library().pdh_version().decode(),
               "device": torch.cuda.get_device_name(0)}
        out.update(vcycle_case(pa, torch, args.cells, args.reps))
        doc = json.dumps(out, indent=1)
        with open(args.out or os.path.join(ROOT, "profiles", "r09_vcycle.json"), "w") as f:
            f.write(doc + "\n")
        print(doc)
        return
    if args.transfer:
        out = {"tool": "tools/solve_bench.py --transfer", "version": pa.load_library().pdh_version().decode(),
               "device": torch.cuda.get_device_name(0), "pairs": []}
        for p in (3, 2):
            out["pairs"].append(transfer_case(pa, torch, args.cells, p, args.reps))
            print(json.dumps(out["pairs"][-1]), flush=True)
        doc = json.dumps(out, indent=1)
        with open(args.out or os.path.join(ROOT, "profiles", "r08_transfer.json"), "w") as f:
            f.write(doc + "\n")
        print(doc)
        return
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
