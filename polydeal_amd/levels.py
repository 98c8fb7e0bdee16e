"""Per-level SIP assembly for agglomerated multigrid hierarchies.

The reference builds one AgglomerationHandler per R-tree level and assembles the level operator with the same
hot path (examples/simplex_agglomerated_multigrid.cc:378-390 calls PolyUtils::assemble_dg_matrix once per
level; include/poly_utils.h:1761-1862 builds the level handlers).  On structured grids the R-tree levels are
exactly blocks of 2^k cells per direction (test/polydeal/rtree_mesh.output, 3DRtree.output), which is what
`block_hierarchy` produces; each level is assembled by the same HIP kernels."""
from __future__ import annotations

from .handler import AgglomerationHandler, BackgroundGrid, FiniteElement, SipVariant, assemble_dg_matrix  # noqa: F401


def block_hierarchy(grid: BackgroundGrid, fe: FiniteElement, blocks, n_q_points_1d=None):
    """One handler per level; `blocks` = cells per direction of a polytope on each level, coarse to fine
    (e.g. [8, 4, 2] on a 64^3 grid gives 8^3, 16^3, 32^3 polytopes)."""
    nq = n_q_points_1d or fe.degree + 1
    levels = []
    for b in blocks:
        ah = AgglomerationHandler(grid)
        ah.define_block_agglomerates(b)
        ah.initialize_fe_values(nq, nq)
        ah.distribute_agglomerated_dofs(fe)
        levels.append(ah)
    return levels


def assemble_levels(levels, fe: FiniteElement, variant: SipVariant | None = None, diag_first=True, device=0):
    """[(rowptr, colind, values)] - the 'V-cycle assembly' of BASELINE.json configs[4]: one assemble_dg_matrix per level
    (examples/simplex_agglomerated_multigrid.cc:378-390), all on ONE context (stream, events, scratch buffers are created once;
    every level replaces the resident problem).  Levels of Cartesian cells are handed over without their quadrature points
    (flatten_cartesian: generated on the device) where the term kernels take them; distorted cells and polytopes too large for those
    kernels go through the points-based description as before."""
    from ._capi import Context, PdhError
    from .handler import HostError

    variant = variant or SipVariant.assemble_dg_matrix()
    out = []
    ctx = Context(device)
    try:
        for ah in levels:
            if fe != ah.fe:
                raise ValueError("FE passed to assemble_levels differs from a level handler's")
            flat = None
            if ah.grid.dim == 3:
                try:
                    flat = ah.flatten_cartesian(variant, diag_first, True)
                    ctx.set_problem(flat)
                except (PdhError, HostError):
                    flat = None
            if flat is None:
                flat = ah.flatten(variant, diag_first, True)
                ctx.set_problem(flat)
            arr = flat.arrays()
            out.append((arr["rowptr"].copy(), arr["colind"].copy(), ctx.assemble()))
    finally:
        ctx.close()
    return out


def level_transfer(ctx, coarse_ah: AgglomerationHandler, fine_ah: AgglomerationHandler):
    """_capi.Transfer between two nested levels on the device of `ctx` (the reference's MGTransferAgglomeration, include/
    multigrid_amg.h:439-490): description from the host mirror, 1-D factors built on the host, nothing but tables uploaded.  `ctx`
    needs no resident problem; close the transfer before it."""
    from ._capi import Transfer
    from .handler import transfer_description

    return Transfer(ctx, transfer_description(coarse_ah, fine_ah))


def two_grid_cycle_device(fine_ctx, coarse_ctx, transfer, d_b, d_x, d_r, d_rc, d_ec, coarse_rel_tol=1e-13):
    """One two-grid cycle on x composed of device calls alone; the caller owns every buffer (device pointers as ints: b, x, r of the
    fine level's size, rc, ec of the coarse level's):
      pre-smooth x (fine_ctx's Chebyshev smoother), r = b - A x, rc = P^T r, ec = 0, A_c ec = rc by coarse_ctx's CG to
      coarse_rel_tol, x += P ec, post-smooth x.
    Both contexts carry their assembled level matrix, the fine one with setup_chebyshev done, the coarse one with the preconditioner
    of its CG; `transfer` lives on fine_ctx, whose stream orders the fine-level work.  Returns the info of the coarse solve."""
    import ctypes as C

    hip = C.CDLL("libamdhip64.so")
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    fine_ctx.chebyshev_step_device(d_b, d_x)
    fine_ctx.residual_device(d_b, d_x, d_r)
    transfer.restrict_device(d_r, d_rc)
    fine_ctx.synchronize()  # the coarse context has a stream of its own
    if hip.hipMemset(C.c_void_p(d_ec), 0, C.c_size_t(8 * transfer.desc.n_coarse_rows)) != 0 or hip.hipDeviceSynchronize() != 0:
        raise RuntimeError("hipMemset of the coarse correction failed")
    info = coarse_ctx.solve_cg_device(d_rc, d_ec, rel_tol=coarse_rel_tol)  # synchronises before it returns
    transfer.prolongate_and_add_device(d_ec, d_x)
    fine_ctx.chebyshev_step_device(d_b, d_x)
    return info


class MultigridHierarchy:
    """What multigrid_hierarchy returns: the level contexts (coarse to fine, each with its assembled matrix), the transfers between
    them and the _capi.Multigrid whose V-cycle is the preconditioner of the finest context.  `info`: per level, what its set-up
    reported (setup_direct on level 0, setup_chebyshev above)."""

    def __init__(self, contexts, transfers, mg, info):
        self.contexts, self.transfers, self.mg, self.info = contexts, transfers, mg, info
        self.finest = contexts[-1]

    def solve_cg(self, b, x0=None, rel_tol=1e-13, abs_tol=0.0, max_iter=None):
        """V-cycle-preconditioned CG on the finest level (Context.solve_cg): (x, info)"""
        return self.finest.solve_cg(b, x0, rel_tol, abs_tol, max_iter)

    def solve_cg_device(self, d_b, d_x, rel_tol=1e-13, abs_tol=0.0, max_iter=None):
        return self.finest.solve_cg_device(d_b, d_x, rel_tol, abs_tol, max_iter)

    def vcycle_device(self, d_b, d_x, zero_initial_guess=False):
        self.mg.vcycle_device(d_b, d_x, zero_initial_guess)

    def close(self):
        """the mg first, then the transfers, then their contexts"""
        if self.mg is not None:
            self.mg.close()
            self.mg = None
        for t in self.transfers:
            t.close()
        self.transfers = []
        for c in self.contexts:
            c.close()
        self.contexts = []


def _set_level_problem(ctx, ah, variant, diag_first):
    """the description of one level handler becomes the resident problem of `ctx`: the Cartesian one where it is taken"""
    from ._capi import PdhError
    from .handler import HostError

    flat = None
    if ah.grid.dim == 3:
        try:
            flat = ah.flatten_cartesian(variant, diag_first, False)
            ctx.set_problem(flat)
        except (PdhError, HostError):
            flat = None
    if flat is None:
        flat = ah.flatten(variant, diag_first, False)  # (no colind: nothing here reads the pattern back)
        ctx.set_problem(flat)


def _setup_level(ctx, l, inner, degree, smoother_precision, smoother_operator="stored", sip_values=True, coarsest="direct"):
    """the solver of level 0 (coarsest 'direct': the dense solve; 'chebyshev': one application of the smoother's polynomial), the smoother
    of every level above: what its set-up reported, and under 'smoother_operator' which operator the level's smoother applies.
    'matrix_free' is taken where the context grants the tables (PDH_EUNSUPPORTED: the level stays 'stored') and its values are the SIP
    assembly of its own description (sip_values)."""
    from ._capi import PDH_EUNSUPPORTED, PdhError

    info = dict(ctx.setup_direct() if l == 0 and coarsest == "direct" else ctx.setup_chebyshev(inner, degree=degree))
    if l > 0 and smoother_precision == "f32":
        ctx.set_smoother_precision("f32")
    info["smoother_operator"] = "stored"
    if l > 0 and smoother_operator == "matrix_free" and sip_values:
        try:
            info["matrix_free"] = ctx.setup_matrix_free()
        except PdhError as e:
            if e.code != PDH_EUNSUPPORTED:
                raise
        else:
            ctx.set_smoother_operator("matrix_free")
            info["smoother_operator"] = "matrix_free"
    return info


def multigrid_hierarchy(levels, fe: FiniteElement, variant: SipVariant | None = None, diag_first=True, degree=3, inner=None, device=0,
                        smoother_precision="f64", coarse_operators="assembled", smoother_operator="stored"):
    """The reference's agglomerated multigrid (examples/simplex_agglomerated_multigrid.cc:378-515) on one device: one context per level
    handler of `levels` (coarse to fine, e.g. block_hierarchy's), each assembled like assemble_levels does (the Cartesian description
    where it is taken); Chebyshev of `degree` over `inner` ('block_jacobi' up to 64 dofs per polytope, 'jacobi' above, unless given) as
    the smoother of every level above the coarsest, the dense direct solve on the coarsest (at most 1024 rows), the level transfers
    and the V-cycle, which becomes the preconditioner of the finest context.  smoother_precision 'f32': every level above the coarsest
    smooths, and forms its residual, with a float32 copy of its matrix (Context.set_smoother_precision); CG and all vectors stay double.
    coarse_operators 'galerkin': only the finest level is assembled, every level below it gets A_(l-1) = P^T A_l P from the level above
    (Transfer.galerkin_device, the reference's AmgProjector::compute_level_matrices, include/multigrid_amg.h:267-305), fine to coarse,
    before any level is set up; at most 64 dofs per polytope.  'assembled' (default): every level assembles the SIP operator on its own
    polytopes.  smoother_operator 'matrix_free': every level above the coarsest whose context grants the tables (Context.setup_matrix_free)
    and whose values are the SIP assembly of its own polytopes - under 'galerkin' the finest only - takes the products of its smoother
    and its residual from them (Context.set_smoother_operator); the other levels stay 'stored'.  info[l]["smoother_operator"] says which
    is in force.  Returns a MultigridHierarchy; close() it."""
    from ._capi import Context, Multigrid

    variant = variant or SipVariant.assemble_dg_matrix()
    if inner is None:
        inner = "block_jacobi" if fe.n_dofs_per_cell <= 64 else "jacobi"
    if smoother_precision not in ("f64", "f32"):
        raise ValueError("smoother_precision must be 'f64' or 'f32'")
    if coarse_operators not in ("assembled", "galerkin"):
        raise ValueError("coarse_operators must be 'assembled' or 'galerkin'")
    if smoother_operator not in ("stored", "matrix_free"):
        raise ValueError("smoother_operator must be 'stored' or 'matrix_free'")
    galerkin = coarse_operators == "galerkin"
    contexts, transfers, info, mg = [], [], [], None
    try:
        for l, ah in enumerate(levels):
            if fe != ah.fe:
                raise ValueError("FE passed to multigrid_hierarchy differs from a level handler's")
            ctx = Context(device)
            contexts.append(ctx)
            _set_level_problem(ctx, ah, variant, diag_first)
            if not galerkin:
                ctx.assemble_device()
                info.append(_setup_level(ctx, l, inner, degree, smoother_precision, smoother_operator))
            if l > 0:
                transfers.append(level_transfer(ctx, levels[l - 1], ah))
        if galerkin:
            contexts[-1].assemble_device()
            for l in range(len(levels) - 1, 0, -1):
                transfers[l - 1].galerkin_device(contexts[l - 1])
            info = [_setup_level(ctx, l, inner, degree, smoother_precision, smoother_operator, l == len(contexts) - 1)
                    for l, ctx in enumerate(contexts)]
        mg = Multigrid(contexts, transfers)
    except Exception:
        MultigridHierarchy(contexts, transfers, mg, info).close()
        raise
    return MultigridHierarchy(contexts, transfers, mg, info)


def _level_pair_description(l, coarse_ah, fine_ah):
    """the description of the transfer between two consecutive level handlers: a p-pair (the same polytopes, one kind of basis, a lower
    degree below) or a nested h-pair of equal degree; anything else is a ValueError naming the pair"""
    from .handler import HostError, p_transfer_description, transfer_description

    who = "levels %d and %d" % (l - 1, l)
    fc, ff = coarse_ah.fe, fine_ah.fe
    if fc.dim != ff.dim or fc.basis != ff.basis:
        raise ValueError(who + " hold different kinds of basis")
    try:
        if fc.degree == ff.degree:
            return transfer_description(coarse_ah, fine_ah)
        if fc.degree < ff.degree:
            return p_transfer_description(coarse_ah, fine_ah)
    except HostError as e:
        raise ValueError("%s are neither a p-pair nor a nested h-pair: %s" % (who, e)) from e
    raise ValueError("%s: the degree falls from %d to %d towards the finer level" % (who, fc.degree, ff.degree))


def p_multigrid_hierarchy(handlers, variant=None, diag_first=True, degree=3, device=0, smoother_precision="f64",
                          smoother_operator="stored", coarsest=None):
    """A V-cycle over levels that differ in polynomial degree, in polytopes, or from pair to pair in either: `handlers` coarse to fine,
    each with its own FE distributed; `variant`: one SipVariant for all levels, or a function of a level's FE where the scalars depend on
    the degree (SipVariant.poisson_example).  Every consecutive pair is a p-pair - the same polytopes (count, bit-equal boxes, order) and kind
    of basis, the lower degree below (handler.p_transfer_description) - or a nested h-pair of equal degree (handler.transfer_description);
    anything else is a ValueError naming the pair.  A p-hierarchy needs no second mesh, so grown agglomerates, FE_AggloDGP and the
    elements beyond 64 dofs have one.  Every level is assembled on its own description like multigrid_hierarchy does (coarse degrees are
    re-assembled, there is no Galerkin product across degrees); its smoother is Chebyshev of `degree` over block Jacobi, over point
    Jacobi where its element has more than 64 dofs.  `coarsest`: 'direct' (the dense solve, at most 1024 rows), 'chebyshev' (one
    application of its smoother's polynomial), None: 'direct' up to 1024 rows.  smoother_precision and smoother_operator act per level
    as in multigrid_hierarchy.  Returns a MultigridHierarchy; close() it."""
    from ._capi import Context, Multigrid, Transfer

    handlers = list(handlers)
    if len(handlers) < 2:
        raise ValueError("a hierarchy has at least two levels")
    if smoother_precision not in ("f64", "f32"):
        raise ValueError("smoother_precision must be 'f64' or 'f32'")
    if smoother_operator not in ("stored", "matrix_free"):
        raise ValueError("smoother_operator must be 'stored' or 'matrix_free'")
    if coarsest not in (None, "direct", "chebyshev"):
        raise ValueError("coarsest must be 'direct', 'chebyshev' or None")
    if coarsest is None:
        coarsest = "direct" if handlers[0].n_dofs <= 1024 else "chebyshev"
    descriptions = [_level_pair_description(l, handlers[l - 1], handlers[l]) for l in range(1, len(handlers))]
    contexts, transfers, info, mg = [], [], [], None
    try:
        for l, ah in enumerate(handlers):
            ctx = Context(device)
            contexts.append(ctx)
            level_variant = variant(ah.fe) if callable(variant) else variant or SipVariant.assemble_dg_matrix()
            _set_level_problem(ctx, ah, level_variant, diag_first)
            ctx.assemble_device()
            inner = "block_jacobi" if ah.fe.n_dofs_per_cell <= 64 else "jacobi"
            info.append(_setup_level(ctx, l, inner, degree, smoother_precision, smoother_operator, coarsest=coarsest))
            if l > 0:
                transfers.append(Transfer(ctx, descriptions[l - 1]))
        mg = Multigrid(contexts, transfers)
    except Exception:
        MultigridHierarchy(contexts, transfers, mg, info).close()
        raise
    return MultigridHierarchy(contexts, transfers, mg, info)
