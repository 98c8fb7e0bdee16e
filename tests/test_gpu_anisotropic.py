"""GPU parity on box meshes whose cells are not cubes (tests/aniso_meshes.py): a different cell size on every axis, per-axis
grading, origins away from zero, slabs that meet neighbours shorter along different axes.  Every case asserts which kernel ran.
Also checks that do not trust the oracle: translation, axis permutation and scaling of the mesh."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import aniso_meshes as am
from flatten_oracle import flatten
from oracle import polydeal_oracle as po
from parity import assert_parity, assert_parity_ah, assert_vector_parity, dof_segments, oracle_evaluate, point_segments

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _fe(basis, dim, p):
    return (po.FE_DGQ if basis == "dgq" else po.FE_AggloDGP)(dim, p)


def _variant(name, fe):
    return {"poisson": lambda: po.variant_poisson_example(fe), "dr": lambda: po.variant_diffusion_reaction(fe),
            "adm": po.variant_assemble_dg_matrix}[name]()


@functools.lru_cache(maxsize=8)
def _case(mesh, basis, p, vname, diag_first, nq=None, **grid_kw):
    dim = am.MESHES[mesh][0]
    fe = _fe(basis, dim, p)
    ah = am.oracle_handler(mesh, fe, nq or p + 1, **grid_kw)
    var = _variant(vname, fe)
    kw = flatten(ah, var, diag_first=diag_first)
    ref = po.assemble_csr(ah, var, diag_first=diag_first)[2]
    return ah, var, kw, ref


def _run(kw, alg="auto", env=None, r0=0, r1=None):
    """values, algorithm in use, row kernel in use; env: variables read at set_problem (PDH_TERMS, PDH_TERMS_SPLIT, ...)"""
    import polydeal_amd as pa

    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        ctx = pa.Context(0)
        ctx.set_algorithm(alg)
        ctx.set_problem(pa.Problem(**kw), r0, r1)
        used, kern = ctx.algorithm_in_use(), ctx.rows_kernel_in_use()
        v = ctx.assemble()
        ctx.close()
    finally:
        for k, o in old.items():
            if o is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = o
    return v, used, kern


ROWS_KINDS = ("pieces", "streamed", "multi")
SMALL_MESHES = [("rect124", "poisson", True), ("rect1116", "dr", False), ("graded", "poisson", False), ("pinwheel", "dr", True),
                ("offset_mod", "adm", True)]


@pytest.mark.parametrize("basis,p", [("dgq", 1), ("dgq", 2), ("dgp", 1), ("dgp", 2), ("dgp", 3)])
@pytest.mark.parametrize("mesh,vname,diag_first", SMALL_MESHES)
def test_small_elements_on_box_meshes(mesh, vname, diag_first, basis, p):
    """The wave term kernel (pdh_terms.h) - what AUTO takes - in both forms of T.split, the kinds of pdh_rows.h (PDH_TERMS=0), the
    moment form with and without the tensor structure of the rules, and the direct form: each against the oracle per block."""
    ah, var, kw, ref = _case(mesh, basis, p, vname, diag_first)
    v, used, kern = _run(kw)
    assert used == "rows" and kern == "terms", (used, kern)
    assert_parity_ah(v, ref, ah, diag_first, what="AUTO (term kernel)")
    for split in ("0", "1"):
        v, used, kern = _run(kw, env={"PDH_TERMS_SPLIT": split})
        assert used == "rows" and kern == "terms"
        assert_parity_ah(v, ref, ah, diag_first, what="term kernel, split=" + split)
    if mesh == "pinwheel":
        # (the 3 x 3 centre has 13 neighbours: more than the kinds of pdh_rows.h take for these elements - forcing them fails loudly)
        import polydeal_amd as pa

        with pytest.raises(pa.PdhError, match="row kernel does not apply"):
            _run(kw, "rows", env={"PDH_TERMS": "0"})
    else:
        v, used, kern = _run(kw, "rows", env={"PDH_TERMS": "0"})
        assert used == "rows" and kern in ROWS_KINDS, kern
        assert_parity_ah(v, ref, ah, diag_first, what="pdh_rows.h " + kern)
    for hint in ({}, {"vq_tensor_n": -1, "fq_tensor_n": -1}):
        v, used, _ = _run(dict(kw, **hint), "moment")
        assert used == "moment"
        assert_parity_ah(v, ref, ah, diag_first, what="moment %s" % hint)
    v, used, _ = _run(kw, "direct")
    assert used == "direct"
    assert_parity_ah(v, ref, ah, diag_first, what="direct")


def _dgq3_auto(mesh, vname, diag_first):
    ah, var, kw, ref = _case(mesh, "dgq", 3, vname, diag_first)
    v, used, kern = _run(kw)
    assert used == "rows" and kern == "terms", (used, kern)
    assert_parity_ah(v, ref, ah, diag_first, what="k_terms_wg on " + mesh)
    return ah, kw, ref


@pytest.mark.parametrize("mesh,vname,diag_first", SMALL_MESHES)
def test_dgq3_on_box_meshes(mesh, vname, diag_first):
    """FE_DGQ(3): the workgroup term kernel (pdh_terms_wg.h, four waves - AUTO's choice), the kinds of pdh_rows.h (PDH_TERMS_DGQ3=0),
    the moment form with and without tensor hints, the direct form; a row range split in three (rank-local rows) for the first mesh."""
    from polydeal_amd.partition import row_range

    ah, kw, ref = _dgq3_auto(mesh, vname, diag_first)
    v, used, kern = _run(kw, env={"PDH_TERMS_DGQ3": "0"})
    assert used == "rows" and kern in ("pieces", "multi"), kern
    assert_parity_ah(v, ref, ah, diag_first, what="pdh_rows.h " + kern)
    for hint in ({}, {"vq_tensor_n": -1, "fq_tensor_n": -1}):
        v, used, _ = _run(dict(kw, **hint), "moment")
        assert used == "moment"
        assert_parity_ah(v, ref, ah, diag_first, what="moment %s" % hint)
    v, used, _ = _run(kw, "direct")
    assert used == "direct"
    assert_parity_ah(v, ref, ah, diag_first, what="direct")
    if mesh == "rect124":
        n, parts = 64, []
        for r in range(3):
            rb, re = row_range(ah.n_agglomerates, n, r, 3)
            v, used, kern = _run(kw, r0=rb, r1=re)
            assert used == "rows" and kern == "terms"
            parts.append(v)
        assert_parity_ah(np.concatenate(parts), ref, ah, diag_first, what="row ranges, world 3")


def test_dgq3_workgroup_kernel_eight_waves():
    """k_terms_wg with eight waves per polytope (PDH_TERMS_WG_WAVES was read once per process, now at every set-up: still a child process of its own)."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_anisotropic as t; "
            "[t._dgq3_auto(*c) for c in t.SMALL_MESHES]; print('ok')" % (ROOT, HERE))
    env = dict(os.environ, PDH_TERMS_WG_WAVES="8")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "ok" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


def test_multi_row_kernel_on_graded_grown_agglomerates():
    """Staircase agglomerates (regions grown over the cell graph) of the per-axis graded grid: FE_DGQ(3) through the MULTI instantiation
    of pdh_rows.h (PDH_TERMS_DGQ3=0) and through the workgroup term kernel, both against the oracle."""
    import polydeal_amd as pa

    mg = pa.BackgroundGrid.subdivided_hyper_cube(3, 6, 0.0, 1.0)
    mah = pa.AgglomerationHandler(mg)
    mah.define_grown_agglomerates(6, seed=2)
    groups = [sorted(mah.get_agglomerate(P)) for P in range(mah.n_agglomerates)]
    grid = po.subdivided_hyper_cube(3, 6, 0.0, 1.0)
    t = grid.vertices.copy()
    grid.vertices[..., 0] = t[..., 0] ** 1.6
    grid.vertices[..., 1] = t[..., 1] ** 0.7
    ah = po.AgglomerationHandler(grid)
    for g in groups:
        ah.define_agglomerate(g)
    fe = po.FE_DGQ(3, 3)
    ah.initialize_fe_values(4, 4)
    ah.distribute_agglomerated_dofs(fe)
    var = po.variant_poisson_example(fe)
    kw = flatten(ah, var)
    ref = po.assemble_csr(ah, var)[2]
    v, used, kern = _run(kw, env={"PDH_TERMS_DGQ3": "0"})
    assert used == "rows" and kern == "multi", kern
    assert_parity_ah(v, ref, ah, what="MULTI")
    v, used, kern = _run(kw)
    assert used == "rows" and kern == "terms", kern
    assert_parity_ah(v, ref, ah, what="k_terms_wg")


@pytest.mark.parametrize("mesh,basis,p,vname,diag_first", [("rect124_2", "dgq", 4, "poisson", True), ("graded_2", "dgq", 4, "dr", False),
                                                            ("rect124_2", "dgp", 6, "dr", False), ("graded_2", "dgp", 6, "poisson", True)])
def test_tiled_kernels_on_box_meshes(mesh, basis, p, vname, diag_first):
    """More than 64 dofs per polytope (pdh_tiled.h, AUTO's direct form in 64 x 64 tiles) on undistorted box cells of unequal sides:
    matrix and right-hand side against the oracle."""
    ah, var, kw, ref = _case(mesh, basis, p, vname, diag_first)
    v, used, kern = _run(kw)
    assert used == "direct" and kern == "none", (used, kern)
    assert_parity_ah(v, ref, ah, diag_first, what="tiled")
    _check_rhs(ah, var, kw)


@pytest.mark.parametrize("basis,p", [("dgq", 1), ("dgq", 2), ("dgq", 3), ("dgp", 2), ("dgp", 3)])
@pytest.mark.parametrize("mesh,vname,diag_first", [("rect2d", "poisson", True), ("offset2d", "dr", False)])
def test_2d_direct_kernels_on_box_meshes(mesh, vname, diag_first, basis, p):
    ah, var, kw, ref = _case(mesh, basis, p, vname, diag_first)
    v, used, kern = _run(kw)
    assert used == "direct", used
    assert_parity_ah(v, ref, ah, diag_first, what="2-D direct")


def _check_rhs(ah, var, kw):
    import polydeal_amd as pa

    f = lambda x: np.sin(2.0 * x[:, 0]) + x[:, 1] ** 2 + x[:, -1]
    g = lambda x: 1.0 + x[:, 0] * x[:, 1] - 0.5 * x[:, -1]
    ref = po.assemble_rhs(ah, var, f, g)
    ctx = pa.Context(0)
    ctx.set_problem(pa.Problem(**kw))
    got = ctx.assemble_rhs(f(kw["vq_x"].T), g(kw["fq_x"].T))
    ctx.close()
    assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref))
    assert_vector_parity(got, ref, dof_segments(ah.n_dofs, ah.fe.n_dofs_per_cell), po.assemble_rhs(ah, var, f, g, absolute=True),
                         what="rhs")


@pytest.mark.parametrize("mesh,basis,p", [("rect124", "dgq", 3), ("graded", "dgp", 2), ("pinwheel", "dgq", 2), ("rect1116", "dgp", 3),
                                          ("rect2d", "dgq", 2)])
def test_rhs_evaluate_and_global_error_on_box_meshes(mesh, basis, p):
    """pdh_assemble_rhs, pdh_evaluate (values and per-axis gradients) and pdh_global_error against the oracle."""
    import polydeal_amd as pa

    ah, var, kw, ref = _case(mesh, basis, p, "poisson", True)
    dim = ah.grid.dim
    _check_rhs(ah, var, kw)
    u = np.random.default_rng(7).standard_normal(ah.n_dofs)
    exact = lambda x: np.sin(1.3 * x[:, 0]) * np.cos(0.7 * x[:, 1]) + x[:, -1] ** 2

    def exact_grad(x):
        g = np.zeros_like(x)
        g[:, 0] = 1.3 * np.cos(1.3 * x[:, 0]) * np.cos(0.7 * x[:, 1])
        g[:, 1] = -0.7 * np.sin(1.3 * x[:, 0]) * np.sin(0.7 * x[:, 1])
        g[:, -1] += 2 * x[:, -1]
        return g

    ctx = pa.Context(0)
    ctx.set_problem(pa.Problem(**kw))
    uh, gh = ctx.evaluate(u, kw["vq_ptr"], kw["vq_x"], want_grad=True)
    l2, h1 = pa.compute_global_error(ctx, kw["vq_ptr"], kw["vq_x"], kw["vq_w"], u, exact, exact_grad)
    ctx.close()
    ev = [po.evaluate_at(ah, u, P, ah.reinit(P)["x"]) for P in range(ah.n_agglomerates)]
    ref_u = np.concatenate([e[0] for e in ev])
    ref_g = np.concatenate([e[1] for e in ev]).T
    assert np.max(np.abs(uh - ref_u)) <= 1e-12 * np.max(np.abs(ref_u))
    for c in range(dim):  # per axis: the gradients differ in size by the aspect ratio
        assert np.max(np.abs(gh[c] - ref_g[c])) <= 1e-12 * np.max(np.abs(ref_g[c])), c
    ev = [oracle_evaluate(ah, u, P, ah.reinit(P)["x"]) for P in range(ah.n_agglomerates)]
    seg = point_segments(kw["vq_ptr"])
    assert_vector_parity(uh, ref_u, seg, np.concatenate([e[2] for e in ev]), what="u_h")
    assert_vector_parity(gh.T, ref_g.T, seg, np.concatenate([e[3] for e in ev]), what="grad u_h")
    rl2, rh1 = po.compute_global_error(ah, u, exact, exact_grad)
    assert abs(l2 - rl2) <= 1e-12 * rl2 and abs(h1 - rh1) <= 1e-12 * rh1


@pytest.mark.parametrize("mesh,basis,p,vname,diag_first", [("rect124", "dgq", 3, "poisson", True), ("rect1116", "dgp", 3, "dr", False),
                                                            ("offset_mod", "dgq", 2, "poisson", False), ("pinwheel", "dgp", 2, "adm", True),
                                                            ("rect124", "dgq", 1, "dr", True)])
def test_cartesian_description_on_box_meshes(mesh, basis, p, vname, diag_first):
    """pdh_set_problem_cartesian: the PRODUCT mirror describes the rectangle's agglomerates without their points, the device generates
    them (pdh_cartgen.hip) - against the oracle per block, and against the points-based description of the same problem to rounding."""
    import polydeal_amd as pa

    pfe = (pa.FE_DGQ if basis == "dgq" else pa.FE_AggloDGP)(3, p)
    mah = am.mirror_handler(mesh, pfe, p + 1)
    pvar = {"poisson": pa.SipVariant.poisson_example(pfe), "dr": pa.SipVariant.diffusion_reaction(pfe),
            "adm": pa.SipVariant.assemble_dg_matrix()}[vname]
    ah, var, kw, ref = _case(mesh, basis, p, vname, diag_first)
    cf = mah.flatten_cartesian(pvar, diag_first, True)
    assert cf.cartesian and cf.c.vq_x is None
    ctx = pa.Context(0)
    ctx.set_problem(cf)
    assert ctx.algorithm_in_use() == "rows" and ctx.rows_kernel_in_use() == "terms"
    vals = ctx.assemble()
    ctx.close()
    ca = cf.arrays()
    orp, oci = ah.sparsity_pattern(diag_first)
    assert np.array_equal(ca["rowptr"], orp) and np.array_equal(ca["colind"], oci)
    assert_parity(vals, ref, orp, oci, pfe.n_dofs_per_cell, what="device-generated points")
    pf = mah.flatten(pvar, diag_first, True)
    ctx = pa.Context(0)
    ctx.set_problem(pf)
    vpts = ctx.assemble()
    ctx.close()
    assert np.max(np.abs(vals - vpts)) <= 1e-13 * np.max(np.abs(vpts))


SELECTION_ELEMENTS = [("dgq", 1), ("dgq", 2), ("dgq", 3), ("dgp", 1), ("dgp", 2), ("dgp", 3)]
SELECTION_CASES = ([(m, None) for m, spec in am.MESHES.items() if spec[0] == 3] +
                   [("offset_mod", off) for off, _, _ in am.OFFSET_BOUNDARY])


@pytest.mark.parametrize("basis,p", SELECTION_ELEMENTS)
@pytest.mark.parametrize("mesh,off", SELECTION_CASES)
def test_host_selection_is_what_set_problem_takes(mesh, off, basis, p, monkeypatch):
    """pdh_check_terms / pdh_check_rows (host only; what the CPU tests pin) name the row kernel that pdh_set_problem builds and AUTO
    runs: the term kernels where the first grants them, else pdh_rows.h where the second does, else none."""
    import polydeal_amd as pa

    for k in ("PDH_TERMS", "PDH_TERMS_DGQ3"):
        monkeypatch.delenv(k, raising=False)
    fe = _fe(basis, 3, p)
    ah = am.oracle_handler(mesh, fe, p + 1) if off is None else am.offset_handler(off, fe, p + 1)
    kw = flatten(ah, po.variant_poisson_example(fe))
    rt, wt, rr, wr = am.kernel_selection(kw)
    want = "terms" if rt == 1 else ("rows" if rr == 1 else "none")
    ctx = pa.Context(0)
    try:
        ctx.set_problem(pa.Problem(**kw))
        used, kern = ctx.algorithm_in_use(), ctx.rows_kernel_in_use()
    finally:
        ctx.close()
    got = kern if kern in ("terms", "none") else "rows"
    assert got == want, (kern, wt, wr)
    assert (used == "rows") == (got != "none"), (used, kern)


# ---------------------------------------------------------------------------------------------------------------------
# Checks that do not trust the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis,p", [("dgq", 3), ("dgp", 3), ("dgq", 2)])
@pytest.mark.parametrize("mesh", ["offset_far", "offset_mod"])
def test_translation(mesh, basis, p):
    """The mesh at its offset on the GPU against the oracle on the SAME mesh moved to the origin, per block to
    max(1e-12, 64 eps max|x| / h_min) (the input points carry eps |x| / h relative to h): a kernel that evaluated polynomials in
    global coordinates would be off by about (|x| / h)^p eps.  Whatever AUTO takes, and forced to the direct and moment forms; the
    moderate offset keeps the term kernels."""
    dim, nd, lo, hi = am.MESHES[mesh][:4]
    ah, var, kw, _ = _case(mesh, basis, p, "poisson", True)
    ah0, _, _, ref0 = _case(mesh, basis, p, "poisson", True, shift=tuple(-np.asarray(lo)))
    h_min = float(np.min((np.asarray(hi) - np.asarray(lo)) / np.asarray(nd)))
    tol = max(1e-12, 64 * 2.2e-16 * float(np.max(np.abs(np.concatenate([lo, hi])))) / h_min)
    v, used, kern = _run(kw)
    if mesh == "offset_mod":
        assert used == "rows" and kern == "terms", (used, kern)
    else:  # (beyond the rounding bound: test_anisotropic_cpu.py pins what AUTO takes there)
        # (degree 3: pdh_rows.h on its general-point paths; FE_DGQ(2): moment form for the diagonal blocks, direct for the coupling)
        assert (used == "rows" and kern in ROWS_KINDS) if p == 3 else used == "mixed", (used, kern)
    assert_parity_ah(v, ref0, ah0, True, tol=tol, what="AUTO %s/%s" % (used, kern))
    for alg in ("direct", "moment"):
        v, used, _ = _run(kw, alg)
        assert used == alg
        assert_parity_ah(v, ref0, ah0, True, tol=tol, what=alg)


def _gpu_matrix(ah, var, alg="auto", env=None):
    kw = flatten(ah, var, with_colind=True)
    v, used, kern = _run(kw, alg, env)
    A = po.csr_to_dense(kw["rowptr"], kw["colind"], v, ah.n_dofs)
    return A, used, kern


@pytest.mark.parametrize("p,env,kernel", [(1, {}, "terms"), (2, {}, "terms"), (3, {}, "terms"), (2, {"PDH_TERMS": "0"}, "streamed"),
                                          (3, {"PDH_TERMS_DGQ3": "0"}, "pieces")])
@pytest.mark.parametrize("mesh", ["rect124", "graded"])
def test_axis_permutation(mesh, p, env, kernel):
    """FE_DGQ on box lengths (L0, L1, L2) and (L1, L2, L0), both on the GPU with the same kernel: polytopes mapped by bounding box,
    dofs by rotating the lexicographic digits - the matrices agree to 1e-13 relative (the oracle is not asked)."""
    perm = (1, 2, 0)
    fe = po.FE_DGQ(3, p)
    var = po.variant_poisson_example(fe)
    ah0 = am.oracle_handler(mesh, fe, p + 1)
    ah1 = am.oracle_handler(mesh, po.FE_DGQ(3, p), p + 1, groups=am.permuted_groups(mesh, perm), perm=perm)
    A0, u0, k0 = _gpu_matrix(ah0, var, env=env)
    A1, u1, k1 = _gpu_matrix(ah1, var, env=env)
    assert (u0, k0) == (u1, k1) == ("rows", kernel), (u0, k0, u1, k1)
    m = am.permutation_map(ah0, ah1, perm)
    assert np.max(np.abs(A1[np.ix_(m, m)] - A0)) <= 1e-13 * np.max(np.abs(A0))


@pytest.mark.parametrize("basis,p", [("dgq", 3), ("dgq", 2), ("dgp", 3)])
@pytest.mark.parametrize("k", [-20, 10])
def test_scale(k, basis, p):
    """The domain scaled by 2^k (poisson variant, no reaction term): A -> 2^(k (d - 2)) A to 1e-14 relative, with the same kernel."""
    fe = _fe(basis, 3, p)
    var = po.variant_poisson_example(fe)
    ah0 = am.oracle_handler("rect124", fe, p + 1)
    ah1 = am.oracle_handler("rect124", _fe(basis, 3, p), p + 1, scale=2.0 ** k)
    kw0, kw1 = flatten(ah0, var), flatten(ah1, var)
    v0, u0, k0 = _run(kw0)
    v1, u1, k1 = _run(kw1)
    assert (u0, k0) == (u1, k1) == ("rows", "terms"), (u0, k0, u1, k1)
    assert np.max(np.abs(v1 - 2.0 ** k * v0)) <= 1e-14 * 2.0 ** k * np.max(np.abs(v0))
