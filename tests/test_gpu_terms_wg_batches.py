"""The FE_DGQ(3) workgroup term kernel (pdh_terms_wg.h) with workgroups that take SEVERAL polytopes: writer waves that store polytope k
from one table buffer while builder waves make the tables of polytope k + 1 in the other.  PDH_TERMS_WG_BATCH = N launches
ceil(n_owned / N) workgroups (without it a small problem has one workgroup per polytope and never leaves the prologue); a workgroup's
first two polytopes are fixed (b and b + number of workgroups), the following come from the device-wide counter: WHICH polytopes follow
each other in a workgroup's buffers beyond the second is not fixed from run to run (with one workgroup it is: all, in order).  Every case:
per-block parity against the oracle (tests/parity.py), and the row kernel in use is asserted."""
import contextlib
import functools
import os

import numpy as np
import pytest

import aniso_meshes as am
from flatten_oracle import flatten
from oracle import polydeal_oracle as po
from parity import assert_parity, assert_parity_ah
from test_gpu_anisotropic import _case, _run

pytestmark = pytest.mark.gpu


def _env(batch, waves=8):
    return {"PDH_TERMS_WG_BATCH": str(batch), "PDH_TERMS_WG_WAVES": str(waves)}


@contextlib.contextmanager
def _environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, o in old.items():
            if o is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = o


def _check(kw, ref, ah, diag_first, env, what):
    v, used, kern = _run(kw, env=env)
    assert used == "rows" and kern == "terms", (used, kern)
    assert_parity_ah(v, ref, ah, diag_first, what="%s %s" % (what, env))


@pytest.mark.parametrize("waves", [8, 4])
@pytest.mark.parametrize("batch", [1, 2, 3, 5, 64])
@pytest.mark.parametrize("diag_first", [True, False])
def test_batch_boundaries(diag_first, batch, waves):
    """8 polytopes in 8, 4, 3, 2 workgroups and in one: a workgroup that only has its prologue; both buffers; buffer 0 used again; a
    workgroup that finds nothing left; one workgroup taking everything."""
    ah, var, kw, ref = _case("rect124", "dgq", 3, "poisson", diag_first)
    assert ah.n_agglomerates == 8
    _check(kw, ref, ah, diag_first, _env(batch, waves), "rect124")


@functools.lru_cache(maxsize=None)
def _cube27():
    """3 x 3 x 3 blocks of 2^3 cells, blocks in lexicographic order: corner, edge, corner, edge, face, ... - 3 to 6 neighbours, 0 to 3
    boundary faces from one polytope to the next"""
    grid = po.subdivided_hyper_cube(3, 6, 0.0, 1.0)
    ah = po.AgglomerationHandler(grid)
    for g in po.block_agglomerates(grid, 2):
        ah.define_agglomerate(g)
    fe = po.FE_DGQ(3, 3)
    ah.initialize_fe_values(4, 4)
    ah.distribute_agglomerated_dofs(fe)
    var = po.variant_poisson_example(fe)
    return ah, flatten(ah, var), po.assemble_csr(ah, var)[2]


@pytest.mark.parametrize("batch", [4, 27])
def test_no_stale_tables_pinwheel(batch):
    """Polytopes of 1 to 13 neighbours follow each other in a buffer: one whose previous user had more runs or sub-faces must not leak entries."""
    ah, var, kw, ref = _case("pinwheel", "dgq", 3, "dr", True)
    _check(kw, ref, ah, True, _env(batch), "pinwheel")


@pytest.mark.parametrize("batch", [4, 27])
def test_no_stale_tables_cube(batch):
    ah, kw, ref = _cube27()
    assert ah.n_agglomerates == 27
    _check(kw, ref, ah, False, _env(batch), "cube27")


@functools.lru_cache(maxsize=None)
def _graded_grown():
    """(the mesh of test_gpu_anisotropic.py::test_multi_row_kernel_on_graded_grown_agglomerates)"""
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
    return ah, flatten(ah, var), po.assemble_csr(ah, var)[2]


def test_staircase_agglomerates():
    ah, kw, ref = _graded_grown()
    _check(kw, ref, ah, False, _env(3), "graded grown")


def test_rank_local_rows():
    """Three row ranges of rect124 (3, 4 and 1 polytopes) in 2, 2 and 1 workgroups; the middle range starts and ends at odd polytopes, so
    no workgroup of a range has the polytopes a workgroup of the whole problem would have."""
    ah, var, kw, ref = _case("rect124", "dgq", 3, "poisson", True)
    n, parts = 64, []
    for p0, p1 in ((0, 3), (3, 7), (7, 8)):
        v, used, kern = _run(kw, env=_env(2), r0=p0 * n, r1=p1 * n)
        assert used == "rows" and kern == "terms", (used, kern)
        parts.append(v)
    assert_parity_ah(np.concatenate(parts), ref, ah, True, what="row ranges, two polytopes per workgroup")


def test_cartesian_description():
    import polydeal_amd as pa

    pfe = pa.FE_DGQ(3, 3)
    mah = am.mirror_handler("rect124", pfe, 4)
    ah, var, kw, ref = _case("rect124", "dgq", 3, "poisson", True)
    cf = mah.flatten_cartesian(pa.SipVariant.poisson_example(pfe), True, True)
    with _environ(_env(3)):
        ctx = pa.Context(0)
        ctx.set_problem(cf)
        assert ctx.algorithm_in_use() == "rows" and ctx.rows_kernel_in_use() == "terms"
        vals = ctx.assemble()
        ctx.close()
    orp, oci = ah.sparsity_pattern(True)
    assert_parity(vals, ref, orp, oci, pfe.n_dofs_per_cell, what="device-generated points, three polytopes per workgroup")


def test_diffusion_reaction():
    ah, var, kw, ref = _case("rect1116", "dgq", 3, "dr", False)
    _check(kw, ref, ah, False, _env(2), "rect1116 dr")


def test_repeated_launches_leave_the_counter_at_zero():
    """The workgroup that leaves last resets the work counter: a second and third assembly of the same resident problem give the same values."""
    import polydeal_amd as pa

    ah, var, kw, ref = _case("rect124", "dgq", 3, "poisson", True)
    with _environ(_env(3)):
        ctx = pa.Context(0)
        ctx.set_problem(pa.Problem(**kw))
        assert ctx.rows_kernel_in_use() == "terms"
        vs = [ctx.assemble().copy() for _ in range(3)]
        ctx.close()
    assert_parity_ah(vs[0], ref, ah, True, what="first launch")
    assert np.array_equal(vs[0], vs[1]) and np.array_equal(vs[0], vs[2])
