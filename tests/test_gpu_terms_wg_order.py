"""The store policies of k_terms_wg's writers (pdh_terms_wg.h: template arguments AUX and DRAIN) in a diagnostic build of the library
(`make -C polydeal_amd/csrc variants`: build/variants/libpolydeal_hip.so, -DPDHT_VARIANTS, which build() of __graft_entry__.py makes with
the library); skipped only where that build is absent.
pdh_debug_terms_wg_variant re-resolves the row launch of ONE resident problem, so all variants of a case write the same allocation.
Every variant the source holds: per-block parity against the oracle (tests/parity.py, 1e-12) and the bits of the baseline (nt stores
left in flight) - the policy changes neither the sums nor their order."""
import ctypes as C
import os

import numpy as np
import pytest

from parity import assert_parity_ah
from test_gpu_anisotropic import ROOT, _case
from test_gpu_terms_wg_batches import _cube27, _env, _environ, _graded_grown

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "build", "variants", "libpolydeal_hip.so")
# (order, aux, drain) of pdh_debug_terms_wg_variant: the baseline (nt stores left in flight), then the library's policy (sc1|nt, drained)
VARIANTS = [(0, 2, 0), (0, 18, 1)]


def _run_variants(kw, env, r0=0, r1=None, launches=1):
    """[values of every launch] per variant, of one context of the diagnostic library"""
    import polydeal_amd as pa

    if not os.path.exists(LIB):
        pytest.skip("no -DPDHT_VARIANTS library in build/variants/ (make -C polydeal_amd/csrc variants)")
    out = []
    with _environ(env):
        ctx = pa.Context(0, lib_path=LIB)
        ctx.lib.pdh_debug_terms_wg_variant.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        ctx.lib.pdh_debug_terms_wg_variant.restype = C.c_int
        ctx.set_problem(pa.Problem(**kw), r0, r1)
        assert ctx.algorithm_in_use() == "rows" and ctx.rows_kernel_in_use() == "terms"
        for order, aux, drain in VARIANTS:
            ctx._chk(ctx.lib.pdh_debug_terms_wg_variant(ctx.h, order, aux, drain))
            out.append([ctx.assemble().copy() for _ in range(launches)])
        ctx.close()
    return out


def _check(kw, ref, ah, diag_first, env, what):
    vs = _run_variants(kw, env)
    for variant, (v,) in zip(VARIANTS, vs):
        assert_parity_ah(v, ref, ah, diag_first, what="%s %s variant %s" % (what, env, variant))
        assert np.array_equal(v, vs[0][0]), (what, variant)


@pytest.mark.parametrize("batch", [1, 3, 64])
@pytest.mark.parametrize("diag_first", [True, False])
def test_rect124(diag_first, batch):
    """8 polytopes: a workgroup each (prologue only), three workgroups, one workgroup taking everything; both row layouts."""
    ah, var, kw, ref = _case("rect124", "dgq", 3, "poisson", diag_first)
    assert ah.n_agglomerates == 8
    _check(kw, ref, ah, diag_first, _env(batch), "rect124")


def test_cube27():
    """One interior polytope with 7 pieces; the own piece at every position of a row."""
    ah, kw, ref = _cube27()
    assert ah.n_agglomerates == 27
    _check(kw, ref, ah, False, _env(4), "cube27")


def test_pinwheel():
    """1 to 13 neighbours: rows of up to 14 pieces, and polytopes of fewer runs behind ones of more in the same table buffer."""
    ah, var, kw, ref = _case("pinwheel", "dgq", 3, "dr", True)
    _check(kw, ref, ah, True, _env(4), "pinwheel")


def test_graded_grown_agglomerates():
    ah, kw, ref = _graded_grown()
    _check(kw, ref, ah, False, _env(3), "graded grown")


def test_single_cell_polytopes():
    """Rules of four points per direction: the 4-slot instantiations."""
    ah, var, kw, ref = _case("rect124_2", "dgq", 3, "poisson", True)
    _check(kw, ref, ah, True, _env(3), "rect124_2")


def test_rank_local_rows_from_an_odd_polytope():
    ah, var, kw, ref = _case("rect124", "dgq", 3, "poisson", True)
    n = 64
    parts = [_run_variants(kw, _env(2), p0 * n, p1 * n) for p0, p1 in ((0, 3), (3, 7), (7, 8))]
    for i, variant in enumerate(VARIANTS):
        v = np.concatenate([p[i][0] for p in parts])
        assert_parity_ah(v, ref, ah, True, what="row ranges, variant %s" % (variant,))
        assert np.array_equal(v, np.concatenate([p[0][0] for p in parts])), variant


def test_three_launches_in_a_row():
    """The workgroup that leaves last puts the work counter back, under every policy and from one policy to the next."""
    ah, var, kw, ref = _case("rect124", "dgq", 3, "poisson", True)
    vs = _run_variants(kw, _env(3), launches=3)
    assert_parity_ah(vs[0][0], ref, ah, True, what="first launch")
    for variant, launches in zip(VARIANTS, vs):
        for v in launches:
            assert np.array_equal(v, vs[0][0]), variant


def test_the_policy_asked_for_reaches_the_resolver():
    """Bit-identical matrices cannot tell whether a switch selected another kernel: a policy the source does not hold (nt drained,
    sc1|nt in flight, any other bits) is refused by pdh_resolve_terms - which therefore reads aux and drain - and so is any order but
    piece-major; a refusal leaves the launch as it was."""
    import polydeal_amd as pa
    from polydeal_amd import _capi

    if not os.path.exists(LIB):
        pytest.skip("no -DPDHT_VARIANTS library in build/variants/ (make -C polydeal_amd/csrc variants)")
    ah, var, kw, ref = _case("rect124", "dgq", 3, "poisson", True)
    with _environ(_env(3)):
        ctx = pa.Context(0, lib_path=LIB)
        fn = ctx.lib.pdh_debug_terms_wg_variant
        fn.argtypes, fn.restype = [C.c_void_p, C.c_int, C.c_int, C.c_int], C.c_int
        assert fn(ctx.h, 0, 2, 0) == _capi.PDH_ESTATE  # (nothing resident yet)
        ctx.set_problem(pa.Problem(**kw))
        assert fn(ctx.h, 0, 2, 0) == _capi.PDH_OK
        for order, aux, drain in ((0, 2, 1), (0, 18, 0), (0, 0, 0), (0, 16, 1)):
            assert fn(ctx.h, order, aux, drain) == _capi.PDH_EUNSUPPORTED, (order, aux, drain)
            assert b"store policy" in ctx.lib.pdh_last_error(ctx.h)
        assert fn(ctx.h, 1, 18, 1) == _capi.PDH_EINVAL
        v = ctx.assemble()
        ctx.close()
    assert_parity_ah(v, ref, ah, True, what="after refused policies")
