"""The single-precision-smoother restatement (tests/mixed_ref.py) on oracle-assembled matrices, no GPU: the conditions that keep the
device tests of tests/test_gpu_smoother_f32.py honest.  The mixed V-cycle lies far enough from the double one that a device ignoring the
precision switch could not pass; it is still a symmetric positive operator; PCG pays at most one iteration for it; the shapes are what
they say; header, library and ctypes agree on what the feature adds."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mixed_cases as mc
import mixed_ref as mr
import pcg_ref
import vcycle_cases as vc
import vcycle_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.2e-16
REL_TOL = 1e-13  # of the PCG runs


def _rel(x, ref):
    return float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("case", vc.CASES, ids=vc.case_id)
def test_the_mixed_cycle_is_far_from_the_double_cycle(case):
    """one and three cycles: |x_mixed - x_double|_inf / |x_double|_inf >= 1000 x the bound the device is held to"""
    H = vc.oracle_hierarchy(case)
    M = mr.Hierarchy(H)
    b = vc.rhs(H.mats[-1].shape[0])
    bound = mc.MIXED_CYCLE_TOL + 10.0 * float(np.linalg.cond(H.mats[0].toarray())) * EPS
    xm, xd = None, None
    for cyc in range(3):
        xm, xd = mr.cycle(M, b, xm), vr.cycle(H, b, xd)
        print("%s: cycle %d: mixed against double %.3e (device bound %.3e)" % (vc.case_id(case), cyc + 1, _rel(xm, xd), bound))
        if cyc in (0, 2):
            assert _rel(xm, xd) >= mc.SEPARATION * bound, (cyc, _rel(xm, xd), bound)
    # levels mix: the finest level alone in F32 is a third operator
    F = mr.Hierarchy(H, f32=[False] * (len(H.mats) - 1) + [True])
    xf = mr.cycle(F, b)
    if len(H.mats) > 2:
        assert _rel(xf, mr.cycle(M, b)) >= mc.SEPARATION * bound
    assert _rel(xf, vr.cycle(H, b)) >= mc.SEPARATION * bound
    # with no level in F32 the restatement is vcycle_ref's, bit for bit
    assert np.array_equal(mr.cycle(mr.Hierarchy(H, f32=[False] * len(H.mats)), b), vr.cycle(H, b))


@pytest.mark.parametrize("sid", list(mc.CHEB_SHAPES))
def test_the_mixed_application_is_far_from_the_double_one(sid):
    """every application the device test compares - inner kinds, degrees 1, 2, 5, zero and non-zero start - lies 1000 bounds from the
    double application where a shadow entry enters it, and IS the double application where none does"""
    import cheb_ref as cr

    A, n = mc.oracle_system(sid)
    b, x0 = mc.vectors(A.shape[0])
    for kind in mc.kinds_of(sid):
        lo, hi = cr.bounds(cr.estimate(A, n, kind)[0])
        S = mr.Smoother(A, n, kind)
        for m in mc.DEGREES:
            for start in (None, x0):
                zm, zd = S.apply(lo, hi, m, b, start), cr.apply(A, n, kind, lo, hi, m, b, start)
                if not mc.shadow_enters(kind, m, start is None):
                    assert np.array_equal(zm, zd)
                elif (sid, kind) not in mc.ILL_CONDITIONED:
                    print("%s %s degree %d %s: %.3e" % (sid, kind, m, "zero" if start is None else "non-zero", _rel(zm, zd)))
                    assert _rel(zm, zd) >= mc.SEPARATION * mc.z_tol(sid, kind), (kind, m, _rel(zm, zd))


@pytest.mark.parametrize("case", vc.CPU_CASES, ids=vc.case_id)
def test_the_mixed_cycle_is_symmetric(case):
    """u^T M v = v^T M u for the applied mixed cycle M (from zero), within the 1e-12 |u| |M v| of test_vcycle_cpu.py"""
    H = mr.Hierarchy(vc.oracle_hierarchy(case))
    rng = np.random.default_rng(5)
    N = H.mats[-1].shape[0]
    for _ in range(3):
        u, v = rng.standard_normal(N), rng.standard_normal(N)
        Mv, Mu = mr.cycle(H, v), mr.cycle(H, u)
        a, b = float(u @ Mv), float(v @ Mu)
        scale = float(np.linalg.norm(u) * np.linalg.norm(Mv))
        print("%s: u^T M v = %.15e, v^T M u = %.15e, difference / scale = %.3e" % (vc.case_id(case), a, b, abs(a - b) / scale))
        assert abs(a - b) <= 1e-12 * scale


def test_the_mixed_cycle_is_positive():
    """dense eigenvalues of the applied mixed cycle on the 256-row case"""
    H = mr.Hierarchy(vc.oracle_hierarchy(vc.CASES[0]))
    N = H.mats[-1].shape[0]
    assert N == 256
    M = np.stack([mr.cycle(H, e) for e in np.eye(N)], axis=1)
    assert np.max(np.abs(M - M.T)) <= 1e-12 * np.max(np.abs(M))
    ev = np.linalg.eigvalsh((M + M.T) / 2)
    print("eigenvalues of the mixed cycle: %.3e .. %.3e" % (ev[0], ev[-1]))
    assert ev[0] > 0


def test_the_rounded_block_inverses_stay_symmetric():
    A = vc.oracle_hierarchy(vc.CASES[0]).mats[-1]
    inv = np.linalg.inv(pcg_ref.diag_blocks(A, 4))
    inv = (inv + inv.transpose(0, 2, 1)) / 2
    r = mr.round32(inv)
    assert np.array_equal(r, r.transpose(0, 2, 1)) and not np.array_equal(r, inv)
    At = mr.rounded_matrix(A)
    assert np.array_equal(At.indices, A.indices) and np.array_equal(At.data, A.data.astype(np.float32).astype(np.float64))
    assert 0 < abs(At - A).max() <= 2.0 ** -24 * abs(A).max()


@pytest.mark.parametrize("case", list(vc.CPU_CASES) + [vc.MESH_PAIR[1]], ids=vc.case_id)
def test_pcg_pays_at_most_one_iteration_for_the_mixed_cycle(case):
    H = vc.oracle_hierarchy(case)
    A = H.mats[-1]
    b = vc.rhs(A.shape[0])
    x_d, it_d, _ = pcg_ref.pcg(A, b, vr.preconditioner(H), rel_tol=REL_TOL)
    x_m, it_m, res = pcg_ref.pcg(A, b, mr.preconditioner(mr.Hierarchy(H)), rel_tol=REL_TOL)
    print("%s: PCG iterations to %.0e: double cycle %d, mixed cycle %d" % (vc.case_id(case), REL_TOL, it_d, it_m))
    assert it_m <= it_d + 1
    assert res <= REL_TOL * np.linalg.norm(b)
    assert np.linalg.norm(x_m - x_d) <= 1e-9 * np.linalg.norm(x_d)


def test_mesh_pair_is_covered():
    assert vc.MESH_PAIR[0] in vc.CPU_CASES  # (the coarser of the pair is a CPU case: the test above runs both)


@pytest.mark.parametrize("sid", list(mc.CHEB_SHAPES))
def test_shapes_are_what_they_say(sid):
    ah, fe, flat = mc.mirror_flat(sid, True)
    mc.check_shape_property(sid, fe.n_dofs_per_cell, ah.n_agglomerates, flat.arrays()["rowptr"])


def test_bounds_follow_the_measured_spreads():
    assert set(mc.MIXED_Z_SPREAD) == {(sid, kind) for sid in mc.CHEB_SHAPES for kind in mc.kinds_of(sid)}
    assert all(0.0 < v < 1e-13 for k, v in mc.MIXED_Z_SPREAD.items() if k not in mc.ILL_CONDITIONED) and 0.0 < mc.MIXED_CYCLE_SPREAD < 1e-13
    assert all(mc.z_tol(*k) == max(100 * v, 1e-13) for k, v in mc.MIXED_Z_SPREAD.items())
    assert mc.MIXED_CYCLE_TOL == max(100 * mc.MIXED_CYCLE_SPREAD, 1e-13)
    assert not mc.shadow_enters("jacobi", 1, True) and mc.shadow_enters("jacobi", 1, False) and mc.shadow_enters("block_jacobi", 1, True)


def test_header_library_and_ctypes_agree_on_the_new_entry_points():
    """fails without the feature: the three symbols are declared, exported, listed and bound with a typed context argument"""
    from polydeal_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "polydeal_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(PDH_\w+)\s+(-?\d+)", hdr)}
    assert defs["PDH_SMOOTHER_F64"] == _capi.PDH_SMOOTHER_F64 == 0 and defs["PDH_SMOOTHER_F32"] == _capi.PDH_SMOOTHER_F32 == 1
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _capi.load_library()
    for sym in ("pdh_set_smoother_precision", "pdh_smoother_precision", "pdh_smoother_vmult_device"):
        assert sym in _capi.EXPORTS and re.search(r"\b%s\s*\(" % sym, body), sym
        assert hasattr(lib, sym), sym
        assert getattr(lib, sym).argtypes[0] is _capi.pdh_ctx_p, sym
    # a NULL context is an argument error answered on the host
    assert lib.pdh_set_smoother_precision(None, _capi.PDH_SMOOTHER_F32) == _capi.PDH_EINVAL
    assert lib.pdh_smoother_precision(None) < 0
    assert lib.pdh_smoother_vmult_device(None, None, None) == _capi.PDH_EINVAL
    for name in ("set_smoother_precision", "smoother_precision", "smoother_vmult_device"):
        assert hasattr(_capi.Context, name), name


def test_the_new_unit_passes_the_isa_lint_and_uses_no_scratch(tmp_path):
    """csrc/pdh_shadow.hip compiled to gfx950 assembly (no GPU): six kernels, no finding of tools/isa_lint.py, no scratch memory - the
    product kernel keeps up to sixteen pieces of a row pair in registers, and a spill would go unnoticed in every other test"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    dst = str(tmp_path / "pdh_shadow.s")
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-result", "-Wno-unused-command-line-argument",
                        "-S", "--cuda-device-only", os.path.join(ROOT, "polydeal_amd", "csrc", "pdh_shadow.hip"), "-o", dst],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    kernels, meta = isa_lint.parse(dst)
    names = sorted(kernels)
    assert len(names) == 6 and sum("k_vmult_f32" in k for k in names) == 1 and sum("k_shadow_rows" in k for k in names) == 2, names
    for name in names:
        assert not isa_lint.lint_kernel(name, kernels[name]), name
        m = meta.get(name + ".kd", meta.get(name, {}))
        assert m.get("private_segment_fixed_size", 0) == 0 and m.get("vgpr_spill_count", 0) == 0, (name, m)
