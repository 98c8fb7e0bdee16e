"""The identities the matrix-free operator rests on, on the CPU (no GPU): the term form restated in NumPy (tests/matfree_ref.py) against
the oracle's matrix on every case of tests/matfree_cases.py, its product by sum factorisation against the dense product, FE_AggloDGP
by embedding against the direct truncated sum, the recorded spread of the yardstick, and the C ABI's host-side answers."""
import ctypes as C

import numpy as np
import pytest

import cheb_cases as cc
import matfree_cases as mc
import parity


@pytest.mark.parametrize("cid", list(mc.CASES))
def test_term_form_is_the_oracles_matrix(cid):
    """dense() equals the oracle's matrix to 1e-12 per block (tests/parity.py) - cells M | K, sub-faces D, coupling X, signs, frames,
    sigma of either owner, boundary weights - and the case has the property it is listed for"""
    ah, _ = mc.oracle_handler(cid)
    mc.check_property(cid, ah)
    A = mc.oracle_matrix(cid)
    got = mc.term_form(cid).csr_values(diag_first=False)
    assert got.shape == A.data.shape
    worst = parity.assert_parity(got, A.data, A.indptr, A.indices, ah.fe.n_dofs_per_cell, what=cid)
    print(cid, "term form against the oracle: %.2e max|A|" % worst)


@pytest.mark.parametrize("cid", list(mc.CASES))
def test_factorised_product_is_the_dense_product(cid):
    """apply(x) by three passes per term equals dense() @ x, per row within 1e-13 sum_j |A_ij| |x_j| (the project's bound of a product;
    dense() itself is a float64 sum of the terms, so the long-double passes are held to the same)"""
    tf = mc.term_form(cid)
    D = tf.dense()
    for x in cc.vectors(D.shape[0]):
        scale = np.abs(D) @ np.abs(x)
        ref = D.astype(np.longdouble) @ x.astype(np.longdouble)
        e64 = float(np.max(np.abs(tf.apply(x) - ref) / scale))
        eld = float(np.max(np.abs(tf.apply(x, np.longdouble) - ref) / scale))
        print(cid, "apply against dense @ x: float64 %.2e, long double %.2e" % (e64, eld))
        assert e64 <= 1e-13 and eld <= 1e-13


@pytest.mark.parametrize("cid", [c for c in mc.CASES if mc.CASES[c][2] == "dgp"])
def test_embedding_is_the_truncated_sum(cid):
    """FE_AggloDGP embedded in the full tensor with zeros, rows of the index set kept, equals the direct sum over the index set"""
    tf = mc.term_form(cid)
    assert tf.n < tf.N ** 3 and len(set(tf.full_index)) == tf.n
    x = cc.vectors(tf.ah.n_dofs)[0]
    y, ref = tf.apply(x), tf.apply_truncated(x)
    scale = np.abs(tf.dense()) @ np.abs(x)
    assert np.max(np.abs(y - ref) / scale) <= 1e-13


def test_recorded_spread_is_the_measured_one():
    """PRODUCT_SPREAD (python tests/matfree_cases.py) on the case it names, and the bound the device is held to"""
    s = mc.product_spread(mc.PRODUCT_SPREAD_CASE)
    print("spread of %s: %.3e (recorded %.3e), PRODUCT_TOL %.3e" % (mc.PRODUCT_SPREAD_CASE, s, mc.PRODUCT_SPREAD, mc.PRODUCT_TOL))
    assert s == pytest.approx(mc.PRODUCT_SPREAD, rel=1e-3)
    assert mc.PRODUCT_TOL == max(100 * mc.PRODUCT_SPREAD, 1e-13)


# ---- C ABI, host only ------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("pdh_setup_matrix_free", "pdh_matrix_free_vmult", "pdh_matrix_free_vmult_device", "pdh_set_smoother_operator",
               "pdh_smoother_operator")


def test_entry_points_exist_and_answer_a_null_context():
    """the five symbols are exported, take a typed context, and answer ctx = NULL on the host with PDH_EINVAL 'ctx is NULL'"""
    from polydeal_amd import _capi

    lib = _capi.load_library()
    lib.pdh_last_error.restype = C.c_char_p
    buf = np.zeros(8)
    for name in NEW_SYMBOLS:
        assert name in _capi.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes[0] is _capi.pdh_ctx_p, name
        args = [None]
        for t in fn.argtypes[1:]:
            args.append(1 if t is C.c_int else (buf.ctypes.data if t is C.c_void_p else None))
        assert fn(*args) == _capi.PDH_EINVAL, name
        assert lib.pdh_last_error(None).decode() == "ctx is NULL", name


def test_smoother_operator_argument_is_range_checked():
    from polydeal_amd import _capi

    assert _capi.smoother_operator_code("stored") == _capi.PDH_SMOOTHER_OP_STORED == 0
    assert _capi.smoother_operator_code("matrix_free") == _capi.PDH_SMOOTHER_OP_MATRIX_FREE == 1
    assert _capi.smoother_operator_code(1) == 1
    for bad in ("f32", "", 2, -1):
        with pytest.raises(ValueError):
            _capi.smoother_operator_code(bad)
    from polydeal_amd.levels import multigrid_hierarchy
    with pytest.raises(ValueError):
        multigrid_hierarchy([], None, inner="jacobi", smoother_operator="float")


def test_the_new_unit_passes_the_isa_lint_and_uses_no_scratch(tmp_path):
    """csrc/pdh_matfree.hip compiled to gfx950 assembly (no GPU): twelve table kernels (six kinds, 4- and 8-slot records), six product
    kernels, no finding of tools/isa_lint.py, no scratch memory"""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import isa_lint

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    dst = str(tmp_path / "pdh_matfree.s")
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-result", "-Wno-unused-command-line-argument",
                        "-S", "--cuda-device-only", os.path.join(root, "polydeal_amd", "csrc", "pdh_matfree.hip"), "-o", dst],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    kernels, meta = isa_lint.parse(dst)
    names = sorted(kernels)
    assert sum("k_mf_tables" in k for k in names) == 12 and sum("k_mf_vmult" in k for k in names) == 6 and len(names) == 18, names
    for name in names:
        assert not isa_lint.lint_kernel(name, kernels[name]), name
        m = meta.get(name + ".kd", meta.get(name, {}))
        assert m.get("private_segment_fixed_size", 0) == 0 and m.get("vgpr_spill_count", 0) == 0, (name, m)
