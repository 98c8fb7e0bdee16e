"""The host-only planner of the level transfers (csrc/pdh_transfer_plan.cpp), no GPU: the 1-D factors of every injection block against
the dense blocks of the oracle, the refusals of pdh_check_transfer with their codes, the order of the children CSR, and the NumPy
restatement of the two-grid cycle (tests/twogrid_ref.py) against the conditions the device test relies on."""
import numpy as np
import pytest

import transfer_cases as tc
from polydeal_amd import _capi


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_kronecker_of_the_1d_matrices_equals_the_oracle_block(case):
    """pdh_check_transfer accepts the case; for every fine polytope the Kronecker product of its 1-D matrices equals the oracle's dense
    block (raw descriptions: the NumPy Kronecker formula) within 1e-14 - the long double Horner evaluation against NumPy's product form
    was observed at 8e-16."""
    c = tc.build(case)
    c.desc.check()
    B = c.desc.matrices_1d()
    assert B.shape == (c.desc.n_fine, c.desc.dim, c.desc.degree + 1, c.desc.degree + 1)
    got = tc.dense_from_blocks(c.desc, tc.kron_blocks(B))
    err = float(np.max(np.abs(got - c.P)))
    print("%s: max |kron - oracle| = %.3e" % (tc.case_id(case), err))
    assert err <= 1e-14
    assert np.max(np.abs(B.sum(axis=3) - 1.0)) <= 1e-14  # the Lagrange polynomials sum to one


def test_handler_description_matches_the_oracle_handlers():
    """parents, boxes and dof offsets exported by the host mirror are those of the oracle's handlers"""
    from polydeal_amd.handler import transfer_parents

    c = tc.build(("pair", 3, 2, 4, 2, 2, 0.1))
    co, fo = c.oracles
    parent = np.array([co.polytope_of_cell(fo.get_agglomerate(F)[0]) for F in range(fo.n_agglomerates)])
    assert np.array_equal(c.desc.parent, parent)
    assert np.array_equal(transfer_parents(*c.handlers), parent)
    assert np.array_equal(c.desc.fine_dof_offset, fo.dof_offset) and np.array_equal(c.desc.coarse_dof_offset, co.dof_offset)
    assert np.array_equal(c.desc.fine_bbox, np.array([np.stack(b) for b in fo.bboxes]))
    assert (c.desc.n_fine_rows, c.desc.n_coarse_rows) == (fo.n_dofs, co.n_dofs)


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_children_are_in_ascending_fine_index(case):
    d = tc.build(case).desc
    ptr, idx = d.children()
    assert ptr[0] == 0 and ptr[-1] == d.n_fine and np.all(np.diff(ptr) >= 1)
    assert np.array_equal(np.sort(idx), np.arange(d.n_fine))
    for C in range(d.n_coarse):
        kids = idx[ptr[C]:ptr[C + 1]]
        assert np.all(np.diff(kids) > 0) and np.all(d.parent[kids] == C)
    if case == ("raw", "uneven"):
        assert list(np.diff(ptr)) == [6, 2]


@pytest.mark.parametrize("dim,n1d", tc.BOX_PAIRS, ids=lambda v: str(v))
def test_box_cases_have_the_shape_they_are_listed_for(dim, n1d):
    """one raw case per (dim, N1D) the kernels instantiate: children counts 1, 2, G + 3 (counts of both levels no multiples of G where
    G > 1), children of a parent not contiguous, permuted offsets, every child a proper sub-box with a different 1-D matrix on every
    axis; and the yardstick itself reproduces the degree-p polynomial far inside the 5e-13 the device test asks (degrees 5 .. 7 too)."""
    c = tc.build(("raw", "boxes_%dd_n%d" % (dim, n1d)))
    d, G = c.desc, tc.boxes_group(dim, n1d)
    assert (d.dim, d.degree + 1, d.n) == (dim, n1d, n1d ** dim) and G == (64 // d.n if d.n < 64 else 1)
    ptr, idx = d.children()
    assert sorted(np.diff(ptr)) == [1, 2, G + 3] and d.n_coarse == 3 and d.n_fine == G + 6
    if G > 1:  # (G = 2: G + 6 fine polytopes fill their waves; the coarse count still leaves an idle group)
        assert (d.n_fine % G or G == 2) and d.n_coarse % G
    assert np.any(np.diff(d.parent) < 0)  # the fine polytopes are not sorted by parent
    assert not np.array_equal(d.fine_dof_offset, d.n * np.arange(d.n_fine)) and not np.array_equal(d.coarse_dof_offset, d.n * np.arange(3))
    B = d.matrices_1d()
    for a in range(dim):
        for b in range(a):
            assert np.min(np.max(np.abs(B[:, a] - B[:, b]), axis=(1, 2))) > 1e-3     # no two axes alike
        assert np.min(np.max(np.abs(B[:, a] - B[:, a].transpose(0, 2, 1)), axis=(1, 2))) > 1e-4  # nor a factor symmetric
    pc = d.coarse_bbox[d.parent]
    assert np.all(d.fine_bbox[:, 0] > pc[:, 0]) and np.all(d.fine_bbox[:, 1] < pc[:, 1])
    f = tc.poly(dim, d.degree)
    err = float(np.max(np.abs(c.P @ tc.interpolate(d, "coarse", f) - tc.interpolate(d, "fine", f))))
    print("boxes %dD N1D %d: interpolant error of the yardstick %.3e" % (dim, n1d, err))
    assert err <= 5e-14


def _variant(base, **over):
    """a copy of a description with some fields replaced"""
    kw = dict(dim=base.dim, degree=base.degree, basis=base.basis, fine_bbox=base.fine_bbox.copy(), coarse_bbox=base.coarse_bbox.copy(),
              fine_dof_offset=base.fine_dof_offset.copy(), coarse_dof_offset=base.coarse_dof_offset.copy(), parent=base.parent.copy(),
              n_fine_rows=base.n_fine_rows, n_coarse_rows=base.n_coarse_rows)
    kw.update(over)
    return _capi.TransferDesc(**kw)


def _edit(a, index, value):
    a = a.copy()
    a[index] = value
    return a


def _malformed():
    b = tc.build(("raw", "uneven")).desc
    shifted = b.fine_bbox.copy()
    shifted[0, :, 0] -= 2e-12  # sticks out of the parent by 2e-12 of its extent (1.0) along x
    inside = b.fine_bbox.copy()
    inside[0, :, 0] -= 5e-13   # within the slack
    yield "agglodgp", _variant(b, basis=_capi.PDH_BASIS_AGGLODGP), _capi.PDH_EUNSUPPORTED
    yield "degree 0", _variant(b, degree=0), _capi.PDH_EUNSUPPORTED
    yield "degree 8 (2-D: more than 64 dofs)", _variant(b, degree=8), _capi.PDH_EUNSUPPORTED
    yield "parent out of range", _variant(b, parent=_edit(b.parent, 3, 2)), _capi.PDH_EINVAL
    yield "negative parent", _variant(b, parent=_edit(b.parent, 3, -1)), _capi.PDH_EINVAL
    yield "coarse polytope without children", _variant(b, parent=np.zeros(8)), _capi.PDH_EINVAL
    yield "degenerate fine box", _variant(b, fine_bbox=_edit(b.fine_bbox, (2, 1, 1), b.fine_bbox[2, 0, 1])), _capi.PDH_EINVAL
    yield "degenerate coarse box", _variant(b, coarse_bbox=_edit(b.coarse_bbox, (1, 1, 0), np.nan)), _capi.PDH_EINVAL
    yield "fine box outside its parent", _variant(b, fine_bbox=shifted), _capi.PDH_EINVAL
    yield "fine box in the wrong parent", _variant(b, parent=_edit(b.parent, 0, 1)), _capi.PDH_EINVAL
    yield "fine dofs overlap", _variant(b, fine_dof_offset=_edit(b.fine_dof_offset, 1, 5)), _capi.PDH_EINVAL
    yield "fine dofs leave the vector", _variant(b, n_fine_rows=b.n_fine_rows - 1), _capi.PDH_EINVAL
    yield "negative fine dof", _variant(b, fine_dof_offset=_edit(b.fine_dof_offset, 0, -1)), _capi.PDH_EINVAL
    yield "coarse dofs overlap", _variant(b, coarse_dof_offset=np.zeros(2)), _capi.PDH_EINVAL
    yield "coarse dofs leave the vector", _variant(b, n_coarse_rows=17), _capi.PDH_EINVAL
    yield "coarse level not smaller", _variant(b, fine_bbox=b.fine_bbox[:2], fine_dof_offset=b.fine_dof_offset[:2], parent=[0, 1],
                                               n_fine_rows=18), _capi.PDH_EINVAL
    yield "within the slack", _variant(b, fine_bbox=inside), _capi.PDH_OK


@pytest.mark.parametrize("what,desc,code", list(_malformed()), ids=[m[0] for m in _malformed()])
def test_check_transfer_refusals(what, desc, code):
    lib = _capi.load_library()
    import ctypes as C
    rc = lib.pdh_check_transfer(C.byref(desc.c))
    assert rc == code, (what, rc, lib.pdh_last_error(None).decode())
    if code != _capi.PDH_OK:
        assert lib.pdh_last_error(None).decode()
        out = np.zeros((desc.n_fine, desc.dim, desc.degree + 1, desc.degree + 1))
        assert lib.pdh_transfer_matrices_1d(C.byref(desc.c), out.ctypes.data) == code  # the other entries refuse alike
    assert lib.pdh_check_transfer(None) == _capi.PDH_EINVAL


def test_host_mirror_refuses_unnested_and_agglodgp_pairs():
    import polydeal_amd as pa
    from polydeal_amd.handler import transfer_description

    handlers = tc.build(("pair", 2, 3, 4, 2, 1, 0.0)).handlers
    with pytest.raises(pa.HostError):
        transfer_description(handlers[1], handlers[0])  # coarse must be smaller (utils.h:120)
    grid = handlers[0].grid
    levels = []
    for b in (4, 2):
        ah = pa.AgglomerationHandler(grid)
        ah.define_block_agglomerates(b)
        ah.initialize_fe_values(2, 2)
        ah.distribute_agglomerated_dofs(pa.FE_AggloDGP(2, 1))
        levels.append(ah)
    with pytest.raises(pa.HostError):
        transfer_description(*levels)


def test_twogrid_restatement_contracts_and_its_spread_is_recorded():
    """tests/twogrid_ref.py on the oracle's matrices: the residual falls below 0.05 of its start within twelve cycles on every pair (the
    condition the device test repeats), and the float64-versus-long-double spread of three cycles stays within the recorded constant."""
    import cheb_ref as cr
    import twogrid_ref as tg

    for pair in tc.TWOGRID_PAIRS:
        Af, Ac, n, P = tc.twogrid_oracle_system(pair)
        assert Ac.shape[0] <= 256
        lo, hi = cr.bounds(cr.estimate(Af, n, "block_jacobi")[0])
        b = tc.twogrid_rhs(Af.shape[0])
        x = np.zeros(len(b))
        for _ in range(12):
            x = tg.cycle(Af, Ac, n, P, lo, hi, tc.TWOGRID_DEGREE, b, x)
        fall = tg.residual_norm(Af, b, x) / np.linalg.norm(b)
        print(pair, "residual after 12 cycles / start = %.3e" % fall)
        assert fall < 0.05
    spread, where = tc.measure_twogrid_spread(verbose=False)
    assert spread <= 2 * tc.TWOGRID_SPREAD, (spread, where)  # (the constant enters the device bound 100-fold)
