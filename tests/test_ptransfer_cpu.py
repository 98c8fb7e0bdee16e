"""p-transfers without a GPU: the injection between two degrees on one box is exact (independent of any table), the planner's tables
(pdh_ptransfer_matrix_1d, pdh_ptransfer_index_map) against the oracle's, every refusal of pdh_check_ptransfer and of
handler.p_transfer_description, and the NumPy restatement of the p-V-cycle (tests/pmg_ref.py) on oracle-assembled matrices: symmetric,
positive, and a better preconditioner than Chebyshev alone.  Cases and recorded figures: tests/ptransfer_cases.py."""
import numpy as np
import pytest

import cheb_ref as cr
import pcg_ref
import pmg_ref
import ptransfer_cases as pc

import polydeal_amd as pa
from polydeal_amd import _capi
from polydeal_amd._capi import PTransferDesc
from polydeal_amd.handler import p_transfer_description


@pytest.mark.parametrize("pair", pc.EXACT_PAIRS, ids=lambda c: "%dto%d" % c)
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("basis", ["dgq", "dgp"])
def test_the_injection_is_exact(basis, dim, pair):
    """the coarse function and the fine function with coefficients P c agree at random points of the box, within 1e-13 sum_j |c_j phi_j(x)|"""
    from oracle import polydeal_oracle as po

    q, p = pair
    mk = po.FE_DGQ if basis == "dgq" else po.FE_AggloDGP
    rng = np.random.default_rng(11)
    c = rng.standard_normal(mk(dim, q).n_dofs_per_cell)
    pts = rng.random((50, dim))
    vc_, vf = mk(dim, q).shape(pts)[0], mk(dim, p).shape(pts)[0]
    coarse, fine = vc_ @ c, vf @ (pmg_ref.block(dim, basis, q, p) @ c)
    scale = np.abs(vc_) @ np.abs(c)
    print("max |coarse - fine| / scale = %.3e" % float(np.max(np.abs(coarse - fine) / scale)))
    assert np.all(np.abs(coarse - fine) <= 1e-13 * scale)


def _desc(dim, basis, q, p, count=2):
    b = pa.PDH_BASIS_DGQ if basis == "dgq" else pa.PDH_BASIS_AGGLODGP
    n_f, n_c = pc.n_dofs(dim, basis, p), pc.n_dofs(dim, basis, q)
    return PTransferDesc(dim=dim, fine_degree=p, coarse_degree=q, basis=b, fine_dof_offset=np.arange(count) * n_f,
                         coarse_dof_offset=np.arange(count) * n_c)


@pytest.mark.parametrize("pair", pc.ALL_PAIRS, ids=lambda c: "%dto%d" % c)
def test_tables_against_the_oracle(pair):
    q, p = pair
    assert pc.MATRIX_1D_TOL == pytest.approx(100 * pc.MATRIX_1D_SPREAD) and pc.MATRIX_1D_SPREAD > 1e-16
    for dim in (2, 3):
        B = _desc(dim, "dgq", q, p).matrix_1d()
        ref = pmg_ref.matrix_1d(q, p)
        print("%dD: max |B - oracle| = %.3e" % (dim, float(np.max(np.abs(B - ref)))))
        assert B.shape == ref.shape == (p + 1, q + 1) and np.max(np.abs(B - ref)) <= pc.MATRIX_1D_TOL
        m = _desc(dim, "dgp", q, p).index_map()
        assert np.array_equal(m, pmg_ref.index_map(dim, q, p))
    if pair == (1, 2):
        assert list(_desc(2, "dgp", 1, 2).index_map()) == [0, 1, 3]
    if pair == (2, 3):
        assert list(_desc(2, "dgp", 2, 3).index_map()) == [0, 1, 2, 4, 5, 7]


def test_the_1d_matrix_against_long_double():
    """the planner rounds a long-double Horner evaluation once: it is closer to the long-double product form than the oracle's own"""
    for q, p in pc.ALL_PAIRS:
        B = _desc(2, "dgq", q, p).matrix_1d()
        assert np.max(np.abs(B.astype(np.longdouble) - pc.matrix_1d_longdouble(q, p))) <= 1e-15


def _refused(d, code, word):
    with pytest.raises(pa.PdhError) as ei:
        d.check()
    assert ei.value.code == code and word in str(ei.value), str(ei.value)


def test_every_refusal_of_check_ptransfer():
    lib = pa.load_library()
    assert lib.pdh_check_ptransfer(None) == _capi.PDH_EINVAL and b"NULL" in lib.pdh_last_error(None)
    ok = dict(dim=3, fine_degree=3, coarse_degree=1, fine_dof_offset=[0, 64], coarse_dof_offset=[8, 0])
    PTransferDesc(**ok).check()
    PTransferDesc(**dict(ok, basis=pa.PDH_BASIS_AGGLODGP, fine_dof_offset=[0, 20], coarse_dof_offset=[4, 0])).check()
    _refused(PTransferDesc(**dict(ok, dim=4)), _capi.PDH_EINVAL, "dim")
    _refused(PTransferDesc(**dict(ok, basis=7)), _capi.PDH_EINVAL, "basis")
    # the order: a bad basis is reported before bad degrees, bad degrees before bad offsets
    _refused(PTransferDesc(**dict(ok, basis=7, fine_degree=9)), _capi.PDH_EINVAL, "basis")
    for q, p in ((0, 2), (2, 2), (3, 2), (1, 8), (7, 8)):
        _refused(PTransferDesc(**dict(ok, coarse_degree=q, fine_degree=p, n_fine_rows=1, n_coarse_rows=1)), _capi.PDH_EUNSUPPORTED, "degree")
    d = PTransferDesc(**ok)
    d.c.n_polytopes = 0
    _refused(d, _capi.PDH_EINVAL, "n_polytopes")
    for field in ("fine_dof_offset", "coarse_dof_offset"):
        d = PTransferDesc(**ok)
        setattr(d.c, field, None)
        _refused(d, _capi.PDH_EINVAL, "dof_offset")
    _refused(PTransferDesc(**dict(ok, fine_dof_offset=[0, 63])), _capi.PDH_EINVAL, "overlap")
    _refused(PTransferDesc(**dict(ok, coarse_dof_offset=[7, 0])), _capi.PDH_EINVAL, "overlap")
    _refused(PTransferDesc(**dict(ok, fine_dof_offset=[0, 65])), _capi.PDH_EINVAL, "leave")
    _refused(PTransferDesc(**dict(ok, fine_dof_offset=[-1, 64])), _capi.PDH_EINVAL, "leave")
    _refused(PTransferDesc(**dict(ok, n_coarse_rows=15)), _capi.PDH_EINVAL, "coarse")
    # the tables of the other basis
    with pytest.raises(pa.PdhError) as ei:
        PTransferDesc(**ok).index_map()
    assert ei.value.code == _capi.PDH_EINVAL
    with pytest.raises(pa.PdhError) as ei:
        PTransferDesc(**dict(ok, basis=pa.PDH_BASIS_AGGLODGP, fine_dof_offset=[0, 20], coarse_dof_offset=[4, 0])).matrix_1d()
    assert ei.value.code == _capi.PDH_EINVAL
    # the h-transfer's refusal of FE_AggloDGP stays
    with pytest.raises(pa.PdhError) as ei:
        _capi.TransferDesc(dim=2, degree=1, basis=pa.PDH_BASIS_AGGLODGP, fine_bbox=np.zeros((2, 2, 2)), coarse_bbox=np.zeros((1, 2, 2)),
                           fine_dof_offset=[0, 4], coarse_dof_offset=[0], parent=[0, 0]).check()
    assert ei.value.code == _capi.PDH_EUNSUPPORTED


def _handler(fe, block=2, lg=2, hi=1.0):
    grid = pa.BackgroundGrid.hyper_cube_refined(fe.dim, 0.0, hi, lg)
    ah = pa.AgglomerationHandler(grid)
    ah.define_block_agglomerates(block)
    ah.initialize_fe_values(fe.degree + 1, fe.degree + 1)
    ah.distribute_agglomerated_dofs(fe)
    return ah


def test_p_transfer_description_and_its_refusals():
    coarse, fine = _handler(pa.FE_DGQ(2, 1)), _handler(pa.FE_DGQ(2, 3))
    d = p_transfer_description(coarse, fine)
    d.check()
    assert (d.dim, d.coarse_degree, d.fine_degree, d.basis, d.n_polytopes) == (2, 1, 3, pa.PDH_BASIS_DGQ, 4)
    assert (d.n_coarse_rows, d.n_fine_rows) == (coarse.n_dofs, fine.n_dofs) == (16, 64)
    assert list(d.fine_dof_offset) == [0, 16, 32, 48] and list(d.coarse_dof_offset) == [0, 4, 8, 12]
    d = p_transfer_description(_handler(pa.FE_AggloDGP(3, 2)), _handler(pa.FE_AggloDGP(3, 3)))
    assert (d.basis, d.n_c, d.n_f) == (pa.PDH_BASIS_AGGLODGP, 10, 20)
    for c, f, word in ((coarse, _handler(pa.FE_DGQ(2, 3), block=1), "different polytopes"),   # another count
                       (coarse, _handler(pa.FE_DGQ(2, 3), hi=2.0), "boxes"),                   # the same count, other boxes
                       (coarse, _handler(pa.FE_AggloDGP(2, 3)), "kinds of basis"),
                       (coarse, _handler(pa.FE_DGQ(2, 1)), "degree"),
                       (fine, coarse, "degree")):
        with pytest.raises(pa.HostError) as ei:
            p_transfer_description(c, f)
        assert word in str(ei.value), str(ei.value)


def test_level_pairs_of_p_multigrid_hierarchy_are_checked_before_any_device_work():
    from polydeal_amd.levels import p_multigrid_hierarchy

    a, b = _handler(pa.FE_DGQ(2, 1)), _handler(pa.FE_DGQ(2, 2), block=1)
    with pytest.raises(ValueError, match="levels 0 and 1"):
        p_multigrid_hierarchy([a, b])  # neither the same polytopes nor the same degree
    with pytest.raises(ValueError, match="levels 1 and 2"):
        p_multigrid_hierarchy([a, _handler(pa.FE_DGQ(2, 2)), _handler(pa.FE_AggloDGP(2, 3))])
    with pytest.raises(ValueError, match="levels 0 and 1"):
        p_multigrid_hierarchy([_handler(pa.FE_DGQ(2, 2)), a])


@pytest.mark.parametrize("name", pc.CPU_HIERARCHIES)
def test_the_restated_p_vcycle_is_symmetric_positive_and_beats_chebyshev(name):
    H = pc.oracle_hierarchy(name)
    A = H.mats[-1]
    N = A.shape[0]
    assert tuple(M.shape[0] for M in H.mats) == pc.ROWS[name]
    rng = np.random.default_rng(5)
    u, v = rng.standard_normal(N), rng.standard_normal(N)
    Mu, Mv = pmg_ref.cycle(H, u), pmg_ref.cycle(H, v)
    asym = abs(float(u @ Mv) - float(v @ Mu)) / (np.linalg.norm(u) * np.linalg.norm(Mv))
    print("%s: asymmetry %.3e" % (name, asym))
    assert asym <= 1e-14 and float(u @ Mu) > 0 and float(v @ Mv) > 0
    b = pc.rhs(N)
    its = pcg_ref.pcg(A, b, pmg_ref.preconditioner(H), rel_tol=1e-13)[1]
    recorded, cheb_recorded = pc.PCG_COUNTS[name]
    print("%s: PCG with the p-V-cycle %d (recorded %d)" % (name, its, recorded))
    assert abs(its - recorded) <= 1
    if cheb_recorded is not None:
        lo, hi = H.bounds[-1]
        cheb = pcg_ref.pcg(A, b, cr.chebyshev_preconditioner(A, H.ns[-1], H.kinds[-1], lo, hi, pc.DEGREE), rel_tol=1e-13)[1]
        print("%s: PCG with Chebyshev(%d) alone %d (recorded %d)" % (name, pc.DEGREE, cheb, cheb_recorded))
        assert its < cheb and abs(cheb - cheb_recorded) <= 1
