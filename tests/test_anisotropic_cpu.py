"""Non-cubic box meshes without a GPU (tests/aniso_meshes.py): the oracle against closed forms that do not trust it, the oracle
against itself under an axis permutation, and which kernel the host selection grants on each mesh - with the origin offset at
which the term kernels stop being taken.

Identities (Nitsche boundary terms, continuous v: the jump terms vanish):
    v = 1   : v^T A v = sum_P sigma_P |dP  n dOmega|                       (uniform sigma: sigma |dOmega|)
    v = x_c : v^T A v = |Omega| - 2 int_dOmega x_c n_c + sum_P sigma_P int_(dP n dOmega) x_c^2
                      = -|Omega| + sum_P sigma_P int_(dP n dOmega) x_c^2      (int x_c n_c = |Omega|, whatever the origin)
for EVERY axis c: on a box mesh with h_0 != h_1 != h_2 a swapped axis factor changes the x_c forms."""
import numpy as np
import pytest

import aniso_meshes as am
from flatten_oracle import flatten
from oracle import polydeal_oracle as po

IDENTITY_MESHES = ["rect124", "rect1116", "offset_mod", "offset_far", "graded", "pinwheel", "rect2d", "offset2d"]
ELEMENTS = [("dgq", 1), ("dgq", 2), ("dgq", 3), ("dgp", 1), ("dgp", 2), ("dgp", 3)]


def _fe(basis, dim, p):
    return (po.FE_DGQ if basis == "dgq" else po.FE_AggloDGP)(dim, p)


def identity_values(ah, var):
    """(quadratic forms, their closed forms) for v = 1, x_0 .. x_{d-1}."""
    A = po.assemble_dense(ah, var)
    dim = ah.grid.dim
    sig = np.array([po.face_sigma(ah, var, P) for P in range(ah.n_agglomerates)])
    area, x2 = am.cell_boundary_integrals(ah)
    lo, hi = am.domain_box_of(ah)
    vol = float(np.prod(hi - lo))
    got, want = [], []
    v = am.coefficients(ah, lambda x: np.ones(len(x)))
    got.append(float(v @ A @ v))
    want.append(float(np.dot(sig, area)))
    for c in range(dim):
        v = am.coefficients(ah, lambda x, c=c: x[:, c])
        got.append(float(v @ A @ v))
        want.append(-vol + float(np.dot(sig, x2[:, c])))
    return np.array(got), np.array(want), sig


@pytest.mark.parametrize("basis,p", ELEMENTS)
@pytest.mark.parametrize("mesh", IDENTITY_MESHES)
def test_oracle_sip_identities_on_box_meshes(mesh, basis, p):
    dim = am.MESHES[mesh][0]
    fe = _fe(basis, dim, p)
    ah = am.oracle_handler(mesh, fe, p + 1)
    var = po.variant_poisson_example(fe)
    got, want, sig = identity_values(ah, var)
    # (the quadratic forms cancel: |x|^2 sigma |dOmega| against entries of up to |x|^2 max|A| - relative to the value)
    assert np.all(np.abs(got - want) <= 1e-11 * np.abs(want)), (got, want, (got - want) / want)
    if np.ptp(sig) == 0.0:  # uniform sigma: the closed forms of the whole box
        lo, hi = am.domain_box(mesh)
        area, x2 = am.box_boundary_integrals(lo, hi)
        vol = float(np.prod(hi - lo))
        closed = np.concatenate([[sig[0] * area], -vol + sig[0] * x2])
        assert np.all(np.abs(want - closed) <= 1e-13 * np.abs(closed)), (want, closed)
    if am.MESHES[mesh][4] is not None or am.MESHES[mesh][5] == "pinwheel":
        assert np.ptp(sig) > 0.0  # (graded / pinwheel: sigma really differs from polytope to polytope)


def test_box_boundary_closed_form():
    """int_dOmega x_c^2 of the closed form against a direct sum over the faces of the unit cube shifted to lo."""
    area, x2 = am.box_boundary_integrals((3.0, -1.0, 0.5), (4.0, -0.5, 2.5))
    assert area == pytest.approx(2 * (0.5 * 2 + 1 * 2 + 1 * 0.5))
    # x_0: faces x = 3, 4 (area 1) + four faces with the mean of x^2 over [3, 4] (37/3) and areas 2 * 1 * 2 + 2 * 1 * 0.5
    assert x2[0] == pytest.approx((9 + 16) * 1.0 + 37.0 / 3.0 * 5.0)


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("mesh", ["rect124", "graded"])
def test_oracle_axis_permutation(mesh, p):
    """FE_DGQ on box lengths (L0, L1, L2) and (L1, L2, L0): polytopes mapped by bounding box, dofs by rotating the lexicographic
    digits - the two oracle matrices agree to 1e-13."""
    perm = (1, 2, 0)
    fe = po.FE_DGQ(3, p)
    var = po.variant_poisson_example(fe)
    ah0 = am.oracle_handler(mesh, fe, p + 1)
    ah1 = am.oracle_handler(mesh, po.FE_DGQ(3, p), p + 1, groups=am.permuted_groups(mesh, perm), perm=perm)
    A0, A1 = po.assemble_dense(ah0, var), po.assemble_dense(ah1, var)
    m = am.permutation_map(ah0, ah1, perm)
    assert np.max(np.abs(A1[np.ix_(m, m)] - A0)) <= 1e-13 * np.max(np.abs(A0))


# ---------------------------------------------------------------------------------------------------------------------
# Which kernel the host selection grants (pdh_check_terms / pdh_check_rows - what AUTO takes for 3-D degree 1 .. 3)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis,p", ELEMENTS)
@pytest.mark.parametrize("mesh", ["rect124", "rect1116", "graded", "pinwheel", "offset_mod", "offset_far", "rect2d", "offset2d"])
def test_kernel_selection_on_box_meshes(mesh, basis, p):
    """Every 3-D box mesh within the rounding bound takes the term kernels (pdh_terms.h; FE_DGQ(3): pdh_terms_wg.h), and with them the
    kinds of pdh_rows.h apply too.  The far offset (|x| / h ~ 4000) leaves them: the rules are tensor-product rules only to about
    eps |x| / h, more than geometry_rounding (capped at 1e-12) accepts - degree 3 keeps pdh_rows.h through its general-point paths,
    the other elements fall back to the moment / direct forms.  A refusal always says why."""
    dim = am.MESHES[mesh][0]
    fe = _fe(basis, dim, p)
    ah = am.oracle_handler(mesh, fe, p + 1)
    rt, wt, rr, wr = am.kernel_selection(flatten(ah, po.variant_poisson_example(fe)))
    if dim == 2:
        assert rt == 0 and rr == 0 and "3-D" in wt and "3-D" in wr, (wt, wr)
    elif mesh == "offset_far":
        assert rt == 0 and "tensor-product rules" in wt and "points are not" in wt, wt  # (which rules: face or volume)
        assert rr == (1 if p == 3 else 0), wr
        if p < 3:
            assert "tensor-product rules" in wr, wr
    else:
        assert rt == 1 and rr == 1, (wt, wr)


@pytest.mark.parametrize("off,terms,rows_p3", am.OFFSET_BOUNDARY)
def test_offset_boundary_of_the_fast_path(off, terms, rows_p3):
    """The 4^3-cell mesh of 2^3 blocks, cells of 0.25, moved by `off` in every axis: the offset at which AUTO silently leaves the
    term kernels (geometry_rounding, pdh_plan.cpp) is pinned here - between |x| / h = 1200 and 1600 for FE_AggloDGP(3) / FE_DGQ(3)
    (lower elements: not monotone in the offset, e.g. FE_DGQ(2) refused at 1200 and taken at 1600 - rounding of the points decides)."""
    for basis, p in (("dgp", 3), ("dgq", 3)):
        fe = _fe(basis, 3, p)
        ah = am.offset_handler(off, fe, p + 1)
        rt, wt, rr, wr = am.kernel_selection(flatten(ah, po.variant_poisson_example(fe)))
        assert rt == terms and rr == rows_p3, (off, basis, wt, wr)
        if not rt:
            assert ("points are not" in wt) if off < 4000 else ("axis-aligned" in wt), wt
        if not rr:
            assert "axis-aligned" in wr, wr
