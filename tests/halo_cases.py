"""The worlds of the vector halo and of CG over the ranks (test infrastructure, no GPU): tests/test_halo_cpu.py checks the planner's sizes
and the coverage the worlds claim, tests/test_gpu_dist_solve.py runs them with W contexts on one device.

The worlds are those of tests/exchange_cases.py (interleaved ownership: hardly a polytope whose neighbours all belong to its own rank),
three SLAB worlds - owner = min(int(W * x of the bounding box's centre), W - 1), so that ranks have interior polytopes and the interior
product runs at all -, the FE_DGQ(4) world (n = 125), the mirror's rank-local descriptions with col_offset (Epetra column order) and an
8-polytope Cartesian description.

`expected_halo` derives - from the face list and the owners alone, no call into the library - what include/polydeal_hip.h promises: per
ordered pair of ranks the polytopes whose n values travel, ascending by first dof, and per rank its interior and boundary polytopes."""
import functools

import numpy as np

import exchange_cases as xc
from flatten_oracle import flatten
from oracle import polydeal_oracle as po


def expected_halo(faces, dof_offset, owner, n, world):
    """faces: (P, Q) of the interior faces, global polytope numbers.  Returns a dict with
         send     {(s, d): [P, ...]}  polytopes of rank s with a face into rank d, ascending by first dof: segment d of s's send buffer
                                       and, the same list, the part of d's ghost tail that s owns
         interior [r] -> polytopes of rank r all of whose neighbours are r's, ascending by first dof;  boundary [r] -> the others"""
    off = np.asarray(dof_offset, dtype=np.int64)
    owner = np.asarray(owner)
    nbrs = [set() for _ in off]
    for P, Q in faces:
        nbrs[P].add(Q)
        nbrs[Q].add(P)
    send = {}
    for P in range(len(off)):
        for d in {int(owner[Q]) for Q in nbrs[P]} - {int(owner[P])}:
            send.setdefault((int(owner[P]), d), []).append(P)
    for key in send:
        send[key].sort(key=lambda P: off[P])
    by_dof = lambda lst: sorted(lst, key=lambda P: off[P])
    interior = [by_dof([P for P in range(len(off)) if owner[P] == r and all(owner[Q] == r for Q in nbrs[P])]) for r in range(world)]
    boundary = [by_dof([P for P in range(len(off)) if owner[P] == r and any(owner[Q] != r for Q in nbrs[P])]) for r in range(world)]
    return dict(send=send, interior=interior, boundary=boundary, off=off, n=n, world=world)


def send_matrix(exp):
    """send[s][d] in doubles (the receive matrix is its transpose)"""
    m = np.zeros((exp["world"], exp["world"]), dtype=np.int64)
    for (s, d), lst in exp["send"].items():
        m[s, d] = len(lst) * exp["n"]
    return m


def _dofs(exp, polytopes):
    return np.concatenate([exp["off"][P] + np.arange(exp["n"]) for P in polytopes] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)


def send_dofs(exp, s):
    """global dof of every entry of rank s's send buffer"""
    return _dofs(exp, [P for d in range(exp["world"]) for P in exp["send"].get((s, d), [])])


def ghost_dofs(exp, d):
    """global dof of every entry of rank d's ghost tail"""
    return _dofs(exp, [P for s in range(exp["world"]) for P in exp["send"].get((s, d), [])])


def coverage(exp, owner):
    send, W = send_matrix(exp), exp["world"]
    peers = {}
    for (s, d), lst in exp["send"].items():
        for P in lst:
            peers[P] = peers.get(P, 0) + 1
    return dict(
        sent_to_two_peers=sum(v >= 2 for v in peers.values()),
        silent_pairs=[(s, d) for s in range(W) for d in range(s) if not send[s, d] and not send[d, s]],
        zero_inside=any(send[r, d] == 0 and send[r, :d].sum() and send[r, d + 1:].sum() for r in range(W) for d in range(W) if d != r),
        interior=[len(v) for v in exp["interior"]],
        single_polytope_rank=bool(np.any(np.bincount(np.asarray(owner), minlength=W) == 1)))


# ---------------------------------------------------------------------------------------------------------------------------------
# worlds
# ---------------------------------------------------------------------------------------------------------------------------------
class World:
    """part: a Partition of tests/exchange_cases.py (problems(), rows(), splits, owner, kw, n, world); dense(): the oracle's matrix in the
    world's numbering, computed once and never written to"""

    def __init__(self, name, part, dense):
        self.name, self.part, self._dense = name, part, dense

    @functools.lru_cache(maxsize=None)
    def dense(self):
        A = self._dense()
        A.setflags(write=False)
        return A

    def expected(self):
        p = self.part
        return expected_halo(p.faces(), p.kw["dof_offset"], p.owner, p.n, p.world)


def _dense_of(part, oah, ovar):
    """the oracle matrix in the numbering of `part` (part.old_to_new from the oracle's)"""
    rp, ci, ref = po.assemble_csr(oah, ovar, diag_first=False)
    m = part.old_to_new
    A = np.zeros((oah.n_dofs, oah.n_dofs))
    rows = np.repeat(np.arange(oah.n_dofs), np.diff(rp))
    A[m[rows], m[ci]] = ref
    return A


# slab worlds: (mesh of exchange_cases, basis, degree, variant, diag_first, W)
SLABS = {
    "slab_dist2d_dgq1": ("dist2d", "dgq", 1, "dr", True, 2),
    "slab_pinwheel_dgp1": ("pinwheel", "dgp", 1, "poisson", False, 3),
    "slab_dist3d_dgq1": ("dist3d", "dgq", 1, "adm", True, 2),
}
# interior polytopes per rank, counted with the oracle when the worlds were chosen
SLAB_INTERIOR = {"slab_dist2d_dgq1": [4, 4], "slab_pinwheel_dgp1": [4, 0, 4], "slab_dist3d_dgq1": [9, 0]}


def slab_owner(bbox, W):
    bbox = np.asarray(bbox)
    return [min(int(W * 0.5 * (b[0][0] + b[1][0])), W - 1) for b in bbox]


@functools.lru_cache(maxsize=None)
def _slab(name):
    mesh, basis, p, vname, diag_first, W = SLABS[name]
    grid, groups = xc._mesh(mesh)
    fe = (po.FE_DGQ if basis == "dgq" else po.FE_AggloDGP)(grid.dim, p)
    ah = po.AgglomerationHandler(grid)
    for g in groups:
        ah.define_agglomerate(g)
    ah.initialize_fe_values(p + 1, p + 1)
    ah.distribute_agglomerated_dofs(fe)
    var = xc._variant(vname, fe)
    kw = flatten(ah, var, diag_first=diag_first)
    part = xc.partition(kw, slab_owner(kw["bbox"], W), world=W)
    return World(name, part, lambda: _dense_of(part, ah, var))


@functools.lru_cache(maxsize=None)
def _dgq4():
    """exchange_cases.dgq4_world() and the oracle handler it was built from (the same construction)"""
    part = xc.dgq4_world()
    grid = po.hyper_cube_refined(3, 0.0, 1.0, 1)
    ah = po.AgglomerationHandler(grid)
    for c in range(grid.n_cells):
        ah.define_agglomerate([c])
    fe = po.FE_DGQ(3, 4)
    ah.initialize_fe_values(5, 5)
    ah.distribute_agglomerated_dofs(fe)
    var = po.variant_poisson_example(fe)
    return World("dgq4", part, lambda: _dense_of(part, ah, var))


class _MirrorColOffset(xc.MirrorPartition):
    """the mirror's rank-local descriptions in Epetra column order: col_offset set, ascending layout"""

    def problems(self):
        return [(self.ah.flatten_local(self.pvar, *self.rows(r), False, True, row_splits=self.splits, epetra_columns=True), self.rows(r))
                for r in range(self.world)]


@functools.lru_cache(maxsize=None)
def _mirror_col_offset():
    mp, oah, ovar = xc.mirror_world()
    part = _MirrorColOffset(mp.ah, mp.pvar, dict(mp.kw, diag_first=0), mp.splits, mp.owner)
    return World("mirror_col_offset", part, lambda: _dense_of(part, oah, ovar))


class _CartesianPartition(xc.MirrorPartition):
    def problems(self):
        return [(self.ah.flatten_cartesian(self.pvar, True, False, *self.rows(r), self.splits), self.rows(r)) for r in range(self.world)]


@functools.lru_cache(maxsize=None)
def _cartesian():
    """8 polytopes (2^3 blocks of 4^3 Cartesian cells), FE_DGQ(2), two ranks, described by flatten_cartesian; the oracle twin is
    built like exchange_cases.mirror_world's"""
    import polydeal_amd as pa
    from polydeal_amd.partition import row_range

    grid = pa.BackgroundGrid.hyper_cube_refined(3, 0.0, 1.0, 2)
    og = po.hyper_cube_refined(3, 0.0, 1.0, 2)
    ah, oah = pa.AgglomerationHandler(grid), po.AgglomerationHandler(og)
    ah.define_block_agglomerates(2)
    for g in po.block_agglomerates(og, 2):
        oah.define_agglomerate(g)
    fe, ofe = pa.FE_DGQ(3, 2), po.FE_DGQ(3, 2)
    for h, f in ((ah, fe), (oah, ofe)):
        h.initialize_fe_values(3, 3)
        h.distribute_agglomerated_dofs(f)
    pvar, ovar = pa.SipVariant.poisson_example(fe), po.variant_poisson_example(ofe)
    n, nA, W = fe.n_dofs_per_cell, ah.n_agglomerates, 2
    assert nA == 8
    splits = [row_range(nA, n, r, W)[0] for r in range(W)] + [ah.n_dofs]
    kw = flatten(oah, ovar, diag_first=True)
    owner = np.searchsorted(np.asarray(splits), np.asarray(kw["dof_offset"]), side="right") - 1
    part = _CartesianPartition(ah, pvar, kw, splits, owner)
    return World("cartesian", part, lambda: _dense_of(part, oah, ovar))


EXTRA = {"dgq4": _dgq4, "mirror_col_offset": _mirror_col_offset, "cartesian": _cartesian}
NAMES = list(xc.ALL_CASES) + [xc.MIRROR_CASE] + list(SLABS) + list(EXTRA)


@functools.lru_cache(maxsize=None)
def world(name):
    if name in SLABS:
        return _slab(name)
    if name in EXTRA:
        return EXTRA[name]()
    return World(name, xc.world(name), lambda: xc.oracle_dense(name).copy())


# the worlds CG runs on (tests/test_gpu_dist_solve.py; tests/test_halo_cpu.py shows that the NumPy reference meets the bounds on them)
CG_WORLDS = ["slab_dist2d_dgq1", "slab_pinwheel_dgp1", "rank_per_polytope", "single_polytope", "mirror_col_offset", "dgq4", "cartesian",
             "one_rank"]


def cg_kinds(name):
    """the preconditioners CG runs with on a world (block Jacobi needs n <= 64)"""
    return ("jacobi",) if name == "dgq4" else ("none", "jacobi", "block_jacobi")


def rhs(name):
    A = world(name).dense()
    return np.random.default_rng(8).standard_normal(A.shape[0])
