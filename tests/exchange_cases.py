"""The worlds of the ghost-block exchange tests (test infrastructure, no GPU): tests/test_exchange_cpu.py checks the planner's sizes and
the coverage every case claims, tests/test_gpu_exchange.py runs the same worlds with W contexts on one device.

A world is an oracle handler, a SIP variant and an OWNER per polytope.  `partition` renumbers the dofs rank by rank (every rank owns one
contiguous row range, the order inside a rank shuffled with a fixed seed), rebuilds the pattern in either layout and sets agg_rank: one
global description (pdh_problem.local = 0) that every rank takes with its own row range.  With interleaved owners the rank that owns
side 0 of a cut face is not always the lower one, so ranks exchange in both directions, M21 blocks land on either side of the diagonal
block and a polytope receives M22 sums from several peers.

`expected_exchange` derives - from the face list and the owners alone, no call into the library - what include/polydeal_hip.h promises
of the buffers: per peer the M21 blocks of the cut faces ascending by (side-0 dof, side-1 dof), then one M22 block per side-1 polytope
ascending by its dof; and for every block the rows and columns of the global matrix it stands for."""
import functools
import os

import numpy as np

import aniso_meshes as am
from flatten_oracle import flatten
from oracle import polydeal_oracle as po

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------------------------------------------
# pattern of a renumbered problem (shared with tests/test_gpu_vcycle.py::_permuted_problem)
# ---------------------------------------------------------------------------------------------------------------------------------
def coupled_polytopes(off, rowptr, colind, n):
    """the polytopes every polytope's rows couple to (itself included), read from the pattern of the numbering `off`"""
    off = np.asarray(off, dtype=np.int64)
    rp, ci = np.asarray(rowptr, dtype=np.int64), np.asarray(colind, dtype=np.int64)
    order = np.argsort(off)
    owner = lambda cols: order[np.searchsorted(off[order], cols, side="right") - 1]  # polytope of a column
    return [np.unique(owner(ci[rp[off[P]]:rp[off[P] + 1]])) for P in range(len(off))]


def block_pattern(blocks, new_off, n, diag_first):
    """(rowptr, colind) of the DG block pattern in the numbering `new_off`: rows ascending, or the diagonal entry first and the rest
    ascending (deal.II's SparsityPattern)"""
    new_off = np.asarray(new_off, dtype=np.int64)
    n_rows = n * len(new_off)
    rp, ci = np.zeros(n_rows + 1, dtype=np.int64), []
    for P in np.argsort(new_off):
        cols = np.sort(np.concatenate([new_off[Q] + np.arange(n) for Q in blocks[P]]))
        for i in range(n):
            d = new_off[P] + i
            rp[d + 1] = len(cols)
            ci.append(np.concatenate([[d], cols[cols != d]]) if diag_first else cols)
    return np.cumsum(rp), np.concatenate(ci).astype(np.int32)


def row_map(off, new_off, n):
    """old row -> new row"""
    m = np.zeros(n * len(off), dtype=np.int64)
    for P in range(len(off)):
        m[off[P]:off[P] + n] = new_off[P] + np.arange(n)
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# partitions
# ---------------------------------------------------------------------------------------------------------------------------------
class Partition:
    """kw: the global description in the new numbering (agg_rank set); splits [W + 1]: first row of every rank; old_to_new: row map from
    the numbering of the oracle handler; owner [n_agg]; local: None | "drop" (rank-local descriptions made by local_description)"""

    def __init__(self, kw, splits, old_to_new, owner, local=None):
        self.kw, self.splits, self.old_to_new, self.owner, self.local = kw, [int(s) for s in splits], old_to_new, np.asarray(owner), local
        self.world = len(splits) - 1
        self.n = kw["n_rows"] // kw["n_agg"]

    def rows(self, r):
        return self.splits[r], self.splits[r + 1]

    def description(self, r):
        """keyword arguments of polydeal_amd.Problem for rank r"""
        return local_description(self.kw, *self.rows(r)) if self.local == "drop" else self.kw

    def problems(self):
        """[(pa.Problem, (row_begin, row_end))] rank by rank"""
        import polydeal_amd as pa

        return [(pa.Problem(**self.description(r)), self.rows(r)) for r in range(self.world)]

    def faces(self):
        """(side-0 polytope, side-1 polytope) of the interior faces, global polytope numbers"""
        fi, fo = np.asarray(self.kw["face_in"]), np.asarray(self.kw["face_out"])
        return [(int(a), int(b)) for a, b in zip(fi, fo) if b >= 0]

    def expected(self):
        return expected_exchange(self.faces(), self.kw["dof_offset"], self.owner, self.n, self.world)


def partition(kw, owner, world=None, seed=7):
    """kw: flatten(ah, var, diag_first) of tests/flatten_oracle.py; owner [n_agg]: rank of every polytope"""
    owner = np.asarray(owner, dtype=np.int64)
    n_agg = kw["n_agg"]
    n = kw["n_rows"] // n_agg
    world = int(owner.max()) + 1 if world is None else world
    off = np.asarray(kw["dof_offset"], dtype=np.int64)
    rng = np.random.default_rng(seed)
    new_off, splits, at = np.zeros(n_agg, dtype=np.int64), [0], 0
    for r in range(world):
        mine = np.nonzero(owner == r)[0]
        assert mine.size, "rank %d owns nothing" % r
        for P in rng.permutation(mine):
            new_off[P] = at
            at += n
        splits.append(at)
    blocks = coupled_polytopes(off, kw["rowptr"], kw["colind"], n)
    rp, ci = block_pattern(blocks, new_off, n, bool(kw["diag_first"]))
    new = dict(kw)
    new.update(dof_offset=new_off.astype(np.int32), rowptr=rp, colind=ci, agg_rank=owner.astype(np.int32), local=0)
    return Partition(new, splits, row_map(off, new_off, n), owner)


def local_description(kw, r0, r1):
    """The rank-local description (pdh_problem.local = 1) of the rows [r0, r1) of a global one: the polytopes that are neither owned nor
    neighbours of an owned one are dropped, ghosts keep their box and dof numbers only (an empty volume range), the faces without an owned
    side go, rowptr / colind are those of the owned rows."""
    off = np.asarray(kw["dof_offset"], dtype=np.int64)
    fi, fo = np.asarray(kw["face_in"], dtype=np.int64), np.asarray(kw["face_out"], dtype=np.int64)
    owned = (off >= r0) & (off < r1)
    keep_f = owned[fi] | ((fo >= 0) & owned[np.maximum(fo, 0)])
    keep = owned.copy()
    keep[fi[keep_f]] = True
    keep[fo[keep_f & (fo >= 0)]] = True
    ids = np.nonzero(keep)[0]
    loc = -np.ones(len(off), dtype=np.int64)
    loc[ids] = np.arange(len(ids))
    vq_ptr, fq_ptr = np.asarray(kw["vq_ptr"], dtype=np.int64), np.asarray(kw["fq_ptr"], dtype=np.int64)
    vq = [np.arange(vq_ptr[a], vq_ptr[a + 1]) if owned[a] else np.zeros(0, dtype=np.int64) for a in ids]
    fids = np.nonzero(keep_f)[0]
    fq = [np.arange(fq_ptr[f], fq_ptr[f + 1]) for f in fids]
    vsel, fsel = np.concatenate(vq), np.concatenate(fq)
    rp = np.asarray(kw["rowptr"], dtype=np.int64)
    out = dict(kw)
    out.update(
        local=1, n_agg=len(ids), n_faces=len(fids), bbox=np.asarray(kw["bbox"])[ids], dof_offset=off[ids].astype(np.int32),
        agg_rank=np.asarray(kw["agg_rank"])[ids], vq_ptr=np.concatenate([[0], np.cumsum([len(v) for v in vq])]),
        vq_x=np.asarray(kw["vq_x"])[:, vsel], vq_w=np.asarray(kw["vq_w"])[vsel],
        face_in=loc[fi[fids]], face_out=np.where(fo[fids] >= 0, loc[np.maximum(fo[fids], 0)], -1),
        fq_ptr=np.concatenate([[0], np.cumsum([len(q) for q in fq])]), fq_x=np.asarray(kw["fq_x"])[:, fsel],
        fq_n=np.asarray(kw["fq_n"])[:, fsel], fq_w=np.asarray(kw["fq_w"])[fsel], fq_w_out=np.asarray(kw["fq_w_out"])[fsel],
        face_sigma=np.asarray(kw["face_sigma"])[fids], rowptr=rp[r0:r1 + 1] - rp[r0], colind=np.asarray(kw["colind"])[rp[r0]:rp[r1]])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# what the exchange must carry, from the faces and the owners alone
# ---------------------------------------------------------------------------------------------------------------------------------
def expected_exchange(faces, dof_offset, owner, n, world):
    """{(s, d): [block, ...]} for every ordered pair of ranks with traffic s -> d, in buffer order; a block is
         ("m21", P, Q): A[rows of Q, columns of P] of the cut face with side 0 = P (owned by s) and side 1 = Q (owned by d)
         ("m22", Q, [P, ...]): the part of A[rows of Q, columns of Q] that the cut faces (P, Q) of rank s contribute.
    The send buffer of s is its segments (s, 0), (s, 1), ... one after the other, the receive buffer of d (0, d), (1, d), ..."""
    off = np.asarray(dof_offset, dtype=np.int64)
    cut = {}
    for P, Q in faces:
        if owner[P] != owner[Q]:
            cut.setdefault((int(owner[P]), int(owner[Q])), []).append((int(off[P]), int(off[Q]), P, Q))
    out = {}
    for key, lst in cut.items():
        lst.sort()
        blocks = [("m21", P, Q) for _, _, P, Q in lst]
        for oq, Q in sorted({(oq, Q) for _, oq, _, Q in lst}):
            blocks.append(("m22", Q, [P for _, _, P, Q2 in lst if Q2 == Q]))
        out[key] = blocks
    return out


def expected_sizes(exp, n, world):
    """send[s][d] in doubles (the receive matrix is its transpose)"""
    send = np.zeros((world, world), dtype=np.int64)
    for (s, d), blocks in exp.items():
        send[s, d] = len(blocks) * n * n
    return send


def segment_offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def coverage(part):
    """the properties of a partition the coverage conditions of tests/test_exchange_cpu.py are stated in"""
    exp, off, W = part.expected(), np.asarray(part.kw["dof_offset"]), part.world
    send = expected_sizes(exp, part.n, W)
    peers_of, faces_from_one = {}, 0
    left = right = 0
    for (s, d), blocks in exp.items():
        for b in blocks:
            if b[0] == "m22":
                peers_of.setdefault(b[1], set()).add(s)
                faces_from_one = max(faces_from_one, len(b[2]))
            else:
                left += off[b[1]] < off[b[2]]
                right += off[b[1]] > off[b[2]]
    return dict(
        both_directions=any(send[s, d] and send[d, s] for s in range(W) for d in range(s)),
        m22_from_two_peers=sum(len(v) >= 2 for v in peers_of.values()), two_faces_from_one_peer=faces_from_one >= 2,
        rank0_receives=bool(send[:, 0].sum()), last_rank_sends=bool(send[W - 1].sum()), m21_left=int(left), m21_right=int(right),
        silent_pairs=[(s, d) for s in range(W) for d in range(s) if not send[s, d] and not send[d, s]],
        zero_inside=any(send[r, d] == 0 and send[r, :d].sum() and send[r, d + 1:].sum() for r in range(W) for d in range(W) if d != r),
        single_polytope_rank=bool(np.any(np.bincount(part.owner, minlength=W) == 1)))


# ---------------------------------------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------------------------------------
def grown_groups(grid, n_sub, seed):
    """n_sub connected regions grown over the cell graph from random seeds, one cell per region in turn (staircase faces)"""
    n_faces = 2 * grid.dim
    rng = np.random.default_rng(seed)
    region = -np.ones(grid.n_cells, dtype=np.int64)
    seeds = rng.choice(grid.n_cells, size=n_sub, replace=False)
    front = [[int(s)] for s in seeds]
    region[seeds] = np.arange(n_sub)
    left = grid.n_cells - n_sub
    while left:
        for k in range(n_sub):
            while front[k]:
                c = front[k][0]
                free = [x for x in (grid.neighbor(c, f) for f in range(n_faces)) if x != po.INVALID and region[x] < 0]
                if not free:
                    front[k].pop(0)
                    continue
                region[free[0]] = k
                front[k].append(int(free[0]))
                left -= 1
                break
    return [sorted(np.nonzero(region == k)[0].tolist()) for k in range(n_sub)]


def _mesh(name):
    """(grid, agglomerates) of a mesh name"""
    if name == "dist2d":     # 4 x 4 blocks of 2 x 2 cells, interior vertices moved
        grid = po.hyper_cube_refined(2, 0.0, 1.0, 3).distort(0.2, seed=3)
        return grid, po.block_agglomerates(grid, 2)
    if name == "dist3d":     # 3 x 3 x 3 blocks of 2^3 cells, interior vertices moved
        grid = po.subdivided_hyper_cube(3, 6).distort(0.15, seed=3)
        return grid, po.block_agglomerates(grid, 2)
    if name == "dist3d_8":   # 2 x 2 x 2 blocks
        grid = po.hyper_cube_refined(3, 0.0, 1.0, 2).distort(0.15, seed=3)
        return grid, po.block_agglomerates(grid, 2)
    if name == "pinwheel":   # tests/aniso_meshes.py: 30 polytopes with 3 .. 13 neighbours
        grid = am.oracle_grid("pinwheel")
        return grid, am.groups_of("pinwheel", grid)
    if name == "grown6":     # 18 regions grown over 6^3 cells: staircase faces
        grid = po.subdivided_hyper_cube(3, 6)
        return grid, grown_groups(grid, 18, seed=4)
    if name == "t3":         # tests/golden/t3.msh refined once (364 quadrilaterals, no face axis-aligned), 20 grown regions
        grid = po.read_msh(os.path.join(GOLDEN, "t3.msh")).refine_global(1)
        return grid, grown_groups(grid, 20, seed=2)
    raise KeyError(name)


def _variant(name, fe):
    return {"poisson": lambda: po.variant_poisson_example(fe), "dr": lambda: po.variant_diffusion_reaction(fe),
            "adm": po.variant_assemble_dg_matrix}[name]()


# id: (mesh, basis, degree, variant, diag_first, W, owner rule a -> rank, local, what it is there for)
#   The ownership rules are interleaved on purpose ((7a + a // 3) % W and its kin): consecutive polytopes fall to different ranks.  Each was
#   checked with coverage() - tests/test_exchange_cpu.py asserts the conditions, a rule that misses one is replaced, never the condition.
CASES = {
    "t3_dgp1": ("t3", "dgp", 1, "poisson", True, 3, lambda a: (7 * a + a // 3) % 3, None, "2-D, n = 3, oblique faces"),
    "dist2d_dgq1": ("dist2d", "dgq", 1, "dr", False, 2, lambda a: (a + a // 4) % 2, None, "2-D, n = 4, id rule, reaction"),
    "dist2d_dgq7": ("dist2d", "dgq", 7, "adm", True, 3, lambda a: (a + a // 5) % 3, "drop", "2-D, n = 64: the largest 2-D block"),
    "pinwheel_dgp1": ("pinwheel", "dgp", 1, "adm", False, 4, lambda a: (7 * a + a // 3) % 4, "drop", "3-D, n = 4, 3 .. 13 neighbours"),
    "grown6_dgp3": ("grown6", "dgp", 3, "poisson", False, 3, lambda a: (5 * a + a // 2) % 3, None, "3-D, n = 20, staircase faces"),
    "dist3d_dgq1": ("dist3d", "dgq", 1, "dr", True, 4, lambda a: (7 * a + a // 3) % 4, None, "3-D, n = 8, 27 polytopes on 4 ranks"),
    "grown6_dgq2": ("grown6", "dgq", 2, "adm", True, 2, lambda a: (a + a // 3) % 2, None, "3-D, n = 27, staircase faces"),
    "pinwheel_dgq3": ("pinwheel", "dgq", 3, "poisson", True, 3, lambda a: (7 * a + a // 3) % 3, None, "3-D, n = 64, 14 blocks in a row"),
    "dist3d_8_dgq3": ("dist3d_8", "dgq", 3, "adm", False, 2, lambda a: (a + a // 2) % 2, None, "3-D, n = 64, ascending layout"),
}
# edge worlds
EDGE_CASES = {
    "one_rank": ("dist2d", "dgq", 1, "poisson", True, 1, lambda a: 0, None, "W = 1: nothing to exchange"),
    "rank_per_polytope": ("dist3d_8", "dgp", 1, "poisson", False, 8, lambda a: (3 * a + 1) % 8, "drop", "W = number of polytopes"),
    # the quadrants of the 4 x 4 polytope grid go to ranks 1, 0 (bottom) and 3, 2 (top): the diagonal pairs 1 | 2 and 0 | 3 share no face, and
    # a rank that sends to both its neighbours has a zero-size segment between the two
    "silent_pair": ("dist2d", "dgp", 1, "adm", True, 4, lambda a: (1, 0, 3, 2)[(a % 4) // 2 + 2 * (a // 8)], None,
                    "pairs of ranks with no common face"),
    # the 3 x 3 x 1 centre of the pinwheel (polytope 4, 13 neighbours) is all rank 2 owns
    "single_polytope": ("pinwheel", "dgp", 1, "dr", False, 3, lambda a: 2 if a == 4 else (a + a // 5) % 2, None, "a rank of one polytope"),
}
ALL_CASES = dict(CASES, **EDGE_CASES)
MIRROR_CASE = "mirror_local"  # rank-local descriptions by AgglomerationHandler.flatten_local (mirror_world below)


def element(cid):
    mesh, basis, p = ALL_CASES[cid][:3]
    dim = 2 if mesh in ("dist2d", "t3") else 3
    return (po.FE_DGQ if basis == "dgq" else po.FE_AggloDGP)(dim, p)


def algorithms(fe):
    """the forms pdh_set_algorithm admits for an element in ghost mode: the moment form exists for 3-D bases of degree 1 .. 3"""
    return ("auto", "moment", "direct") if fe.dim == 3 and 1 <= fe.degree <= 3 else ("auto", "direct")


@functools.lru_cache(maxsize=None)
def handler(cid):
    """(oracle handler, variant) of a case"""
    mesh, basis, p, vname = ALL_CASES[cid][:4]
    grid, groups = _mesh(mesh)
    fe = element(cid)
    ah = po.AgglomerationHandler(grid)
    for g in groups:
        ah.define_agglomerate(g)
    ah.initialize_fe_values(p + 1, p + 1)
    ah.distribute_agglomerated_dofs(fe)
    return ah, _variant(vname, fe)


@functools.lru_cache(maxsize=None)
def world(cid):
    """the Partition of a case"""
    if cid == MIRROR_CASE:
        return mirror_world()[0]
    diag_first, W, rule, local = ALL_CASES[cid][4:8]
    ah, var = handler(cid)
    part = partition(flatten(ah, var, diag_first=diag_first), [rule(a) for a in range(ah.n_agglomerates)], world=W)
    part.local = local
    return part


@functools.lru_cache(maxsize=None)
def reference(cid):
    """(oracle handler, values of the oracle's CSR in ITS numbering and the case's layout): computed once, never written to"""
    if cid == MIRROR_CASE:
        oah, ovar = mirror_world()[1:]
        diag_first = True
    else:
        oah, ovar = handler(cid)
        diag_first = ALL_CASES[cid][4]
    ref = po.assemble_csr(oah, ovar, diag_first=diag_first)[2]
    ref.setflags(write=False)
    return oah, ref


def oracle_dense(cid):
    """the oracle matrix in the NEW numbering of the case, dense"""
    oah, ref = reference(cid)
    part = world(cid)
    rp, ci = oah.sparsity_pattern(bool(part.kw["diag_first"]))
    m = part.old_to_new
    A = np.zeros((oah.n_dofs, oah.n_dofs))
    rows = np.repeat(np.arange(oah.n_dofs), np.diff(rp))
    A[m[rows], m[ci]] = ref
    return A


def to_oracle_order(part, oah, per_rank_values):
    """the ranks' values (each in its own row order and layout) as one array in the order of the oracle's CSR"""
    diag_first = bool(part.kw["diag_first"])
    rp, ci = np.asarray(part.kw["rowptr"], dtype=np.int64), np.asarray(part.kw["colind"], dtype=np.int64)
    got = np.concatenate(per_rank_values)
    assert got.shape == (rp[-1],)
    N = oah.n_dofs
    rows = np.repeat(np.arange(N), np.diff(rp))
    key_new = rows * N + ci
    orp, oci = oah.sparsity_pattern(diag_first)
    orows = np.repeat(np.arange(N), np.diff(orp))
    key_old = part.old_to_new[orows] * N + part.old_to_new[oci]
    order = np.argsort(key_new)
    at = np.searchsorted(key_new[order], key_old)
    assert np.array_equal(key_new[order][at], key_old)
    return got[order][at]


def dgq4_world():
    """3-D FE_DGQ(4), n = 125, one polytope per cell of 2^3 cells, two ranks"""
    grid = po.hyper_cube_refined(3, 0.0, 1.0, 1)
    ah = po.AgglomerationHandler(grid)
    for c in range(grid.n_cells):
        ah.define_agglomerate([c])
    fe = po.FE_DGQ(3, 4)
    ah.initialize_fe_values(5, 5)
    ah.distribute_agglomerated_dofs(fe)
    return partition(flatten(ah, po.variant_poisson_example(fe)), [a % 2 for a in range(8)])



# ---------------------------------------------------------------------------------------------------------------------------------
# rank-local descriptions from the product's own flatten_local (consecutive row ranges of the mirror's numbering)
# ---------------------------------------------------------------------------------------------------------------------------------
class MirrorPartition(Partition):
    def __init__(self, ah, pvar, kw, splits, owner):
        super().__init__(kw, splits, np.arange(kw["n_rows"], dtype=np.int64), owner)
        self.ah, self.pvar = ah, pvar

    def description(self, r):
        raise NotImplementedError("flatten_local views are not keyword arguments: problems()")

    def problems(self):
        df = bool(self.kw["diag_first"])
        return [(self.ah.flatten_local(self.pvar, *self.rows(r), df, True, row_splits=self.splits), self.rows(r)) for r in range(self.world)]


@functools.lru_cache(maxsize=None)
def mirror_world():
    """(MirrorPartition, oracle handler, oracle variant): 3-D FE_DGQ(2) on 4^3 distorted cells in 2^3 blocks, diffusion-reaction, 3 ranks of
    3, 3 and 2 polytopes in the mirror's own numbering"""
    import polydeal_amd as pa
    from polydeal_amd.partition import row_range

    grid = pa.BackgroundGrid.hyper_cube_refined(3, 0.0, 1.0, 2)
    grid.distort(0.1, seed=5)
    og = po.hyper_cube_refined(3, 0.0, 1.0, 2)
    for c in range(og.n_cells):
        og.vertices[c] = grid.cell_vertices(c)
    ah, oah = pa.AgglomerationHandler(grid), po.AgglomerationHandler(og)
    ah.define_block_agglomerates(2)
    for g in po.block_agglomerates(og, 2):
        oah.define_agglomerate(g)
    fe, ofe = pa.FE_DGQ(3, 2), po.FE_DGQ(3, 2)
    for h, f in ((ah, fe), (oah, ofe)):
        h.initialize_fe_values(3, 3)
        h.distribute_agglomerated_dofs(f)
    pvar, ovar = pa.SipVariant.diffusion_reaction(fe), po.variant_diffusion_reaction(ofe)
    n, nA, W = fe.n_dofs_per_cell, ah.n_agglomerates, 3
    splits = [row_range(nA, n, r, W)[0] for r in range(W)] + [ah.n_dofs]
    kw = flatten(oah, ovar, diag_first=True)
    off = np.asarray(kw["dof_offset"])
    owner = np.searchsorted(np.asarray(splits), off, side="right") - 1
    kw["agg_rank"] = owner.astype(np.int32)
    return MirrorPartition(ah, pvar, kw, splits, owner), oah, ovar
