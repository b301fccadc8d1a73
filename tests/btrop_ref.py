"""numpy / scipy statement of the 2-D elliptic system of the barotropic mode, written from what the system IS, not from the loops
that apply it (POP_SolversMod.F90 btropOperator :2414-2426 and its nine weights :771-822 are NOT restated here):

    A psi = div(HU grad psi) - TAREA / (beta c2dtp dtp grav) psi                      (barotropic.F90:519-548)

with `grad` (operators.F90:178-187: the four-cell difference at a U point, zero where KMU = 0) and the area-integrated `div`
(:101-114: the four-corner sum at a T cell) assembled as ONE sparse matrix over the ocean cells of the whole domain from HU, DXU,
DYU, KMT, KMU alone.  Nothing here imports the oracle or the device library; tests/pins.py feeds it arrays through its adapters.

  * numbering: the owned ocean T cells of all blocks are numbered 1 .. n and the field of numbers is halo-updated, so every ghost
    cell carries its owner's number -- cyclic, closed, multi-block and padded layouts alike (owned = ib..ie, jb..je of get_block);
  * assembly: per owned ocean T cell the sum over its four corner U points with KMU > 0 of (divergence weight of the corner) x
    (gradient stencil of the corner); the centre term from its closed form.  Symmetry is NOT built in (this is not -G^T W G): it
    is a property the callers check on the result (A - A^T);
  * the direct solve (scipy.sparse.linalg.spsolve) the iterative solvers are compared with;
  * the EVP block preconditioner (POP_SolversMod.F90:2268-2369) as what it is supposed to be: on each sub-block of the partition
    (:2992-3040) that holds no land and lies inside the block, the exact inverse of the five-point operator `centre + four
    diagonal neighbours` with a zero rim; elsewhere r / centre.

Out of scope, deliberately: the TRIPOLE FOLD.  On popcfg.synthetic_grid the identity `nine-point operator = div(HU grad)` does not
hold at the fold row (6e-2 on the oracle, the assembled matrix asymmetric by 8e-2): that grid is test data whose metrics are not
mirror-symmetric about the fold.  A pin there needs a physically consistent tripole fixture first; no tolerance here admits it."""
import math

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve

GRAV = 980.6                     # pop_constants.F90:235
ALPHA, THETA = 1.0 / 3.0, 0.5    # time_management.F90:437-438: time-centring of grad(ps) on leapfrog / forward steps
EVP_SIZE = 8                     # POP_SolversMod.F90: EvpXbs = EvpYbs = 8


def step_parameters(leapfrog, dtp):
    """(beta, c2dtp) of step_mod.F90:302-320: leapfrog steps centre the surface pressure gradient with alpha over 2 dtp, forward
    (Euler / Matsuno / averaging) steps with theta over dtp"""
    return (ALPHA, 2.0 * dtp) if leapfrog else (THETA, dtp)


def owned_mask(shape, blocks):
    """(nblocks, ny_block, nx_block) mask of the cells ib..ie, jb..je (1-based, inclusive) of every block: padded blocks are shorter"""
    own = np.zeros(shape, dtype=bool)
    for b, B in enumerate(blocks):
        own[b, B["jb"] - 1:B["je"], B["ib"] - 1:B["ie"]] = True
    return own


def number_cells(kmt, blocks, halo):
    """-> (idx, wet, n): idx (nblocks, ny, nx) the 0-based number of the ocean cell every cell (ghosts included) is a copy of, -1 where
    there is none (land, closed boundaries, padding); wet = the owned ocean cells, in the order of their numbers.
    halo(a): the halo update of a (nblocks, ny, nx) float64 array, returning the updated array."""
    wet = owned_mask(kmt.shape, blocks) & (kmt > 0)
    n = int(wet.sum())
    num = np.zeros(kmt.shape)
    num[wet] = np.arange(1, n + 1)
    num = halo(num)
    idx = np.rint(num).astype(np.int64) - 1
    assert np.array_equal(num, np.rint(num)) and np.array_equal(idx[wet], np.arange(n)), "the halo update changed owned cells"
    return idx, wet, n


def check_numbering(idx, wet, blocks):
    """the same numbering from get_block's global indices: every cell whose (i_glob, j_glob) is a cell of the domain carries the number
    of the owner of that cell, every other cell none.  Returns how many ghost cells carry an ocean cell's number."""
    table = {}
    for b, B in enumerate(blocks):
        jj, ii = np.nonzero(wet[b])
        for j, i in zip(jj, ii):
            table[(int(B["j_glob"][j]), int(B["i_glob"][i]))] = int(idx[b, j, i])
    assert len(table) == int(wet.sum()), "two owned cells share a global index"
    own = owned_mask(idx.shape, blocks)
    nghost = 0
    for b, B in enumerate(blocks):
        for j in range(idx.shape[1]):
            for i in range(idx.shape[2]):
                jg, ig = int(B["j_glob"][j]), int(B["i_glob"][i])
                expect = table.get((jg, ig), -1) if (jg >= 1 and ig >= 1) else -1
                assert idx[b, j, i] == expect, "block %d cell (%d, %d): number %d, owner of (%d, %d) has %d" % (b, i, j, idx[b, j, i], ig, jg, expect)
                nghost += int(expect >= 0 and not own[b, j, i])
    return nghost


def assemble_div_hu_grad(idx, wet, HU, DXU, DYU, KMU):
    """div(HU grad .) at level 1 as a scipy CSR matrix over the numbered cells.  For the T cell (i, j) the corner U points are
    (i + di, j + dj), di, dj in {0, -1}.  operators.F90:104-111: the corner's UX enters the area-integrated divergence with weight
    +DYU / 2 on the eastern corners (di = 0), -DYU / 2 on the western ones; its UY with +DXU / 2 on the northern corners (dj = 0),
    -DXU / 2 on the southern ones.  :181-184: the gradient at the U point (iu, ju) is taken over the T cells (iu + c, ju + a), c, a in
    {0, 1}: GRADX has +1 / (2 DXU) on the eastern pair (c = 1), -1 / (2 DXU) on the western; GRADY +1 / (2 DYU) on the northern pair
    (a = 1), -1 / (2 DYU) on the southern.  Corners with KMU = 0 carry no gradient (:180)."""
    b, j, i = np.nonzero(wet)
    row = idx[b, j, i]
    rows, cols, vals = [], [], []
    for dj in (0, -1):
        for di in (0, -1):
            ju, iu = j + dj, i + di
            sel = KMU[b, ju, iu] > 0
            bs, js, is_ = b[sel], ju[sel], iu[sel]
            hu, dxu, dyu = HU[bs, js, is_], DXU[bs, js, is_], DYU[bs, js, is_]
            wx = (0.5 if di == 0 else -0.5) * dyu * hu
            wy = (0.5 if dj == 0 else -0.5) * dxu * hu
            for a in (0, 1):
                for c in (0, 1):
                    gx = (0.5 if c == 1 else -0.5) / dxu
                    gy = (0.5 if a == 1 else -0.5) / dyu
                    col = idx[bs, js + a, is_ + c]
                    assert (col >= 0).all(), "an ocean U point next to a cell without an ocean owner"
                    rows.append(row[sel]); cols.append(col); vals.append(wx * gx + wy * gy)
    n = int(wet.sum())
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()


def centre_term(tarea, beta, c2dtp, dtp):
    """barotropic.F90:536: -TAREA / (beta c2dtp dtp grav) on ocean cells (tarea: their areas, in numbering order)"""
    return -tarea / (beta * c2dtp * dtp * GRAV)


def initial_centre_term(tarea, dtp):
    """barotropic.F90:236-238: what POP_SolversPrep sees (EVP preprocessing, Lanczos): -TAREA / (alpha 2 dtp dtp grav)"""
    return -tarea / (ALPHA * 2.0 * dtp * dtp * GRAV)


def system_matrix(G, centre):
    return (G + sp.diags(centre)).tocsr()


def asymmetry(M):
    """max |M - M^T| / max |M|"""
    D = (M - M.T).tocoo()
    return (np.abs(D.data).max() if D.nnz else 0.0) / np.abs(M.data).max()


def direct_solve(M, b):
    return spsolve(M.tocsc(), b)


def norm2(v):
    return math.sqrt(math.fsum(float(x) * float(x) for x in v))


# ------------------------------------------------------------------------------------------------------------------
# EVP block preconditioner
# ------------------------------------------------------------------------------------------------------------------
def evp_partition(ncell, size=EVP_SIZE):
    """EvpBlockPartition (POP_SolversMod.F90:2992-3040) for a block row of `ncell` physical cells, as 0-based [start, stop) ranges of
    block-array indices (two ghost cells first).  The routine is called with m = ncell + 2: mb = (m - 3) / size + 1 pieces; all but the
    last two are `size` wide, the last two share what is left so that the last one is not too small (:3036-3038)."""
    m = ncell + 2
    mb = (m - 3) // size + 1
    edge = [2] * (mb + 1)                # the routine's mdi(p + 1): the 1-based index of the cell before piece p = its first cell, 0-based
    if mb == 1:
        edge[1] = m
    else:
        for p in range(1, mb - 1):
            edge[p] = 2 + p * size
        edge[mb - 1] = (edge[mb - 2] + m) // 2
        edge[mb] = m
    return [(edge[p], edge[p + 1]) for p in range(mb)]


def evp_subblocks(shape, blocks, wne):
    """every sub-block of every block: (b, j0, j1, i0, i1, land).  EvpPre (:2478-2487): a sub-block is treated as land when a
    north-east weight of one of its cells is zero, or when it reaches beyond the block's own cells -- the comparisons as the
    reference writes them, in its slice indices is = i0 - 1, ie = i1 (1-based first / last cell i0 + 1, i1): is + 2 < ib, ie - 1 > ie_block."""
    nb, ny, nx = shape
    out = []
    for b, B in enumerate(blocks):
        for j0, j1 in evp_partition(ny - 4):
            for i0, i1 in evp_partition(nx - 4):
                land = bool((wne[b, j0:j1, i0:i1] == 0.0).any())
                land |= (i0 + 1 < B["ib"]) or (i1 - 1 > B["ie"])
                land |= (j0 + 1 < B["jb"]) or (j1 - 1 > B["je"])
                out.append((b, j0, j1, i0, i1, land))
    return out


def north_east_weight(HU, DXU, DYU, KMU):
    """the coupling of the T cell (i, j) to (i + 1, j + 1): one corner, the U point (i, j), with both products of assemble_div_hu_grad
    positive: HU (DYU / DXU + DXU / DYU) / 4; zero where the U point is land"""
    ok = KMU > 0
    dxu, dyu = np.where(ok, DXU, 1.0), np.where(ok, DYU, 1.0)
    return np.where(ok, 0.25 * HU * (dyu / dxu + dxu / dyu), 0.0)


def five_point_centre(wne, kmt, tarea, dtp):
    """the centre weight of EVP's reduced operator at preprocessing time: -(sum of the four corners' weights) + the initial centre
    term on ocean cells (the first row and column of the block arrays have no south-west corner in the array: left at the term alone)"""
    c = -wne.copy()
    c[:, 1:, :] -= wne[:, :-1, :]
    c[:, :, 1:] -= wne[:, :, :-1]
    c[:, 1:, 1:] -= wne[:, :-1, :-1]
    return c + np.where(kmt > 0, initial_centre_term(tarea, dtp), 0.0)


def evp_local_matrix(centre, wne, b, j0, j1, i0, i1):
    """dense five-point operator of one sub-block with a zero Dirichlet rim; unknowns in (j, i) order"""
    h, w = j1 - j0, i1 - i0
    L = np.zeros((h * w, h * w))
    for jj in range(h):
        for ii in range(w):
            p = jj * w + ii
            J, I = j0 + jj, i0 + ii
            L[p, p] = centre[b, J, I]
            for dj, di, wt in ((1, 1, wne[b, J, I]), (-1, 1, wne[b, J - 1, I]), (1, -1, wne[b, J, I - 1]), (-1, -1, wne[b, J - 1, I - 1])):
                if 0 <= jj + dj < h and 0 <= ii + di < w:
                    L[p, (jj + dj) * w + ii + di] = wt
    return L


def evp_apply(centre, wne, subblocks, r):
    """P r of the whole field, sub-block by sub-block: the dense solve, or r / centre (0 where the centre weight is 0)"""
    out = np.zeros_like(r)
    for b, j0, j1, i0, i1, land in subblocks:
        if land:
            c = centre[b, j0:j1, i0:i1]
            out[b, j0:j1, i0:i1] = np.where(c != 0.0, r[b, j0:j1, i0:i1] / np.where(c != 0.0, c, 1.0), 0.0)
        else:
            L = evp_local_matrix(centre, wne, b, j0, j1, i0, i1)
            out[b, j0:j1, i0:i1] = np.linalg.solve(L, r[b, j0:j1, i0:i1].reshape(-1)).reshape(j1 - j0, i1 - i0)
    return out


def evp_inverse_matrix(centre, wne, subblocks, idx, n):
    """P^-1 over the numbered cells (dense, n x n): block-diagonal, the local operators of the solved sub-blocks and the centre weight
    of the ocean cells of the others"""
    M = np.zeros((n, n))
    for b, j0, j1, i0, i1, land in subblocks:
        q = idx[b, j0:j1, i0:i1].reshape(-1)
        if land:
            c = centre[b, j0:j1, i0:i1].reshape(-1)
            M[q[q >= 0], q[q >= 0]] = c[q >= 0]
        else:
            assert (q >= 0).all()
            M[np.ix_(q, q)] = evp_local_matrix(centre, wne, b, j0, j1, i0, i1)
    return M
