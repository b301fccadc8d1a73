"""What tests of every kind share, at the bottom of the helper stack (it imports no other module of tests/): the two tolerances, the
cells a comparison looks at, the error measure, the prognostic fields (STATE: name, tracer index) and the work fields a step leaves
behind (WORK), and the tripole halo rule.

Tolerances (fp64):
  * phases without a global reduction (tracer/momentum tendencies, Thomas solves, state, halos):
    TOL_LOCAL = 1e-13 relative to the field's max -- both sides are compiled with
    -ffp-contract=off in the reference's evaluation order, so only library-function rounding
    (sqrt, division are correctly rounded; exp/atan differ by ulps) separates them;
  * anything downstream of the barotropic solver: TOL_SOLVE = 1e-8, because the GPU sums dot
    products in a fixed tree instead of the serial (j,i) order; the PCG iteration count must be
    IDENTICAL (north_star: "PCG iteration count unchanged")."""
import numpy as np

TOL_LOCAL = 1e-13
TOL_SOLVE = 1e-8
STATE = [("TRACER", 0), ("TRACER", 1), ("UVEL", 0), ("VVEL", 0), ("RHO", 0), ("PSURF", 0), ("UBTROP", 0), ("VBTROP", 0),
         ("GRADPX", 0), ("GRADPY", 0), ("PGUESS", 0)]
WORK = ["DH", "DHU", "ZX", "ZY", "VVC", "RHS"]


def interior(a):
    return a[..., 2:-2, 2:-2]


def relerr(a, b):
    d = np.abs(a - b).max()
    s = np.abs(b).max()
    return d / s if s > 0 else d


def physical(m):
    """(nblocks, ny_block, nx_block) mask of the physical cells ib:ie, jb:je of the local blocks (m: a device or host model, or
    orclib.AsModel of an oracle)"""
    mask = np.zeros((m.nblocks, m.nyb, m.nxb), dtype=bool)
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        mask[lb, b["jb"] - 1:b["je"], b["ib"] - 1:b["ie"]] = True
    return mask


def block_masks(m):
    """phys: the physical cells of every local block; near: cells with non-zero global indices whose eight neighbours have them too"""
    nb, ny, nx = m.nblocks, m.nyb, m.nxb
    phys = physical(m)
    cell = np.zeros((nb, ny, nx), dtype=bool)
    short = 0
    for lb, bid in enumerate(m.local_block_ids()):
        blk = m.get_block(bid)
        cell[lb] = (blk["j_glob"] != 0)[:, None] & (blk["i_glob"] != 0)[None, :]
        short += (blk["ie"] < nx - 2) or (blk["je"] < ny - 2)
    near = cell.copy()
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            sh = np.ones_like(cell)
            js = slice(max(dj, 0), ny + min(dj, 0)); jd = slice(max(-dj, 0), ny + min(-dj, 0))
            is_ = slice(max(di, 0), nx + min(di, 0)); id_ = slice(max(-di, 0), nx + min(-di, 0))
            sh[:, jd, id_] = cell[:, js, is_]
            near &= sh
    return {"phys": phys, "near": near, "short": short}


def pick(gpu, a, inner):
    """the cells a comparison looks at: the physical cells (inner) or every cell of the block arrays; with padded blocks (block
    size not dividing the domain, tests/test_gpu_padded.py sets gpu.masks) the physical cells of each block, resp. the cells that
    exist and whose neighbours exist (the padding holds nothing, and a ghost cell next to it is formed from it)"""
    m = getattr(gpu, "masks", None)
    if m is None:
        return interior(a) if inner else a
    sel = m["phys"] if inner else m["near"]
    if a.ndim == 4:
        sel = np.broadcast_to(sel[:, None], a.shape)
    return a[sel]


def tripole_expected(G, ig, jg, nx, ny, loc, kind, hw=2):
    """Expected block array after a tripole halo update, the rule of test/unit/halo/POP.F90Tripole
    (:330-345 centre, :598-618 E face, :1112-1150 NE corner + symmetrised top row, N face alike; vector kinds
    change the sign of the mirrored copy, :1480-1495).  G is the global field (ny, nx), 0-based storage."""
    sgn = 1 if kind == "scalar" else -1
    nyb, nxb = len(jg), len(ig)
    out = np.zeros((nyb, nxb), dtype=G.dtype)
    Gat = lambda gi, gj: G[gj - 1, gi - 1]

    def sym(gi):
        a = Gat(gi, ny)
        if loc == "NEcorner":
            p = gi if gi in (nx, nx // 2) else nx - gi
        else:
            p = nx + 1 - gi
        b = Gat(p, ny)
        m = 0.5 * (abs(float(a)) + abs(float(b)))
        if np.issubdtype(G.dtype, np.integer):
            m = int(np.floor(m + 0.5))          # nint
        return -m if a < 0 else m

    top = any(v < 0 for v in jg)
    for j in range(nyb):
        for i in range(nxb):
            gi, gj = ig[i], jg[j]
            if gi <= 0:
                continue
            if gj > 0:
                if top and gj == ny and loc in ("NEcorner", "Nface"):
                    out[j, i] = sym(gi)
                else:
                    out[j, i] = Gat(gi, gj)
            elif gj < 0:                        # tripole ghost row n = -gj - ny
                n = -gj - ny
                if loc == "center":
                    out[j, i] = sgn * Gat(nx - gi + 1, ny + 1 - n)
                elif loc == "Eface":
                    out[j, i] = sgn * Gat(nx - gi if gi != nx else nx, ny + 1 - n)
                elif loc == "NEcorner":
                    out[j, i] = sgn * Gat(nx - gi if gi != nx else nx, ny - n)
                else:
                    out[j, i] = sgn * Gat(nx + 1 - gi, ny - n)
    return out
