"""Shared pieces of the submesoscale tests: the state as a function of the global indices, the cases, the branch count, and the linear state
with its hand-written closed form (pinned on the host by tests/test_submeso_host.py, repeated on the device by tests/test_gpu_submeso.py)."""
import numpy as np

import submeso_ref

GM = dict(hmix_tracer=3)
KPP = dict(hmix_tracer=3, vmix_choice=3)


def field(m, hx, dtz, noise, front=0.0):
    """T, S of the local blocks as functions of the global indices (so ghost cells agree with their source cells): a large-scale
    pattern of amplitude hx [K], a decrease of dtz [K] per level, cell-to-cell variation of amplitude noise, and a step of `front` K
    across the middle longitude"""
    T = np.zeros((m.nblocks, m.km, m.nyb, m.nxb)); S = np.zeros_like(T)
    nx, ny = m.cfg.nx_global, m.cfg.ny_global
    k = np.arange(1, m.km + 1, dtype=np.float64)[:, None, None]
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        i = np.asarray(b["i_glob"], dtype=np.float64)[None, None, :]
        j = np.asarray(b["j_glob"], dtype=np.float64)[None, :, None]
        wig = np.sin(12.9898 * i + 78.233 * j + 37.719 * k) * np.cos(4.1 * i - 2.3 * j)
        T[lb] = 18.0 - dtz * k + hx * np.cos(2.0 * np.pi * i / nx) * np.cos(np.pi * j / ny) + noise * wig + front * (i > nx / 2)
        S[lb] = 0.035 + 1.0e-4 * hx * np.sin(2.0 * np.pi * i / nx + 0.3 * j) + 2.0e-5 * k * min(dtz, 1.0)
    return T, S


def branches(r, phys):
    """how many physical ocean columns take each branch of HLS = max(WORK1, WORK2, hor_length_scale)"""
    sel = phys & (r["KMT"] > 0)
    w1, w2, h = r["WORK1"][sel], r["WORK2"][sel], r["HLS"][sel]
    return {"work1": int(((w1 == h) & (w1 > w2)).sum()), "work2": int(((w2 == h) & (w2 >= w1)).sum()),
            "floor": int(((h > w1) & (h > w2)).sum())}


# (id, pop_config keywords, submeso keywords, state, grid from pop_create_with_grid, branch of the max that must be taken on > 20 columns)
CASES = [
    ("const-vmix", GM, {}, (2.0, 0.3, 0.2), False, None),
    ("kpp", KPP, {}, (2.0, 0.3, 0.2), False, None),
    ("kpp-stepped", dict(KPP, stepped_bathymetry=1), {}, (2.0, 0.3, 0.2), False, None),
    ("const-length-scale", KPP, dict(luse_const_horiz_len_scale=1, hor_length_scale=2.0e5), (2.0, 0.3, 0.2), False, None),
    ("padded-blocks", dict(KPP, block_size_x=20, block_size_y=16), {}, (2.0, 0.3, 0.2), False, None),
    ("tripole", dict(KPP, ns_boundary=2, block_size_x=48, block_size_y=10), {}, (2.0, 0.3, 0.2), True, None),
    ("front-work1", GM, dict(time_scale_constant=3.456e5), (8.0, 0.0, 3.0), False, "work1"),
    ("stratified-work2", GM, {}, (0.1, 2.0, 0.0), False, "work2"),
    ("weak-floor", GM, {}, (1.0e-3, 1.0e-4, 0.0), False, "floor"),
]


def linear_state(m, T0=16.0, a=2.0 ** -6, c=-2.0 ** -5, b=-2.0 ** -3, S0=0.035):
    """T = T0 + a i + c j + b k (global indices, 1-based level), uniform S, on the blocks of `m`; and the cells whose four neighbours
    carry the next global index (not across the cyclic seam or a closed boundary, where the field is not linear)"""
    T = np.zeros((m.nblocks, m.km, m.nyb, m.nxb))
    lin = np.zeros((m.nblocks, m.nyb, m.nxb), dtype=bool)
    for lb, bid in enumerate(m.local_block_ids()):
        blk = m.get_block(bid)
        ig = np.asarray(blk["i_glob"], dtype=np.float64)[None, None, :]
        jg = np.asarray(blk["j_glob"], dtype=np.float64)[None, :, None]
        T[lb] = T0 + a * ig + c * jg + b * np.arange(1, m.km + 1, dtype=np.float64)[:, None, None]
        i1, j1 = np.asarray(blk["i_glob"]), np.asarray(blk["j_glob"])
        oi = np.zeros(m.nxb, dtype=bool); oj = np.zeros(m.nyb, dtype=bool)
        oi[1:-1] = (i1[2:] == i1[1:-1] + 1) & (i1[:-2] == i1[1:-1] - 1)
        oj[1:-1] = (j1[2:] == j1[1:-1] + 1) & (j1[:-2] == j1[1:-1] - 1)
        lin[lb] = oj[:, None] & oi[None, :]
    return T, np.full_like(T, S0), lin


def closed_form(r, a, c, b, eff, hls0):
    """Level-1 and level-2 tendency of T for the linear state with ML_DEPTH = zw(1) and a constant length scale, written out by hand.
    Only the two half cells of level 1 lie above ML_DEPTH (reference depths dz(1)/4 and 3 dz(1)/4, both with (1 - 2 r)^2 = 1/4), so
    the shape value is (1 - 1/4)(1 + 5/84); BX = -grav DRDT a and BY = -grav DRDT c on all four faces; TZ(1) = 0 and TZ(2) = -b.
    Returns (GTK1, GTK2, the largest single term of the flux sum) on the cells whose four neighbours lie inside the block."""
    f, vg = r["f"], r["vg"]
    dz1, dz2 = vg["dz"][1], vg["dz"][2]
    shape = (1.0 - 0.25) * (1.0 + 5.0 / 84.0)
    A = eff * dz1 ** 2 * shape * r["TS"] / hls0
    drdt = r["DRDT"][:, 0]
    sfx = A * (-submeso_ref.GRAV * drdt * a) * np.minimum(f["DXT"], 111.0e5)     # east = west face
    sfy = A * (-submeso_ref.GRAV * drdt * c) * np.minimum(f["DYT"], 111.0e5)
    hyx, hxy = f["HTE"] / f["HUS"], f["HTN"] / f["HUW"]
    fx = np.zeros_like(sfx); fy = np.zeros_like(sfx)
    fx[..., :-1] = 0.25 * hyx[..., :-1] * (-b) * (sfx[..., :-1] + sfx[..., 1:])
    fy[..., :-1, :] = 0.25 * hxy[..., :-1, :] * (-b) * (sfy[..., :-1, :] + sfy[..., 1:, :])
    g1, g2, big = (np.full_like(sfx, np.nan) for _ in range(3))
    I = (Ellipsis, slice(1, -1), slice(1, -1))
    W = (Ellipsis, slice(1, -1), slice(0, -2))
    Sx = (Ellipsis, slice(0, -2), slice(1, -1))
    fz = -0.25 * (sfx[I] * hyx[I] * a + sfy[I] * hxy[I] * c + sfx[I] * hyx[W] * a + sfy[I] * hxy[Sx] * c)
    tar = f["TAREA_R"][I]
    g1[I] = (fx[I] - fx[W] + fy[I] - fy[Sx] - fz) / dz1 * tar
    g2[I] = fz / dz2 * tar
    big[I] = np.maximum.reduce([np.abs(fx[I]), np.abs(fx[W]), np.abs(fy[I]), np.abs(fy[Sx]), np.abs(fz)]) / dz1 * tar
    return g1, g2, big


# every flux is a product of at most 12 factors (eff, ML^2, shape, TIME_SCALE, 1 / HLS, grav, DRDT, a, the grid scale, HYX, 1/4, b), the
# tendency sums six of them and is scaled twice: fewer than 32 roundings of at most one ulp of the largest term each, in the restatement
# and in the hand-written form alike
CLOSED_FORM_ULPS = 64


def open_ocean(r):
    """cells whose own column and four neighbours reach the bottom level"""
    K = r["KMT"]
    km = r["DRDT"].shape[1]
    ok = np.zeros(K.shape, dtype=bool)
    ok[:, 1:-1, 1:-1] = (K[:, 1:-1, 1:-1] == km) & (K[:, 1:-1, 2:] == km) & (K[:, 1:-1, :-2] == km) & (K[:, 2:, 1:-1] == km) & (K[:, :-2, 1:-1] == km)
    return ok
