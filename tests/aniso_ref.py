"""NumPy restatement of the anisotropic viscosity of the reference (source/hmix_aniso.F90), the independent side of the
tests of hmix_momentum = 3 (tests/test_aniso_host.py, tests/test_gpu_aniso.py).  Written from the Fortran, in its operation
order; arrays are the library's block arrays (nblocks, [km,] ny_block, nx_block), eoshift = a shift inside each block with
zero fill at its edges."""
import numpy as np

OMEGA = 7.292123625e-5          # pop_constants.F90
RADIUS = 6370.0e5
PI = 4.0 * np.arctan(1.0)
RADIAN = 180.0 / PI


def eoshift(a, di, dj):
    """out(i, j) = a(i + di, j + dj) inside each block (the last two axes), 0 beyond its edges (Fortran eoshift)"""
    out = np.zeros_like(a)
    ny, nx = a.shape[-2:]
    ys, yd = (slice(dj, ny), slice(0, ny - dj)) if dj >= 0 else (slice(0, ny + dj), slice(-dj, ny))
    xs, xd = (slice(di, nx), slice(0, nx - di)) if di >= 0 else (slice(0, nx + di), slice(-di, nx))
    out[..., yd, xd] = a[..., ys, xs]
    return out


def geometry(HTN, HTE, DXUR, DYUR, dtu):
    """init_aniso :372-393"""
    H2S, H1W = HTE.copy(), HTN.copy()
    H2N, H1E = eoshift(H2S, 0, 1), eoshift(H1W, 1, 0)
    WA = H2S + H2N
    WB = eoshift(WA, -1, 0)
    K1W = 2.0 * (WA - WB) / (WA + WB) / H1W
    K1E = eoshift(K1W, 1, 0)
    WA = H1W + H1E
    WB = eoshift(WA, 0, -1)
    K2S = 2.0 * (WA - WB) / (WA + WB) / H2S
    K2N = eoshift(K2S, 0, 1)
    AMAX = 0.125 / (dtu * (DXUR * DXUR + DYUR * DYUR))
    return dict(H1E=H1E, H1W=H1W, H2N=H2N, H2S=H2S, K1E=K1E, K1W=K1W, K2N=K2N, K2S=K2S, AMAX_CFL=AMAX)


def to_global(m, a, nxg, nyg):
    """gather_global: the physical cells of every local block into a (ny_global, nx_global) array (one rank holding all blocks)"""
    G = np.zeros((nyg, nxg), dtype=a.dtype)
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        for j in range(b["jb"] - 1, b["je"]):
            for i in range(b["ib"] - 1, b["ie"]):
                ig, jg = b["i_glob"][i], b["j_glob"][j]
                if ig > 0 and jg > 0:
                    G[jg - 1, ig - 1] = a[lb, j, i]
    return G


def scatter_necorner(m, G, nxg, nyg):
    """scatter_global(.., field_loc_NEcorner, field_type_scalar) (mpi/gather_scatter.F90:1015-1041): every cell of every local
    block reads its global address; 0 where the index is 0; rows beyond a tripole fold read the mirrored address"""
    out = np.zeros((m.nblocks, m.nyb, m.nxb))
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        for j in range(m.nyb):
            for i in range(m.nxb):
                ig, jg = b["i_glob"][i], b["j_glob"][j]
                if ig == 0 or jg == 0:
                    continue
                if jg > 0:
                    out[lb, j, i] = G[jg - 1, ig - 1]
                else:
                    js, isrc = nyg + (jg + nyg), nxg - ig
                    isrc = isrc + nxg if isrc < 1 else (isrc - nxg if isrc > nxg else isrc)
                    out[lb, j, i] = G[js - 1, isrc - 1]
    return out


def dist_row(kmu_row, htn_row, k, v5):
    """compute_ccsm_var_viscosity :1173-1240 on one global row: nearest western boundary, then the distance to it"""
    nx = len(kmu_row)
    iwp = [ig for ig in range(1, nx + 1) if kmu_row[ig - 1] < k and kmu_row[(ig % nx)] >= k]
    nw = [0] * (nx + 1)
    if iwp:
        for n in range(len(iwp) - 1):
            for ig in range(iwp[n], iwp[n + 1]):
                nw[ig] = iwp[n]
        for ig in range(1, nx + 1):
            if nw[ig] == 0:
                nw[ig] = iwp[-1]
    D = np.zeros(nx + 1)        # 1-based
    for ig in range(1, nx + 1):
        index = nw[ig]
        indexo = index + v5
        if index == 0:
            D[ig] = 1.0e10
        elif index <= ig <= indexo:
            D[ig] = 0.0
        elif ig > indexo:
            D[ig] = htn_row[ig - 1] + D[ig - 1]
        elif ig < index:
            if indexo <= nx:
                if ig == 1:
                    d = 0.0
                    for ii in range(indexo + 1, nx + 1):
                        d = htn_row[ii - 1] + d
                    D[ig] = htn_row[ig - 1] + d
                else:
                    D[ig] = htn_row[ig - 1] + D[ig - 1]
            else:
                D[ig] = 0.0 if ig <= indexo - nx else htn_row[ig - 1] + D[ig - 1]
    return D[1:]


def var_viscosity(m, cfg, AMAX):
    """compute_ccsm_var_viscosity :1153-1291 and the taper of init_aniso :444-464 -> F_PARA, F_PERP (nblocks, km, ny, nx)"""
    nxg, nyg, km = cfg.nx_global, cfg.ny_global, cfg.km
    d = lambda v, dflt: v if v != 0 else dflt
    v1, v2, v3, v4 = d(cfg.vconst_1, 1.e7), d(cfg.vconst_2, 24.5), d(cfg.vconst_3, 0.2), d(cfg.vconst_4, 1.e-8)
    v5, v6, v7 = d(cfg.vconst_5, 3), d(cfg.vconst_6, 1.e7), d(cfg.vconst_7, 45.0)
    ULAT, DXU = m.get("ULAT"), m.get("DXU")
    KMU_G = to_global(m, m.geti("KMU"), nxg, nyg)
    HTN_G = to_global(m, m.get("HTN"), nxg, nyg)
    beta_f = 2.0 * OMEGA * np.cos(ULAT) / RADIUS
    FPARA = np.zeros((m.nblocks, km, m.nyb, m.nxb))
    FPERP = np.zeros_like(FPARA)
    for k in range(1, km + 1):
        DG = np.array([dist_row(KMU_G[jg], HTN_G[jg], k, v5) for jg in range(nyg)])
        DIST = scatter_necorner(m, DG, nxg, nyg)
        bv = np.minimum(np.abs(ULAT * RADIAN), v7) * 90.0 / v7 / RADIAN
        bu = v1 * (1.0 + v2 * (1.0 - np.cos(2.0 * bv)))
        bv = v3 * beta_f * (DXU * DXU * DXU)
        t = v4 * DIST
        bv = bv * np.exp(-(t * t))
        FPERP[:, k - 1] = np.maximum(bu, bv)
        FPARA[:, k - 1] = np.maximum(bv, v6)
    if not cfg.lsmag_aniso:
        FPARA = np.minimum(FPARA, AMAX[:, None])
        FPERP = np.minimum(FPERP, AMAX[:, None])
    return FPARA, FPERP


def vertical_dz(km):
    """dz(1..km) [cm] of the internal vertical grid (grid.F90:1565-1640), index 0 unused"""
    zmax, dz_sfc, dz_deep, eps = 5500.0, 25.0, 400.0, 1.0e-10

    def profile(zl):
        dz, depth = [], 0.0
        for _ in range(km):
            r = depth / zl
            dz.append(dz_deep - (dz_deep - dz_sfc) * np.exp(-(r * r)))
            depth = depth + dz[-1]
        return depth, dz
    zl0, zl1 = eps, zmax
    d0, d1 = profile(zl0)[0], profile(zl1)[0]
    dzv = None
    while (zl1 - zl0) / zmax > eps:
        zl = zl0 + 0.5 * (zl1 - zl0)
        depth, dzv = profile(zl)
        if (d0 - zmax) * (depth - zmax) < 0.0:
            d1, zl1 = depth, zl
        elif (d1 - zmax) * (depth - zmax) < 0.0:
            d0, zl0 = depth, zl
    return np.concatenate([[0.0], np.array(dzv) * 100.0])


def hdiffu(U, V, f, cfg, FPARA=None, FPERP=None, DZU=None):
    """hdiffu_aniso :680-1032 on every level: U, V (nblocks, km, ny, nx) at the mix time level; f: geometry(...) plus UAREA, KMU,
    ANGLE, ULAT, DXU, DYU (2-D block arrays); DZU (nblocks, km, ny, nx) with partial bottom cells.  Returns HDU, HDV (valid on
    the physical cells; the outermost ring of each block, where eoshift fills 0, may hold 0 / 0)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return _hdiffu(U, V, f, cfg, FPARA, FPERP, DZU)


def _hdiffu(U, V, f, cfg, FPARA, FPERP, DZU):
    km = U.shape[1]
    g = {n: f[n][:, None] for n in ("H1E", "H1W", "H2N", "H2S", "K1E", "K1W", "K2N", "K2S", "AMAX_CFL")}
    if DZU is not None:
        GW = np.minimum(DZU, eoshift(DZU, -1, 0)) / DZU
        GE = np.minimum(DZU, eoshift(DZU, 1, 0)) / DZU
        GS = np.minimum(DZU, eoshift(DZU, 0, -1)) / DZU
        GN = np.minimum(DZU, eoshift(DZU, 0, 1)) / DZU
    else:
        GW = GE = GS = GN = np.ones_like(U)
    U0, V0 = U, V
    uw, ue, us, un = GW * eoshift(U, -1, 0), GE * eoshift(U, 1, 0), GS * eoshift(U, 0, -1), GN * eoshift(U, 0, 1)
    vw, ve, vs, vn = GW * eoshift(V, -1, 0), GE * eoshift(V, 1, 0), GS * eoshift(V, 0, -1), GN * eoshift(V, 0, 1)
    # strain :731-763
    w1 = (U0 - uw) / g["H1W"]; w2 = (ue - U0) / g["H1E"]
    w3 = 0.5 * g["K2S"] * (V0 + vs); w4 = 0.5 * g["K2N"] * (V0 + vn)
    E11 = [w1 + w3, w1 + w4, w2 + w4, w2 + w3]
    w1 = (V0 - vs) / g["H2S"]; w2 = (vn - V0) / g["H2N"]
    w3 = 0.5 * g["K1W"] * (U0 + uw); w4 = 0.5 * g["K1E"] * (U0 + ue)
    E22 = [w1 + w3, w2 + w3, w2 + w4, w1 + w4]
    w1 = (U0 - us) / g["H2S"]; w2 = (un - U0) / g["H2N"]; w3 = (V0 - vw) / g["H1W"]; w4 = (ve - V0) / g["H1E"]
    w5 = g["K2S"] * (U0 + us); w6 = g["K2N"] * (U0 + un); w7 = g["K1W"] * (V0 + vw); w8 = g["K1E"] * (V0 + ve)
    E12 = [w1 + w3 - 0.5 * (w5 + w7), w2 + w3 - 0.5 * (w6 + w7), w2 + w4 - 0.5 * (w6 + w8), w1 + w4 - 0.5 * (w5 + w8)]
    # viscosities :807-869
    if cfg.lsmag_aniso:
        ds = f["DSMIN"][:, None]; fps = f["F_PERP_SMAG"][:, None]
        V1, V2 = [], []
        for iq in range(4):
            w6 = np.sqrt(2.0 * (E11[iq] * E11[iq] + E22[iq] * E22[iq]) + E12[iq] * E12[iq])
            t1 = cfg.c_para * 1.0 * w6 * ds * ds
            t2 = cfg.c_perp * fps * w6 * ds * ds
            if cfg.lvariable_hmix_aniso:
                t1, t2 = np.maximum(t1, FPARA), np.maximum(t2, FPERP)
            V1.append(np.minimum(t1, g["AMAX_CFL"])); V2.append(np.minimum(t2, g["AMAX_CFL"]))
    elif cfg.lvariable_hmix_aniso:
        V1, V2 = [FPARA] * 4, [FPERP] * 4
    else:
        V1, V2 = [np.full_like(U, cfg.visc_para)] * 4, [np.full_like(U, cfg.visc_perp)] * 4
    # coefficients and stress :881-926
    S11, S22, S12 = [], [], []
    for iq in range(4):
        v1, v2 = V1[iq], V2[iq]
        if cfg.aniso_alignment == 1:
            n1, n2 = np.cos(f["ANGLE"])[:, None], -np.sin(f["ANGLE"])[:, None]
            A = 0.5 * (v1 + v2) - 2.0 * (v1 - v2) * ((n1 * n2) * (n1 * n2))
            B = 0.5 * (v1 + v2) - 2.0 * (v1 - v2) * ((n1 * n2) * (n1 * n2))
            Cc = (v1 - v2) * n1 * n2 * (n1 * n1 - n2 * n2)
            D = v2 + 2.0 * (v1 - v2) * ((n1 * n2) * (n1 * n2))
        else:
            A = B = 0.5 * (v1 + v2); Cc = 0.0; D = v2
        S11.append(A * E11[iq] - B * E22[iq] + Cc * E12[iq])
        S22.append(-(B * E11[iq]) + A * E22[iq] - Cc * E12[iq])
        S12.append(Cc * (E11[iq] - E22[iq]) + D * E12[iq])
    E = lambda a: eoshift(a, 1, 0)
    W = lambda a: eoshift(a, -1, 0)
    N = lambda a: eoshift(a, 0, 1)
    S = lambda a: eoshift(a, 0, -1)
    H2S, H2N, H1W, H1E, K1E, K1W, K2N, K2S = (g[n] for n in ("H2S", "H2N", "H1W", "H1E", "K1E", "K1W", "K2N", "K2S"))
    # x-component :943-977
    w1 = H2S * S11[0] + H2N * S11[1]
    w2 = H2S * S11[3] + H2N * S11[2]
    w3 = (E(H2S) * E(S11[0]) + E(H2N) * E(S11[1])) * GE
    w4 = (W(H2S) * W(S11[3]) + W(H2N) * W(S11[2])) * GW
    FX = 0.25 * (w2 + w3 - w1 - w4)
    w1 = H1W * S12[0] + H1E * S12[3]
    w2 = H1W * S12[1] + H1E * S12[2]
    w3 = (N(H1W) * N(S12[0]) + N(H1E) * N(S12[3])) * GN
    w4 = (S(H1W) * S(S12[1]) + S(H1E) * S(S12[2])) * GS
    FX = FX + 0.25 * ((w2 + w3) * (1.0 + 0.5 * H2N * K2N) - (w1 + w4) * (1.0 - 0.5 * H2S * K2S))
    w1 = H2S * S22[0] + H2N * S22[1]
    w2 = H2S * S22[3] + H2N * S22[2]
    w3 = (E(H2S) * E(S22[0]) + E(H2N) * E(S22[1])) * GE
    w4 = (W(H2S) * W(S22[3]) + W(H2N) * W(S22[2])) * GW
    FX = FX - 0.125 * ((w2 + w3) * H1E * K1E + (w1 + w4) * H1W * K1W)
    # y-component :985-1018
    w1 = H1W * S22[0] + H1E * S22[3]
    w2 = H1W * S22[1] + H1E * S22[2]
    w3 = (N(H1W) * N(S22[0]) + N(H1E) * N(S22[3])) * GN
    w4 = (S(H1W) * S(S22[1]) + S(H1E) * S(S22[2])) * GS
    FY = 0.25 * (w2 + w3 - w1 - w4)
    w1 = H2S * S12[0] + H2N * S12[1]
    w2 = H2S * S12[3] + H2N * S12[2]
    w3 = (E(H2S) * E(S12[0]) + E(H2N) * E(S12[1])) * GE
    w4 = (W(H2S) * W(S12[3]) + W(H2N) * W(S12[2])) * GW
    FY = FY + 0.25 * ((w2 + w3) * (1.0 + 0.5 * H1E * K1E) - (w1 + w4) * (1.0 - 0.5 * H1W * K1W))
    w1 = H1W * S11[0] + H1E * S11[3]
    w2 = H1W * S11[1] + H1E * S11[2]
    w3 = (N(H1W) * N(S11[0]) + N(H1E) * N(S11[3])) * GN
    w4 = (S(H1W) * S(S11[1]) + S(H1E) * S(S11[2])) * GS
    FY = FY - 0.125 * ((w2 + w3) * H2N * K2N + (w1 + w4) * H2S * K2S)
    wet = f["KMU"][:, None] >= np.arange(1, km + 1)[None, :, None, None]
    UAREA = f["UAREA"][:, None]
    return np.where(wet, FX / UAREA, 0.0), np.where(wet, FY / UAREA, 0.0)


def smag_fields(DXU, DYU, ULAT, cfg):
    """DSMIN (init_aniso :396) and F_PERP_SMAG (:519-528)"""
    sl = cfg.smag_lat if cfg.smag_lat != 0 else 20.0
    sg = cfg.smag_lat_gauss if cfg.smag_lat_gauss != 0 else 98.0
    W = np.abs(ULAT) * RADIAN
    F = np.where(W >= sl, 1.0 - cfg.smag_lat_fact * np.exp(-((W - sl) * (W - sl) / sg)), 1.0 - cfg.smag_lat_fact)
    return np.minimum(DXU, DYU), F
