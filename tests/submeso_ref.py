"""NumPy restatement of the submesoscale mixed-layer eddy scheme (mix_submeso.F90:341-772 submeso_sf, :779-1005 submeso_flux) and of
the part of tracer_diffs_and_isopyc_slopes it reads (hmix_gm_submeso_share.F90:216-429: RX, RY, TX, TY, TZ, RZ_SAVE).

Written array-wise, a whole block at a time, level by level, with the reference's stored stream function SF_SUBM_X / SF_SUBM_Y of
shape (block, face, half, level, j, i) -- the device code keeps six 2-D fields and forms each value again where it is read.
Arrays are (nblocks, km, ny_block, nx_block) or (nblocks, ny_block, nx_block); levels are 0-based here (level k of the reference
is index k - 1), the vertical grid arrays carry the reference's index (slot 0 unused or dzw(0))."""
import numpy as np

import aniso_ref

GRAV = 980.6                      # pop_constants.F90:235
MAX_HOR_GRID_SCALE = 111.0e5      # mix_submeso.F90:188
EAST, WEST, NORTH, SOUTH = 0, 1, 0, 1
KTP, KBT = 0, 1


def vertical(km):
    """dz, dzw, zw, zt of the internal vertical grid (grid.F90:1565-1640, 1642-1660), indexed as the reference"""
    dz = aniso_ref.vertical_dz(km)
    dzw, zw, zt = np.zeros(km + 1), np.zeros(km + 1), np.zeros(km + 1)
    dzw[0], dzw[km] = 0.5 * dz[1], 0.5 * dz[km]
    zw[1], zt[1] = dz[1], dzw[0]
    for k in range(1, km):
        dzw[k] = 0.5 * (dz[k] + dz[k + 1])
        zw[k + 1] = zw[k] + dz[k + 1]
        zt[k + 1] = zt[k] + dzw[k]
    return {"dz": dz, "dzw": dzw, "zw": zw, "zt": zt}


def params(cfg):
    """mix_submeso_nml with the zero-means-default rule of include/pop_amd.h"""
    return {"eff": cfg.efficiency_factor or 0.07, "tsc": cfg.time_scale_constant or 3.456e5, "hls0": cfg.hor_length_scale or 5.0e5,
            "const_hls": bool(cfg.luse_const_horiz_len_scale)}


def time_scale(FCORT, tsc):
    return 1.0 / np.sqrt(FCORT ** 2 + 1.0 / (tsc ** 2))


def _e(a):
    """a(i+1, j); 0 beyond the block (the reference's block-local arrays start at 0 and the loops stop one short)"""
    o = np.zeros_like(a); o[..., :-1] = a[..., 1:]; return o


def _w(a):
    o = np.zeros_like(a); o[..., 1:] = a[..., :-1]; return o


def _n(a):
    o = np.zeros_like(a); o[..., :-1, :] = a[..., 1:, :]; return o


def _s(a):
    o = np.zeros_like(a); o[..., 1:, :] = a[..., :-1, :]; return o


def shared(T, S, DRDT, DRDS, KMT):
    """RX, RY (nb, 2, km, ny, nx), TX, TY, TZ (nb, 2 tracers, km, ny, nx), RZ_SAVE (nb, km, ny, nx)"""
    nb, km, ny, nx = T.shape
    lev = np.arange(1, km + 1)[None, :, None, None]
    kmt = KMT[:, None]
    kmte, kmtn = _e(KMT)[:, None], _n(KMT)[:, None]
    ME = ((lev <= kmt) & (lev <= kmte)).astype(np.float64)
    MN = ((lev <= kmt) & (lev <= kmtn)).astype(np.float64)
    TEMP = np.maximum(-2.0, T)
    TXP, TYP = ME * (_e(TEMP) - TEMP), MN * (_n(TEMP) - TEMP)
    X = np.stack([T, S], axis=1)
    TX, TY = ME[:, None] * (_e(X) - X), MN[:, None] * (_n(X) - X)
    TZ = np.zeros_like(X)
    TZ[:, :, 1:] = X[:, :, :-1] - X[:, :, 1:]
    RX, RY = np.zeros((nb, 2, km, ny, nx)), np.zeros((nb, 2, km, ny, nx))
    RX[:, EAST] = DRDT * TXP + DRDS * TX[:, 1]
    RY[:, NORTH] = DRDT * TYP + DRDS * TY[:, 1]
    RX[:, WEST] = DRDT * _w(TXP) + DRDS * _w(TX[:, 1])
    RY[:, SOUTH] = DRDT * _s(TYP) + DRDS * _s(TY[:, 1])
    RZ = np.zeros((nb, km, ny, nx))
    TZP = TEMP[:, :-1] - TEMP[:, 1:]
    RZ[:, 1:] = np.minimum(DRDT[:, 1:] * TZP + DRDS[:, 1:] * TZ[:, 1, 1:], 0.0)
    return RX, RY, TX, TY, TZ, RZ


def submeso_sf(ML, RX, RY, RZ, KMT, DXT, DYT, TS, P, vg):
    """ML_DEPTH -> BX, BY (nb, 2, ny, nx), HLS, WORK1, WORK2 (the two scales of the max), SF_X, SF_Y (nb, 2, 2, km, ny, nx)"""
    nb, _, km, ny, nx = RX.shape
    dz, dzw, zw, zt = vg["dz"], vg["dzw"], vg["zw"], vg["zt"]
    ocean = KMT > 0
    BX, BY = np.zeros((nb, 2, ny, nx)), np.zeros((nb, 2, ny, nx))
    cont = ocean.copy()
    for k in range(1, km + 1):
        zw_top = zw[k - 1] if k > 1 else 0.0
        W3 = np.where(cont & (ML > zw[k]), dz[k], 0.0)
        last = cont & (ML <= zw[k]) & (ML > zw_top)
        W3 = np.where(last, ML - zw_top, W3)
        for n in range(2):
            BX[:, n] = np.where(cont, BX[:, n] + RX[:, n, k - 1] * W3, BX[:, n])
            BY[:, n] = np.where(cont, BY[:, n] + RY[:, n, k - 1] * W3, BY[:, n])
        cont = cont & ~last
    with np.errstate(divide="ignore", invalid="ignore"):
        for n in range(2):
            BX[:, n] = np.where(ocean, -GRAV * BX[:, n] / ML, BX[:, n])
            BY[:, n] = np.where(ocean, -GRAV * BY[:, n] / ML, BY[:, n])
    HLS, W1, W2 = np.zeros((nb, ny, nx)), np.zeros((nb, ny, nx)), np.zeros((nb, ny, nx))
    if P["const_hls"]:
        HLS = np.where(ocean, P["hls0"], 0.0)
    else:
        W1 = np.sqrt(0.5 * ((BX[:, 0] ** 2 + BX[:, 1] ** 2) / DXT ** 2 + (BY[:, 0] ** 2 + BY[:, 1] ** 2) / DYT ** 2))
        W1 = np.where(ocean, W1 * ML * (TS ** 2), 0.0)
        cont = ocean.copy()
        for k in range(2, km + 1):
            W3 = np.where(cont & (ML > zt[k]), dzw[k - 1], 0.0)
            last = cont & (ML <= zt[k]) & (ML >= zt[k - 1])
            W3 = np.where(last, ((ML - zt[k - 1]) ** 2) * (1.0 / dzw[k - 1]), W3)
            W2 = np.where(cont, W2 + np.sqrt(-RZ[:, k - 1] * W3), W2)
            cont = cont & ~last
        W2 = np.where(ocean, np.sqrt(GRAV) * W2 * TS, W2)
        HLS = np.where(ocean, np.maximum(np.maximum(W1, W2), P["hls0"]), 0.0)
    SFX, SFY = np.zeros((nb, 2, 2, km, ny, nx)), np.zeros((nb, 2, 2, km, ny, nx))
    gx, gy = np.minimum(DXT, MAX_HOR_GRID_SCALE), np.minimum(DYT, MAX_HOR_GRID_SCALE)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(1, km + 1):
            for kk, rd in ((KTP, zt[k] - 0.25 * dz[k]), (KBT, zt[k] + 0.25 * dz[k])):
                on = (rd < ML) & (KMT >= k)
                W3 = (1.0 - (2.0 * rd / ML)) ** 2
                WW = (1.0 - W3) * (1.0 + (5.0 / 21.0) * W3)
                A = P["eff"] * (ML ** 2) * WW * TS / HLS
                for n in range(2):
                    SFX[:, n, kk, k - 1] = np.where(on, A * BX[:, n] * gx, 0.0)
                    SFY[:, n, kk, k - 1] = np.where(on, A * BY[:, n] * gy, 0.0)
    return {"BX": BX, "BY": BY, "HLS": HLS, "WORK1": W1, "WORK2": W2, "SFX": SFX, "SFY": SFY}


def submeso_flux(SFX, SFY, TX, TY, TZ, KMT, HYX, HXY, TAREA_R, vg):
    """TDTK of both tracers (nb, 2, km, ny, nx): valid where all four neighbours lie inside the block (the physical cells)"""
    nb, _, _, km, ny, nx = SFX.shape
    dz = vg["dz"]
    out = np.zeros((nb, 2, km, ny, nx))
    kmte, kmtn = _e(KMT), _n(KMT)
    FZTOP = np.zeros((nb, 2, ny, nx))
    for k in range(1, km + 1):
        CX = np.where((k <= KMT) & (k <= kmte), HYX * 0.25, 0.0)
        CY = np.where((k <= KMT) & (k <= kmtn), HXY * 0.25, 0.0)
        KMASK = np.where(k < KMT, 1.0, 0.0)
        kp1 = k if k == km else k + 1
        a, b = k - 1, kp1 - 1
        for n in range(2):
            tz, tzp = TZ[:, n, a], TZ[:, n, b]
            FX = CX * (SFX[:, EAST, KTP, a] * tz + SFX[:, EAST, KBT, a] * tzp + _e(SFX[:, WEST, KTP, a]) * _e(tz) + _e(SFX[:, WEST, KBT, a]) * _e(tzp))
            FY = CY * (SFY[:, NORTH, KTP, a] * tz + SFY[:, NORTH, KBT, a] * tzp + _n(SFY[:, SOUTH, KTP, a]) * _n(tz) + _n(SFY[:, SOUTH, KBT, a]) * _n(tzp))
            if k < km:
                tx, ty, txp, typ = TX[:, n, a], TY[:, n, a], TX[:, n, b], TY[:, n, b]
                WK1 = SFX[:, EAST, KBT, a] * HYX * tx + SFY[:, NORTH, KBT, a] * HXY * ty + SFX[:, WEST, KBT, a] * _w(HYX) * _w(tx) + SFY[:, SOUTH, KBT, a] * _s(HXY) * _s(ty)
                WK2 = 1.0 * (SFX[:, EAST, KTP, b] * HYX * txp + SFY[:, NORTH, KTP, b] * HXY * typ + SFX[:, WEST, KTP, b] * _w(HYX) * _w(txp) +
                             SFY[:, SOUTH, KTP, b] * _s(HXY) * _s(typ))
                fz = -KMASK * 0.25 * (WK1 + WK2)
                out[:, n, a] = (FX - _w(FX) + FY - _s(FY) + FZTOP[:, n] - fz) * (1.0 / dz[k]) * TAREA_R
                FZTOP[:, n] = fz
            else:
                out[:, n, a] = (FX - _w(FX) + FY - _s(FY) + FZTOP[:, n]) * (1.0 / dz[k]) * TAREA_R
                FZTOP[:, n] = 0.0
    return out


def submeso_velocities(SFX, SFY, ML, KMT, HYX, HXY, HTE, HTN, TAREA_R, vg):
    """U_SUBM, V_SUBM, WTOP_SUBM of every level (nb, km, ny, nx) (:599-661); W valid on the physical cells"""
    nb, _, _, km, ny, nx = SFX.shape
    dz, zw = vg["dz"], vg["zw"]
    kmte, kmtn = _e(KMT), _n(KMT)
    U, V, W = (np.zeros((nb, km, ny, nx)) for _ in range(3))
    USMT, VSMT, WTOP = (np.zeros((nb, ny, nx)) for _ in range(3))
    MLMAX = np.maximum.reduce([ML, _e(ML), _w(ML), _n(ML), _s(ML)])
    for k in range(1, km + 1):
        kp1, factor = (k, 0.0) if k == km else (k + 1, 1.0)
        a, b = k - 1, kp1 - 1
        W1 = (SFX[:, EAST, KBT, a] + factor * SFX[:, EAST, KTP, b] + _e(SFX[:, WEST, KBT, a]) + factor * _e(SFX[:, WEST, KTP, b])) * 0.25 * HYX
        W2 = (SFY[:, NORTH, KBT, a] + factor * SFY[:, NORTH, KTP, b] + _n(SFY[:, SOUTH, KBT, a]) + factor * _n(SFY[:, SOUTH, KTP, b])) * 0.25 * HXY
        USMB = np.where((k < KMT) & (k < kmte), W1, 0.0)
        VSMB = np.where((k < KMT) & (k < kmtn), W2, 0.0)
        W1 = np.where((k <= KMT) & (k <= kmte), USMT - USMB, 0.0)
        W2 = np.where((k <= KMT) & (k <= kmtn), VSMT - VSMB, 0.0)
        U[:, a], V[:, a], W[:, a] = W1 * (1.0 / dz[k]) / HTE, W2 * (1.0 / dz[k]) / HTN, WTOP
        WTOP = np.where((k < KMT) & (zw[k] < MLMAX), WTOP + TAREA_R * (W1 - _w(W1) + W2 - _s(W2)), 0.0)
        USMT, VSMT = USMB, VSMB
    return U, V, W


def from_model(m, cfg, T, S, ML=None, drd=None):
    """everything above for the state (T, S) of model `m`: the expansion coefficients from PopModel.state (which needs the device; a
    host-only model is given drd = (DRDT, DRDS) instead), the metrics from pop_get_field; ML: the mixed-layer depth (default: HMXL
    with KPP, zw(1) otherwise)"""
    vg = vertical(m.km)
    P = params(cfg)
    KMT = m.geti("KMT")
    if drd is not None:
        DRDT, DRDS = drd
    else:
        DRDT, DRDS = np.empty_like(T), np.empty_like(T)
        for k in range(m.km):
            _, DRDT[:, k], DRDS[:, k] = m.state(k + 1, T[:, k], S[:, k], derivs=True)
    f = {n: m.get(n) for n in ("DXT", "DYT", "HTE", "HTN", "HUS", "HUW", "TAREA_R", "FCORT")}
    HYX, HXY = f["HTE"] / f["HUS"], f["HTN"] / f["HUW"]
    TS = time_scale(f["FCORT"], P["tsc"])
    if ML is None:
        ML = m.get("HMXL") if cfg.vmix_choice == 3 else np.full(KMT.shape, vg["zw"][1])
    RX, RY, TX, TY, TZ, RZ = shared(T, S, DRDT, DRDS, KMT)
    r = submeso_sf(ML, RX, RY, RZ, KMT, f["DXT"], f["DYT"], TS, P, vg)
    r["TEND"] = submeso_flux(r["SFX"], r["SFY"], TX, TY, TZ, KMT, HYX, HXY, f["TAREA_R"], vg)
    r["U"], r["V"], r["W"] = submeso_velocities(r["SFX"], r["SFY"], ML, KMT, HYX, HXY, f["HTE"], f["HTN"], f["TAREA_R"], vg)
    r.update(ML=ML, TS=TS, vg=vg, KMT=KMT, DRDT=DRDT, DRDS=DRDS, f=f)
    return r
