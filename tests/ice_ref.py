"""NumPy restatement of frazil ice formation: ice_formation (ice.F90:439-614), ice_flx_to_coupler (:663-715), tfreez (:725-757) and
the constants they read (ice.F90:156, 197-198; pop_constants.F90:56, 235, 239-250, 262, 336).

Array statements over (nblocks, km, ny_block, nx_block) / (nblocks, ny_block, nx_block), a whole model at a time, in the reference's
order of operations; levels are 0-based here (level k of the reference is index k - 1).  The surface layer is the variable-thickness
one (sfc_layer_varthick).  Nothing here is imported from the library under test: the constants below are typed in from the reference.

shr_frz_freezetemp (CIME's shr_frz_mod) is not part of POP; the three forms are the ones the library documents."""
import numpy as np

import aniso_ref

GRAV = 980.6            # pop_constants.F90:235
EPS2 = 1.0e-20          # pop_constants.F90:56
PPT_TO_SALT = 1.0e-3    # pop_constants.F90:262
SALT_TO_PPT = 1000.0
DEFAULTS = dict(ice_freq_opt=0, licecesm2=0, kmxice=1, lactive_ice=0, lfw_as_salt_flx=0, tfreeze_option=0,   # ice.F90:158-162, forcing_sfwf.F90:268
                sea_ice_salinity=4.0, ocn_ref_salinity=34.7, latent_heat_fusion=3.34e9,                      # pop_constants.F90:239-250
                cp_sw=3.996e7, rho_sw=4.1 / 3.996, rho_fw=1.0)
TFREEZE = ("minus1p8", "linear_salt", "mushy")


def params(**kw):
    """ice_nml and the constants with the code defaults, then the keywords; plus the derived constants"""
    p = dict(DEFAULTS, **kw)
    p["cp_over_lhfusion"] = p["rho_sw"] * p["cp_sw"] / (p["latent_heat_fusion"] * p["rho_fw"])   # ice.F90:156
    p["salice"] = p["sea_ice_salinity"] * PPT_TO_SALT                                             # :197-198
    p["salref"] = p["ocn_ref_salinity"] * PPT_TO_SALT
    p["hflux_factor"] = 1000.0 / (p["rho_sw"] * p["cp_sw"])                                       # pop_constants.F90:336
    return p


def tfreez(S, option):
    """freezing point [deg C] of salinity S [g/g]: 0 'minus1p8', 1 'linear_salt', 2 'mushy', each bounded below by -2"""
    psu = np.maximum(np.asarray(S, dtype=np.float64) * SALT_TO_PPT, 0.0)
    if option == 0:
        t = np.full_like(psu, -1.8)
    elif option == 1:
        t = -0.0544 * psu
    elif option == 2:
        t = psu / (-18.48 + 0.01848 * psu)
    else:
        raise ValueError(option)
    return np.maximum(t, -2.0)


def thickness(km, KMT, DZBC=None):
    """DZT (nblocks, km, ny, nx): dz(k) of the internal vertical grid, the bottom cell's own thickness at k = KMT with partial bottom cells"""
    dz = aniso_ref.vertical_dz(km)[1:]
    TH = np.broadcast_to(dz[None, :, None, None], (KMT.shape[0], km) + KMT.shape[1:]).copy()
    if DZBC is not None:
        k = np.arange(1, km + 1)[None, :, None, None]
        TH = np.where(k == KMT[:, None], DZBC[:, None], TH)
    return TH


def formation(T, S, PSURF, KMT, AQICE, TH, p, time_weight, dt1):
    """ice_formation on copies of T, S (4-D) with PSURF, KMT, AQICE (3-D) and the thicknesses TH = DZT.  Returns a dict: T, S, QICE,
    AQICE, FW_FREEZE (None in the salt form), the surface thickness W, and `branch`: boolean cell masks of the branches taken
    (sub-surface ones 4-D with False outside 2 .. kmxice)."""
    T, S, AQICE = T.copy(), S.copy(), AQICE.copy()
    cpl, salice, salref, opt = p["cp_over_lhfusion"], p["salice"], p["salref"], p["tfreeze_option"]
    salt = bool(p["lfw_as_salt_flx"])
    ref_val = salref - salice
    QICE = np.zeros_like(AQICE)
    POTICE = np.zeros_like(AQICE)
    br = {n: np.zeros(T.shape, dtype=bool) for n in ("sub_freeze", "sub_melt", "sub_limited", "sub_nothing")}

    def classify(raw, Q, ocean):
        return (ocean & (raw > 0.0), ocean & (raw < 0.0) & (raw >= Q) & (Q < 0.0), ocean & (raw < Q) & (Q < 0.0),
                ocean & (np.maximum(raw, Q) == 0.0))
    for k in range(p["kmxice"], 1, -1):          # :459-525
        i = k - 1
        ocean = k <= KMT
        TFRZ = tfreez(S[:, i], opt)
        raw = (TFRZ - T[:, i]) * TH[:, i]
        POTICE = np.where(ocean, raw, POTICE)
        for n, msk in zip(("sub_freeze", "sub_melt", "sub_limited", "sub_nothing"), classify(raw, QICE, ocean)):
            br[n][:, i] = msk
        POTICE = np.maximum(POTICE, QICE)
        T[:, i] = T[:, i] + POTICE / TH[:, i]
        if salt:
            S[:, i] = S[:, i] + ref_val * POTICE * cpl / TH[:, i]
        else:
            S[:, i] = (S[:, i] * (TH[:, i] + cpl * QICE) + cpl * (S[:, i - 1] * (POTICE - QICE) - salice * POTICE)) / TH[:, i]
        QICE = QICE - POTICE
    ocean = 1 <= KMT                              # :535-569
    TFRZ = tfreez(S[:, 0], opt)
    W = TH[:, 0] + PSURF / GRAV + EPS2
    raw = (TFRZ - T[:, 0]) * W
    POTICE = np.where(ocean, raw, POTICE)
    br["sfc_freeze"], br["sfc_melt"], br["sfc_limited"], br["sfc_nothing"] = classify(raw, QICE, ocean)
    POTICE = np.maximum(POTICE, QICE)
    T[:, 0] = T[:, 0] + POTICE / W
    if salt:
        S[:, 0] = S[:, 0] + ref_val * POTICE * cpl / W
    else:
        S[:, 0] = (S[:, 0] * (W + cpl * QICE) - salice * QICE * cpl) / W
    QICE = QICE - POTICE
    AQICE = AQICE + time_weight * QICE            # :577-614
    TFRZ = tfreez(S[:, 0], opt)
    raw = (TFRZ - T[:, 0]) * W
    POTICE = np.where(ocean, raw, POTICE)
    br["offset_melt"] = ocean & (raw < 0.0) & (raw >= AQICE) & (AQICE < 0.0)
    br["offset_limited"] = ocean & (raw < AQICE) & (AQICE < 0.0)
    POTICE = np.maximum(POTICE, AQICE)
    T[:, 0] = T[:, 0] + POTICE / W
    FW_FREEZE = None
    if salt:
        S[:, 0] = S[:, 0] + ref_val * POTICE * cpl / W
    else:
        FW_FREEZE = time_weight * np.minimum(POTICE, QICE) * cpl / dt1
    AQICE = AQICE - time_weight * POTICE
    return dict(T=T, S=S, QICE=QICE, AQICE=AQICE, FW_FREEZE=FW_FREEZE, W=W, branch=br)


def flx_to_coupler(T1, S1, PSURF, KMT, AQICE, TH1, tlast_ice, halve, p):
    """ice_flx_to_coupler on the surface level of TRACER(cur): returns AQICE (halved for avg, avgfit, robert), QICE, QFLUX"""
    TFRZ = tfreez(S1, p["tfreeze_option"])
    W = TH1 + PSURF / GRAV + EPS2
    WORK2 = np.where(1 <= KMT, (TFRZ - T1) * W, 0.0)
    AQICE = 0.5 * AQICE if halve else AQICE.copy()
    QICE = np.where(AQICE < 0.0, -AQICE, WORK2)
    QFLUX = np.zeros_like(QICE) if tlast_ice == 0.0 else QICE / tlast_ice / p["hflux_factor"]
    return AQICE, QICE, QFLUX


def pressz(km):
    """reference pressure [bars] of the levels (state_mod.F90:1041, 1765-1766) on the internal vertical grid, index 0 unused"""
    dz = aniso_ref.vertical_dz(km)
    zt = np.zeros(km + 1)
    zt[1] = 0.5 * dz[1]
    for k in range(1, km):
        zt[k + 1] = zt[k] + 0.5 * (dz[k] + dz[k + 1])
    d = zt * 0.01
    return 0.059808 * (np.exp(-0.025 * d) - 1.0) + 0.100766 * d + 2.28405e-7 * d ** 2


def rho(T, S, pbar):
    """MWJF density [g/cm^3] (state_mod.F90:418-498 with state_range_opt 'enforce') at the pressure pbar [bars]"""
    p = 10.0 * pbar
    TQ = np.maximum(np.minimum(T, 999.0), -2.0)
    SQ = 1000.0 * np.maximum(np.minimum(S, 0.999), 0.0)
    SQR = np.sqrt(SQ)
    n0 = 9.99843699e+2 + p * (1.04004591e-2 + p * -3.24041825e-8)
    n2 = -5.45928211e-2 + p * (1.03970529e-7 + p * -1.23869360e-11)
    ns1t0 = 2.96938239e+0 + p * 5.18761880e-6
    d0 = 1.0 + p * 5.30848875e-6
    d1 = 7.28606739e-3 + p ** 3 * -1.27934137e-17
    d3 = 3.68390573e-7 + p ** 2 * -3.03175128e-16
    W1 = n0 + TQ * (7.35212840e+0 + TQ * (n2 + 3.98476704e-4 * TQ)) + SQ * (ns1t0 + -7.23268813e-3 * TQ + 2.12382341e-3 * SQ)
    W2 = d0 + TQ * (d1 + TQ * (-4.60835542e-5 + TQ * (d3 + 1.80809186e-10 * TQ))) + \
        SQ * (2.14691708e-3 + TQ * (-9.27062484e-6 + TQ * TQ * -1.78343643e-10) + SQR * (4.76534122e-6 + TQ * TQ * 1.63410736e-9))
    return 0.001 * W1 / W2
