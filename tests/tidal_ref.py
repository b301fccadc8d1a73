"""NumPy restatement of Jayne tidal mixing as the native KPP path applies it: the init-time fields of tidal_mixing.F90 (energy flux
:2246-2295, vertical function and TIDAL_COEF_3D :1266-1309, 2512-2548, 2631-2661, region boxes :880-1003) and the per-column
recurrence of tidal_compute_diff (:3046-3140, 3374-3429) inside ri_iwmix (vmix_kpp.F90:1791-1857).

Arrays are (nblocks, km, ny_block, nx_block) or (nblocks, ny_block, nx_block); levels are 0-based here (level k of the reference is
index k - 1), the vertical grid arrays carry the reference's index.  Written a whole block at a time, level by level, as the
reference's array statements are."""
import numpy as np

import submeso_ref

GRAV = submeso_ref.GRAV
RHO_FW = 1.0                      # pop_constants.F90:240
RADIAN = 180.0 / (4.0 * np.arctan(1.0))
MAX_REGIONS = 9                   # tidal_mixing.F90:262


def params(nml):
    """dict of a pop_tidal_nml (the ctypes mirror PopTidalNml); 0 in a double member = the code default"""
    nr = nml.num_tidal_min_regions
    return {"q": nml.tidal_local_mixing_fraction or 0.33, "eff": nml.tidal_mixing_efficiency or 0.2,
            "decay": nml.vertical_decay_scale or 500.0e2, "mix_max": nml.tidal_mix_max or 100.0,
            "lmax": bool(nml.ltidal_max), "stabc": bool(nml.ltidal_stabc) and not nml.lccsm_control_compatible,
            "lregions": bool(nml.ltidal_min_regions),
            "regions": [dict(min_value=nml.tidal_min_values[r], TLATmin=nml.tidal_TLATmin_regions[r], TLATmax=nml.tidal_TLATmax_regions[r],
                             TLONmin=nml.tidal_TLONmin_regions[r], TLONmax=nml.tidal_TLONmax_regions[r],
                             klevels=nml.tidal_min_regions_klevels[r]) for r in range(nr)]}


def vertical_func(KMT, HT, vg, decay):
    """VERTICAL_FUNC (nb, km, ny, nx) and WORK; 0 where the reference's WORK is 0 (KMT <= 1)"""
    km = len(vg["dz"]) - 1
    zw, dzw = vg["zw"], vg["dzw"]
    WORK = np.zeros(KMT.shape)
    for k in range(1, km + 1):
        WORK = np.where(k < KMT, WORK + np.exp(-(HT - zw[k]) / decay) * dzw[k], WORK)
    VF = np.zeros((KMT.shape[0], km) + KMT.shape[1:])
    ok = KMT > 1
    W = np.where(ok, WORK, 1.0)
    for k in range(1, km + 1):
        VF[:, k - 1] = np.where(ok & (k < KMT), np.exp(-(HT - zw[k]) / decay) / W, np.where(ok & (k == KMT), 1.0 / W, 0.0))
    return VF, WORK


def coef_3d(KMT, HT, flux_wm2, vg, P):
    """TIDAL_ENERGY_FLUX_2D [g/s^3] and TIDAL_COEF_3D"""
    EF = 1000.0 * flux_wm2
    QE = P["q"] * EF
    RCALCT = np.where(KMT >= 1, 1.0, 0.0)
    C2 = (P["eff"] / RHO_FW) * RCALCT * QE
    VF, _ = vertical_func(KMT, HT, vg, P["decay"])
    return EF, C2[:, None] * VF


def region_box(TLAT, TLON, has_address, P):
    """REGION_BOX2D from the latitudes / longitudes in radians; has_address: the cell has a global address (scatter_global leaves 0
    elsewhere)"""
    box = np.zeros(TLAT.shape, dtype=np.int32)
    if not P["lregions"]:
        return box
    lat, lon = TLAT * RADIAN, TLON * RADIAN
    for r, R in enumerate(P["regions"]):
        inlat = (lat >= R["TLATmin"]) & (lat <= R["TLATmax"])
        if R["TLONmin"] <= R["TLONmax"]:
            inlon = (lon >= R["TLONmin"]) & (lon <= R["TLONmax"])
        else:   # the box wraps around 360: (A .and. B) .or. C
            inlon = ((lon >= R["TLONmin"]) & (lon <= 360.0)) | (lon <= R["TLONmax"])
        box = np.where(inlat & inlon, r + 1, box)
    return np.where(has_address, box, 0).astype(np.int32)


def box_3d(BOX, KMT, km, P):
    """REGION_BOX3D (:981-1003) as a mask and the minimum that applies there"""
    on = np.zeros((BOX.shape[0], km) + BOX.shape[1:], dtype=bool)
    val = np.zeros(on.shape)
    for r, R in enumerate(P["regions"] if P["lregions"] else []):
        kl = R["klevels"]
        if kl not in (2, 6):
            continue
        for k in range(kl + 1, km + 1):
            hit = (BOX == r + 1) & (k >= KMT - kl) & (k <= KMT - 1)
            on[:, k - 1] |= hit
            val[:, k - 1] = np.where(hit, R["min_value"], val[:, k - 1])
    return on, val


def recurrence(DBLOC, COEF, KMT, BOX, thick, bvdc, prandtl, P):
    """TIDAL_N2, TIDAL_DIFF, KVMIX, KVMIX_M (nb, km, ny, nx); thick(k): what DBLOC(k) is divided by (a scalar, or an array with
    partial bottom cells); bvdc[k]: bckgrnd_vdc(k).  Everything is 0 at k >= KMT."""
    nb, km, ny, nx = DBLOC.shape
    N2, TD, KV, KVM = (np.zeros(DBLOC.shape) for _ in range(4))
    br = {n: np.zeros(DBLOC.shape, dtype=bool) for n in ("neg", "cap", "stab", "region")}   # which branch a cell above the bottom takes
    on, val = box_3d(BOX, KMT, km, P)
    prev = np.zeros(KMT.shape)
    for k in range(1, km + 1):
        a = k - 1
        wet = k < KMT
        with np.errstate(divide="ignore", invalid="ignore"):
            n2 = DBLOC[:, a] / thick(k)
            td = np.where(n2 > 0.0, COEF[:, a] / np.where(n2 > 0.0, n2, 1.0), 0.0)
        br["neg"][:, a] = wet & ~(n2 > 0.0)
        br["cap"][:, a] = wet & (td > P["mix_max"])           # limited by ltidal_max (or, without it, left above tidal_mix_max)
        if P["lmax"]:
            td = np.minimum(td, P["mix_max"])
        if P["stabc"] and k > 2:
            lev = (k == KMT - 1) | (k == KMT - 2)
            br["stab"][:, a] = wet & lev & (prev > td)
            td = np.where(lev, np.maximum(td, prev), td)
        br["region"][:, a] = wet & on[:, a] & (val[:, a] > td)
        td = np.where(on[:, a], np.maximum(td, val[:, a]), td)
        td = np.where(wet, td, 0.0)
        prev = td
        bvvc = prandtl * bvdc[k]
        N2[:, a] = np.where(wet, n2, 0.0)
        TD[:, a] = td
        KV[:, a] = np.where(wet, np.minimum(bvdc[k] + td, P["mix_max"]), 0.0)
        KVM[:, a] = np.where(wet, prandtl * np.minimum(bvvc / prandtl + td, P["mix_max"]), 0.0)
    return {"N2": N2, "DIFF": TD, "KVMIX": KV, "KVMIX_M": KVM, "branch": br}


def thickness(vg, KMT=None, DZBC=None):
    """thick(k) of recurrence(): zgrid(k) - zgrid(k+1), or 0.5 (DZT(k) + DZT(k+1)) with partial bottom cells"""
    km = len(vg["dz"]) - 1
    zgrid = np.concatenate([-vg["zt"], [-vg["zw"][km]]])
    if DZBC is None:
        return lambda k: zgrid[k] - zgrid[k + 1]

    def dzt(k):
        return np.zeros(KMT.shape) if k > km else np.where(k == KMT, DZBC, vg["dz"][k])
    return lambda k: 0.5 * (dzt(k) + dzt(k + 1))


def dbloc(m, T, S, KMT):
    """buoydiff (vmix_kpp.F90:3509-3621): DBLOC(k) = grav (1 - rho(T_k, S_k at level k+1) / rho(T_k+1, S_k+1 at level k+1)) with the
    temperatures clamped at -2, 0 at k >= KMT; the densities through PopModel.state"""
    nb, km, ny, nx = T.shape
    D = np.zeros(T.shape)
    TT = np.maximum(T, -2.0)
    for k in range(1, km):
        rkm = m.state(k + 1, TT[:, k - 1], S[:, k - 1])
        rk = m.state(k + 1, TT[:, k], S[:, k])
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.where(rk != 0.0, GRAV * (1.0 - rkm / np.where(rk != 0.0, rk, 1.0)), 0.0)
        D[:, k - 1] = np.where(k >= KMT, 0.0, d)
    return D


def has_address(m):
    out = np.zeros((m.nblocks, m.nyb, m.nxb), dtype=bool)
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        out[lb] = (np.asarray(b["j_glob"]) != 0)[:, None] & (np.asarray(b["i_glob"]) != 0)[None, :]
    return out


def host_from_model(m, nml, flux_wm2):
    """the init-time fields for model m (works host-only): flux_wm2 with its ghost cells already filled"""
    P = params(nml)
    vg = submeso_ref.vertical(m.km)
    KMT = m.geti("KMT")
    EF, COEF = coef_3d(KMT, m.get("HT"), flux_wm2, vg, P)
    BOX = region_box(m.get("TLAT"), m.get("TLON"), has_address(m), P) if P["lregions"] else np.zeros(KMT.shape, dtype=np.int32)
    return {"P": P, "vg": vg, "KMT": KMT, "EF": EF, "COEF": COEF, "BOX": BOX}


def from_model(m, cfg, nml, flux_wm2, T, S):
    """everything above for the state (T, S) of a device model on which init_tidal_mixing(flux, nml) has run"""
    r = host_from_model(m, nml, flux_wm2)
    KMT, vg = r["KMT"], r["vg"]
    r["DBLOC"] = dbloc(m, T, S, KMT)
    bvdc = np.full(m.km + 2, cfg.bckgrnd_vdc1)
    DZBC = m.get("DZBC") if cfg.partial_bottom_cells else None
    r.update(recurrence(r["DBLOC"], r["COEF"], KMT, r["BOX"], thickness(vg, KMT, DZBC), bvdc, cfg.Prandtl, r["P"]))
    r["bvdc"] = bvdc
    return r
