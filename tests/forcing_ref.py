"""NumPy restatement of the coupled surface forcing, written from the reference, not from the kernels: ANGLET (grid.F90:660-735), the
short-wave factor of qsw_distrb_opt '12hr' (forcing_coupled.F90:358-408), ocn_import's unit conversions and rotate_wind_stress
(drivers/mct/ocn_import_export.F90:171-239, forcing_coupled.F90:1495-1500), pop_set_coupled_forcing (forcing_coupled.F90:677-945)
and the per-step tail of set_surface_forcing (forcing.F90:379-437).  Every formula keeps the reference's order of operations, so a
library built without fused multiply-adds gives the same bits.

Arrays are block arrays (nblocks, ny_block, nx_block).  The halo updates are the library's own host update (tested on its own in
tests/test_layout.py and the tripole tests): single-rank models only."""
import math

import numpy as np

import ice_ref

X2O_FIELDS = ("taux", "tauy", "snow", "rain", "evap", "meltw", "rofl", "rofi", "salt", "swnet", "sen", "lwup", "lwdn", "melth", "ifrac",
              "pslv", "duu10n")
# what update_ghost_cells_coupler_fluxes updates, of what is built, in its order (forcing_coupled.F90:1165-1328)
IMPORTED = ("SNOW_F", "PREC_F", "EVAP_F", "MELT_F", "ROFF_F", "IOFF_F", "SALT_F", "SENH_F", "LWUP_F", "LWDN_F", "MELTH_F", "SHF_QSW", "IFRAC",
            "ATM_PRESS", "U10_SQR")
SECONDS_IN_DAY = 86400.0


def consts(ice=None, latent_heat_vapor_mks=2.501e6, latent_heat_fusion_mks=3.337e5):
    """the constants the formulas read: the coupled values of pop_constants.F90:283-290, :314, :336, :364-365, :385, :405; ice: the
    ice_ref.params of pop_init_ice (None: its code defaults)"""
    p = ice if ice is not None else ice_ref.params()
    return dict(lhv=latent_heat_vapor_mks, lhf=latent_heat_fusion_mks, hflux_factor=p["hflux_factor"],
                salinity_factor=-p["ocn_ref_salinity"] * 1.0e-4, sflux_factor=0.1, fwmass_to_fwflux=0.1, momentum_factor=10.0,
                tfreeze_option=p["tfreeze_option"], lactive_ice=p["lactive_ice"], salice=p["salice"],
                lfw_as_salt_flx=p["lfw_as_salt_flx"])


# ---- ANGLET ------------------------------------------------------------------------------------------------------------------------
def scatter_necorner(m, G):
    """scatter_global of an NE-corner field without a sign change (grid.F90:1524-1525): the block arrays of the global array G
    (ny_global, nx_global); cells without a global index stay 0"""
    ny, nx = G.shape
    out = np.zeros((m.nblocks, m.nyb, m.nxb))
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        for j, gj in enumerate(b["j_glob"]):
            for i, gi in enumerate(b["i_glob"]):
                if gi == 0 or gj == 0:
                    continue
                if gj > 0:
                    out[lb, j, i] = G[gj - 1, gi - 1]
                else:                                   # beyond the tripole fold: row ny - n, column nx - gi (nx stays nx)
                    n = -gj - ny
                    out[lb, j, i] = G[ny - n - 1, (nx - gi if gi != nx else nx) - 1]
    return out


def anglet(m, ANGLE):
    """grid.F90:686-732 from the global ANGLE record: the four-corner average (AT0 = ATW = ATS = ATSW = p25, :2908-2911) with the
    +-pi unwrapping on the physical cells, row j_glob = 1 zeroed, then the halo update (centre, angle)"""
    A = scatter_necorner(m, ANGLE)
    T = np.zeros_like(A)
    pi = 4.0 * math.atan(1.0)
    pi2 = 2.0 * pi
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        for j in range(b["jb"] - 1, b["je"]):
            for i in range(b["ib"] - 1, b["ie"]):
                a0, aw, as_, asw = A[lb, j, i], A[lb, j, i - 1], A[lb, j - 1, i], A[lb, j - 1, i - 1]
                if a0 < 0.0:
                    if abs(aw - a0) > pi:
                        aw = aw - pi2
                    if abs(as_ - a0) > pi:
                        as_ = as_ - pi2
                    if abs(asw - a0) > pi:
                        asw = asw - pi2
                T[lb, j, i] = a0 * 0.25 + aw * 0.25 + as_ * 0.25 + asw * 0.25
            if b["j_glob"][j] == 1:
                T[lb, j, :] = 0.0
    m.halo_update_host_loc(T, fill=0.0, loc="center", kind="angle")
    return T


# ---- qsw_12hr_factor ---------------------------------------------------------------------------------------------------------------
def half_step_weights(nspi, tmix_opt, time_mix_freq):
    """weight_forcing of the loop (forcing_coupled.F90:375-378) for count = 1 .. nspi: avgfit (2) and robert (3) as the reference
    writes it; 'avg' (1): every time_mix_freq-th step; no time mixing (0): none"""
    w = []
    for count in range(1, nspi + 1):
        if tmix_opt in (2, 3):
            half = count == 2 or count % time_mix_freq == 0
        elif tmix_opt == 1:
            half = count % time_mix_freq == 0
        else:
            half = False
        w.append(0.5 if half else 1.0)
    return w


def qsw_12hr_factor(dt1, nspi, tmix_opt, time_mix_freq):
    """forcing_coupled.F90:360-386 -> (factor (nspi,), weights)"""
    pi = 4.0 * math.atan(1.0)
    w = half_step_weights(nspi, tmix_opt, time_mix_freq)
    f = [0.0] * nspi
    time_for_forcing, sum_forcing = 0.0, 0.0
    for n in range(nspi):
        frac_day_forcing = time_for_forcing / SECONDS_IN_DAY
        cycle_function = math.cos(pi * (2.0 * frac_day_forcing - 1.0))
        f[n] = 2.0 * (cycle_function + abs(cycle_function)) * cycle_function
        time_for_forcing = time_for_forcing + w[n] * dt1
        sum_forcing = sum_forcing + w[n] * dt1 * f[n]
    return np.array([x * SECONDS_IN_DAY / sum_forcing for x in f]), w


# ---- ocn_import, rotate_wind_stress ------------------------------------------------------------------------------------------------
def import_fields(m, x2o, k):
    """the imported fields and SMFT after their halo updates.  x2o: dict of block arrays (a missing field is zero); reads RCALCT,
    COS_ANGLET, SIN_ANGLET from the model.  The reference fills the physical cells and lets the halo update do the rest; so does this."""
    z = np.zeros((m.nblocks, m.nyb, m.nxb))
    x = {n: np.asarray(x2o.get(n, z), dtype=np.float64) for n in X2O_FIELDS}
    RC, ca, sa = m.get("RCALCT"), m.get("COS_ANGLET"), m.get("SIN_ANGLET")
    f = {}
    f["SNOW_F"] = x["snow"].copy()
    f["PREC_F"] = x["rain"] + f["SNOW_F"]
    f["EVAP_F"], f["MELT_F"], f["ROFF_F"], f["IOFF_F"], f["SALT_F"] = (x[n].copy() for n in ("evap", "meltw", "rofl", "rofi", "salt"))
    f["SHF_QSW"] = x["swnet"] * RC * k["hflux_factor"]
    f["SENH_F"], f["LWUP_F"], f["LWDN_F"], f["MELTH_F"] = (x[n].copy() for n in ("sen", "lwup", "lwdn", "melth"))
    f["IFRAC"] = x["ifrac"] * RC
    f["ATM_PRESS"] = 10.0 * x["pslv"] * RC
    f["U10_SQR"] = 100.0 * 100.0 * x["duu10n"] * RC
    f["SMFT1"] = (x["taux"] * ca + x["tauy"] * sa) * RC * k["momentum_factor"]
    f["SMFT2"] = (x["tauy"] * ca - x["taux"] * sa) * RC * k["momentum_factor"]
    for n in ("SMFT1", "SMFT2"):
        m.halo_update_host_loc(f[n], fill=0.0, loc="center", kind="vector")
    for n in IMPORTED:
        m.halo_update_host_loc(f[n], fill=0.0, loc="center", kind="scalar")
    return f


def tgrid_to_ugrid(m, A):
    """grid.F90:3399-3415: the northeast four-point average, 0 in the last row and column of the block array"""
    AU0, AUN, AUE, AUNE = (m.get(n) for n in ("AU0", "AUN", "AUE", "AUNE"))
    U = np.zeros_like(A)
    U[:, :-1, :-1] = (AU0[:, :-1, :-1] * A[:, :-1, :-1] + AUN[:, :-1, :-1] * A[:, 1:, :-1] + AUE[:, :-1, :-1] * A[:, :-1, 1:]
                      + AUNE[:, :-1, :-1] * A[:, 1:, 1:])
    return U


def combine(m, f, k, T1, S1, liceform, nt=2):
    """pop_set_coupled_forcing on the imported fields f -> dict of STF1, SMF1, SMF2, SHF_QSW, SHF_QSW_RAW, SHF_COMP_QSW and FW, TFW1 .. or
    STF2, and with ice formation SFWF_COMP_CPL, TFW_COMP_CPL1 / 2.  T1, S1: the surface level of TRACER(cur)"""
    RC = m.get("RCALCT")
    o = {"SMFT1": f["SMFT1"], "SMFT2": f["SMFT2"]}
    o["SMF1"], o["SMF2"] = tgrid_to_ugrid(m, f["SMFT1"]), tgrid_to_ugrid(m, f["SMFT2"])
    o["STF1"] = (f["EVAP_F"] * k["lhv"] + f["SENH_F"] + f["LWUP_F"] + f["LWDN_F"] + f["MELTH_F"]
                 - (f["SNOW_F"] + f["IOFF_F"]) * k["lhf"]) * RC * k["hflux_factor"]
    if not k["lfw_as_salt_flx"]:
        FW = RC * (f["PREC_F"] + f["EVAP_F"] + f["ROFF_F"] + f["IOFF_F"]) * k["fwmass_to_fwflux"]
        W1 = RC * f["MELT_F"] * k["fwmass_to_fwflux"]
        W2 = np.zeros_like(S1) if k["lactive_ice"] else ice_ref.tfreez(S1, k["tfreeze_option"])     # tmelt (ice.F90:764-790)
        o["TFW1"] = FW * T1 + W1 * W2
        o["FW"] = FW + W1
        with np.errstate(divide="ignore", invalid="ignore"):
            sm = np.where(f["MELT_F"] != 0.0, f["SALT_F"] / f["MELT_F"], 0.0)
        o["TFW2"] = RC * f["MELT_F"] * k["fwmass_to_fwflux"] * sm
        for n in range(3, nt + 1):
            o["TFW%d" % n] = np.zeros_like(FW)
        if liceform:
            o["SFWF_COMP_CPL"], o["TFW_COMP_CPL1"], o["TFW_COMP_CPL2"] = o["FW"].copy(), o["TFW1"].copy(), o["TFW2"].copy()
    else:
        o["STF2"] = RC * ((f["PREC_F"] + f["EVAP_F"] + f["MELT_F"] + (1.0 - 0.0) * f["ROFF_F"] + f["IOFF_F"]) * k["salinity_factor"]
                          + f["SALT_F"] * k["sflux_factor"])
    o["SHF_QSW"] = f["SHF_QSW"].copy()
    o["SHF_QSW_RAW"] = f["SHF_QSW"].copy()
    o["SHF_COMP_QSW"] = f["SHF_QSW"].copy()
    return o


def surface_step(o, k, factor, nsteps_this_interval, FW_FREEZE=None, S1=None):
    """the tail of set_surface_forcing (forcing.F90:379-437) -> dict of SHF_QSW and, with FW_FREEZE (ice formation on, the fresh-water
    form), FW, TFW1, TFW2"""
    index_qsw = nsteps_this_interval % len(factor) + 1
    r = {"SHF_QSW": factor[index_qsw - 1] * o["SHF_COMP_QSW"], "index_qsw": index_qsw}
    if FW_FREEZE is not None:
        r["FW"] = o["SFWF_COMP_CPL"] + FW_FREEZE
        r["TFW1"] = o["TFW_COMP_CPL1"] + FW_FREEZE * ice_ref.tfreez(S1, k["tfreeze_option"])
        r["TFW2"] = o["TFW_COMP_CPL2"] + FW_FREEZE * k["salice"]
    return r


def seeded_x2o(m, seed, zero_melt_every=3):
    """x2o fields of both signs on every cell of the block arrays (land and ghost cells included: the import masks the first and the halo
    update overwrites the second), meltw = 0 on every zero_melt_every-th cell.  TEST DATA in the coupler's units."""
    rng = np.random.default_rng(seed)
    shp = (m.nblocks, m.nyb, m.nxb)
    scale = dict(taux=0.2, tauy=0.2, snow=2e-5, rain=8e-5, evap=6e-5, meltw=3e-5, rofl=2e-5, rofi=1e-5, salt=1e-6, swnet=250.0, sen=40.0,
                 lwup=400.0, lwdn=350.0, melth=30.0, ifrac=1.0, pslv=1.0e5, duu10n=60.0)
    x = {n: s * rng.standard_normal(shp) for n, s in scale.items()}
    x["ifrac"] = rng.random(shp)
    x["duu10n"] = np.abs(x["duu10n"])
    cell = np.arange(x["meltw"].size).reshape(shp)
    x["meltw"][cell % zero_melt_every == 0] = 0.0
    return x


# ---- marginal-sea balance (ms_balance.F90) -------------------------------------------------------------------------------------------
MAX_MS, MAX_ITER = 7, 16


def gather_global(m, A, shape):
    """gather_global: the physical cells of every block into a global (ny_global, nx_global) array"""
    G = np.zeros(shape, dtype=A.dtype)
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        for j in range(b["jb"] - 1, b["je"]):
            for i in range(b["ib"] - 1, b["ie"]):
                if b["i_glob"][i] > 0 and b["j_glob"][j] > 0:
                    G[b["j_glob"][j] - 1, b["i_glob"][i] - 1] = A[lb, j, i]
    return G


def scatter_center(m, G):
    """scatter_global of a centre-located scalar: ghost cells take their source cell, mirrored beyond a tripole fold"""
    ny, nx = G.shape
    out = np.zeros((m.nblocks, m.nyb, m.nxb), dtype=G.dtype)
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        for j, gj in enumerate(b["j_glob"]):
            for i, gi in enumerate(b["i_glob"]):
                if gi == 0 or gj == 0:
                    continue
                if gj > 0:
                    out[lb, j, i] = G[gj - 1, gi - 1]
                else:
                    n = -gj - ny
                    out[lb, j, i] = G[ny + 1 - n - 1, nx - gi + 1 - 1]
    return out


def init_ms_balance(m, regions, region_mask, max_points=5000):
    """init_ms_balance (ms_balance.F90:170-405) -> list of dicts per marginal sea (number, ipts, jpts (1-based), fracs, area,
    warn_two_regions, warn_max_points, MASK_FRAC block array); raises ValueError where the reference aborts.  Single-rank model."""
    radian = 180.0 / (4.0 * math.atan(1.0))
    shape = region_mask.shape
    TLAT_G = gather_global(m, m.get("TLAT") * radian, shape)
    TLON_G = gather_global(m, m.get("TLON") * radian, shape)
    AREAT_G = gather_global(m, m.get("DXT") * m.get("DYT"), shape)
    ny, nx = shape
    if sum(1 for r in regions if r[0] < 0) > MAX_MS:
        raise ValueError("maximum number of marginal seas exceeded")
    seas = []
    for number, name, mblat, mblon, want_area in regions:
        if number >= 0:
            continue
        ipts, jpts, areas, area = [], [], [], 0.0
        lat_reach = lon_reach = 1.0
        done = False
        for _ in range(MAX_ITER):
            box = (mblat - lat_reach <= TLAT_G) & (mblat + lat_reach >= TLAT_G) & (mblon - lon_reach <= TLON_G) & (mblon + lon_reach >= TLON_G)
            for j, i in zip(*np.nonzero(box)):               # row-major: j outer, i inner, as the reference's loops
                if (i + 1, j + 1) in zip(ipts, jpts) or region_mask[j, i] <= 0:
                    continue
                if len(ipts) == max_points:
                    done = True
                    break
                ipts.append(int(i) + 1); jpts.append(int(j) + 1); areas.append(float(AREAT_G[j, i]))
                area = area + areas[-1]
                if area >= want_area:
                    done = True
                    break
            if done:
                break
            lat_reach, lon_reach = lat_reach + 1.0, lon_reach + 1.0
        if not ipts:
            raise ValueError("no points selected for distribution area")
        fracs, sum_frac = [], 0.0
        for a in areas:
            fracs.append(a / area)
            sum_frac = sum_frac + fracs[-1]
        fracs[-1] = fracs[-1] + (1.0 - sum_frac)
        MASK_G = np.zeros(shape)
        for i, j, f in zip(ipts, jpts, fracs):
            MASK_G[j - 1, i - 1] = f
        regs = {int(region_mask[j - 1, i - 1]) for i, j in zip(ipts, jpts)}
        seas.append(dict(number=number, ipts=np.array(ipts), jpts=np.array(jpts), fracs=np.array(fracs), area=area,
                         warn_two_regions=len(regs) > 1, warn_max_points=len(ipts) == max_points, MASK_FRAC=scatter_center(m, MASK_G),
                         IND=scatter_center(m, (region_mask == number).astype(np.float64))))
    return seas


def ms_consts(ice, sea_ice_salinity=4.0, rho_fw=1.0):
    """c_q, c_s, c_a, c_t of ms_balancing for flux_type 'salt' (ms_balance.F90:558-566); ice: ice_ref.params"""
    ors = ice["ocn_ref_salinity"]
    return dict(c_q=-(1.0e4 / ice["latent_heat_fusion"]) * (ors - sea_ice_salinity) / ors, c_s=-(1.0e3 / ors) * (rho_fw / ice["rho_sw"]),
                c_a=1.0e-4, c_t=-ors)


def ms_terms(m, f, seas, c, QFLUX):
    """per sea the TRANSPORT block array (ms_balance.F90:602-607), and STF2's overwrite inside the seas applied to a copy of STF2"""
    DXT, DYT = m.get("DXT"), m.get("DYT")
    WORK = f["EVAP_F"] + f["PREC_F"] + f["MELT_F"] + f["ROFF_F"] + f["IOFF_F"]
    qpos = np.maximum(0.0, QFLUX)
    T = (qpos * c["c_q"] + WORK * 1.0 + f["SALT_F"] * c["c_s"]) * DXT * DYT * c["c_a"]
    over = -qpos * c["c_q"] * c["c_t"] * 1.0e-4
    return [np.where(s["IND"] != 0.0, T, 0.0) for s in seas], over


def ms_apply(m, STF2, seas, c, over, transports):
    """STF2 after ms_balancing with the given transport of every sea: overwrite inside the seas, then the distribution, region order"""
    DXT, DYT = m.get("DXT"), m.get("DYT")
    out = STF2.copy()
    for s in seas:
        out = np.where(s["IND"] != 0.0, over, out)
    for s, tr in zip(seas, transports):
        out = out + s["MASK_FRAC"] * tr * c["c_t"] / (DXT * DYT)
    return out
