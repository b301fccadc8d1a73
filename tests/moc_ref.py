"""NumPy restatement of the meridional overturning circulation of source/diags_on_lat_aux_grid.F90, written from the reference and not
from the kernels: init_lat_aux_grid (:121-597), init_moc_ts_transport_arrays (:603-936) and compute_moc (:942-1288), with the
vertical velocity of comp_flux_vel (advection.F90:1970-2132), WTK at the top of cell k -- what advection.F90:1750 accumulates as WVEL.

Everything works on the gathered global arrays, (ny_global, nx_global), as the reference's ioroot does; the global triple loops
stand as they are, vectorised per bin.  compute_moc is linear in its inputs, so the MOC of the time means is the weighted mean of
the per-step sums; `entries` forms every term of every step in the reference's order of operations, adds the terms of a bin
exactly (math.fsum) and combines the few numbers per entry in extended precision, and returns with each entry the sum of |term| and
the number of non-zero terms, so that a test can bound the device's error by (N + 8) 2^-53 sum|term| whatever its order of summation.

The second half of the file is test data: the bent grid and the region mask of the MOC tests."""
import math

import numpy as np

import aniso_ref

U53 = 2.0 ** -53
EPS_GRID = 1.0e-7
RADIAN = 180.0 / (4.0 * math.atan(1.0))
GRID_TYPES = {"sou": 1, "ful": 2, "use": 3}


class Refused(Exception):
    """exit_POP of the reference, with its message"""


def nint(x):
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


# ---- global arrays -------------------------------------------------------------------------------------------------------------
def to_global(m, a, fill=0):
    """local blocks (nblocks, [nz,] ny_block, nx_block) of a single-rank model -> ([nz,] ny_global, nx_global), physical cells"""
    a = np.asarray(a)
    b4 = a if a.ndim == 4 else a[:, None]
    out = np.full((b4.shape[1], m.cfg.ny_global, m.cfg.nx_global), fill, dtype=a.dtype)
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        jg, ig = np.asarray(b["j_glob"]), np.asarray(b["i_glob"])
        js = [j for j in range(b["jb"] - 1, b["je"]) if jg[j] > 0]
        is_ = [i for i in range(b["ib"] - 1, b["ie"]) if ig[i] > 0]
        out[:, (jg[js] - 1)[:, None], (ig[is_] - 1)[None, :]] = b4[lb][:, js][:, :, is_]
    return out if a.ndim == 4 else out[0]


def block_of(m):
    """(ny_global, nx_global): the id of the block that owns the cell"""
    out = np.zeros((m.cfg.ny_global, m.cfg.nx_global), dtype=np.int32)
    for bid in range(1, m.nblocks_tot + 1):
        b = m.get_block(bid)
        jg, ig = np.asarray(b["j_glob"])[b["jb"] - 1:b["je"]], np.asarray(b["i_glob"])[b["ib"] - 1:b["ie"]]
        out[(jg[jg > 0] - 1)[:, None], (ig[ig > 0] - 1)[None, :]] = bid
    return out


def latitudes(m):
    """TLATD_G, ULATD_G and KMT as the reference gathers them (TLATD = TLAT * radian, :384-392)"""
    return to_global(m, m.get("TLAT") * RADIAN), to_global(m, m.get("ULAT") * RADIAN), to_global(m, m.geti("KMT"))


# ---- init_lat_aux_grid -----------------------------------------------------------------------------------------------------------
def lat_aux_grid(TLATD_G, ULATD_G, lat_aux_grid_type="southern", lat_aux_begin=-90.0, lat_aux_end=90.0, n_lat_aux_grid=180,
                 partial_bottom_cells=False):
    """(lat_aux_edge (n + 1,), lat_aux_center (n,)); arrays are indexed [j - 1, i - 1]"""
    kind = GRID_TYPES.get(lat_aux_grid_type[:3], -1000)                                  # :312-326
    if kind == -1000:
        raise Refused("(init_lat_aux_grid) unknown auxilary latitudinal grid choice")
    if partial_bottom_cells:                                                             # :367-371
        raise Refused("(init_lat_aux_grid): if (partial_bottom_cells), then 1st modify  subroutines compute_moc and compute_tracer_transports")
    T, U = TLATD_G, ULATD_G
    ny, nx = T.shape
    n = n_lat_aux_grid
    if kind in (1, 2):                                                                   # :394-399, i_copy = 1
        dlat = 2.0 * (U[0, 0] - T[0, 0])
        southern_edge = U[0, 0] - dlat
    if kind == 1:
        j_dim_sh = int(np.count_nonzero(T[:, 0] < 0.0))                                  # :409
        if j_dim_sh == 0:
            raise Refused("(init_lat_aux_grid) there are no Southern Hemisphere grid points")
        copy = T[:j_dim_sh, 0]                                                           # :422-430: the first value that is not the fill value
        if np.any(np.abs(T[:j_dim_sh] - copy[:, None]) > EPS_GRID):                      # :432-441
            raise Refused("(init_lat_aux_grid): SH is not a regular at-lon grid. Use a different choice for lat_aux_grid_type.")
        np_minus_northern_edge = 90.0 + southern_edge                                    # :454-472
        if np_minus_northern_edge >= 0.5 * dlat:
            n = nint(np_minus_northern_edge / dlat)
            if n == 0:
                raise Refused("(init_lat_aux_grid) n_lat_aux_grid is zero")
            dlat = np_minus_northern_edge / float(n)
            n = 2 * j_dim_sh + n
        else:
            n = 2 * j_dim_sh
    if kind == 2:                                                                        # :476-493
        n = ny
        if np.any(T != T[:, :1]):
            raise Refused("(init_lat_aux_grid): The model grid is not a regular lat-lon grid. Use a different choice for lat_aux_grid_type.")
    if kind == 3 and lat_aux_end <= lat_aux_begin:                                       # :497-502
        raise Refused("(init_lat_aux_grid) lat_aux_end should be > lat_aux_begin")
    edge, center = np.zeros(n + 1), np.zeros(n)                                          # edge[j - 1] = lat_aux_edge(j)
    if kind == 1:                                                                        # :520-551
        edge[0] = southern_edge
        edge[1:j_dim_sh + 1] = U[:j_dim_sh, 0]
        jj = j_dim_sh
        for j in range(j_dim_sh + 2, 2 * j_dim_sh + 2):
            edge[j - 1] = -edge[jj - 1]
            jj -= 1
        center[:j_dim_sh] = T[:j_dim_sh, 0]
        jj = j_dim_sh
        for j in range(j_dim_sh + 1, 2 * j_dim_sh + 1):
            center[j - 1] = -center[jj - 1]
            jj -= 1
        if n == 2 * j_dim_sh:
            edge[n] = 90.0
        else:
            for j in range(2 * j_dim_sh + 2, n + 2):
                edge[j - 1] = edge[2 * j_dim_sh] + (j - 2 * j_dim_sh - 1) * dlat
            for j in range(2 * j_dim_sh + 1, n + 1):
                center[j - 1] = edge[2 * j_dim_sh] + (j - 2 * j_dim_sh - 0.5) * dlat
    elif kind == 2:                                                                      # :553-558
        edge[0] = southern_edge
        edge[1:] = U[:, 0]
        center[:] = T[:, 0]
    else:                                                                                # :560-570
        dlat = (lat_aux_end - lat_aux_begin) / float(n)
        for j in range(1, n + 2):
            edge[j - 1] = lat_aux_begin + float(j - 1) * dlat
        for j in range(1, n + 1):
            center[j - 1] = lat_aux_begin + 0.5 * dlat + float(j - 1) * dlat
    return edge, center


# ---- init_moc_ts_transport_arrays ----------------------------------------------------------------------------------------------
def region_masks(REGION_MASK, n_transport_reg, reg2_numbers=()):
    """REGION_MASK_LAT_AUX(:, :, m) as (n_transport_reg, ny, nx) of 0 / 1 (:651-753)"""
    if n_transport_reg < 1:
        raise Refused("(init_moc_ts_transport_arrays)  n_transport_reg must be > 0  --  check namelist transports_nml")
    if n_transport_reg > 2:
        raise Refused("(init_moc_ts_transport_arrays)  n_transport_reg must be < 3  --  check namelist transports_nml")
    if n_transport_reg > 1 and len(reg2_numbers) <= 0:
        raise Refused("(init_moc_ts_transport_arrays)  no transport regions have been detected --  check namelist transports_nml")
    RM = [(REGION_MASK > 0).astype(np.int32)]
    if n_transport_reg > 1:
        RM.append(np.isin(np.abs(REGION_MASK), list(reg2_numbers)).astype(np.int32))
    return np.stack(RM)


def region_start(RM, TLATD_G):
    """lat_aux_region_start(m) as a list (:755-787); the library refuses j_southern = 1, where the reference reads row 0"""
    start = [0] * RM.shape[0]
    if RM.shape[0] > 1:
        ny = TLATD_G.shape[0]
        rows = np.nonzero(RM[1].any(axis=1))[0]
        j_southern = int(rows[0]) + 1 if rows.size else ny
        row = TLATD_G[j_southern - 1]
        if np.any(np.abs(row[:, None] - row[None, :]) > EPS_GRID):
            raise Refused('(init_moc_ts_transport_arrays) SH is not a regular lat-lon grid. The southern boundary for region 2 ("Atlantic") cannot be specified.')
        start[1] = j_southern - 1
    return start


def bin_map(TLATD_G, edge):
    """the 1-based bin b of every cell, lat_aux_edge(b) <= TLATD_G < lat_aux_edge(b + 1) (the loop index n = b + 1 of :811, :1061); 0:
    in no bin.  The edges of the tests increase, so a cell lies in at most one bin."""
    assert np.all(np.diff(edge) > 0)
    out = np.zeros(TLATD_G.shape, dtype=np.int32)
    for n in range(2, edge.size + 1):
        out[(TLATD_G >= edge[n - 2]) & (TLATD_G < edge[n - 1])] = n - 1
    return out


def mask_lat_depth(BIN, KMT_G, RM, n_lat, km):
    """MASK_LAT_DEPTH(n, k, m) as a bool array (n_lat, km, n_transport_reg) (:804-823)"""
    out = np.ones((n_lat, km, RM.shape[0]), dtype=bool)
    for k in range(1, km + 1):
        for n in range(2, n_lat + 2):
            for m in range(RM.shape[0]):
                if np.any((BIN == n - 1) & (k <= KMT_G) & (RM[m] == 1)):
                    out[n - 2, k - 1, m] = False
    return out


def n_moc_comp(cfg):
    """:842-844: registry_match('diag_gm_bolus'), registry_match('init_submeso')"""
    n = 1
    if cfg.hmix_tracer == 3 and cfg.gm_diag_bolus:
        n = 2
    if getattr(cfg, "lsubmesoscale_mixing", 0):
        n = 3
    return n


# ---- compute_moc ---------------------------------------------------------------------------------------------------------------
def _sh(A, di, dj):
    """A(i + di, j + dj) where the block holds such a neighbour, 0 elsewhere (never for a physical cell)"""
    out = np.zeros_like(A)
    ny, nx = A.shape[-2:]
    js, jd = (slice(0, ny + dj), slice(-dj, ny)) if dj < 0 else (slice(dj, ny), slice(0, ny - dj))
    is_, id_ = (slice(0, nx + di), slice(-di, nx)) if di < 0 else (slice(di, nx), slice(0, nx - di))
    out[..., jd, id_] = A[..., js, is_]
    return out


def geometry(m):
    g = {n: m.get(n) for n in ("TAREA", "TAREA_R", "DXU", "DYU")}
    g["HTN"] = m.get("HTN") if m.cfg.hmix_tracer == 3 else np.zeros_like(g["DXU"])   # only the bolus and submesoscale terms read it
    g["KMT"] = m.geti("KMT")
    g["dz"] = aniso_ref.vertical_dz(m.km)
    return g


def read_step(m):
    """after pop_baroclinic_driver: the velocities advt saw, DH of pop_dhdt, the stored bolus and submesoscale velocities"""
    s = dict(U=m.get("UVEL", 1), V=m.get("VVEL", 1), DH=m.get("DH"))
    if m.cfg.hmix_tracer == 3 and m.cfg.gm_diag_bolus:
        s["WISOP"], s["VISOP"] = m.get("WISOP"), m.get("VISOP")
    if getattr(m.cfg, "lsubmesoscale_mixing", 0):
        s["WSUBM"], s["VSUBM"] = m.get("WSUBM"), m.get("VSUBM")
    return s


def wvel(g, s, km):
    """WTK at the top of every cell (nblocks, km, ny, nx): WTK(1) = DH, WTK(k + 1) = WTKB(k) of comp_flux_vel"""
    U, V = s["U"], s["V"]
    fu, fv = U * g["DYU"][:, None], V * g["DXU"][:, None]
    UTE = 0.5 * (fu + _sh(fu, 0, -1)); UTW = 0.5 * (_sh(fu, -1, 0) + _sh(fu, -1, -1))       # advection.F90:2071-2079
    VTN = 0.5 * (fv + _sh(fv, -1, 0)); VTS = 0.5 * (_sh(fv, 0, -1) + _sh(fv, -1, -1))
    W = np.zeros_like(U)
    w = s["DH"].copy()
    for k in range(1, km + 1):
        W[:, k - 1] = w
        if k < km:
            FC = (VTN[:, k - 1] - VTS[:, k - 1] + UTE[:, k - 1] - UTW[:, k - 1]) * g["TAREA_R"]
            w = np.where(k < g["KMT"], w + g["dz"][k] * FC, 0.0)                             # :2101-2114
        else:
            w = np.zeros_like(w)
    return W


def step_terms(m, g, s, ncomp):
    """the terms of one step on the global arrays: W[c] (km, ny, nx) = merge(W * TAREA, 0, k <= KMT) (:1027, 1036, 1045) and
    S[c] (km, ny, nx) = the southern-boundary terms (:1097-1104, 1114, 1125); a component without its switch stays 0"""
    km = m.km
    wet = np.arange(1, km + 1)[None, :, None, None] <= g["KMT"][:, None]
    TAREA, DXU, HTN = g["TAREA"][:, None], g["DXU"][:, None], g["HTN"][:, None]
    zero = np.zeros_like(s["U"])
    Wc = [np.where(wet, wvel(g, s, km) * TAREA, 0.0)]
    W1 = 0.5 * s["V"] * DXU
    Sc = [W1 + _sh(W1, -1, 0)]                     # WORK1(i) + WORK1(i-1); the column the reference zeroes is a ghost column
    if ncomp > 1:
        Wc.append(np.where(wet, s["WISOP"] * TAREA, 0.0) if "WISOP" in s else zero)
        Sc.append(s["VISOP"] * HTN if "VISOP" in s else zero)
    if ncomp > 2:
        Wc.append(np.where(wet, s["WSUBM"] * TAREA, 0.0))
        Sc.append(s["VSUBM"] * HTN)
    return [to_global(m, a) for a in Wc], [to_global(m, a) for a in Sc]


def entries(steps, weights, tavg_sum, BIN, RM, start, dz, n_lat):
    """steps: the step_terms of every accumulated step; weights: their dtavg.  Returns (value, magnitude, count), each
    (n_lat + 1, km + 1, ncomp, nreg): TAVG_MOC_G in Sverdrups (:1054-1189), the same expression over |term|, and the number of non-zero
    terms that enter the entry."""
    L = np.longdouble
    ncomp, km = len(steps[0][0]), steps[0][0][0].shape[0]
    nreg = RM.shape[0]
    val = np.zeros((n_lat + 1, km + 1, ncomp, nreg), dtype=L)
    mag, cnt = val.copy(), np.zeros(val.shape, dtype=np.int64)
    for m in range(nreg):
        for c in range(ncomp):
            bv, bm, bc = (np.zeros((n_lat, km), dtype=L) for _ in range(3))
            for n in range(2, n_lat + 2):
                sel = (BIN == n - 1) & (RM[m] == 1)
                if not sel.any():
                    continue
                for (Wc, _), w in zip(steps, weights):
                    t = Wc[c][:, sel]
                    for k in range(km):
                        bv[n - 2, k] += L(w) * L(math.fsum(t[k])); bm[n - 2, k] += L(w) * L(math.fsum(np.abs(t[k])))
                        bc[n - 2, k] += np.count_nonzero(t[k])
            val[1:, :km, c, m] = np.cumsum(bv, axis=0); mag[1:, :km, c, m] = np.cumsum(bm, axis=0)      # :1057-1083
            cnt[1:, :km, c, m] = np.cumsum(bc, axis=0).astype(np.int64)
            if m >= 1:                                                                                  # :1133-1182
                j = start[m]
                sel = RM[m][j] == 1                 # REGION_MASK_LAT_AUX(i, j + 1, m), rows 0-based here
                sv, sm, sc = (np.zeros(km, dtype=L) for _ in range(3))
                for (_, Sc), w in zip(steps, weights):
                    t = Sc[c][:, j - 1, sel]
                    for k in range(km):
                        sv[k] += L(w) * L(math.fsum(t[k])); sm[k] += L(w) * L(math.fsum(np.abs(t[k]))); sc[k] += np.count_nonzero(t[k])
                ms, mm, mc = np.zeros(km + 1, dtype=L), np.zeros(km + 1, dtype=L), np.zeros(km + 1, dtype=L)
                for k in range(km, 0, -1):          # moc_s(k) = moc_s(k + 1) - dz(k) * s(k)
                    ms[k - 1] = ms[k] - L(dz[k]) * sv[k - 1]; mm[k - 1] = mm[k] + L(dz[k]) * sm[k - 1]; mc[k - 1] = mc[k] + sc[k - 1]
                val[:, :km, c, m] += ms[None, :km]; mag[:, :km, c, m] += mm[None, :km]
                cnt[:, :km, c, m] += mc[None, :km].astype(np.int64)
    scale = L(1.0e-12) / L(tavg_sum)
    return val * scale, mag * scale, cnt


def bound(mag, cnt):
    """(N + 8) 2^-53 sum|term|: the first-order bound of any order of summation of N terms; the 8 covers the rounded weight of a step,
    1 / tavg_sum and the scaling, dz * s and the addition of the boundary transport, the unit factor and the restatement's own fsum"""
    return (cnt + 8) * np.longdouble(U53) * mag


# ---- test data -----------------------------------------------------------------------------------------------------------------
def bent_grid(cfg, bend=True, lat_span=160.0, one_longitude=False):
    """popcfg.synthetic_grid with ULAT bent north of the equator by a longitude-dependent amount of about one row (TEST DATA: the
    other records stay as they are); the southern hemisphere stays regular, so the 'southern' check passes.  one_longitude: every
    ULON is 0, so that the rows of TLAT, a Cartesian average of the corner points, hold one number each -- bit for bit, which the
    'full' grid type asks for"""
    from popcfg import synthetic_grid
    g = synthetic_grid(cfg, lat_span=lat_span)
    if one_longitude:
        g["ULON"] = np.zeros_like(g["ULON"])
    if bend:
        ny, nx = g["ULAT"].shape
        dlat = lat_span / ny / RADIAN
        i = np.arange(1, nx + 1, dtype=np.float64)[None, :]
        lat = g["ULAT"]
        g["ULAT"] = np.ascontiguousarray(np.where(lat > 1.0e-9, lat + dlat * np.sin(2.0 * np.pi * i / nx) * np.clip(lat / (2.0 * dlat), 0.0, 1.0), lat))
    return g


def region_mask(KMT_G, j_southern=12):
    """REGION_MASK (TEST DATA): +1 on ocean cells, a sector of +6 north of row j_southern (columns 1 .. 12), a marginal sea of -7"""
    R = np.where(KMT_G > 0, 1, 0).astype(np.int32)
    ny, nx = R.shape
    sector = np.zeros_like(R, dtype=bool); sector[j_southern - 1:, :12] = True
    sea = np.zeros_like(R, dtype=bool); sea[29:33, 21:26] = True
    R[sector & (KMT_G > 0)] = 6
    R[sea & (KMT_G > 0)] = -7
    return R


REG2 = (6,)
GM = dict(hmix_tracer=3, ah=0.8e7, gm_diag_bolus=1)
SOUTHERN = dict(lat_aux_grid_type="southern")
USER = dict(lat_aux_grid_type="user-specified", lat_aux_begin=-60.0, lat_aux_end=60.0, n_lat_aux_grid=24)
# name -> (config keywords, submeso_config keywords or None, grid keywords, transports_nml keywords, two regions)
CASES = {
    "avgfit": (dict(), None, dict(), SOUTHERN, True),                                   # centred advection, const vmix, an averaging step
    "kpp_robert": (dict(vmix_choice=3, km=24, tmix_opt=3), None, dict(), SOUTHERN, False),
    "gm_bolus": (dict(GM), None, dict(), USER, True),                                   # some ocean cells lie in no bin
    # KPP: the mixed layer of submeso_sf is HMXL, deeper than the first level, so WSUBM moves (it is 0 where the layer ends at zw(1))
    "gm_submeso": (dict(GM, vmix_choice=3, km=24), dict(submeso_diag=1), dict(), SOUTHERN, True),
    "submeso_no_bolus": (dict(hmix_tracer=3, ah=0.8e7, vmix_choice=3, km=24), dict(submeso_diag=1), dict(), SOUTHERN, False),   # component 2 stays 0
    "full": (dict(), None, dict(bend=False, one_longitude=True), dict(lat_aux_grid_type="full"), True),
}
