"""NumPy restatement of the northward tracer transports of source/diags_on_lat_aux_grid.F90, written from the reference and not from
the kernels: n_transport_comp (:886-889), compute_tracer_transports (:1294-1594) and the per-column inputs the reference feeds it from
tavg (tavg.F90:7556-7614):

    ADV   = sum_k -dz(k) LTK(k), k <= KMT                advection.F90:1803-1821, LTK of advt_centered (:2243-2301) with the flux
                                                         velocities of comp_flux_vel (:2068-2127)
    HDIF  = sum_k dz(k) HDTK(k), k <= KMT                horizontal_mix.F90:592-609, HDTK of hdifft_del2 (hmix_del2.F90:1062-1095)
    VNF   = sum_k FN(k) TAREA dz(k)                      diags_on_lat_aux_grid.F90:1484, FN = FVN (T + T_north), FVN = p5 VTN TAREA_R
                                                         (advection.F90:1746, 1777)
    ADV_I, VNF_I / ADV_SM, VNF_SM                        hmix_gm_share.F90:276-361 / mix_submeso.F90:679-748, from the library's
                                                         UISOP, VISOP / USUBM, VSUBM fields

Every column formula is written once as a function of an `Ops` object: with Ops(False) it is the reference's expression in its order of
operations; with Ops(True) every input is replaced by its magnitude and every subtraction by an addition, which gives the sum of the
magnitudes of the terms the formula adds -- the scale of its first-order rounding bound.  Fields are handled block by block,
(nblocks, [km,] ny_block, nx_block) with their ghost cells, as the reference's block loops do; moc_ref.to_global gathers them.

The second half restates compute_tracer_transports on the gathered global arrays (the triple loop vectorised per bin), once as the
reference runs it in r8 (`compute_tracer_transports`) and once with exact sums (`entries`, the manner of moc_ref.entries), and holds
the helpers the device tests share."""
import math

import numpy as np

import moc_ref
from moc_ref import _sh, to_global

UNDEFINED_NF = 9.9692099683868690e+36                          # netcdf.inc NF_FILL_FLOAT, undefined_nf
HFLUX_FACTOR = 1000.0 / ((4.1 / 3.996) * 3.996e7)              # pop_constants.F90:336 with rho_sw = 4.1/3.996, cp_sw = 3.996e7
COLUMN_FIELDS = ("TRN_ADV", "TRN_HDIF", "TRN_VNF", "TRN_ADV_ISOP", "TRN_VNF_ISOP", "TRN_ADV_SUBM", "TRN_VNF_SUBM")
BIN_FIELDS = ("TRN_ADV", "TRN_HDIF", "TRN_ADV_ISOP", "TRN_ADV_SUBM")      # components 2, 3, 4, 5 (:1453-1461)
BND_FIELDS = ("TRN_VNF", "TRN_VNF_ISOP", "TRN_VNF_SUBM")                  # trans_s(2), (4), (5) (:1513-1517)
BND_COMP = (1, 3, 4)                                                      # 0-based component each boundary term is added to


def n_transport_comp(cfg):
    """:886-889: registry_match('diag_gm_bolus'), registry_match('init_submeso')"""
    n = 3
    if cfg.hmix_tracer == 3 and cfg.gm_diag_bolus:
        n = 4
    if getattr(cfg, "lsubmesoscale_mixing", 0):
        n = 5
    return n


# ---- the per-column terms --------------------------------------------------------------------------------------------------------
class Ops:
    """mag = False: the expression itself; mag = True: |inputs| and every subtraction an addition"""

    def __init__(self, mag):
        self.mag = mag

    def x(self, a):
        return np.abs(a) if self.mag else a

    def sub(self, a, b):
        return a + b if self.mag else a - b

    def neg(self, a):
        return a if self.mag else -a


def geometry(m):
    g = {n: m.get(n) for n in ("TAREA", "TAREA_R", "DXU", "DYU", "DTN", "DTS", "DTE", "DTW")}
    for n in ("KMT", "KMTN", "KMTS", "KMTE", "KMTW"):
        g[n] = m.geti(n)
    if m.cfg.hmix_tracer == 3:
        g["HTE"], g["HTN"] = m.get("HTE"), m.get("HTN")
    g["dz"] = moc_ref.aniso_ref.vertical_dz(m.km)
    return g


def mix_level(m):
    """time level of the mix-time fields of the step pop_time_manager set up: old on a leapfrog step, else cur"""
    return 0 if m.dim("leapfrogts") else 1


def read_step(m):
    """after pop_baroclinic_driver: what the tracer right-hand side of the step read"""
    tm = mix_level(m)
    s = dict(U=m.get("UVEL", 1), V=m.get("VVEL", 1), DH=m.get("DH"), T=[m.get("TRACER", 1, n) for n in (0, 1)],
             TMIX=[m.get("TRACER", tm, n) for n in (0, 1)])
    if m.cfg.hmix_tracer == 3 and m.cfg.gm_diag_bolus:
        s["UISOP"], s["VISOP"] = m.get("UISOP"), m.get("VISOP")
    if getattr(m.cfg, "lsubmesoscale_mixing", 0):
        s["USUBM"], s["VSUBM"] = m.get("USUBM"), m.get("VSUBM")
    return s


def flux_velocities(g, s, o):
    """UTE, UTW, VTN, VTS (nblocks, km, ny, nx) of comp_flux_vel (advection.F90:2071-2079); UTW = UTE(i-1), VTS = VTN(j-1)"""
    fu, fv = o.x(s["U"]) * g["DYU"][:, None], o.x(s["V"]) * g["DXU"][:, None]
    UTE = 0.5 * (fu + _sh(fu, 0, -1)); UTW = 0.5 * (_sh(fu, -1, 0) + _sh(fu, -1, -1))
    VTN = 0.5 * (fv + _sh(fv, -1, 0)); VTS = 0.5 * (_sh(fv, 0, -1) + _sh(fv, -1, -1))
    return UTE, UTW, VTN, VTS


def centered_column(g, s, n, km, mag=False):
    """(ADV, VNF) of tracer n with centred advection, (nblocks, ny, nx).  Rounding operations on the longest path to ADV: the flux
    velocity (2: products, sum; the p5 is exact), the divergence (3), times the tracer (1), the five-term sum (4), TAREA_R (1), the
    two vertical terms (2), dz * L (1), the sum over km levels (km) = 14 + km; WTK adds its own march, dz * FC per level and the sum
    over the levels above (km at most) = 14 + 2 km.  To VNF: 2 + TAREA_R (1) + the product with T + T_north (1) + TAREA (1) + dz (1) +
    km = 6 + km."""
    o = Ops(mag)
    UTE, UTW, VTN, VTS = flux_velocities(g, s, o)
    T = o.x(s["T"][n])
    dz, KMT = g["dz"], g["KMT"]
    dz2r = [0.0] + [0.5 / dz[k] for k in range(1, km + 1)]
    ADV, VNF = np.zeros_like(g["TAREA"]), np.zeros_like(g["TAREA"])
    w = o.x(s["DH"]).copy()                                                     # WTK(1) = DH (advection.F90:2090)
    for k in range(1, km + 1):
        q = k - 1
        hdiv = o.sub(o.sub(VTN[:, q], VTS[:, q]) + UTE[:, q], UTW[:, q])
        if k < km:                                                              # :2101-2114
            wb = np.where(k < KMT, w + dz[k] * (hdiv * g["TAREA_R"]), 0.0)
        else:
            wb = np.zeros_like(w)
        Tk = T[:, q]
        L = o.sub(o.sub(hdiv * Tk + VTN[:, q] * _sh(Tk, 0, 1), VTS[:, q] * _sh(Tk, 0, -1)) + UTE[:, q] * _sh(Tk, 1, 0), UTW[:, q] * _sh(Tk, -1, 0))
        L = 0.5 * L * g["TAREA_R"]                                              # :2247-2253
        if k != 1:                                                              # :2272-2285, variable-thickness surface layer
            L = L + dz2r[k] * w * (T[:, q - 1] + Tk)
        if k < km:                                                              # :2291-2299
            L = o.sub(L, dz2r[k] * wb * (Tk + T[:, q + 1]))
        ADV = ADV + np.where(k <= KMT, o.neg(dz[k] * L), 0.0)                   # :1815-1817
        FVN = 0.5 * VTN[:, q] * g["TAREA_R"]                                    # :1746
        VNF = VNF + FVN * (Tk + _sh(Tk, 0, 1)) * g["TAREA"] * dz[k]             # :1777, diags_on_lat_aux_grid.F90:1484
        w = wb
    return ADV, VNF


def del2_column(g, s, n, km, ah, mag=False):
    """HDIF of tracer n with Laplacian mixing, (nblocks, ny, nx).  Rounding operations: the central coefficient (3), times the
    tracer (1), the five-term sum (4), ah (1), dz (1), the sum over the levels (km) = 10 + km."""
    o = Ops(mag)
    TM = o.x(s["TMIX"][n])
    dz, KMT = g["dz"], g["KMT"]
    HDIF = np.zeros_like(g["TAREA"])
    for k in range(1, km + 1):
        wet = k <= KMT
        CN, CS = np.where((k <= g["KMTN"]) & wet, g["DTN"], 0.0), np.where((k <= g["KMTS"]) & wet, g["DTS"], 0.0)     # :1064-1071
        CE, CW = np.where((k <= g["KMTE"]) & wet, g["DTE"], 0.0), np.where((k <= g["KMTW"]) & wet, g["DTW"], 0.0)
        CC = o.neg(CN + CS + CE + CW)
        Tk = TM[:, k - 1]
        H = ah * (CC * Tk + CN * _sh(Tk, 0, 1) + CS * _sh(Tk, 0, -1) + CE * _sh(Tk, 1, 0) + CW * _sh(Tk, -1, 0))      # :1089-1093
        HDIF = HDIF + np.where(wet, dz[k] * H, 0.0)                                                                   # horizontal_mix.F90:597
    return HDIF


def eddy_column(g, U, V, TMIX, km, mag=False):
    """(ADV_x, VNF_x) of one tracer from an eddy-induced or submesoscale velocity pair on the east / north faces
    (hmix_gm_share.F90:278-307, 349-354; mix_submeso.F90:681-700, 732-737).  Rounding operations to ADV_x: a face product (3: HTE U,
    the tracer sum, their product; the p5 is exact), the four-term combination (3), dz TAREA_R and its product (2), the sum over the
    levels (km) = 8 + km; to VNF_x: V HTN TAREA_R (2), the tracer sum and the product (2), TAREA (1), dz (1), km = 6 + km."""
    o = Ops(mag)
    U, V, TM = o.x(U), o.x(V), o.x(TMIX)
    dz, KMT = g["dz"], g["KMT"]
    HTE, HTN = g["HTE"], g["HTN"]
    ADV, VNF = np.zeros_like(g["TAREA"]), np.zeros_like(g["TAREA"])
    for k in range(1, km + 1):
        Tk = TM[:, k - 1]
        W1 = 0.5 * HTE * U[:, k - 1] * (Tk + _sh(Tk, 1, 0))
        W3 = o.sub(W1, _sh(W1, -1, 0))                                          # eoshift(WORK1, dim=1, shift=-1): the value of column i - 1
        W1 = 0.5 * HTN * V[:, k - 1] * (Tk + _sh(Tk, 0, 1))
        W3 = o.sub(W3 + W1, _sh(W1, 0, -1))
        ADV = ADV + np.where(k <= KMT, o.neg(dz[k] * g["TAREA_R"] * W3), 0.0)
        VNF = VNF + (0.5 * V[:, k - 1] * HTN * g["TAREA_R"]) * (Tk + _sh(Tk, 0, 1)) * g["TAREA"] * dz[k]
    return ADV, VNF


# ---- compute_tracer_transports ---------------------------------------------------------------------------------------------------
def masked_entries(MASK, ncomp):
    """bool (n_lat + 1, ncomp, nreg): where :1563-1578 put undefined_nf; MASK = MASK_LAT_DEPTH as (n_lat, km, nreg)"""
    n_lat, _, nreg = MASK.shape
    M1 = MASK[:, 0, :]
    out = np.zeros((n_lat + 1, ncomp, nreg), dtype=bool)
    for m in range(nreg):
        for n in range(1, n_lat):                                               # n = 1 .. n_lat_aux_grid - 1
            if M1[n - 1, m] and M1[n, m]:
                out[n, :, m] = True                                             # TR_TRANS_G(n + 1, :, m)
        if M1[0, m]:
            out[0, :, m] = True
        if M1[n_lat - 1, m]:
            out[n_lat, :, m] = True
    for m in range(1, nreg):
        out[:, 0, m] = True
        out[:, 2, m] = True
    return out


def compute_tracer_transports(tracer_index, WORK_G, FN_G, BIN, RM, start, MASK, ncomp):
    """the routine as the reference runs it in r8, on the time means.  WORK_G: the gathered -X * TAREA of ADV, HDIF[, ADV_I[, ADV_SM]]
    (a missing one None); FN_G: the gathered sum over k of FN * TAREA * dz of FN[, FN_I[, FN_SM]].  Returns TR_TRANS_G as
    (n_lat + 1, ncomp, nreg).  The total is accumulated as the reference does, WORK1_G + WORK2_G per cell (:1453)."""
    n_lat, nreg = MASK.shape[0], RM.shape[0]
    TR = np.zeros((n_lat + 1, ncomp, nreg))
    ny, nx = BIN.shape
    for n in range(2, n_lat + 2):
        TR[n - 1] = TR[n - 2]
        for m in range(nreg):
            for j in range(ny):
                for i in np.nonzero((BIN[j] == n - 1) & (RM[m][j] == 1))[0]:
                    TR[n - 1, 0, m] = TR[n - 1, 0, m] + WORK_G[0][j, i] + WORK_G[1][j, i]
                    for f in range(1, ncomp):
                        if WORK_G[f - 1] is not None:
                            TR[n - 1, f, m] = TR[n - 1, f, m] + WORK_G[f - 1][j, i]
    for m in range(1, nreg):
        j = start[m]
        for f, comp in enumerate(BND_COMP):
            if comp < ncomp and FN_G[f] is not None:
                trans_s = 0.0
                for i in np.nonzero(RM[m][j] == 1)[0]:                          # REGION_MASK_LAT_AUX(i, j + 1, m), rows 0-based here
                    trans_s = trans_s + FN_G[f][j - 1, i]
                TR[:, comp, m] = TR[:, comp, m] + trans_s
    if tracer_index == 1:
        TR = TR * (1.0e-19 / HFLUX_FACTOR)
    TR[masked_entries(MASK, ncomp)] = UNDEFINED_NF
    return TR


def entries(tracer_index, steps, weights, tavg_sum, BIN, RM, start, ncomp):
    """steps: per accumulated step (bin terms, boundary terms) on the global arrays -- the -X * TAREA of BIN_FIELDS and the VNF of
    BND_FIELDS, a missing one None; weights: their dtavg.  Returns (value, magnitude, count), each (n_lat + 1, ncomp, nreg): the
    unmasked transports with the terms of an entry added exactly (math.fsum) and the few numbers per entry combined in extended
    precision, the same expression over |term|, and the number of non-zero terms that enter the entry."""
    L = np.longdouble
    n_lat, nreg = steps[0][2], RM.shape[0]
    val = np.zeros((n_lat + 1, ncomp, nreg), dtype=L)
    mag, cnt = val.copy(), np.zeros(val.shape, dtype=np.int64)
    for m in range(nreg):
        for f in range(1, ncomp):
            bv, bm, bc = (np.zeros(n_lat, dtype=L) for _ in range(3))
            for n in range(2, n_lat + 2):
                sel = (BIN == n - 1) & (RM[m] == 1)
                if not sel.any():
                    continue
                for (Bt, _, _), w in zip(steps, weights):
                    if Bt[f - 1] is None:
                        continue
                    t = Bt[f - 1][sel]
                    bv[n - 2] += L(w) * L(math.fsum(t)); bm[n - 2] += L(w) * L(math.fsum(np.abs(t))); bc[n - 2] += np.count_nonzero(t)
            val[1:, f, m] = np.cumsum(bv); mag[1:, f, m] = np.cumsum(bm); cnt[1:, f, m] = np.cumsum(bc).astype(np.int64)
        val[:, 0, m] = val[:, 1, m] + val[:, 2, m]; mag[:, 0, m] = mag[:, 1, m] + mag[:, 2, m]; cnt[:, 0, m] = cnt[:, 1, m] + cnt[:, 2, m]
        if m >= 1:
            j = start[m]
            sel = RM[m][j] == 1
            for f, comp in enumerate(BND_COMP):
                if comp >= ncomp:
                    continue
                sv, sm, sc = L(0), L(0), 0
                for (_, St, _), w in zip(steps, weights):
                    if St[f] is None:
                        continue
                    t = St[f][j - 1, sel]
                    sv += L(w) * L(math.fsum(t)); sm += L(w) * L(math.fsum(np.abs(t))); sc += int(np.count_nonzero(t))
                val[:, comp, m] += sv; mag[:, comp, m] += sm; cnt[:, comp, m] += sc
    scale = L(1.0) / L(tavg_sum)
    if tracer_index == 1:
        scale = scale * L(1.0e-19) / L(HFLUX_FACTOR)
    return val * scale, mag * scale, cnt


def device_step_terms(m, TAREA, n, n_lat):
    """the terms of one step from the device's own column fields of tracer n (0-based): (bin terms, boundary terms, n_lat)"""
    def field(name):
        try:
            return m.get(name, 1, n)
        except Exception:                                                       # the configuration does not form it
            return None
    B = [field(f) for f in BIN_FIELDS]
    S = [field(f) for f in BND_FIELDS]
    return ([None if a is None else to_global(m, -(a * TAREA)) for a in B], [None if a is None else to_global(m, a) for a in S], n_lat)


# ---- helpers of the device tests ---------------------------------------------------------------------------------------------------
def make(pkg, case, request=1, tuning=None, heat=True, salt=True, moc=False, cfg_extra=None, walls=False, two_regions=None, perturb_salt=True):
    """a model of moc_ref.CASES on the bent grid with perturbed tracers, init_transports done and the transports requested in stream
    `request` (0: not requested); returns (model, ref) with what the restatements need.  walls (TEST DATA): land in columns 1 and 12
    from the row south of the sector of moc_ref.region_mask northwards, so that region 2 is closed on its west and east sides"""
    from popcfg import named_config
    kw, sub, gkw, nml, two = moc_ref.CASES[case]
    two = two if two_regions is None else two_regions
    kw = dict(kw, **(cfg_extra or {}))
    cfg = named_config("tiny", **kw)
    if sub is not None:
        cfg = pkg.submeso_config(cfg, **sub)
    grid = moc_ref.bent_grid(cfg, **gkw)
    if walls:
        grid["KMT"] = grid["KMT"].copy()
        grid["KMT"][10:, 0] = 0; grid["KMT"][10:, 11] = 0
    m = pkg.PopModel(cfg, grid=grid, tuning=tuning)
    wet = np.arange(1, m.km + 1)[None, :, None, None] <= m.geti("KMT")[:, None]
    rng = np.random.default_rng(5)
    for n in ((0, 1) if perturb_salt else (0,)):
        for tl in (0, 1):
            T = m.get("TRACER", tl, n)
            amp = 0.05 if n == 0 else 1.0e-5                                    # salinity in g/g
            m.set("TRACER", np.where(wet, T + amp * rng.standard_normal(T.shape), 0.0), tl=tl, n=n)
            m.halo_update("TRACER", tl, n)
    T, U, KMT = moc_ref.latitudes(m)
    R = moc_ref.region_mask(KMT) if two else None
    m.init_transports(R, moc_ref.REG2 if two else (), **nml)
    if moc:
        m.moc_request(moc)
    if request:
        m.transport_request(request, heat, salt)
    edge, _ = m.lat_aux_grid()
    RM = moc_ref.region_masks(R if two else (KMT > 0).astype(np.int32), 2 if two else 1, moc_ref.REG2 if two else ())
    ref = dict(BIN=moc_ref.bin_map(T, edge), RM=RM, start=moc_ref.region_start(RM, T), KMT=KMT, n_lat=edge.size - 1,
               ncomp=n_transport_comp(cfg), TAREA=m.get("TAREA"), MASK=m.moc_mask(), steps=([], []), weights=[])
    return m, ref


def step(m, ref=None):
    """one step phase by phase; ref: the device's column fields are read where the site left them, after pop_baroclinic_driver"""
    m.time_manager(); m.dhdt(); m.baroclinic_driver()
    if ref is not None:
        for n in (0, 1):
            ref["steps"][n].append(device_step_terms(m, ref["TAREA"], n, ref["n_lat"]))
        ref["weights"].append(m.scalar("dtt") * m.scalar("time_weight"))        # dtavg of tavg_set_flag: dtt, half of it when averaging
    m.barotropic_driver(); m.baroclinic_correct_adjust(); m.step_tail()


def check(got, ref, tracer, tavg_sum, what, factor=1):
    """pop_transport_get of tracer (1 | 2) against the exact sums of the accumulated steps' own column fields: unmasked entries within
    moc_ref.bound, masked ones exactly undefined_nf and exactly where the restatement puts them"""
    val, mag, cnt = entries(tracer, ref["steps"][tracer - 1], ref["weights"], tavg_sum, ref["BIN"], ref["RM"], ref["start"], ref["ncomp"])
    masked = masked_entries(ref["MASK"], ref["ncomp"])
    assert got.shape == masked.shape
    assert np.array_equal(got == UNDEFINED_NF, masked), what
    b = moc_ref.bound(mag, cnt) * factor
    err = np.where(masked, 0, np.abs(got.astype(np.longdouble) - val))
    w = np.unravel_index(np.argmax(np.where((b > 0) & ~masked, err / np.where(b > 0, b, 1), 0)), err.shape)
    print("%-22s tracer %d max|TR| %.6e  entry %s: TR %.17e  |diff| %.3e  bound %.3e  terms %d  |diff| / bound %.3f" %
          (what, tracer, np.abs(got[~masked]).max(), tuple(int(x) for x in w), got[w], err[w], b[w], cnt[w], float(err[w] / b[w]) if b[w] > 0 else 0.0))
    assert np.all(err <= b), (what, w, got[w], val[w], err[w], b[w])
    assert np.all(got[(mag == 0) & ~masked] == 0.0)                              # nothing to add: exactly 0
    return val, mag, cnt
