"""NumPy restatement of the global and CFL diagnostics (source/diagnostics.F90), written from the reference, not from the kernels:
diag_global_preupdate (:1174-1431), diag_global_afterupdate (:1548-1770), cfl_advect (:2262-2425) with the flux velocities of
comp_flux_vel (advection.F90:1970-2132), cfl_hdiff (:2695-2767) with the numbers of hmix_del2.F90:944-956 / :1125-1137,
hmix_del4.F90:865-876 / :1089-1100, hmix_aniso.F90:1043-1055 and hmix_gm.F90:2162-2172, and cfl_check (:2837-3145).

Global sums: every term is formed in the reference's order of operations on whole block arrays; `terms(...)` returns them so that a
test can sum them exactly (math.fsum) and bound the device's error by N * 2^-53 * sum|term|, whatever the order of summation.
Maxima: the reference's scans -- per block in (j, i) order with a strict >, blocks by maxloc (the first block that holds the
largest), levels with a strict > starting from -1 -- so values and addresses are compared for equality."""
import math

import numpy as np

import aniso_ref
from common import physical

GRAV = 980.6                                     # pop_constants.F90:235
SALT_TO_PPT = 1000.0
HFLUX_FACTOR = 1000.0 / ((4.1 / 3.996) * 3.996e7)   # pop_constants.F90:336 with the code defaults of rho_sw, cp_sw
SALINITY_FACTOR = -34.7 * 1.0e-4                 # :364-365 with ocn_ref_salinity = 34.7
LEFT_OUT = ["diag_ke_adv", "diag_ke_hmix", "diag_ke_vmix", "diag_ke_press", "diag_pe", "diag_tracer_adv", "diag_tracer_hdiff",
            "diag_tracer_vdiff", "diag_tracer_source", "diag_tracer_roff_vsf", "diag_tracer_exchcirc", "diag_transport", "diag_velocity"]
CFL_NAMES = ("advu", "advv", "advw", "advt", "hdifft", "hdiffu", "vdifft", "vdiffu")
U53 = 2.0 ** -53


def blocks(m):
    """get_block of every local block, in local (= block-id) order"""
    return [m.get_block(b) for b in m.local_block_ids()]


def grid(m, pbc=False):
    km = m.km
    g = {n: m.get(n) for n in ("TAREA", "UAREA", "HU", "TAREA_R", "DXU", "DYU", "DXUR", "DYUR", "DXTR", "DYTR")}
    g["KMT"], g["KMU"] = m.geti("KMT"), m.geti("KMU")
    g["RCALCT"], g["RCALCU"] = (g["KMT"] >= 1).astype(np.float64), (g["KMU"] >= 1).astype(np.float64)
    dz = aniso_ref.vertical_dz(km)
    k = np.arange(1, km + 1)[None, :, None, None]
    shape = (m.nblocks, km, m.nyb, m.nxb)
    DZT = np.broadcast_to(dz[1:][None, :, None, None], shape).copy()
    DZU = DZT.copy()
    if pbc:                                      # grid.F90:926-1016: the bottom cell's own thickness at k = KMT / KMU
        DZT = np.where(k == g["KMT"][:, None], m.get("DZBC")[:, None], DZT)
        DZU = np.where(k == g["KMU"][:, None], m.get("DZUB")[:, None], DZU)
    g.update(dz=dz, DZT=DZT, DZU=DZU, k=k, pbc=pbc, P=physical(m))
    g["TFACT"] = g["TAREA"] * g["RCALCT"]
    g["UFACT"] = g["UAREA"] * g["RCALCU"]        # (no tripole grid in the tests: the top row is not halved)
    return g


# ---- global sums -------------------------------------------------------------------------------------------------------------
def read_pre(m):
    """the sources of diag_global_preupdate, read before pop_step_tail (its halo updates and PGUESS change no physical cell of them)"""
    mix = 0 if m.dim("leapfrogts") else 1
    s = dict(U=m.get("UVEL", 1), V=m.get("VVEL", 1), SMF1=m.get("SMF", n=0), SMF2=m.get("SMF", n=1), UB=m.get("UBTROP", 1), VB=m.get("VBTROP", 1),
             GX=m.get("GRADPX", 1), GY=m.get("GRADPY", 1), DH=m.get("DH"), DHU=m.get("DHU"), PSC=m.get("PSURF", 1), PSN=m.get("PSURF", 2),
             PSM=m.get("PSURF", mix), TN=[m.get("TRACER", 2, n) for n in range(m.nt)], TO=[m.get("TRACER", 0, n) for n in range(m.nt)])
    s["c2dtt"] = (2.0 if m.dim("leapfrogts") else 1.0) * m.scalar("dtt")
    return s


def read_after(m):
    """the sources of diag_global_afterupdate, read after pop_step_tail"""
    return dict(U=m.get("UVEL", 1), V=m.get("VVEL", 1), PS=m.get("PSURF", 1), T=[m.get("TRACER", 1, n) for n in range(m.nt)],
                TFW=[m.get("TFW", n=n) for n in range(m.nt)])


def pre_terms(g, s):
    """name -> array of terms over (block, [level,] j, i), already divided by nothing: the quotient comes last"""
    UF, TF, TAREA = g["UFACT"], g["TFACT"], g["TAREA"]
    U1, V1 = s["U"][:, 0], s["V"][:, 0]
    t = {"diag_ws": (U1 * s["SMF1"] + V1 * s["SMF2"]) * UF,                                   # :1259
         "diag_press_free": -(s["UB"] * s["GX"] + s["VB"] * s["GY"]) * g["HU"] * UF,          # :1284-1288
         "diag_ke_free": 0.5 * (U1 * U1 + V1 * V1) * s["DHU"] * UF,                           # :1292-1294
         "diag_ke_psfc": s["PSC"] * s["DH"] * TF}                                             # :1298
    wet = g["k"] <= g["KMT"][:, None]
    dz1 = g["dz"][1]
    for n in range(len(s["TN"])):                # :1326-1357
        W = g["DZT"] * TAREA[:, None] * (s["TN"][n] - s["TO"][n])
        W[:, 0] = TAREA * ((dz1 + s["PSN"] / GRAV) * s["TN"][n][:, 0] - (dz1 + s["PSM"] / GRAV) * s["TO"][n][:, 0])
        W = np.where(wet, W, 0.0)
        t["dtracer_avg", n] = W
        t["dtracer_abs", n] = np.abs(W)
    return t


def after_terms(g, s):
    UF, TF, TAREA = g["UFACT"], g["TFACT"], g["TAREA"]
    t = {"diag_sealevel": s["PS"] / GRAV * TF}                                                # :1637
    t["diag_ke"] = np.where(g["KMU"][:, None] >= g["k"], 0.5 * (s["U"] * s["U"] + s["V"] * s["V"]) * UF[:, None] * g["DZU"], 0.0)   # :1643-1659
    wet = g["KMT"][:, None] >= g["k"]
    dz1 = g["dz"][1]
    for n in range(len(s["T"])):                 # :1663-1692
        W = s["T"][n] * TAREA[:, None] * g["DZT"]
        W[:, 0] = s["T"][n][:, 0] * TAREA * (1.0 + s["PS"] / (dz1 * GRAV)) * dz1
        t["avg_tracer", n] = np.where(wet, W, 0.0)
        t["sfc_tracer_flux", n] = s["TFW"][n] * TF                                            # :1696-1703
    return t


def exact(terms, P):
    """(exact sum, sum of |term|, number of non-zero terms) over the physical cells"""
    a = terms[P] if terms.ndim == 3 else terms.transpose(0, 2, 3, 1)[P]
    a = a.ravel()
    return math.fsum(a), math.fsum(np.abs(a)), int(np.count_nonzero(a))


# ---- CFL numbers -------------------------------------------------------------------------------------------------------------
def read_cfl(m):
    """after pop_baroclinic_driver: the velocities advt saw, DH of pop_dhdt, the coefficients of this step's horizontal mixing"""
    s = dict(U=m.get("UVEL", 1), V=m.get("VVEL", 1), DH=m.get("DH"))
    cfg = m.cfg
    if cfg.hmix_tracer == 3:
        s["KI"] = [m.get("KAPPA_ISOP", n=0), m.get("KAPPA_ISOP", n=1)]
    if cfg.hmix_momentum == 3 and getattr(cfg, "lvariable_hmix_aniso", 0):
        s["F_PARA"] = m.get("F_PARA")
    if cfg.lvariable_hmix:
        d4t, d4u = cfg.hmix_tracer == 4, cfg.hmix_momentum == 4
        if cfg.hmix_tracer in (2, 4):
            s["AHF"] = m.get("D4AHF" if d4t else "AHF")
        if cfg.hmix_momentum in (2, 4):
            s["AMF"] = m.get("D4AMF" if d4u else "AMF")
    return s


def _sh(A, di, dj):
    """A(i+di, j+dj) on the cells that have such a neighbour inside the block, 0 elsewhere (never a physical cell here)"""
    out = np.zeros_like(A)
    ny, nx = A.shape[-2:]
    js, jd = (slice(0, ny + dj), slice(-dj, ny)) if dj < 0 else (slice(dj, ny), slice(0, ny - dj))
    is_, id_ = (slice(0, nx + di), slice(-di, nx)) if di < 0 else (slice(di, nx), slice(0, nx - di))
    out[..., jd, id_] = A[..., js, is_]
    return out


def cfl_fields(m, g, s):
    """name -> (candidate field (nblocks, km, ny, nx), start value of the block scan, factor applied to the block maximum)"""
    cfg, km, k = m.cfg, m.km, g["k"]
    dt, dtu = m.scalar("dtt"), m.scalar("dtu")              # dt(k) = dtt at every level (no dttxcel)
    U, V = s["U"], s["V"]
    DYU, DXU, TR = g["DYU"][:, None], g["DXU"][:, None], g["TAREA_R"][:, None]
    fu, fv = U * DYU, V * DXU
    if g["pbc"]:
        fu, fv = fu * g["DZU"], fv * g["DZU"]
    UTE = 0.5 * (fu + _sh(fu, 0, -1)); UTW = 0.5 * (_sh(fu, -1, 0) + _sh(fu, -1, -1))       # advection.F90:2045-2079
    VTN = 0.5 * (fv + _sh(fv, -1, 0)); VTS = 0.5 * (_sh(fv, 0, -1) + _sh(fv, -1, -1))
    WTK = np.zeros_like(U); WTKB = np.zeros_like(U)
    w = s["DH"].copy()                                       # WTK at the top of level 1
    KMT = g["KMT"]
    for kk in range(1, km + 1):
        WTK[:, kk - 1] = w
        if kk < km:
            FC = (VTN[:, kk - 1] - VTS[:, kk - 1] + UTE[:, kk - 1] - UTW[:, kk - 1]) * g["TAREA_R"]
            w = np.where(kk < KMT, w + FC if g["pbc"] else w + g["dz"][kk] * FC, 0.0)       # :2101-2114
        else:
            w = np.zeros_like(w)
        WTKB[:, kk - 1] = w
    if g["pbc"]:                                             # diagnostics.F90:2315-2333
        E = np.abs(UTE * TR / g["DZU"]) * dt; W = np.abs(UTW * TR / g["DZU"]) * dt
        N = np.abs(VTN * TR / g["DZU"]) * dt; S = np.abs(VTS * TR / g["DZU"]) * dt
        T = np.abs(WTK / g["DZT"]) * dt; B = np.abs(WTKB / g["DZT"]) * dt
    else:
        dzk = g["dz"][1:][None, :, None, None]
        E = np.abs(UTE * TR) * dt; W = np.abs(UTW * TR) * dt; N = np.abs(VTN * TR) * dt; S = np.abs(VTS * TR) * dt
        T = np.abs(WTK / dzk) * dt; B = np.abs(WTKB / dzk) * dt
    TOT = 0.5 * (E + W + N + S + T + B)
    # a cell's two candidates are scanned one after the other with a strict >: the cell counts with the larger
    f = {"advu": (np.maximum(E, W), -1.0, None), "advv": (np.maximum(N, S), -1.0, None), "advw": (np.maximum(T, B), -1.0, None),
         "advt": (TOT, -1.0, None)}
    mt = (g["DXTR"] * g["DXTR"] + g["DYTR"] * g["DYTR"])[:, None]
    mu = (g["DXUR"] * g["DXUR"] + g["DYUR"] * g["DYUR"])[:, None]
    wet_t, wet_u = g["KMT"][:, None] > k, g["KMU"][:, None] > k
    ones = np.ones_like(U)
    if cfg.hmix_tracer == 3:                                 # hmix_gm.F90:2164-2169
        ht = 4.0 * (0.5 * (s["KI"][0] + s["KI"][1])) * mt
    elif cfg.hmix_tracer == 4:                               # hmix_del4.F90:1090-1099
        ht = (-16.0 * cfg.ah * s["AHF"][:, None] if "AHF" in s else -16.0 * cfg.ah * ones) * (mt * mt)
    else:                                                    # hmix_del2.F90:1127-1136
        ht = (4.0 * cfg.ah * s["AHF"][:, None] if "AHF" in s else 4.0 * cfg.ah * ones) * mt
    f["hdifft"] = (np.abs(np.where(wet_t, ht, 0.0)), 0.0, dt)
    hu = None
    if cfg.hmix_momentum == 3:                               # hmix_aniso.F90:1043-1055: not formed with lsmag_aniso
        if not cfg.lsmag_aniso:
            hu = (4.0 * s["F_PARA"] if "F_PARA" in s else 4.0 * cfg.visc_para * ones) * mu
    elif cfg.hmix_momentum == 4:                             # hmix_del4.F90:866-875
        hu = (-16.0 * cfg.am * s["AMF"][:, None] if "AMF" in s else -16.0 * cfg.am * ones) * (mu * mu)
    else:                                                    # hmix_del2.F90:946-955
        hu = (4.0 * cfg.am * s["AMF"][:, None] if "AMF" in s else 4.0 * cfg.am * ones) * mu
    f["hdiffu"] = (np.abs(np.where(wet_u, hu, 0.0)) if hu is not None else np.zeros_like(U), 0.0, dtu)
    return f


def cfl_check(m, g, fields):
    """name -> dict(value_k, ij_k, value, ijk, unique_k): cfl_advect / cfl_hdiff per block, then cfl_check"""
    km, B = m.km, blocks(m)
    out = {}
    for name in CFL_NAMES:
        vk, ijk_k, uniq = np.zeros(km), np.zeros((km, 2), dtype=np.int32), np.ones(km, dtype=bool)
        if name in fields:
            F, start, factor = fields[name]
            for kk in range(km):
                bval, badd = [], []
                for lb, blk in enumerate(B):
                    sub = F[lb, kk, blk["jb"] - 1:blk["je"], blk["ib"] - 1:blk["ie"]]
                    best, add = start, (0, 0)
                    p = int(np.argmax(sub))                  # the first cell in (j, i) order that holds the largest
                    j, i = divmod(p, sub.shape[1])
                    if sub[j, i] > best:
                        best, add = sub[j, i], (blk["i_glob"][blk["ib"] - 1 + i], blk["j_glob"][blk["jb"] - 1 + j])
                    bval.append(best * factor if factor is not None else best)
                    badd.append(add)
                w = int(np.argmax(bval))                     # maxloc: the first block
                vk[kk], ijk_k[kk] = bval[w], badd[w]
                phys = F[:, kk][g["P"]]
                uniq[kk] = np.count_nonzero(phys == phys.max()) == 1
        value, ijk = -1.0, (0, 0, 0)
        for kk in range(km):                                 # :3081-3144
            if vk[kk] > value:
                value, ijk = vk[kk], (int(ijk_k[kk, 0]), int(ijk_k[kk, 1]), kk + 1)
        out[name] = dict(value_k=vk, ij_k=ijk_k, value=value, ijk=ijk, unique_k=uniq)
    return out
