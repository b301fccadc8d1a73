"""NumPy restatement of the time-averaged output (source/tavg.F90) and of the accumulate_tavg_field call sites the library serves,
written from the reference, not from the kernels: methods (tavg.F90:3202-3240), weights (tavg_set_flag :1549-1557), reset values
(:3746-3840), normalisation (:3888-3969) and the expression of every entry in the reference's order of operations, squares as x*x.

Sources come from PopModel.get / geti / scalar at the place in the phase sequence where the reference reads them:
  forcing  before dhdt                       forcing.F90:502-577, surface_hgt.F90:294-313
  state    before baroclinic_driver          baroclinic.F90:772-806
  tracer   the same; with the Robert filter after step_tail, from the levels the filter left (step_mod.F90:1290-1298)
  vmix     after baroclinic_driver           (nothing later in the driver rewrites them, except VDC under Gent-McWilliams)
  hmix     after baroclinic_driver
  btrop    after barotropic_driver           barotropic.F90:687-693
"""
import numpy as np

import aniso_ref

GRAV = 980.6                                     # pop_constants.F90:235
BIGNUM = 1.0e30                                  # tavg.F90
HFLUX_FACTOR = 1000.0 / ((4.1 / 3.996) * 3.996e7)   # pop_constants.F90:336 with the code defaults of rho_sw, cp_sw
SALINITY_FACTOR = -34.7 * 1.0e-4                 # pop_constants.F90:364-365
SECONDS_IN_YEAR, MPERCM = 86400.0 * 365.0, 0.01
MAX_STREAMS = 9                                  # tavg.F90:83
SITES = ("forcing", "state", "tracer", "vmix", "hmix", "btrop", "qflux")
# entries whose value is formed with a division: equal to rounding, every other entry bit for bit
DIVISION = ("SSH", "SSH_2", "SSH2", "H3", "SHF", "SHF_QSW", "SHF_QSW_2", "SFWF", "QFLUX")
LEFT_OUT = ("UET", "VNT", "WTT", "WVEL", "PD", "ADVT", "ADVU", "GRADX", "HDIFFU", "VDIFFU", "UDP", "HDIFT", "DIA_IMPVF_TEMP", "RESID_T",
            "RESID_S", "TEMP_27", "BSF")


def table(km, passive=(), fw_as_salt=False, hflux_factor=HFLUX_FACTOR, salinity_factor=SALINITY_FACTOR):
    """name -> (site, ndims, method, kmax, f(src) -> value); src maps a source name to its array.  A 3-D value has km levels; a 2-D
    entry with kmax > 1 (or from a 3-D value) is fed level by level, k = 1 .. kmax, into one 2-D buffer.  passive: the names of
    the tracers n = 3 .. nt."""
    t = {}

    def e(name, site, ndims, f, method="avg", kmax=None):
        t[name] = (site, ndims, method, kmax if kmax is not None else (km if ndims == 3 else 1), f)

    ocean = lambda s, v: np.where(s["KMT"] > 0, v, 0.0)
    e("SHF", "forcing", 2, lambda s: ocean(s, (s["STF1"] + s["SHF_QSW"]) / hflux_factor))
    for n in ("SHF_QSW", "SHF_QSW_2"):
        e(n, "forcing", 2, lambda s: ocean(s, s["SHF_QSW"] / hflux_factor))
    if fw_as_salt:
        e("SFWF", "forcing", 2, lambda s: ocean(s, s["STF2"] / salinity_factor))
    else:
        e("SFWF", "forcing", 2, lambda s: ocean(s, s["FW"] * SECONDS_IN_YEAR * MPERCM))
    e("TAUX", "forcing", 2, lambda s: s["SMF1"]); e("TAUX2", "forcing", 2, lambda s: s["SMF1"] * s["SMF1"])
    e("TAUY", "forcing", 2, lambda s: s["SMF2"]); e("TAUY2", "forcing", 2, lambda s: s["SMF2"] * s["SMF2"])
    e("FW", "forcing", 2, lambda s: s["FW"])
    e("SSH", "forcing", 2, lambda s: s["PSURF"] / GRAV); e("SSH_2", "forcing", 2, lambda s: s["PSURF"] / GRAV)
    e("SSH2", "forcing", 2, lambda s: (s["PSURF"] / GRAV) * (s["PSURF"] / GRAV))
    e("H3", "forcing", 2, lambda s: (s["GRADPX"] / GRAV) * (s["GRADPX"] / GRAV) + (s["GRADPY"] / GRAV) * (s["GRADPY"] / GRAV))
    for n, src in (("UVEL", "U"), ("UVEL_2", "U"), ("VVEL", "V"), ("VVEL_2", "V")):
        e(n, "state", 3, lambda s, src=src: s[src])
    e("UVEL2", "state", 3, lambda s: s["U"] * s["U"]); e("VVEL2", "state", 3, lambda s: s["V"] * s["V"])
    e("KE", "state", 3, lambda s: 0.5 * (s["U"] * s["U"] + s["V"] * s["V"]))
    e("UV", "state", 3, lambda s: s["U"] * s["V"])
    e("U1_8", "state", 2, lambda s: s["U"], kmax=8); e("V1_8", "state", 2, lambda s: s["V"], kmax=8)   # define_tavg_field(..., 2): one 2-D buffer, k <= 8
    e("U1_1", "state", 2, lambda s: s["U"][:, 0]); e("V1_1", "state", 2, lambda s: s["V"][:, 0])
    for n, src in (("TEMP", "T"), ("TEMP_2", "T"), ("SALT", "S"), ("SALT_2", "S"), ("RHO", "RHO")):
        e(n, "tracer", 3, lambda s, src=src: s[src])
    e("TEMP_MAX", "tracer", 3, lambda s: s["T"], "max"); e("TEMP_MIN", "tracer", 3, lambda s: s["T"], "min")
    e("SALT_MAX", "tracer", 3, lambda s: s["S"], "max"); e("SALT_MIN", "tracer", 3, lambda s: s["S"], "min")
    e("TEMP2", "tracer", 3, lambda s: s["T"] * s["T"]); e("SALT2", "tracer", 3, lambda s: s["S"] * s["S"])
    e("ST", "tracer", 3, lambda s: s["T"] * s["S"])
    e("T1_8", "tracer", 2, lambda s: s["T"], kmax=8); e("S1_8", "tracer", 2, lambda s: s["S"], kmax=8)
    e("SST", "tracer", 2, lambda s: s["T"][:, 0]); e("SST2", "tracer", 2, lambda s: s["T"][:, 0] * s["T"][:, 0])
    e("SSS", "tracer", 2, lambda s: s["S"][:, 0]); e("SSS2", "tracer", 2, lambda s: s["S"][:, 0] * s["S"][:, 0])
    e("dTEMP_POS_3D", "tracer", 3, lambda s: np.maximum(s["T"] - s["TOLD"], 0.0))
    e("dTEMP_NEG_3D", "tracer", 3, lambda s: np.minimum(s["T"] - s["TOLD"], 0.0))
    e("dTEMP_POS_2D", "tracer", 2, lambda s: np.maximum(s["T"] - s["TOLD"], 0.0), kmax=km)
    e("dTEMP_NEG_2D", "tracer", 2, lambda s: np.minimum(s["T"] - s["TOLD"], 0.0), kmax=km)

    def rho_vint(s):      # baroclinic.F90:2392-2414: varthick surface layer at k = 1, DZT below (partial bottom cells or not)
        th = s["DZT"].copy()
        th[:, 0] = s["DZT"][:, 0] * 0.0 + (s["dz1"] + s["PSURF"] / GRAV)
        k = np.arange(1, km + 1)[None, :, None, None]
        return np.where(k <= s["KMT"][:, None], s["RHO"] * th, 0.0)
    e("RHO_VINT", "tracer", 2, rho_vint, kmax=km)
    for i, nm in enumerate(passive):
        key = "TR%d" % (i + 2)
        e(nm, "tracer", 3, lambda s, key=key: s[key]); e(nm + "_2", "tracer", 3, lambda s, key=key: s[key])
        e(nm + "_SQR", "tracer", 3, lambda s, key=key: s[key] * s[key])
        e(nm + "_SURF", "tracer", 2, lambda s, key=key: s[key][:, 0])
    e("VDC_T", "vmix", 3, lambda s: s["VDC_T"]); e("VDC_S", "vmix", 3, lambda s: s["VDC_S"]); e("VVC", "vmix", 3, lambda s: s["VVC"])
    e("KPP_SRC_TEMP", "vmix", 3, lambda s: s["KPP_SRC1"]); e("KPP_SRC_SALT", "vmix", 3, lambda s: s["KPP_SRC2"])
    e("HBLT", "vmix", 2, lambda s: s["HBLT"]); e("XBLT", "vmix", 2, lambda s: s["HBLT"], "max"); e("TBLT", "vmix", 2, lambda s: s["HBLT"], "min")
    for n, meth in (("HMXL", "avg"), ("HMXL_2", "avg"), ("XMXL", "max"), ("XMXL_2", "max"), ("TMXL", "min")):
        e(n, "vmix", 2, lambda s: s["HMXL"], meth)
    for n, meth in (("HMXL_DR", "avg"), ("HMXL_DR_2", "avg"), ("XMXL_DR", "max"), ("TMXL_DR", "min")):
        e(n, "vmix", 2, lambda s: s["HMXL_DR"], meth)
    e("HMXL_DR2", "vmix", 2, lambda s: s["HMXL_DR"] * s["HMXL_DR"])
    e("KVMIX", "vmix", 3, lambda s: s["KVMIX"]); e("KVMIX_M", "vmix", 3, lambda s: s["KVMIX_M"])
    for n in ("UISOP", "VISOP", "WISOP", "USUBM", "VSUBM", "WSUBM"):
        e(n, "hmix", 3, lambda s, n=n: s[n])
    e("SU", "btrop", 2, lambda s: s["HU"] * s["UBTROP"]); e("SV", "btrop", 2, lambda s: s["HU"] * s["VBTROP"])
    e("QFLUX", "qflux", 2, lambda s: s["QFLUX"], "qflux")
    return t


def reset_value(method):
    return BIGNUM if method == "min" else -BIGNUM if method == "max" else 0.0


def accumulate(buf, value, method, dtavg, const=None):
    """accumulate_tavg_field_2d_3d on whole arrays; returns the new buffer"""
    if method == "avg":
        return buf + dtavg * value
    if method == "qflux":
        return buf + const * np.maximum(0.0, value)
    if method == "min":
        return np.where(value < buf, value, buf)
    if method == "max":
        return np.where(value > buf, value, buf)
    if method == "constant":
        return value.copy()
    raise KeyError(method)


def normalise(buf, method, tavg_sum, tavg_sum_qflux=0.0):
    """tavg_norm_field_all: a copy; ZeroDivisionError where the reference has no defined result"""
    if method == "avg":
        if tavg_sum == 0.0:
            raise ZeroDivisionError("tavg_sum is 0")
        return buf * (1.0 / tavg_sum)
    if method == "qflux":
        if tavg_sum_qflux == 0.0:
            raise ZeroDivisionError("tavg_sum_qflux is 0")
        return buf * (1.0 / tavg_sum_qflux)
    return buf.copy()


def read_sources(m, site, robert_tail=False, pbc=False):
    """the sources of one site from the model, as the site finds them"""
    km = m.km
    s = {"KMT": m.geti("KMT")}
    if site == "forcing":
        s.update(STF1=m.get("STF", n=0), STF2=m.get("STF", n=1), SHF_QSW=m.get("SHF_QSW"), FW=m.get("FW"), SMF1=m.get("SMF", n=0),
                 SMF2=m.get("SMF", n=1), PSURF=m.get("PSURF", 1), GRADPX=m.get("GRADPX", 1), GRADPY=m.get("GRADPY", 1))
    elif site == "state":
        s.update(U=m.get("UVEL", 1), V=m.get("VVEL", 1))
    elif site == "tracer":
        cur, old = (0, 2) if robert_tail else (1, 0)       # step_rf has rotated: its curtime is oldtime now, its oldtime newtime
        s.update(T=m.get("TRACER", cur, 0), S=m.get("TRACER", cur, 1), TOLD=m.get("TRACER", old, 0), RHO=m.get("RHO", cur), PSURF=m.get("PSURF", cur))
        for n in range(2, m.nt):
            s["TR%d" % n] = m.get("TRACER", cur, n)
        dz = aniso_ref.vertical_dz(km)
        k = np.arange(1, km + 1)[None, :, None, None]
        DZT = np.broadcast_to(dz[1:][None, :, None, None], s["T"].shape).copy()
        if pbc:
            DZT = np.where(k == s["KMT"][:, None], m.get("DZBC")[:, None], DZT)
        s["DZT"], s["dz1"] = DZT, dz[1]
    elif site == "vmix":
        vdc = m.get("VDC", n=0)
        s.update(VDC_T=vdc[:, 1:km + 1], VDC_S=m.get("VDC", n=1 if m.cfg.vmix_choice == 3 else 0)[:, 1:km + 1], VVC=m.get("VVC"))
        if m.cfg.vmix_choice == 3:
            s.update(HBLT=m.get("HBLT"), KPP_SRC1=m.get("KPP_SRC", n=0), KPP_SRC2=m.get("KPP_SRC", n=1))
            if m.cfg.kpp_ml_diagnostics:
                s.update(HMXL=m.get("HMXL"), HMXL_DR=m.get("HMXL_DR"))
        for n in ("KVMIX", "KVMIX_M"):
            try:
                s[n] = m.get(n)
            except Exception:
                pass
    elif site == "hmix":
        for n in ("UISOP", "VISOP", "WISOP", "USUBM", "VSUBM", "WSUBM"):
            try:
                s[n] = m.get(n)
            except Exception:
                pass
    elif site == "btrop":
        s.update(HU=m.get("HU"), UBTROP=m.get("UBTROP", 1), VBTROP=m.get("VBTROP", 1))
    elif site == "qflux":
        s.update(QFLUX=m.get("QFLUX"))
    return s


class TavgRef:
    """the module state of tavg.F90 for a request list {name: stream}"""

    def __init__(self, m, requests, pbc=False, **table_kw):
        self.m, self.pbc = m, pbc
        self.tab = table(m.km, **table_kw)
        self.req = dict(requests)
        self.on = {ns: True for ns in set(self.req.values())}
        self.sum = {ns: 0.0 for ns in range(1, MAX_STREAMS + 1)}
        self.sum_qflux = dict(self.sum)
        self.dtavg = 0.0
        self.buf = {}
        shape2 = (m.nblocks, m.nyb, m.nxb)
        for name in self.req:
            site, ndims, method, kmax, f = self.tab[name]
            self.buf[name] = np.full(shape2 if ndims == 2 else (m.nblocks, kmax, m.nyb, m.nxb), reset_value(method))

    def set_flag(self, avg_ts):
        """tavg_set_flag, right after time_manager"""
        dtt = self.m.scalar("dtt")
        self.dtavg = 0.5 * dtt if avg_ts else dtt
        for ns, on in self.on.items():
            if on:
                self.sum[ns] = self.sum[ns] + self.dtavg

    def reset(self, ns):
        for name, s in self.req.items():
            if s == ns:
                self.buf[name][...] = reset_value(self.tab[name][2])
        self.sum[ns] = 0.0
        if any(s == ns and self.tab[n][2] == "qflux" for n, s in self.req.items()):
            self.sum_qflux[ns] = 0.0

    def site(self, site, src=None, const=None, **kw):
        """one site with the current dtavg; src: sources read earlier (default: now)"""
        names = [n for n, ns in self.req.items() if self.tab[n][0] == site and self.on[ns]]
        if not names:
            return
        s = src if src is not None else read_sources(self.m, site, pbc=self.pbc, **kw)
        for name in names:
            _, ndims, method, kmax, f = self.tab[name]
            v = f(s)
            if ndims == 2 and v.ndim == 4:             # one 2-D buffer fed once per level, k = 1 .. kmax in that order
                for k in range(kmax):
                    self.buf[name] = accumulate(self.buf[name], v[:, k], method, self.dtavg, const)
            else:
                self.buf[name] = accumulate(self.buf[name], v, method, self.dtavg, const)

    def normalised(self, name):
        ns = self.req[name]
        return normalise(self.buf[name], self.tab[name][2], self.sum[ns], self.sum_qflux[ns])
