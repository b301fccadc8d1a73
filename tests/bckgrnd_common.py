"""Shared pieces of the tests of the latitude-varying KPP background: the grid on which every branch of the field holds ocean, the surface
fluxes, the restated field of a model, the oracle fed with a state, the fields and cases of the comparison with the oracle."""
import numpy as np

import bckgrnd_ref
from bckgrnd_ref import CESM, RADIAN
from orclib import AsModel
from tidal_common import KPP

STEPPED = dict(KPP, stepped_bathymetry=1)
FIELDS = (("VDC0", ("VDC", 1, 0)), ("VDC1", ("VDC", 1, 1)), ("VVC", ("VVC",)), ("HBLT", ("HBLT",)), ("SRC0", ("KPP_SRC", 1, 0)),
          ("SRC1", ("KPP_SRC", 1, 1)))
ORACLE_CASES = [("tiny", {}, False), ("banda-grid", {}, True), ("dbl-diff", dict(ldbl_diff=1), False), ("no-rich", dict(lrich=0), False)]


def banda_arctic_grid(cfg, lat_south=-42.0, lat_north=78.0):
    """Global grid records as popcfg.synthetic_grid forms them, for a lat-lon grid from lat_south to lat_north with a KMT of its own.
    On 48 x 40 the rows are 3 degrees apart and the T points lie near -40.5, ..., -7.5, -4.5, -1.5, ..., 70.5, 73.5, 76.5 degrees and
    3.75, 11.25, ... degrees east: one row inside each Banda Sea box (4 or 5 columns each) and three rows in the Arctic cap.  Land
    (a strip at 210-250 E north of 35 S) stays away from the boxes and from the northern edge's ocean; the ocean takes 3, 5, km - 2
    and km levels in turn.  TEST DATA: the code under test only ever sees arrays."""
    nx, ny, km = cfg.nx_global, cfg.ny_global, cfg.km
    radius = 6370.0e5
    i = np.arange(1, nx + 1, dtype=np.float64)[None, :]
    j = np.arange(1, ny + 1, dtype=np.float64)[:, None]
    dlat, dlon = (lat_north - lat_south) / ny, 360.0 / nx
    ulat = (lat_south + j * dlat) / RADIAN + 0.0 * i
    lon = i * dlon + 0.0 * j
    ulon = np.where(lon > 180.0, lon - 360.0, lon) / RADIAN
    east = 1.0 + 0.04 * np.cos(2.0 * np.pi * i / nx)
    north = 1.0 + 0.04 * np.cos(2.0 * np.pi * (i - 0.5) / nx)
    cell, cellx = dlat * radius / RADIAN, dlon * radius / RADIAN
    kmt = np.array([3, 5, km - 2, km], dtype=np.int32)[(np.arange(nx)[None, :] + 2 * np.arange(ny)[:, None]) % 4]
    kmt = np.where((ulat * RADIAN > -35.0) & (ulat * RADIAN < 60.0) & (lon > 210.0) & (lon < 250.0), 0, kmt).astype(np.int32)
    g = {"ULAT": ulat, "ULON": ulon, "HTN": cellx * np.cos(ulat) * north, "HTE": cell * east + 0.0 * j,
         "HUS": cellx * np.cos((lat_south + (j - 0.5) * dlat) / RADIAN) * east, "HUW": cell * north + 0.0 * j,
         "ANGLE": np.zeros((ny, nx)), "KMT": kmt}
    return {n: np.ascontiguousarray(a) for n, a in g.items()}


def surface_flux(TLAT):
    """surface tracer fluxes (parity.force_kpp_case): cooling, hence an unstable boundary layer and a non-zero non-local source
    KPP_SRC, in the north; heating in the south"""
    return -3.0e-2 * np.sin(TLAT) - 1.0e-2, 2.0e-6 * np.cos(2.0 * TLAT)


def set_flux(m):
    stf_t, stf_s = surface_flux(m.get("TLAT"))
    m.set("STF", stf_t, n=0); m.set("STF", stf_s, n=1)
    return stf_t, stf_s


def restated(m, cfg, bck=CESM):
    return bckgrnd_ref.field(m.get("TLAT"), m.get("TLON"), cfg.bckgrnd_vdc1, **bck)


def feed_oracle(orc, T, S):
    """the tracers at every time level and the densities that belong to them (on a device model too: tests/test_gpu_tidal.py's _feed)"""
    for tl in (0, 1, 2):
        for n, X in ((0, T), (1, S)):
            orc.f3("TRACER", tl, n)[...] = X
    state = AsModel(orc).state
    R = np.stack([state(k + 1, T[:, k], S[:, k]) for k in range(orc.km)], axis=1)
    for tl in (0, 1):
        orc.f3("RHO", tl)[...] = R
    return R
