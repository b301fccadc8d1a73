"""Shared pieces of the ice-formation GPU tests (tests/test_gpu_ice.py, tests/mr_gpu_ice.py): a caller's grid whose KMT includes
1 and 2, and a cold start -- an upper ocean at the freezing point under strong surface cooling, formed cell by cell from the model's own
initial temperature with arithmetic only, so that every decomposition of a domain holds the same bits in the same cells."""
import numpy as np

from popcfg import synthetic_dzbc, synthetic_grid

COOLING = -0.02          # STF(1) [deg C cm/s]: about -800 W/m^2, 0.03 degrees per hour off a 25 m layer


def ice_grid(cfg, pbc=False):
    """popcfg.synthetic_grid with every fifth ocean column 1 level deep and every fifth 2 levels deep (the rest 3 .. km, land 0), so that
    the k <= KMT masks of ice_formation matter with kmxice = 3.  TEST DATA."""
    g = synthetic_grid(cfg)
    k = g["KMT"]
    ii, jj = np.arange(cfg.nx_global)[None, :], np.arange(cfg.ny_global)[:, None]
    sel = (ii + 2 * jj) % 5
    k = np.where((k > 0) & (sel == 0), 1, np.where((k > 0) & (sel == 1), 2, k)).astype(np.int32)
    g["KMT"] = np.ascontiguousarray(k)
    if pbc:
        g["DZBC"] = synthetic_dzbc(cfg, g["KMT"])
    return g


def wet_mask(m):
    return np.arange(1, m.km + 1)[None, :, None, None] <= m.geti("KMT")[:, None]


def cold_start(m, surface=-1.95):
    """T = surface + 0.04 frac(37 T0) + 0.01 (k - 1) on the ocean cells of the three time levels (T0: the model's initial temperature),
    the density that belongs to it, and the cooling COOLING on every ocean column.  The surface level starts below every freezing
    point the library forms, so ice forms from the first step on."""
    wet = wet_mask(m)
    T0 = m.get("TRACER", 1, 0)
    x = T0 * 37.0
    k = np.arange(m.km, dtype=np.float64)[None, :, None, None]
    T = np.where(wet, surface + 0.04 * (x - np.floor(x)) + 0.01 * k, 0.0)
    S = m.get("TRACER", 1, 1)
    RHO = np.stack([m.state(kk + 1, T[:, kk], S[:, kk]) for kk in range(m.km)], axis=1)
    for tl in (0, 1, 2):
        m.set("TRACER", T, tl=tl, n=0)
    for tl in (0, 1):
        m.set("RHO", RHO, tl=tl)
    m.set("STF", np.where(m.geti("KMT") > 0, COOLING, 0.0), n=0)
    return T
