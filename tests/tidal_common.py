"""Shared pieces of the tidal-mixing tests and of whoever else needs an energy flux or the noisy state: the multi-rank workers
tests/mr_gpu_tidal.py and tests/mr_gpu_bckgrnd.py, the background, tavg, land and passive tests, profiles/bckgrnd_ab.py."""
import numpy as np

import tidal_ref
from popcfg import synthetic_grid
from submeso_common import field

KPP = dict(vmix_choice=3, bckgrnd_vdc1=0.16)
NOISY = (2.0, 0.3, 0.2)
# three boxes: plain, wrapping around 360 degrees (it overwrites part of the first), and one with klevels = 2
BOXES = [dict(TLATmin=-30.0, TLATmax=30.0, TLONmin=20.0, TLONmax=100.0, min_value=20.0, klevels=6),
         dict(TLATmin=-60.0, TLATmax=-20.0, TLONmin=300.0, TLONmax=40.0, min_value=35.0, klevels=6),
         dict(TLATmin=30.0, TLATmax=70.0, TLONmin=150.0, TLONmax=205.0, min_value=50.0, klevels=2)]


def stepped_grid(cfg):
    """popcfg.synthetic_grid with the KMT record overwritten: land stays, the ocean takes 3, 4, 5 and km in turn"""
    g = synthetic_grid(cfg)
    ny, nx = g["KMT"].shape
    ii, jj = np.arange(nx)[None, :], np.arange(ny)[:, None]
    pick = np.array([3, 4, 5, cfg.km], dtype=np.int32)[(ii + 2 * jj) % 4]
    g["KMT"] = np.ascontiguousarray(np.where(g["KMT"] > 0, pick, 0).astype(np.int32))
    return g


def smooth_flux(m, amp, seed=5):
    """energy flux [W/m^2] of the local blocks: a smooth function of the global indices times a seeded factor in [0.5, 1.5]; the ghost
    cells are left to the halo update"""
    nx, ny = m.cfg.nx_global, m.cfg.ny_global
    fac = 0.5 + np.random.default_rng(seed).random((ny + 1, nx + 1))
    F = np.zeros((m.nblocks, m.nyb, m.nxb))
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        i = np.clip(np.asarray(b["i_glob"]), 0, nx)[None, :]
        j = np.clip(np.asarray(b["j_glob"]), 0, ny)[:, None]
        F[lb] = amp * (1.0 + 0.5 * np.cos(2.0 * np.pi * i / nx) * np.sin(np.pi * j / ny)) * fac[j, i]
    return F


def noisy_state(m, state=NOISY, vert=0.25):
    """field() of the submeso tests plus a temperature term that changes from level to level: the cell-to-cell variation of field()
    advances by 37.719 = 6 * 2 pi + 0.02 radians per level, so on its own it leaves every interface stably stratified.  With 0.3 K per
    level and +-0.25 K of this term about a fifth of the interfaces are unstable (the tests assert that both signs of N2 occur)."""
    T, S = field(m, *state)
    k = np.arange(1, m.km + 1, dtype=np.float64)[:, None, None]
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        i = np.asarray(b["i_glob"], dtype=np.float64)[None, None, :]
        j = np.asarray(b["j_glob"], dtype=np.float64)[None, :, None]
        T[lb] += vert * np.sin(1.7 * k + 0.9 * i + 1.3 * j)
    return T, S


def set_state(m, state=NOISY):
    """the tracers at both time levels, ghost cells from the halo update; returns what the model holds"""
    T, S = noisy_state(m, state)
    for tl in (0, 1):
        m.set("TRACER", T, tl, 0); m.set("TRACER", S, tl, 1)
        m.halo_update("TRACER", tl, 0); m.halo_update("TRACER", tl, 1)
    return m.get("TRACER", 1, 0), m.get("TRACER", 1, 1)


def unit_flux(m):
    F = smooth_flux(m, 1.0)
    m.halo_update_host_loc(F)          # what pop_init_tidal_mixing does to its copy of the record
    return F


def amplitude(pkg, m, cfg, F1, T, S):
    """the flux amplitude [W/m^2] of a case, from the restatement alone: TIDAL_DIFF is linear in the flux until it is limited, so with
    the amplitude tidal_mix_max / (median of the unit-flux TIDAL_DIFF over the stably stratified cells of the four levels above
    the bottom) about half of those cells reach the cap and half stay below it"""
    r = tidal_ref.from_model(m, cfg, pkg.tidal_nml(ltidal_max=0, ltidal_stabc=0), F1, T, S)
    lev = np.arange(1, m.km + 1)[None, :, None, None]
    kmt = r["KMT"][:, None]
    sel = (lev < kmt) & (lev >= kmt - 4) & (r["N2"] > 0.0)
    return 100.0 / np.median(r["DIFF"][sel])


def branches(r, phys):
    p3 = np.broadcast_to(phys[:, None], r["N2"].shape)
    return {n: int((b & p3).sum()) for n, b in r["branch"].items()}


# (id, pop_config keywords, tidal_nml keywords, regions, grid: None | 'stepped' | 'synthetic', branches that must be taken on > 20 cells)
CASES = [
    ("default", {}, {}, None, None, ("neg", "cap", "stab")),
    ("stepped-kmt", {}, {}, None, "stepped", ("neg", "cap", "stab")),
    ("no-max", {}, dict(ltidal_max=0), None, None, ("neg", "cap")),
    ("no-stabc", {}, dict(ltidal_stabc=0), None, None, ("neg", "cap", "stab-off")),
    ("regions", dict(stepped_bathymetry=1), {}, BOXES, None, ("neg", "region")),
    ("partial-bottom-cells", dict(partial_bottom_cells=1, stepped_bathymetry=1), {}, None, None, ("neg", "cap", "stab")),
    ("padded-blocks", dict(block_size_x=20, block_size_y=16), {}, None, None, ("neg", "cap", "stab")),
    ("tripole", dict(ns_boundary=2, block_size_x=48, block_size_y=10), {}, None, "synthetic", ("neg", "cap", "stab")),
    ("no-rich", dict(lrich=0), {}, None, None, ("neg", "cap", "stab")),
    ("dbl-diff", dict(ldbl_diff=1), {}, None, None, ("neg", "cap", "stab")),
]
