"""Shared pieces of the anisotropic-viscosity tests: the random velocity state, the restatement fed from a model, the ANGLE grid, the cases."""
import numpy as np

import aniso_ref
from popcfg import synthetic_grid

GX3V7 = dict(aniso_alignment="east", lvariable_hmix_aniso=1, vconst_4=2.0e-8)


def state(m, seed):
    """random U, V (0 below KMU) at time levels old and current, ghost cells from the halo update"""
    rng = np.random.default_rng(seed)
    kmu = m.geti("KMU")
    wet = kmu[:, None] >= np.arange(1, m.km + 1)[None, :, None, None]
    U = np.where(wet, rng.standard_normal((m.nblocks, m.km, m.nyb, m.nxb)), 0.0)
    V = np.where(wet, rng.standard_normal(U.shape), 0.0)
    for tl in (0, 1):
        m.set("UVEL", U, tl); m.set("VVEL", V, tl)
        m.halo_update_loc("UVEL", tl, 0, "NEcorner", "vector"); m.halo_update_loc("VVEL", tl, 0, "NEcorner", "vector")
    return m.get("UVEL", 1), m.get("VVEL", 1)


def reference(m, cfg, U, V):
    f = aniso_ref.geometry(m.get("HTN"), m.get("HTE"), m.get("DXUR"), m.get("DYUR"), m.scalar("dtu"))
    for n in ("UAREA", "ANGLE", "ULAT", "DXU", "DYU"):
        f[n] = m.get(n)
    f["KMU"] = m.geti("KMU")
    if cfg.lsmag_aniso:
        f["DSMIN"], f["F_PERP_SMAG"] = m.get("DSMIN"), m.get("F_PERP_SMAG")
    fpa = fpe = dzu = None
    if cfg.lvariable_hmix_aniso:
        fpa, fpe = m.get("F_PARA"), m.get("F_PERP")
    if cfg.partial_bottom_cells:
        dz = aniso_ref.vertical_dz(m.km)
        kmu, dzub = f["KMU"], m.get("DZUB")
        ks = np.arange(1, m.km + 1)[None, :, None, None]
        dzu = np.where(kmu[:, None] == ks, dzub[:, None], dz[1:][None, :, None, None] + 0.0 * U)
    return aniso_ref.hdiffu(U, V, f, cfg, fpa, fpe, dzu)


def angle_grid(c5):
    g = synthetic_grid(c5)
    nx, ny = c5.nx_global, c5.ny_global
    g["ANGLE"] = 0.4 * np.sin(2.0 * np.pi * np.arange(nx) / nx)[None, :] * np.cos(np.pi * np.arange(ny) / ny)[:, None]
    return g


CASES = [
    ("grid-constant", "tiny", {}, dict(visc_para=2.0e9, visc_perp=0.5e9), False),
    ("east-variable-angle", "tiny", {}, dict(aniso_alignment="east", lvariable_hmix_aniso=1), True),
    ("smag", "tiny", {}, dict(lsmag_aniso=1, c_para=8.0, c_perp=4.0, smag_lat_fact=0.98), False),
    ("smag-variable-east", "tiny", {}, dict(aniso_alignment="east", lsmag_aniso=1, lvariable_hmix_aniso=1, c_para=8.0, c_perp=4.0,
                                            smag_lat_fact=0.98), True),
    ("partial-bottom-cells", "tiny", {"partial_bottom_cells": 1, "stepped_bathymetry": 1}, dict(visc_para=2.0e9, visc_perp=0.5e9), False),
    ("padded-blocks", "tiny", {"block_size_x": 20, "block_size_y": 16}, dict(lvariable_hmix_aniso=1), False),
    ("tripole-east-variable", "tiny", {"ns_boundary": 2, "block_size_x": 48, "block_size_y": 10}, dict(GX3V7), True),
]
