"""Shared pieces of the coupled-forcing GPU tests (tests/test_gpu_forcing.py): the cases, the model of a case on a grid whose ANGLE
is not zero, and the restatement fed from a model."""
import math

import numpy as np

import forcing_ref
import ice_ref
from ice_common import cold_start, ice_grid
from popcfg import named_config

# name -> (config keywords, partial bottom cells, pop_ice_nml keywords or None)
FW_ICE = dict(ice_freq_opt="coupled", licecesm2=1, kmxice=3, lfw_as_salt_flx=0, tfreeze_option=1)
SALT_ICE = dict(ice_freq_opt="coupled", licecesm2=1, kmxice=3, lfw_as_salt_flx=1, tfreeze_option=2, lactive_ice=1)
CASES = {
    "fw": (dict(), False, None),                                          # the fresh-water form, no pop_init_ice: tmelt = -1.8
    "fw-ice": (dict(), False, FW_ICE),                                    # ... with ice formation: the *_COMP copies, FW_FREEZE every step
    "fw-active-ice": (dict(), False, dict(FW_ICE, lactive_ice=1, ice_freq_opt="never")),   # tmelt = 0
    "salt": (dict(), False, SALT_ICE),                                    # lfw_as_salt_flx: the virtual salt flux
    "fw-pbc": (dict(partial_bottom_cells=1), True, None),
    "salt-pbc": (dict(partial_bottom_cells=1), True, SALT_ICE),
    "fw-padded": (dict(block_size_x=11, block_size_y=9), False, FW_ICE),  # 15 x 13 cells per block: an odd plane, the 8-byte form
    "salt-padded": (dict(block_size_x=11, block_size_y=9), False, SALT_ICE),
    "salt-nt4": (dict(nt=4), False, SALT_ICE),
    "fw-nt4": (dict(nt=4), False, None),
    "fw-tripole": (dict(ns_boundary=2), False, FW_ICE),
}


def angle_grid(cfg, pbc=False):
    """ice_common.ice_grid with an ANGLE that varies smoothly between -0.9 and 0.9 radians and is symmetric under the tripole fold's
    mirror i -> nx - i (an NE-corner field), so that the rotation mixes the two stress components everywhere.  TEST DATA."""
    g = ice_grid(cfg, pbc=pbc)
    nx, ny = cfg.nx_global, cfg.ny_global
    i = np.arange(1, nx + 1, dtype=np.float64)[None, :]
    j = np.arange(1, ny + 1, dtype=np.float64)[:, None]
    g["ANGLE"] = np.ascontiguousarray(0.9 * np.cos(2.0 * math.pi * i / nx) * np.sin(math.pi * j / ny) + 0.0 * j)
    return g


def make(pkg, case, cold=False, **nml):
    cfgkw, pbc, ice = CASES[case]
    cfg = named_config("tiny", **cfgkw)
    m = pkg.PopModel(cfg, grid=angle_grid(cfg, pbc))
    if ice is not None:
        m.init_ice(**ice)
    m.init_coupled_forcing(**nml)
    if cold:
        cold_start(m)
    return m


def consts_of(case):
    ice = CASES[case][2]
    return forcing_ref.consts(ice_ref.params(**{k: (pkg_opt(k, v)) for k, v in ice.items()}) if ice is not None else None)


def pkg_opt(k, v):
    if k == "ice_freq_opt" and isinstance(v, str):
        return {"never": 0, "coupled": 1}[v]
    return v


def liceform_of(case):
    ice = CASES[case][2]
    return ice is not None and ice["ice_freq_opt"] != "never"


def restate_import(m, case, x2o):
    """the restatement of one pop_set_coupled_forcing on the model's current state -> (imported fields, combined fields)"""
    k = consts_of(case)
    f = forcing_ref.import_fields(m, x2o, k)
    o = forcing_ref.combine(m, f, k, m.get("TRACER", 1, 0)[:, 0], m.get("TRACER", 1, 1)[:, 0], liceform_of(case), nt=m.nt)
    return f, o


def device_fields(m, names):
    """name -> array; 'STF1' = get('STF', n=0), 'TFW_COMP_CPL2' = get('TFW_COMP_CPL', n=1) ..."""
    out = {}
    for n in names:
        if n[-1].isdigit() and n[:-1] in ("STF", "SMF", "SMFT", "TFW", "TFW_COMP_CPL"):
            out[n] = m.get(n[:-1], 1, int(n[-1]) - 1)
        else:
            out[n] = m.get(n)
    return out


def ms_setup(m):
    """A synthetic REGION_MASK on 'tiny' (global (ny, nx) int32) and its region table: open ocean 1, a sector of region 2 east of it, land
    0, and two marginal seas -- number -3 straddling the corner of four blocks (12 x 10 blocks: i 11 .. 14, j 19 .. 22) and number -5
    inside one block -- each with a search centre two cells away and an area of a few cells.  TEST DATA."""
    import forcing_ref
    cfg = m.cfg
    ny, nx = cfg.ny_global, cfg.nx_global
    kmt = forcing_ref.gather_global(m, m.geti("KMT"), (ny, nx))
    R = np.where(kmt > 0, 1, 0).astype(np.int32)
    R[:, 13:][kmt[:, 13:] > 0] = 2
    seas = {-3: (slice(18, 22), slice(10, 14)), -5: (slice(25, 28), slice(4, 7))}
    for num, (js, is_) in seas.items():
        R[js, is_][kmt[js, is_] > 0] = num
        assert (R == num).sum() >= 6, "the synthetic sea %d lies on land" % num
    radian = 180.0 / math.pi
    TLAT = forcing_ref.gather_global(m, m.get("TLAT"), (ny, nx)) * radian
    DX, DY = forcing_ref.gather_global(m, m.get("DXT"), (ny, nx)), forcing_ref.gather_global(m, m.get("DYT"), (ny, nx))
    dlon = 360.0 / nx
    regions = [(1, "open ocean", 0.0, 0.0, 0.0), (2, "east sector", 0.0, 0.0, 0.0)]
    for num, (js, is_) in seas.items():
        jc, ic = js.stop + 1, is_.stop                       # a cell north-east of the sea
        regions.append((num, "sea%d" % -num, float(TLAT[jc, ic]), float((ic + 0.5) * dlon), 7.5 * float(DX[jc, ic] * DY[jc, ic])))
    return regions, R
