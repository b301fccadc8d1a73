"""Shared pieces of the tavg tests (tests/test_gpu_tavg.py, tests/test_gpu_diag.py, tests/test_gpu_land_schemes.py): the cases, the model
of a case with its seeded state, the requests spread over the two streams and the raw buffers."""
import numpy as np

from ice_common import cold_start, ice_grid
from popcfg import named_config
from tidal_common import smooth_flux

KPP = dict(vmix_choice=3, km=24, kpp_ml_diagnostics=1)
GM = dict(hmix_tracer=3, ah=0.8e7, gm_diag_bolus=1)
ICE_NML = dict(ice_freq_opt="coupled", licecesm2=1, kmxice=3, lfw_as_salt_flx=1, tfreeze_option=1)

# name -> (config keywords, what else the case needs)
CASES = {
    "avgfit": (dict(), {}),
    "leapfrog": (dict(tmix_opt=0), {}),
    "avg": (dict(tmix_opt=1, time_mix_freq=3), {}),
    "robert": (dict(tmix_opt=3), {}),
    "kpp": (dict(KPP), {}),
    "pbc": (dict(partial_bottom_cells=1), dict(pbc=True)),
    "nt4": (dict(nt=4), dict(iage=3)),
    "gm": (dict(GM), {}),
    "submeso": (dict(GM), dict(submeso=True)),
    "tidal": (dict(vmix_choice=3, km=24, bckgrnd_vdc1=0.16), dict(tidal=True)),
    "ice": (dict(), dict(ice=True)),
    "padded": (dict(block_size_x=11, block_size_y=9), {}),          # 15 x 13 cells per block: an odd plane, the 8-byte form of k_tavg_cells
}


def make(pkg, case, tuning=None, cfgkw=None):
    kw, extra = CASES[case]
    cfg = named_config("tiny", **dict(kw, **(cfgkw or {})))
    if extra.get("submeso"):
        cfg = pkg.submeso_config(cfg, submeso_diag=1)
    grid = ice_grid(cfg, pbc=bool(extra.get("pbc"))) if (extra.get("pbc") or extra.get("ice")) else None
    m = pkg.PopModel(cfg, grid=grid, tuning=tuning)
    if extra.get("tidal"):
        F = smooth_flux(m, 1.0e3)
        m.halo_update_host_loc(F)
        m.init_tidal_mixing(F, tidal_diag=1)
    if extra.get("ice"):
        m.init_ice(**ICE_NML)
    if extra.get("iage"):
        m.init_iage(extra["iage"])
    wet = np.arange(1, m.km + 1)[None, :, None, None] <= m.geti("KMT")[:, None]
    if cfg.nt > 2:                                  # the plain passive tracer starts from a multiple of the salinity
        F = np.where(wet, m.get("TRACER", 1, 1) * 20.0 + 1.0, 0.0)
        for tl in (0, 1, 2):
            m.set("TRACER", F, tl=tl, n=3)
    if extra.get("ice"):
        cold_start(m)
    # a seeded perturbation of the temperature, another one in each of the two time levels, so that the tracers move from the first
    # step on (min and max buffers part, dTEMP_* holds both signs).  Ghost cells through the halo update, as every decomposition has them
    rng = np.random.default_rng(3)
    for tl in (0, 1):
        T = m.get("TRACER", tl, 0)
        m.set("TRACER", np.where(wet, T + 0.05 * rng.standard_normal(T.shape), 0.0), tl=tl, n=0)
        m.halo_update("TRACER", tl, 0)
    return m


def request(m, names):
    req = {n: 1 + (i % 2) for i, n in enumerate(names)}
    for n, ns in req.items():
        m.tavg_request(ns, n)
    return req


def buffers(m, req):
    return {n: m.tavg_get(n, normalize=False) for n in req}
