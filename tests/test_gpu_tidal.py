"""Jayne tidal mixing on the GPU (pop_init_tidal_mixing, k_kpp_tidal): the diagnostics against the NumPy restatement (tests/tidal_ref.py),
the coefficients below the boundary layer against a run without tidal mixing, a saturated case against the unchanged CPU oracle
through blmix, the viscosity average and a step, every KPP kernel form, zero flux, and two ranks."""
import os

import numpy as np
import pytest

import tidal_ref
from bckgrnd_common import feed_oracle
from common import TOL_LOCAL, TOL_SOLVE, physical, relerr
from mr_launch import ROOT, run_check
from orclib import Oracle
from popcfg import named_config, synthetic_grid
from submeso_common import field
from tidal_common import CASES, KPP, NOISY, amplitude, branches, set_state, stepped_grid, unit_flux

pytestmark = pytest.mark.gpu


def run(pkg, cfg, grid=None, tuning=None, state=NOISY, amp=None, regions=None, **nml_kw):
    """a model with the state set, tidal mixing initialised (tidal_diag on unless the keywords say otherwise) and the "vmix" phase run
    once; returns the model, its namelist, the flux [W/m^2] and the tracers"""
    m = pkg.PopModel(cfg, grid=grid, tuning=tuning)
    T, S = set_state(m, state)
    F1 = unit_flux(m)
    if amp is None:
        amp = amplitude(pkg, m, cfg, F1, T, S)
    F = amp * F1
    nml = m.init_tidal_mixing(F, regions=regions, **dict(dict(tidal_diag=1), **nml_kw))
    m.time_manager()
    m.run_phase("vmix")
    return m, nml, F, T, S, amp


def compare(m, r, phys):
    p3 = np.broadcast_to(phys[:, None], (m.nblocks, m.km, m.nyb, m.nxb))
    for name, key in (("TIDAL_N2", "N2"), ("TIDAL_DIFF", "DIFF"), ("KVMIX", "KVMIX"), ("KVMIX_M", "KVMIX_M")):
        a, b = m.get(name)[p3], r[key][p3]
        assert np.isfinite(a).all(), name
        s = np.abs(b).max()
        assert s > 0, name
        err = np.abs(a - b).max() / s
        print("%s: max |device - restatement| / max |restatement| = %.3e" % (name, err))
        assert err <= TOL_LOCAL, name


@pytest.mark.parametrize("name,kw5,kwn,regions,gridkind,need", CASES, ids=[c[0] for c in CASES])
def test_fields_match_restatement(pkg, name, kw5, kwn, regions, gridkind, need):
    cfg = named_config("tiny", **dict(KPP, **kw5))
    grid = stepped_grid(cfg) if gridkind == "stepped" else synthetic_grid(cfg) if gridkind == "synthetic" else None
    m, nml, F, T, S, amp = run(pkg, cfg, grid=grid, regions=regions, **kwn)
    r = tidal_ref.from_model(m, cfg, nml, F, T, S)
    phys = physical(m)
    nb = branches(r, phys)
    if "stab-off" in need:      # the cells the stability control would have raised
        on = tidal_ref.from_model(m, cfg, pkg.tidal_nml(tidal_diag=1), F, T, S)
        nb["stab-off"] = branches(on, phys)["stab"]
        assert nb["stab"] == 0
    print(name, "flux amplitude %.3e W/m^2, branches:" % amp, nb)
    for b in need:
        assert nb[b] > 20, (b, nb)
    compare(m, r, phys)
    m.close()


def test_below_the_boundary_layer(pkg):
    """with and without tidal mixing on the same state: HBLT bitwise equal, and below both boundary layers VDC_on - VDC_off = KVMIX -
    bckgrnd_vdc, VVC_on - VVC_off = the U-point average of KVMIX_M - bckgrnd_vvc where all four columns qualify"""
    cfg = named_config("tiny", **dict(KPP, stepped_bathymetry=1))
    on, nml, F, T, S, amp = run(pkg, cfg)
    off = pkg.PopModel(cfg)
    set_state(off)
    off.time_manager(); off.run_phase("vmix")
    assert np.array_equal(on.get("HBLT"), off.get("HBLT"))
    kbl = np.maximum(on.geti("KBL"), off.geti("KBL"))[:, None]
    KMT = on.geti("KMT")[:, None]
    lev = np.arange(1, on.km + 1)[None, :, None, None]
    phys = physical(on)
    ok = (lev > kbl) & (lev < KMT)
    sel = ok & phys[:, None]
    print("cells below both boundary layers: %d" % sel.sum())
    assert sel.sum() > 100
    bvdc, bvvc = cfg.bckgrnd_vdc1, cfg.Prandtl * cfg.bckgrnd_vdc1
    dk = on.get("KVMIX") - bvdc
    for n in (0, 1):
        d = on.get("VDC", 1, n)[:, 1:-1] - off.get("VDC", 1, n)[:, 1:-1]
        err = np.abs(d - dk)[sel].max() / np.abs(dk[sel]).max()
        print("VDC(%d) on - off against KVMIX - bckgrnd_vdc: %.3e" % (n, err))
        assert err <= TOL_LOCAL
    dm = np.where(ok, on.get("KVMIX_M") - bvvc, 0.0)
    au = [on.get(n)[:, None] for n in ("AU0", "AUN", "AUE", "AUNE")]
    avg, ok4 = np.zeros(dm.shape), np.zeros(dm.shape, dtype=bool)
    avg[..., :-1, :-1] = au[0][..., :-1, :-1] * dm[..., :-1, :-1] + au[1][..., :-1, :-1] * dm[..., 1:, :-1] + \
        au[2][..., :-1, :-1] * dm[..., :-1, 1:] + au[3][..., :-1, :-1] * dm[..., 1:, 1:]
    ok4[..., :-1, :-1] = ok[..., :-1, :-1] & ok[..., 1:, :-1] & ok[..., :-1, 1:] & ok[..., 1:, 1:]
    sel4 = ok4 & phys[:, None]
    print("U cells whose four columns lie below both boundary layers: %d" % sel4.sum())
    assert sel4.sum() > 100
    d = on.get("VVC") - off.get("VVC")
    err = np.abs(d - avg)[sel4].max() / np.abs(avg[sel4]).max()
    print("VVC on - off against the average of KVMIX_M - bckgrnd_vvc: %.3e" % err)
    assert err <= TOL_LOCAL
    on.close(); off.close()


def _feed(gpu, orc, T, S):
    """the same tracers at every time level of both models and the densities that belong to them (parity.force_kpp_case)"""
    R = feed_oracle(orc, T, S)
    for tl in (0, 1, 2):
        gpu.set("TRACER", T, tl=tl, n=0); gpu.set("TRACER", S, tl=tl, n=1)
    for tl in (0, 1):
        gpu.set("RHO", R, tl=tl)


def _saturated(pkg, orclib_built):
    """a stably stratified state (field() without cell-to-cell variation, no initial perturbation) and a flux so large that TIDAL_DIFF =
    tidal_mix_max at every level above the bottom: the coefficients are then what the oracle forms with bckgrnd_vdc1 = tidal_mix_max
    and no tidal mixing"""
    cfg = named_config("tiny", **dict(KPP, init_ts_perturbation=0.0))
    gpu = pkg.PopModel(cfg)
    orc = Oracle(named_config("tiny", **dict(KPP, init_ts_perturbation=0.0, bckgrnd_vdc1=100.0)))
    T, S = field(gpu, 2.0, 0.3, 0.0)
    for k in range(gpu.km):      # ghost cells from their source cells (field() is a function of the global indices, which closed boundaries lack)
        for X in (T, S):
            x = np.ascontiguousarray(X[:, k]); gpu.halo_update_host_loc(x); X[:, k] = x
    _feed(gpu, orc, T, S)
    F1 = unit_flux(gpu)
    unit = tidal_ref.from_model(gpu, cfg, pkg.tidal_nml(ltidal_max=0, ltidal_stabc=0), F1, T, S)
    wet = np.arange(1, gpu.km + 1)[None, :, None, None] < unit["KMT"][:, None]
    assert wet.sum() > 1000 and np.all(unit["N2"][wet] > 0.0)
    amp = 2.0 * 100.0 / unit["DIFF"][wet].min()
    nml = gpu.init_tidal_mixing(amp * F1, tidal_diag=1)
    r = tidal_ref.from_model(gpu, cfg, nml, amp * F1, T, S)
    assert np.all(r["DIFF"][wet] == 100.0) and np.all(r["KVMIX"][wet] == 100.0)
    return gpu, orc, amp


def test_saturated_phase_matches_oracle(pkg, orclib_built):
    gpu, orc, amp = _saturated(pkg, orclib_built)
    gpu.time_manager(); orc.L.orc_time_manager(orc.h)
    gpu.run_phase("vmix"); orc.run_phase("tracer_rhs")
    inner = lambda a: a[..., 2:-2, 2:-2]
    errs = {"VDC1": relerr(inner(gpu.get("VDC", 1, 0)), inner(orc.vdc(0))), "VDC2": relerr(inner(gpu.get("VDC", 1, 1)), inner(orc.vdc(1))),
            "VVC": relerr(inner(gpu.get("VVC")), inner(orc.f3("VVC"))), "HBLT": relerr(inner(gpu.get("HBLT")), inner(orc.f2("HBLT"))),
            "KPP_SRC0": relerr(inner(gpu.get("KPP_SRC", 1, 0)), inner(orc.f3("KPP_SRC", 1, 0))),
            "KPP_SRC1": relerr(inner(gpu.get("KPP_SRC", 1, 1)), inner(orc.f3("KPP_SRC", 1, 1)))}
    print("saturated (flux amplitude %.3e W/m^2) against the oracle:" % amp, {k: "%.3e" % v for k, v in errs.items()})
    assert np.abs(gpu.get("VDC", 1, 0)).max() >= 100.0
    for k, v in errs.items():
        assert v <= TOL_LOCAL, (k, v)
    gpu.close(); orc.close()


def test_saturated_step_matches_oracle(pkg, orclib_built):
    gpu, orc, amp = _saturated(pkg, orclib_built)
    gpu.step(); orc.step()
    inner = lambda a: a[..., 2:-2, 2:-2]
    for name, n in (("TRACER", 0), ("TRACER", 1), ("UVEL", 0)):
        e = relerr(inner(gpu.get(name, 1, n)), inner(orc.f3(name, 1, n)))
        print("after one step %s(%d): %.3e" % (name, n, e))
        assert e <= TOL_SOLVE, name
    gpu.close(); orc.close()


OUT = ("VDC0", "VDC1", "VVC", "HBLT", "TIDAL_DIFF", "KVMIX", "KVMIX_M")


def _outputs(m):
    return {"VDC0": m.get("VDC", 1, 0), "VDC1": m.get("VDC", 1, 1), "VVC": m.get("VVC"), "HBLT": m.get("HBLT"), "TIDAL_DIFF": m.get("TIDAL_DIFF"),
            "KVMIX": m.get("KVMIX"), "KVMIX_M": m.get("KVMIX_M"), "SRC0": m.get("KPP_SRC", 1, 0), "SRC1": m.get("KPP_SRC", 1, 1)}


@pytest.fixture(scope="module")
def base_outputs(pkg):
    cfg = named_config("tiny", **KPP)
    m, nml, F, T, S, amp = run(pkg, cfg, tuning={"kpp_col": 0})
    out = _outputs(m)
    m.close()
    return cfg, amp, out


@pytest.mark.parametrize("tuning", [{"kpp_col": 3}, {"kpp_col": 4}, {"kpp_col": 8}, {"kpp_col": 25}, {"kpp_interior_generic": 1}],
                         ids=["col3", "col4", "col8", "col25", "interior-generic"])
def test_every_kernel_form(pkg, base_outputs, tuning):
    """the interior forms are bitwise equal to each other (kernels_kpp.hpp), so the sums k_kpp_tidal forms are too"""
    cfg, amp, base = base_outputs
    m, nml, F, T, S, _ = run(pkg, cfg, tuning=tuning, amp=amp)
    out = _outputs(m)
    m.close()
    for n, a in out.items():
        e = relerr(a, base[n])
        print("%s %s: %.3e%s" % (tuning, n, e, "" if np.array_equal(a, base[n]) else " (not bitwise)"))
        assert e <= TOL_LOCAL, n
        assert np.array_equal(a, base[n]), n


def test_km60_register_interior_form(pkg):
    cfg = named_config("tiny", **dict(KPP, nx_global=24, ny_global=20, km=60))
    a, nml, F, T, S, amp = run(pkg, cfg)
    r = tidal_ref.from_model(a, cfg, nml, F, T, S)
    compare(a, r, physical(a))
    b, *_ = run(pkg, cfg, tuning={"kpp_interior_generic": 1}, amp=amp)
    oa, ob = _outputs(a), _outputs(b)
    for n in oa:
        assert relerr(oa[n], ob[n]) <= TOL_LOCAL and np.array_equal(oa[n], ob[n]), n
    a.close(); b.close()


def _three_steps(pkg, cfg, tuning, flux_amp, call=True):
    m = pkg.PopModel(cfg, tuning=tuning)
    if call:
        m.init_tidal_mixing(flux_amp * unit_flux(m))
    for _ in range(3):
        m.step()
    out = {n: m.get(*a) for n, a in (("T", ("TRACER", 1, 0)), ("S", ("TRACER", 1, 1)), ("U", ("UVEL", 1, 0)), ("P", ("PSURF", 1, 0)),
                                     ("VVC", ("VVC", 1, 0)), ("VDC", ("VDC", 1, 0)), ("HBLT", ("HBLT", 1, 0)), ("SRC", ("KPP_SRC", 1, 0)))}
    m.close()
    return out


def test_look_ahead_on_and_off(pkg):
    cfg = named_config("tiny", **dict(KPP, stepped_bathymetry=1))
    a = _three_steps(pkg, cfg, {"kpp_ahead": 1}, 1.0e3)
    b = _three_steps(pkg, cfg, {"kpp_ahead": 0}, 1.0e3)
    plain = _three_steps(pkg, cfg, {"kpp_ahead": 0}, 0.0, call=False)
    for n in a:
        assert np.isfinite(a[n]).all() and np.array_equal(a[n], b[n]), n
    assert not np.array_equal(a["T"], plain["T"])


def test_zero_flux_changes_nothing(pkg):
    cfg = named_config("tiny", **dict(KPP, stepped_bathymetry=1))
    z, *_ = run(pkg, cfg, amp=0.0, tidal_diag=0)
    p = pkg.PopModel(cfg)
    set_state(p)
    p.time_manager(); p.run_phase("vmix")
    for n, a in (("VDC", ("VDC", 1, 0)), ("VDC2", ("VDC", 1, 1)), ("VVC", ("VVC",)), ("HBLT", ("HBLT",)), ("SRC0", ("KPP_SRC", 1, 0)), ("SRC1", ("KPP_SRC", 1, 1))):
        assert np.array_equal(z.get(*a), p.get(*a)), n
    with pytest.raises(pkg.PopError, match="tidal_diag"):
        z.get("KVMIX")
    z.close(); p.close()


def test_two_ranks_equal_single_rank():
    run_check(["--nproc-per-node", "2", os.path.join(ROOT, "tests", "mr_gpu_tidal.py"), "--tidal", "amp=1.0e3",
                "--config", "tiny", "--steps", "2", "--no-restart", "--kw", "vmix_choice=3,bckgrnd_vdc1=0.16,stepped_bathymetry=1"], 300)
