"""The submesoscale mixed-layer eddy scheme on the GPU (lsubmesoscale_mixing): k_submeso_column / k_submeso_flux against the NumPy
restatement (tests/submeso_ref.py), the closed form of tests/test_submeso_host.py on the device, properties that need no comparison
(conservation, confinement, velocities, potential energy) and bitwise checks of the schedule."""
import os

import numpy as np
import pytest

import submeso_ref
from common import TOL_LOCAL, physical
from mr_launch import ROOT, run_check
from popcfg import named_config, synthetic_grid
from submeso_common import CASES, CLOSED_FORM_ULPS, GM, KPP, branches, closed_form, field, linear_state, open_ocean

pytestmark = pytest.mark.gpu


def run(pkg, cfg, state=(2.0, 0.3, 0.2), grid=None, tuning=None, TS=None):
    """model with the tracers set at both time levels (ghost cells from the halo update), the vertical-mixing coefficients (HMXL with
    KPP) and the hmix_tracer phase run once"""
    m = pkg.PopModel(cfg, grid=grid, tuning=tuning)
    T, S = TS if TS is not None else field(m, *state)
    for tl in (0, 1):
        m.set("TRACER", T, tl, 0); m.set("TRACER", S, tl, 1)
        m.halo_update("TRACER", tl, 0); m.halo_update("TRACER", tl, 1)
    m.time_manager()
    m.run_phase("vmix")
    m.run_phase("hmix_tracer")
    return m, m.get("TRACER", 1, 0), m.get("TRACER", 1, 1)


def compare(m, r, phys):
    """SUBM_ML_DEPTH, HLS_SUBM, SUBM_ADV_TEND n = 0, 1 on every physical cell, relative to the field's maximum"""
    p3 = np.broadcast_to(phys[:, None], (m.nblocks, m.km, m.nyb, m.nxb))
    pairs = [("SUBM_ML_DEPTH", m.get("SUBM_ML_DEPTH")[phys], r["ML"][phys]), ("HLS_SUBM", m.get("HLS_SUBM")[phys], r["HLS"][phys])]
    pairs += [("SUBM_ADV_TEND %d" % n, m.get("SUBM_ADV_TEND", 1, n)[p3], r["TEND"][:, n][p3]) for n in (0, 1)]
    for name, a, b in pairs:
        assert np.isfinite(a).all(), name
        s = np.abs(b).max()
        assert s > 0, name
        err = np.abs(a - b).max() / s
        print("%s: max |device - restatement| / max |restatement| = %.3e" % (name, err))
        assert err <= TOL_LOCAL, name


@pytest.mark.parametrize("name,kw5,kw7,state,with_grid,branch", CASES, ids=[c[0] for c in CASES])
def test_fields_and_tendency_match_restatement(pkg, name, kw5, kw7, state, with_grid, branch):
    c5 = named_config("tiny", **kw5)
    grid = synthetic_grid(c5) if with_grid else None
    cfg = pkg.submeso_config(c5, submeso_diag=1, **kw7)
    m, T, S = run(pkg, cfg, state, grid)
    r = submeso_ref.from_model(m, cfg, T, S)
    phys = physical(m)
    nb = branches(r, phys)
    print(name, "branches of the max:", nb)
    if branch:
        assert nb[branch] > 20, nb
    compare(m, r, phys)
    m.close()


def test_closed_form_on_the_device(pkg):
    """tests/test_submeso_host.py::test_restatement_against_closed_form with the model's own DRDT, on the device's tendency"""
    a, c, b = 2.0 ** -6, -2.0 ** -5, -2.0 ** -3
    cfg = pkg.submeso_config(named_config("tiny", **GM), luse_const_horiz_len_scale=1, submeso_diag=1)
    m0 = pkg.PopModel(cfg)
    T, S, lin = linear_state(m0, a=a, c=c, b=b)
    m0.close()
    m, T1, S1 = run(pkg, cfg, TS=(T, S))
    r = submeso_ref.from_model(m, cfg, T1, S1)
    ok = open_ocean(r) & lin & physical(m)
    assert ok.sum() > 100
    g1, g2, big = closed_form(r, a, c, b, 0.07, 5.0e5)
    t = m.get("SUBM_ADV_TEND", 1, 0)
    tol = CLOSED_FORM_ULPS * np.finfo(float).eps
    assert np.abs(t[:, 0][ok]).max() > 0.0
    print("closed form: level 1 %.3e, level 2 %.3e (in units of the largest term)" % ((np.abs(t[:, 0] - g1)[ok] / big[ok]).max(), (np.abs(t[:, 1] - g2)[ok] / big[ok]).max()))
    assert (np.abs(t[:, 0] - g1)[ok] <= tol * big[ok]).all()
    assert (np.abs(t[:, 1] - g2)[ok] <= tol * big[ok]).all()
    assert np.all(t[:, 2:][np.broadcast_to(ok[:, None], t[:, 2:].shape)] == 0.0)
    m.close()


def _kpp_model(pkg, state=(2.0, 0.3, 0.2), **kw):
    cfg = pkg.submeso_config(named_config("tiny", **dict(KPP, stepped_bathymetry=1)), submeso_diag=1, **kw)
    m, T, S = run(pkg, cfg, state)
    return cfg, m, T, S


def test_tendency_conserves_tracer_content(pkg):
    """sum of SUBM_ADV_TEND dz TAREA over the ocean = 0 to rounding, relative to the sum of magnitudes (the bound of
    tests/test_gpu_gm.py::test_gm_conserves_tracer_content: 2e-9)"""
    cfg, m, T, S = _kpp_model(pkg)
    vg = submeso_ref.vertical(m.km)
    vol = (m.get("TAREA") * physical(m))[:, None] * vg["dz"][1:][None, :, None, None]
    for n in (0, 1):
        t = m.get("SUBM_ADV_TEND", 1, n)
        assert np.abs(t).max() > 0.0
        tot, mag = (t * vol).sum(), np.abs(t * vol).sum()
        print("tracer %d: sum %.3e, sum of magnitudes %.3e" % (n, tot, mag))
        assert abs(tot) <= 2.0e-9 * mag
    m.close()


def test_tendency_is_confined_to_the_mixed_layer(pkg):
    """exactly 0.0 at every level k >= 2 with zt(k-1) + dz(k-1)/4 >= max(ML_DEPTH) over the cell and its four neighbours"""
    cfg, m, T, S = _kpp_model(pkg)
    vg = submeso_ref.vertical(m.km)
    ml = m.get("SUBM_ML_DEPTH")
    mx = np.maximum.reduce([ml, submeso_ref._e(ml), submeso_ref._w(ml), submeso_ref._n(ml), submeso_ref._s(ml)])
    depth = (vg["zt"] + 0.25 * vg["dz"])[1:m.km]                                  # of level k - 1, k = 2 .. km
    below = (depth[None, :, None, None] >= mx[:, None]) & physical(m)[:, None]
    assert below.sum() > 0 and (~below).sum() > 0
    for n in (0, 1):
        t = m.get("SUBM_ADV_TEND", 1, n)
        assert np.all(t[:, 1:][below] == 0.0)
        assert np.abs(t[:, 1:][~below]).max() > 0.0
    m.close()


def test_velocities(pkg):
    """U_SUBM, V_SUBM against the restatement; the transport through every face column sums to zero (the bound of the bolus test of
    tests/test_gpu_gm.py: 1e-12 of the largest column sum of magnitudes); WSUBM is 0 at the top of level 1 and at and below the bottom level"""
    cfg, m, T, S = _kpp_model(pkg)
    r = submeso_ref.from_model(m, cfg, T, S)
    phys = physical(m)
    p3 = np.broadcast_to(phys[:, None], (m.nblocks, m.km, m.nyb, m.nxb))
    dz = r["vg"]["dz"][1:][None, :, None, None]
    for nm, key in (("USUBM", "U"), ("VSUBM", "V"), ("WSUBM", "W")):
        a, b = m.get(nm), r[key]
        s = np.abs(b[p3]).max()
        assert s > 0 and np.abs(a[p3] - b[p3]).max() / s <= TOL_LOCAL, nm
    for nm in ("USUBM", "VSUBM"):
        tr = m.get(nm) * dz
        tot, mag = tr.sum(axis=1)[phys], np.abs(tr).sum(axis=1)[phys]
        assert mag.max() > 0.0 and np.abs(tot).max() <= 1.0e-12 * mag.max(), nm
    w = m.get("WSUBM")
    kmt = m.geti("KMT")
    lev = np.arange(1, m.km + 1)[None, :, None, None]
    assert np.all(w[:, 0][phys] == 0.0)
    assert np.all(w[(lev > kmt[:, None]) & p3] == 0.0)
    m.close()


def test_tendency_lowers_potential_energy(pkg):
    """A temperature-only front (uniform S, so that the sign does not hang on MWJF's cross terms) under a KPP mixed layer: the scheme
    slumps the front, d/dt of sum rho g z dV = g sum DRDT dT/dt z dV < 0 (z positive upwards, so depth enters with a minus sign)"""
    cfg = pkg.submeso_config(named_config("tiny", **KPP), submeso_diag=1)
    m0 = pkg.PopModel(cfg); T, S = field(m0, 0.5, 0.05, 0.0, front=3.0); m0.close()
    S[:] = 0.035
    m, T1, S1 = run(pkg, cfg, TS=(T, S))
    r = submeso_ref.from_model(m, cfg, T1, S1)
    vol = (m.get("TAREA") * physical(m))[:, None] * r["vg"]["dz"][1:][None, :, None, None]
    z = -r["vg"]["zt"][1:][None, :, None, None]
    t = m.get("SUBM_ADV_TEND", 1, 0)
    dpe = submeso_ref.GRAV * (r["DRDT"] * t * z * vol).sum()
    scale = submeso_ref.GRAV * np.abs(r["DRDT"] * t * z * vol).sum()
    print("dPE/dt = %.6e, sum of magnitudes %.6e" % (dpe, scale))
    assert scale > 0.0 and dpe < -1.0e-3 * scale
    m.close()


# ---- bitwise checks
def test_gtk_is_gm_plus_submeso(pkg):
    c5 = named_config("tiny", **dict(KPP, stepped_bathymetry=1, gm_transition_layer=1))
    on, _, _ = run(pkg, pkg.submeso_config(c5, submeso_diag=1))
    off, _, _ = run(pkg, pkg.submeso_config(c5, lsubmesoscale_mixing=0))
    for n in (0, 1):
        td = on.get("SUBM_ADV_TEND", 1, n)
        assert np.abs(td).max() > 0.0
        assert np.array_equal(on.get("GM_GTK", 1, n), off.get("GM_GTK", 1, n) + td)
    on.close(); off.close()


def _steps(pkg, cfg, n, tuning=None, phases=False):
    m = pkg.PopModel(cfg, tuning=tuning)
    for _ in range(n):
        if phases:
            m.time_manager(); m.dhdt(); m.baroclinic_driver(); m.barotropic_driver(); m.baroclinic_correct_adjust(); m.step_tail()
        else:
            m.step()
    out = {(nm, k): m.get(nm, 1, k).copy() for nm, k in (("TRACER", 0), ("TRACER", 1), ("UVEL", 0), ("PSURF", 0))}
    m.close()
    return out


def _same(a, b):
    for key in a:
        assert np.array_equal(a[key], b[key]), key


CESM_TINY = dict(KPP, stepped_bathymetry=1, gm_transition_layer=1, tadvect=2, tmix_opt=3)


def test_switch_off_equals_layout6(pkg):
    c5 = named_config("tiny", **CESM_TINY)
    c6 = pkg.anisotropic_config(c5, aniso_alignment="east", lvariable_hmix_aniso=1)
    _same(_steps(pkg, c6, 4), _steps(pkg, pkg.submeso_config(c6, lsubmesoscale_mixing=0, efficiency_factor=0.5), 4))


def test_submeso_changes_the_run_and_all_levels_is_bitwise(pkg):
    c5 = named_config("tiny", **CESM_TINY)
    cfg = pkg.submeso_config(c5)
    a = _steps(pkg, cfg, 4)
    off = _steps(pkg, pkg.submeso_config(c5, lsubmesoscale_mixing=0), 4)
    assert not np.array_equal(a[("TRACER", 0)], off[("TRACER", 0)])
    assert np.isfinite(a[("TRACER", 0)]).all()
    _same(a, _steps(pkg, cfg, 4, tuning={"submeso_all_levels": 1}))
    _same(a, _steps(pkg, pkg.submeso_config(c5, submeso_diag=1), 4))


def test_step_equals_phase_sequence(pkg):
    cfg = pkg.submeso_config(named_config("tiny", **CESM_TINY))
    _same(_steps(pkg, cfg, 4), _steps(pkg, cfg, 4, phases=True))


def test_restart_is_exact(pkg, tmp_path):
    cfg = pkg.submeso_config(named_config("tiny", **CESM_TINY))
    a = pkg.PopModel(cfg)
    for _ in range(3):
        a.step()
    path = str(tmp_path / "r")
    a.write_restart(path)
    for _ in range(2):
        a.step()
    b = pkg.PopModel(cfg)
    b.read_restart(path)
    for _ in range(2):
        b.step()
    for n, k in (("UVEL", 0), ("TRACER", 0), ("TRACER", 1), ("PSURF", 0)):
        assert np.array_equal(a.get(n, 1, k), b.get(n, 1, k)), n
    a.close(); b.close()


@pytest.mark.parametrize("nranks,kw,grid", [(2, "", 0), (3, "block_size_x=20,block_size_y=16", 0), (2, "ns_boundary=2", 1)])
def test_multirank_equals_single_rank(nranks, kw, grid):
    base = "hmix_tracer=3,vmix_choice=3"
    run_check(["--nproc-per-node", str(nranks), os.path.join(ROOT, "tests", "mr_gpu_submeso.py"), "--submeso", "time_scale_constant=8.64e4",
                "--config", "tiny", "--steps", "3", "--grid", str(grid), "--kw", base + ("," + kw if kw else "")], 300)


def test_gx1v7_cesm_setup(pkg):
    """the gx1v7 CESM set-up (Gent-McWilliams with the transition layer and the once-a-day 'bfre' kappa, upwind3, Robert filter, P-CSI with
    EVP, 'anis') with the submesoscale scheme and CESM's time_scale_constant: 10 finite steps, and the tendency of step 10 against the
    restatement"""
    c5 = named_config("gx1v7", hmix_tracer=3, gm_transition_layer=1, gm_kappa_type=1, gm_kappa_freq=2, tadvect=2, tmix_opt=3, solver_choice=3,
                      preconditioner_choice=1)
    c6 = pkg.anisotropic_config(c5, aniso_alignment="east", lvariable_hmix_aniso=1)
    cfg = pkg.submeso_config(c6, time_scale_constant=8.64e4, submeso_diag=1)
    m = pkg.PopModel(cfg)
    for _ in range(9):
        m.step()
    # step 10 is a leapfrog step: its mix-time tracers are the old ones of the state before it
    T, S = m.get("TRACER", 0, 0), m.get("TRACER", 0, 1)
    m.step()
    for n in ("UVEL", "VVEL", "PSURF", "HLS_SUBM", "SUBM_ML_DEPTH"):
        assert np.isfinite(m.get(n, 1)).all(), n
    for k in (0, 1):
        assert np.isfinite(m.get("TRACER", 1, k)).all() and np.isfinite(m.get("SUBM_ADV_TEND", 1, k)).all()
    r = submeso_ref.from_model(m, cfg, T, S, ML=m.get("SUBM_ML_DEPTH"))
    compare(m, r, physical(m))
    m.close()
