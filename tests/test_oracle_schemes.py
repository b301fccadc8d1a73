"""The CPU oracle's restatements of the newest schemes (oracle/orc_tidal.inc, orc_aniso.inc, orc_submeso.inc) against the NumPy
restatements the device's phase tests use (tests/tidal_ref.py, bckgrnd_ref.py, aniso_ref.py, submeso_ref.py): the same cases, the
same states, every physical cell, relative to the field's maximum, at TOL_LOCAL.  No GPU: the helpers the device tests take from
aniso_common, submeso_common, tidal_common and bckgrnd_common are fed through orclib.AsModel, which serves them from an Oracle what they
ask of a device model."""
import numpy as np
import pytest

import aniso_common
import aniso_ref
import bckgrnd_common
import bckgrnd_ref
import orclib
import submeso_common
import submeso_ref
import tidal_common
import tidal_ref
from bckgrnd_common import banda_arctic_grid
from bckgrnd_ref import CESM
from common import TOL_LOCAL, physical
from orclib import AsModel, Oracle
from parity import force_kpp_case
from popcfg import named_config, synthetic_dzbc, synthetic_grid
from tidal_common import stepped_grid


def relmax(a, b, sel):
    s = np.abs(b[sel]).max()
    assert s > 0
    return np.abs(a - b)[sel].max() / s


# ------------------------------------------------------------------ configuration layouts and refusals

def test_config_layouts_5_6_7_step(pkg, orclib_built):
    c5 = named_config("tiny", vmix_choice=3, hmix_tracer=3)
    c6 = pkg.anisotropic_config(c5, hmix_momentum=2)
    c7 = pkg.submeso_config(c5, lsubmesoscale_mixing=0)
    assert (c5.struct_version, c6.struct_version, c7.struct_version) == (5, 6, 7)
    out = []
    for c in (c5, c6, c7):
        o = Oracle(c)
        it = [o.step() for _ in range(2)]
        out.append((it, o.f3("TRACER", 1, 0).copy()))
        o.close()
    for it, T in out[1:]:
        assert it == out[0][0] and np.array_equal(T, out[0][1])
    bad = named_config("tiny")
    bad.struct_version = 8
    with pytest.raises(RuntimeError, match="struct_version is 8, this library reads 5, 6 and 7"):
        Oracle(bad)


def test_omitted_options_are_refused_with_a_message(pkg, orclib_built):
    c5 = named_config("tiny", vmix_choice=3, bckgrnd_vdc1=0.16)
    with pytest.raises(RuntimeError, match="flow"):
        Oracle(pkg.anisotropic_config(c5, aniso_alignment="flow"))
    with pytest.raises(RuntimeError, match="lsmag_aniso"):
        Oracle(pkg.anisotropic_config(c5, lsmag_aniso=1, smag_lat_fact=0.98, c_para=8.0, c_perp=8.0))
    with pytest.raises(RuntimeError, match="hmix_tracer = 3"):
        Oracle(pkg.submeso_config(c5))
    with pytest.raises(RuntimeError, match="partial_bottom_cells"):
        Oracle(pkg.submeso_config(named_config("tiny", hmix_tracer=3, partial_bottom_cells=1)))
    # with anis on as well: the submeso refusals still apply
    for ht in (2, 4):
        with pytest.raises(RuntimeError, match="hmix_tracer = 3"):
            Oracle(pkg.submeso_config(pkg.anisotropic_config(named_config("tiny", hmix_tracer=ht))))
    # the older refusals carry a message of their own, not that of an earlier failure
    for kw, msg in ((dict(hmix_tracer=3, partial_bottom_cells=1), "hmix_gm.F90:782"), (dict(hmix_tracer=3, gm_kappa_type=2, kappa_depth_2=0.0), "kappa_depth_2"),
                    (dict(nt=1), "nt: 2 to 8")):
        with pytest.raises(RuntimeError, match=msg):
            Oracle(named_config("tiny", **kw))
    o = Oracle(c5)
    F = np.ones((o.nblocks, o.nyb, o.nxb))
    for kw, msg in ((dict(ltidal_min_regions=1, num_tidal_min_regions=1), "ltidal_min_regions"), (dict(tidal_mixing_method=1), "jayne"),
                    (dict(tidal_mixing_method=2), "jayne"), (dict(tidal_mix_max=-1.0), "negative")):
        with pytest.raises(RuntimeError, match=msg):
            o.init_tidal_mixing(F, **kw)
    with pytest.raises(RuntimeError, match="count mismatch"):
        o.init_tidal_mixing(F[:1])
    with pytest.raises(RuntimeError, match="negative"):
        o.init_kpp_bckgrnd(bckgrnd_vdc_ban=-1.0)
    o.init_kpp_bckgrnd()
    with pytest.raises(RuntimeError, match="second time"):
        o.init_kpp_bckgrnd()
    o.step()
    with pytest.raises(RuntimeError, match="already run"):
        o.init_tidal_mixing(F)
    o.close()
    for kw, msg in ((dict(vmix_choice=1), "vmix_choice = 3"), (dict(vmix_choice=3, bckgrnd_vdc2=0.1), "bckgrnd_vdc2 = 0")):
        o = Oracle(named_config("tiny", **kw))
        with pytest.raises(RuntimeError, match=msg):
            o.init_tidal_mixing(np.ones((o.nblocks, o.nyb, o.nxb)))
        with pytest.raises(RuntimeError, match=msg):
            o.init_kpp_bckgrnd()
        o.close()


# ------------------------------------------------------------------ anisotropic viscosity: CASES of tests/aniso_common.py

ANISO_CASES = [c for c in aniso_common.CASES if not c[3].get("lsmag_aniso")]      # the Smagorinsky viscosities are not restated in the oracle


@pytest.mark.parametrize("name,cname,kw5,kw6,angle", ANISO_CASES, ids=[c[0] for c in ANISO_CASES])
def test_aniso_matches_restatement(pkg, orclib_built, name, cname, kw5, kw6, angle):
    """the init-time fields (geometry, AMAX_CFL, F_PARA, F_PERP) and the friction HDU, HDV of one clinic on the random velocities of
    the device's phase test"""
    c5 = named_config(cname, **kw5)
    grid = aniso_common.angle_grid(c5) if angle else None
    if grid is not None and c5.partial_bottom_cells:
        grid["DZBC"] = synthetic_dzbc(c5, grid["KMT"])
    cfg = pkg.anisotropic_config(c5, **kw6)
    m = AsModel(Oracle(cfg, grid=grid))
    U, V = aniso_common.state(m, 5)
    m.time_manager()
    m.run_phase("hmix_momentum")
    phys = physical(m)
    p3 = np.broadcast_to(phys[:, None], U.shape)
    g = aniso_ref.geometry(m.get("HTN"), m.get("HTE"), m.get("DXUR"), m.get("DYUR"), m.scalar("dtu"))
    for n, want in g.items():
        a = m.get(n)      # K1E, K1W vanish on a lat-lon grid: compared absolutely there, as common.relerr does
        err = relmax(a, want, phys) if np.abs(want[phys]).max() > 0 else np.abs(a - want)[phys].max()
        assert err <= TOL_LOCAL, (n, err)
    if cfg.lvariable_hmix_aniso:
        fpa, fpe = aniso_ref.var_viscosity(m, cfg, g["AMAX_CFL"])
        for n, want in (("F_PARA", fpa), ("F_PERP", fpe)):
            err = relmax(m.get(n), want, p3)
            print("%s %s: max |oracle - restatement| / max |restatement| = %.3e" % (name, n, err))
            assert err <= TOL_LOCAL, n
    ru, rv = aniso_common.reference(m, cfg, U, V)
    for n, want in (("HDU", ru), ("HDV", rv)):
        a = m.get(n)
        assert np.isfinite(a).all(), n
        err = relmax(a, want, p3)
        print("%s %s: max |oracle - restatement| / max |restatement| = %.3e" % (name, n, err))
        assert err <= TOL_LOCAL, n
    m.close()


# ------------------------------------------------------------------ the submesoscale scheme: CASES of tests/submeso_common.py

@pytest.mark.parametrize("name,kw5,kw7,state,with_grid,branch", submeso_common.CASES, ids=[c[0] for c in submeso_common.CASES])
def test_submeso_matches_restatement(pkg, orclib_built, name, kw5, kw7, state, with_grid, branch):
    c5 = named_config("tiny", **kw5)
    grid = synthetic_grid(c5) if with_grid else None
    cfg = pkg.submeso_config(c5, submeso_diag=1, **kw7)
    m = AsModel(Oracle(cfg, grid=grid))
    T, S = submeso_common.field(m, *state)
    for tl in (0, 1):
        m.set("TRACER", T, tl, 0); m.set("TRACER", S, tl, 1)
        m.halo_update("TRACER", tl, 0); m.halo_update("TRACER", tl, 1)
    m.time_manager()
    m.run_phase("vmix"); m.run_phase("hmix_tracer")
    T, S = m.get("TRACER", 1, 0), m.get("TRACER", 1, 1)
    r = submeso_ref.from_model(m, cfg, T, S)
    phys = physical(m)
    nb = submeso_common.branches(r, phys)
    print(name, "branches of the max:", nb)
    if branch:
        assert nb[branch] > 20, nb
    p3 = np.broadcast_to(phys[:, None], T.shape)
    assert relmax(m.get("SUBM_TIME_SCALE"), r["TS"], phys) <= TOL_LOCAL
    for fname, a, want, sel in [("SUBM_ML_DEPTH", m.get("SUBM_ML_DEPTH"), r["ML"], phys), ("HLS_SUBM", m.get("HLS_SUBM"), r["HLS"], phys)] + \
            [("SUBM_ADV_TEND %d" % n, m.get("SUBM_ADV_TEND", 1, n), r["TEND"][:, n], p3) for n in (0, 1)]:
        assert np.isfinite(a).all(), fname
        err = relmax(a, want, sel)
        print("%s %s: max |oracle - restatement| / max |restatement| = %.3e" % (name, fname, err))
        assert err <= TOL_LOCAL, fname
    m.close()


# ------------------------------------------------------------------ tidal mixing: CASES of tests/tidal_common.py

def tidal_run(cfg, grid=None, **nml_kw):
    """test_gpu_tidal.run on the oracle: state, flux amplitude (from the restatement alone), init, one evaluation of the coefficients"""
    m = AsModel(Oracle(cfg, grid=grid))
    T, S = tidal_common.set_state(m)
    F1 = tidal_common.unit_flux(m)
    amp = tidal_common.amplitude(orclib, m, cfg, F1, T, S)      # orclib.tidal_nml stands in for the package's
    F = amp * F1
    nml = m.orc.init_tidal_mixing(F, **dict(dict(tidal_diag=1), **nml_kw))
    m.time_manager()
    m.run_phase("vmix")
    return m, nml, F, T, S, amp


TIDAL_CASES = [c for c in tidal_common.CASES if c[3] is None]      # ltidal_min_regions is not restated in the oracle: the 'regions' row stays NumPy-only


@pytest.mark.parametrize("name,kw5,kwn,regions,gridkind,need", TIDAL_CASES, ids=[c[0] for c in TIDAL_CASES])
def test_tidal_matches_restatement(orclib_built, name, kw5, kwn, regions, gridkind, need):
    cfg = named_config("tiny", **dict(tidal_common.KPP, **kw5))
    grid = stepped_grid(cfg) if gridkind == "stepped" else synthetic_grid(cfg) if gridkind == "synthetic" else None
    m, nml, F, T, S, amp = tidal_run(cfg, grid=grid, **kwn)
    r = tidal_ref.from_model(m, cfg, nml, F, T, S)
    phys = physical(m)
    nb = tidal_common.branches(r, phys)
    if "stab-off" in need:
        on = tidal_ref.from_model(m, cfg, orclib.tidal_nml(tidal_diag=1), F, T, S)
        nb["stab-off"] = tidal_common.branches(on, phys)["stab"]
        assert nb["stab"] == 0
    print(name, "flux amplitude %.3e W/m^2, branches:" % amp, nb)
    for b in need:
        assert nb[b] > 20, (b, nb)
    p3 = np.broadcast_to(phys[:, None], r["N2"].shape)
    assert np.array_equal(m.get("TIDAL_ENERGY_FLUX"), r["EF"])
    for fname, key in (("TIDAL_COEF_3D", "COEF"), ("TIDAL_N2", "N2"), ("TIDAL_DIFF", "DIFF"), ("KVMIX", "KVMIX"), ("KVMIX_M", "KVMIX_M")):
        a = m.get(fname)
        assert np.isfinite(a).all(), fname
        err = relmax(a, r[key], p3)
        print("%s: max |oracle - restatement| / max |restatement| = %.3e" % (fname, err))
        assert err <= TOL_LOCAL, fname
    m.close()


# ------------------------------------------------------------------ the varying background: ORACLE_CASES of tests/bckgrnd_common.py and test_with_tidal_mixing of tests/test_gpu_bckgrnd.py

def _first_rows(m):
    return [(b["jb"] - 1 if b["j_glob"][b["jb"] - 1] == 1 else None) for b in (m.get_block(i) for i in m.local_block_ids())]


@pytest.mark.parametrize("name,kw5,own_grid", bckgrnd_common.ORACLE_CASES, ids=[c[0] for c in bckgrnd_common.ORACLE_CASES])
def test_bckgrnd_matches_restatement(orclib_built, name, kw5, own_grid):
    """BCKGRND_VDC / BCKGRND_VVC and TLON against tests/bckgrnd_ref.py; then, as test_gpu_bckgrnd.test_rows_match_oracle does for the
    device, the coefficients of the varying run against runs with the uniform bckgrnd_vdc1 = v on the columns where the field is v
    (bit for bit here: both sides are this library, the varying field only changes which number is added)"""
    cfg = named_config("tiny", **dict(tidal_common.KPP, **kw5))
    grid = banda_arctic_grid(cfg) if own_grid else None
    m = AsModel(Oracle(cfg, grid=grid))
    T, S = tidal_common.noisy_state(m)
    for k in range(m.km):
        for X in (T, S):
            x = np.ascontiguousarray(X[:, k]); m.halo_update_host_loc(x); X[:, k] = x
    bckgrnd_common.feed_oracle(m.orc, T, S)
    m.orc.init_kpp_bckgrnd(**CESM)
    m.time_manager(); m.run_phase("vmix")
    phys = physical(m)
    ocean = phys & (m.geti("KMT") > 0)
    ref, masks = bckgrnd_common.restated(m, cfg)
    tl = bckgrnd_ref.tlon(m.get("ULAT"), m.get("ULON"), _first_rows(m))
    for fname, a, b in (("TLON", m.get("TLON"), tl), ("BCKGRND_VDC", m.get("BCKGRND_VDC"), ref), ("BCKGRND_VVC", m.get("BCKGRND_VVC"), cfg.Prandtl * ref)):
        err = relmax(a, b, phys)
        print("%s %s: max |oracle - restatement| / max |restatement| = %.3e" % (name, fname, err))
        assert err <= TOL_LOCAL, fname
    if own_grid:
        assert min(int((masks[n] & ocean).sum()) for n in ("banda_north", "banda_middle", "banda_south")) >= 4
    field = m.get("BCKGRND_VDC")
    values = np.unique(field[ocean])
    assert 3 <= len(values) <= cfg.ny_global + 1
    got = {"VDC0": m.get("VDC", 1, 0), "VDC1": m.get("VDC", 1, 1), "SRC0": m.get("KPP_SRC", 1, 0), "HBLT": m.get("HBLT")}
    assert got["VDC0"].max() > 1.0 or kw5.get("lrich") == 0
    seen = np.zeros(ocean.shape, dtype=bool)
    for v in values[::max(1, len(values) // 6)]:      # a sixth of the rows: the identity is the same statement on each
        orc = Oracle(named_config("tiny", **dict(tidal_common.KPP, **dict(kw5, bckgrnd_vdc1=float(v)))), grid=grid)
        bckgrnd_common.feed_oracle(orc, T, S)
        orc.L.orc_time_manager(orc.h); orc.run_phase("tracer_rhs")
        want = {"VDC0": orc.vdc(0), "VDC1": orc.vdc(1), "SRC0": orc.f3("KPP_SRC", 1, 0), "HBLT": orc.f2("HBLT")}
        sel = ocean & (field == v)
        seen |= sel
        for n in got:
            s = sel if got[n].ndim == 3 else np.broadcast_to(sel[:, None], got[n].shape)
            assert np.array_equal(got[n][s], want[n][s]), (n, v)
        orc.close()
    assert seen.sum() > 20
    m.close()


def test_bckgrnd_with_tidal_mixing(orclib_built):
    """test_gpu_bckgrnd.test_with_tidal_mixing on the oracle: KVMIX = min(b + TIDAL_DIFF, tidal_mix_max), KVMIX_M = Prandtl
    min((Prandtl b) / Prandtl + TIDAL_DIFF, tidal_mix_max); both orders of the two init calls give the same bits"""
    cfg = named_config("tiny", **bckgrnd_common.STEPPED)
    out = []
    for tidal_first in (False, True):
        m = AsModel(Oracle(cfg))
        T, S = tidal_common.set_state(m)
        bckgrnd_common.set_flux(m)
        F1 = tidal_common.unit_flux(m)
        amp = tidal_common.amplitude(orclib, m, cfg, F1, T, S)
        if tidal_first:
            nml = m.orc.init_tidal_mixing(amp * F1, tidal_diag=1)
        m.orc.init_kpp_bckgrnd(**CESM)
        if not tidal_first:
            nml = m.orc.init_tidal_mixing(amp * F1, tidal_diag=1)
        m.time_manager(); m.run_phase("vmix")
        out.append({n: m.get(*a) for n, a in bckgrnd_common.FIELDS + tuple((n, (n,)) for n in ("TIDAL_DIFF", "KVMIX", "KVMIX_M"))})
        if tidal_first:
            m.close()
            continue
        r = tidal_ref.from_model(m, cfg, nml, amp * F1, T, S)
        b, _ = bckgrnd_common.restated(m, cfg)
        b = b[:, None]
        Pr, mx = cfg.Prandtl, nml.tidal_mix_max
        wet = (np.arange(1, m.km + 1)[None, :, None, None] < r["KMT"][:, None]) & physical(m)[:, None]
        kv = np.where(wet, np.minimum(b + r["DIFF"], mx), 0.0)
        kvm = np.where(wet, Pr * np.minimum((Pr * b) / Pr + r["DIFF"], mx), 0.0)
        above, below = int(((b + r["DIFF"] > mx) & wet).sum()), int(((b + r["DIFF"] < mx) & wet).sum())
        assert above > 20 and below > 20
        for fname, want in (("TIDAL_DIFF", r["DIFF"]), ("KVMIX", kv), ("KVMIX_M", kvm)):
            err = relmax(m.get(fname), want, wet)
            print("%s: max |oracle - restatement| / max |restatement| = %.3e" % (fname, err))
            assert err <= TOL_LOCAL, fname
        assert np.abs(m.get("KVMIX") - r["KVMIX"])[wet].max() > 0.1
        m.close()
    for n in out[0]:
        assert np.array_equal(out[0][n], out[1][n]), n


# ------------------------------------------------------------------ the state of case 4 of tests/test_gpu_schemes_oracle.py

class _NoDevice:
    def set(self, *a, **kw):
        pass


def test_case4_state_is_stable_to_an_ulp_of_pow(orclib_built, tmp_path):
    """The device and the oracle evaluate the same expressions in the same order; what separates them before the first solve is the
    rounding of the math library (TOL_LOCAL's premise, tests/common.py).  A state can serve a comparison at TOL_LOCAL only if
    the oracle itself moves by much less than that when a library function returns the neighbouring double.  Measured here without a
    device: the first baroclinic driver of case 4 by the oracle and by a second build of it whose pow is off by one ulp in half of its
    calls (tests/pow_ulp.h).  force_kpp_case on the Banda / Arctic grid: HBLT 5.8e-13, VDC 8.1e-13, VVC 4.0e-13, TRACER 2.0e-13, UVEL
    1.4e-13 -- it cannot serve, asserted; cesm_case.force_kpp_case_above_deep_water: 4.1e-15, 8.9e-15, 4.8e-15, 9.7e-15, 7.9e-16,
    asserted below a fifth of the bound run_phases gives the field, and the boundary layer still takes more than 50 distinct depths
    over a factor ten."""
    import os
    import subprocess
    import cesm_case as cc
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "pop_oracle.c")
    lib = str(tmp_path / "libpop_oracle_pow_ulp.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fno-builtin-sin", "-fno-builtin-cos", "-D_GNU_SOURCE",
                           "-DPOW_ULP_ONE_IN=2", "-include", os.path.join(os.path.dirname(os.path.abspath(__file__)), "pow_ulp.h"), "-shared", "-o", lib, src, "-lm"])
    cfg = named_config("tiny", vmix_choice=3, bckgrnd_vdc1=0.16, km=24, ldbl_diff=1)

    def first_driver(state, lib):
        o = Oracle(cfg, grid=banda_arctic_grid(cfg), lib=lib)
        state(_NoDevice(), o)
        o.init_kpp_bckgrnd(**CESM)
        o.L.orc_time_manager(o.h); o.L.orc_dhdt(o.h); o.L.orc_baroclinic_driver(o.h)
        sel = physical(AsModel(o))
        out = {"HBLT": o.f2("HBLT")[sel], "VDC": o.vdc(0)[:, 1:-1][np.broadcast_to(sel[:, None], o.f3("VVC").shape)]}
        for f, a in (("VVC", o.f3("VVC")), ("TRACER", o.f3("TRACER", 2, 0)), ("UVEL", o.f3("UVEL", 2))):
            out[f] = a[np.broadcast_to(sel[:, None], a.shape)]
        out = {f: a.copy() for f, a in out.items()}
        o.close()
        return out
    bound = {"HBLT": TOL_LOCAL * 10, "VDC": TOL_LOCAL * 10, "VVC": TOL_LOCAL, "TRACER": TOL_LOCAL, "UVEL": TOL_LOCAL}
    err = {}
    for name, state in (("force_kpp_case", force_kpp_case), ("above_deep_water", cc.force_kpp_case_above_deep_water)):
        a, b = first_driver(state, None), first_driver(state, lib)
        err[name] = {f: np.abs(a[f] - b[f]).max() / np.abs(a[f]).max() for f in a}
        print(name, {f: "%.2e" % e for f, e in err[name].items()})
        h = a["HBLT"][a["HBLT"] > 0]
        assert len(np.unique(np.round(h, 1))) > 50 and h.max() > 10.0 * h.min()
    assert any(e > 0.0 for e in err["above_deep_water"].values())        # the second build does differ
    assert err["force_kpp_case"]["VVC"] > TOL_LOCAL and err["force_kpp_case"]["TRACER"] > TOL_LOCAL
    for f, e in err["above_deep_water"].items():
        assert e <= bound[f] / 5.0, (f, e)
