"""Frazil ice formation on the device (pop_init_ice, pop_ice_formation, pop_ice_flx_to_coupler, pop_ice_export_reset): the kernel
against the NumPy restatement tests/ice_ref.py with every branch occupied; ice inside the library's own step bit for bit a run that
calls ice_formation where the reference has it; the corrector's freeze clamp; the coupler entries; exact restart; the file of a context
without ice.  Base config 'tiny' (48 x 40 x 16, blocks 12 x 10) on a caller's grid whose KMT includes 0, 1 and 2."""
import numpy as np
import pytest

import ice_ref
from common import STATE, TOL_LOCAL
from ice_common import cold_start, ice_grid, wet_mask
from popcfg import named_config

pytestmark = pytest.mark.gpu

SUB = ("sub_freeze", "sub_melt", "sub_limited", "sub_nothing")
SFC = ("sfc_freeze", "sfc_melt", "sfc_limited", "sfc_nothing")
OFFSET = ("offset_melt", "offset_limited")
ICE_FIELDS = ("QICE", "AQICE", "FW_FREEZE")


def close(got, want, what):
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    assert err <= TOL_LOCAL * scale, "%s: max |diff| %g, max |field| %g" % (what, err, scale)


# ---- 1. the kernel against the restatement -------------------------------------------------------------------------------------
KERNEL_CASES = [(o, s, k, False) for o in (0, 1, 2) for s in (0, 1) for k in (3, 1)] + [(2, 0, 3, True)]


@pytest.mark.parametrize("option,salt,kmxice,pbc", KERNEL_CASES,
                         ids=["%s-%s-kmxice%d%s" % (ice_ref.TFREEZE[o], "salt" if s else "fw", k, "-pbc" if b else "") for o, s, k, b in KERNEL_CASES])
def test_kernel_matches_restatement(pkg, option, salt, kmxice, pbc):
    cfg = named_config("tiny", partial_bottom_cells=1 if pbc else 0)
    m = pkg.PopModel(cfg, grid=ice_grid(cfg, pbc))
    m.init_ice(tfreeze_option=option, lfw_as_salt_flx=salt, kmxice=kmxice)       # 'never': the test decides when ice forms
    p = ice_ref.params(tfreeze_option=option, lfw_as_salt_flx=salt, kmxice=kmxice)
    assert m.scalar("cp_over_lhfusion") == p["cp_over_lhfusion"]
    KMT, wet, km = m.geti("KMT"), wet_mask(m), m.km
    assert all((KMT == v).sum() >= 100 for v in (0, 1, 2)) and (KMT > 3).sum() >= 100
    TH = ice_ref.thickness(km, KMT, m.get("DZBC") if pbc else None)
    pz, dt1 = ice_ref.pressz(km), m.scalar("dtt")
    rng = np.random.default_rng(7)
    T = np.where(wet, rng.uniform(-2.6, -1.0, wet.shape), 0.0)
    S = np.where(wet, rng.uniform(0.030, 0.037, wet.shape), 0.0)
    PS = np.where(KMT > 0, ice_ref.GRAV * rng.uniform(-60.0, 60.0, KMT.shape), 0.0)
    AQ = np.zeros_like(PS)
    count = {n: 0 for n in SUB + SFC + OFFSET}
    for call, tw in enumerate((1.0, 0.5)):
        if call:                                                                # warmer water under the step with time_weight = 0.5
            T = np.where(wet, T + rng.uniform(-0.2, 0.4, wet.shape), 0.0)
            m.time_manager(); m.time_manager()                                  # avgfit: the second step of a run is an averaging step
        assert m.scalar("time_weight") == tw
        m.set("TRACER", T, tl=1, n=0); m.set("TRACER", S, tl=1, n=1); m.set("PSURF", PS, tl=1)
        rho_before = m.get("RHO", 1)
        m.ice_formation(1)
        r = ice_ref.formation(T, S, PS, KMT, AQ, TH, p, tw, dt1)
        got = {"T": m.get("TRACER", 1, 0), "S": m.get("TRACER", 1, 1), "QICE": m.get("QICE"), "AQICE": m.get("AQICE"),
               "FW_FREEZE": m.get("FW_FREEZE")}
        for n in ("T", "S", "QICE", "AQICE"):
            close(got[n], r[n], "%s, call %d" % (n, call + 1))
        if salt:
            assert not got["FW_FREEZE"].any()
        else:
            close(got["FW_FREEZE"], r["FW_FREEZE"], "FW_FREEZE, call %d" % (call + 1))
            assert r["FW_FREEZE"].min() < 0.0
        RHO = m.get("RHO", 1)
        want = np.stack([ice_ref.rho(got["T"][:, k], got["S"][:, k], pz[k + 1]) for k in range(kmxice)], axis=1)
        close(RHO[:, :kmxice], want, "RHO, call %d" % (call + 1))
        assert np.array_equal(RHO[:, kmxice:], rho_before[:, kmxice:])          # the levels below kmxice are not touched
        assert np.array_equal(got["T"][:, kmxice:], T[:, kmxice:]) and np.array_equal(got["S"][:, kmxice:], S[:, kmxice:])
        land = KMT == 0                                                          # land and closed-boundary ghost columns stay exactly 0
        assert not got["T"][np.broadcast_to(land[:, None], T.shape)].any() and not got["QICE"][land].any() and not got["AQICE"][land].any()
        for n, msk in r["branch"].items():
            count[n] += int(msk.sum())
        T, S, AQ = got["T"], got["S"], got["AQICE"]                              # the second call starts from the device's own result
    # every branch of the march must hold cells (a condition of the recipe, not a measurement).  With kmxice = 1 there is no
    # sub-surface level and QICE is 0 when the surface level is reached, so only its freeze / nothing branches can be taken.
    need = SUB + SFC + OFFSET if kmxice > 1 else ("sfc_freeze", "sfc_nothing") + OFFSET
    print("branch occupancy:", count)
    assert all(count[n] >= 50 for n in need), count
    m.close()


# ---- 2. inside the step, bit for bit -------------------------------------------------------------------------------------------
NML = dict(kmxice=3, lfw_as_salt_flx=1, tfreeze_option=1)
STEP_CASES = {
    "default": (dict(), NML, None),                                                                     # tiny: avgfit, step 2 averages
    "fw-form": (dict(), dict(NML, lfw_as_salt_flx=0, tfreeze_option=0), None),
    "leapfrog": (dict(tmix_opt=0), dict(NML, tfreeze_option=2), None),
    "avgfit": (dict(time_mix_freq=4), NML, None),                                                       # steps 2 and 4 average
    "robert": (dict(tmix_opt=3), NML, None),
    "kpp-ahead": (dict(vmix_choice=3, km=24, tmix_opt=0), NML, dict(kpp_ahead=1)),
    "del4": (dict(hmix_momentum=4, hmix_tracer=4, am=-1.0e22, ah=-1.0e21, tmix_opt=0), NML, dict(d2t_fuse=1, d2u_fuse=1)),
    "nt4-iage": (dict(nt=4), NML, None),
}


def start(pkg, cfg, nml, tuning=None, ice=True):
    m = pkg.PopModel(cfg, grid=ice_grid(cfg), tuning=tuning)
    if ice:
        m.init_ice(**nml)
    if cfg.nt > 2:
        m.init_iage(3)
        F = np.where(wet_mask(m), m.get("TRACER", 1, 1) * 20.0 + 1.0, 0.0)
        for tl in (0, 1, 2):
            m.set("TRACER", F, tl=tl, n=3)
    cold_start(m)
    return m


def explicit_step(m, robert):
    """one step by its phases, ice formed where the reference forms it (baroclinic.F90:1442-1450; step_mod.F90:1250-1273)"""
    m.time_manager(); m.dhdt(); m.baroclinic_driver(); m.barotropic_driver(); m.baroclinic_correct_adjust()
    if not robert:
        m.ice_formation(2)
    m.step_tail()
    if robert:            # the tail has rotated: what were curtime and newtime are oldtime and curtime now
        m.ice_formation(0); m.ice_formation(1)


def same_state(a, b, what, nt=2):
    for name, n in STATE + [("TRACER", n) for n in range(2, nt)]:
        for tl in (0, 1):
            assert np.array_equal(a.get(name, tl, n), b.get(name, tl, n)), "%s: %s n=%d tl=%d" % (what, name, n, tl)
    for name in ICE_FIELDS:
        assert np.array_equal(a.get(name), b.get(name)), "%s: %s" % (what, name)
    assert a.scalar("tlast_ice") == b.scalar("tlast_ice") and a.scalar("tlast_ice") > 0.0


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_step_forms_ice_where_the_reference_does(pkg, case):
    kw, nml, tuning = STEP_CASES[case]
    cfg_a, cfg_b = named_config("tiny", **kw), named_config("tiny", reset_to_freezing=0, **kw)
    assert cfg_a.reset_to_freezing == 1                        # liceform switches the clamp off (baroclinic.F90:1418)
    A = start(pkg, cfg_a, dict(nml, ice_freq_opt="coupled", licecesm2=1), tuning)
    B = start(pkg, cfg_b, dict(nml, ice_freq_opt="never"), tuning)
    twin = start(pkg, cfg_b, None, tuning, ice=False) if cfg_a.nt > 2 else None
    robert = cfg_a.tmix_opt == 3
    # work formed ahead (the KPP look-ahead, del4's first Laplacians for the next step) lives only between whole steps with no field
    # read in between: those two cases step A without looking and compare at the end
    uninterrupted = tuning is not None
    seen_avg = 0
    for s in range(4):
        A.step()
        seen_avg += A.dim("avg_ts")
        if twin is None:
            explicit_step(B, robert)
        else:                                                  # ice_formation touches no passive tracer
            B.time_manager(); B.dhdt(); B.baroclinic_driver(); B.barotropic_driver(); B.baroclinic_correct_adjust()
            before = [B.get("TRACER", 2, n) for n in (2, 3)]
            B.ice_formation(2)
            assert all(np.array_equal(before[i], B.get("TRACER", 2, 2 + i)) for i in (0, 1))
            B.step_tail()
        q = B.get("QICE")
        assert q.min() < 0.0 and (q < 0.0).sum() >= 50, "no ice formed in step %d" % (s + 1)
        if not uninterrupted or s == 3:
            same_state(A, B, "%s step %d" % (case, s + 1), cfg_a.nt)
        if twin is not None and s == 0:
            # the passive tracers of the first step are those of a run without ice: they were advanced before any ice formed.  (Later
            # steps differ: ice changes the density, and with it the velocities that carry the passive tracers.)
            twin.step()
            for n in (2, 3):
                assert np.array_equal(A.get("TRACER", 1, n), twin.get("TRACER", 1, n))
            assert A.get("TRACER", 1, 2).max() > 0.0 and A.get("TRACER", 1, 3).max() > 0.0
    dtt = A.scalar("dtt")
    if cfg_a.tmix_opt == 2:
        assert seen_avg >= 1 and A.scalar("tlast_ice") == sum(dtt * (0.5 if a else 1.0) for a in [0, 1] + ([0, 1] if case == "avgfit" else [0, 0]))
    else:
        assert seen_avg == 0 and A.scalar("tlast_ice") == 4 * dtt
    if case == "kpp-ahead":
        assert A.dim("kpp_ahead_used") >= 2                    # the look-ahead ran beside ice formation
    if case == "del4":
        assert A.dim("d2t_fused") == 1 and A.dim("d2t_last_formed") == 1
    # after a step every ghost cell holds its source cell's value
    # (cells beyond a closed boundary have no source cell: they are land)
    ocean = A.geti("KMT") > 0
    for name, n in (("TRACER", 0), ("TRACER", 1), ("RHO", 0)) + tuple((f, 0) for f in ICE_FIELDS):
        before = A.get(name, 1, n)
        A.halo_update(name, 1, n)
        after = A.get(name, 1, n)
        sel = ocean if before.ndim == 3 else np.broadcast_to(ocean[:, None], before.shape)
        assert np.array_equal(before[sel], after[sel]), name
    for m in (A, B, twin):
        if m is not None:
            m.close()


# ---- 3. the corrector's freeze clamp -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt,clamped", [("coupled", False), ("never", True)])
def test_freeze_clamp_is_off_with_liceform(pkg, opt, clamped):
    cfg = named_config("tiny", reset_to_freezing=1, tmix_opt=0)
    m = pkg.PopModel(cfg, grid=ice_grid(cfg))
    m.init_ice(ice_freq_opt=opt, licecesm2=1)
    cold_start(m, surface=-2.5)
    m.time_manager(); m.dhdt(); m.baroclinic_driver(); m.barotropic_driver()
    m.run_phase("correct")                                     # the corrector alone: no ice has formed yet
    phys = (slice(None), slice(2, -2), slice(2, -2))           # the corrector solves the physical cells; the tail fills the ghost cells
    t1 = m.get("TRACER", 2, 0)[:, 0][phys][m.geti("KMT")[phys] > 0]
    if clamped:
        assert t1.min() == -2.0 and (t1 == -2.0).sum() >= 100
    else:
        assert t1.min() < -2.3 and (t1 < -2.0).sum() >= 100
    m.close()


# ---- 4. the coupler's two entries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tmix_opt,halve", [(2, True), (3, True), (0, False)])
def test_flx_to_coupler_and_export_reset(pkg, tmix_opt, halve):
    cfg = named_config("tiny", tmix_opt=tmix_opt)
    m = pkg.PopModel(cfg, grid=ice_grid(cfg))
    m.init_ice(tfreeze_option=2)
    p = ice_ref.params(tfreeze_option=2)
    KMT, wet = m.geti("KMT"), wet_mask(m)
    TH1 = ice_ref.thickness(m.km, KMT)[:, 0]
    rng = np.random.default_rng(11)
    for tlast in (0.0, m.scalar("dtt")):
        if tlast:
            m.step()                                           # increment_tlast_ice: one step of time_weight 1
        assert m.scalar("tlast_ice") == tlast
        T1 = np.where(KMT > 0, rng.uniform(-2.4, -1.2, KMT.shape), 0.0)
        T = m.get("TRACER", 1, 0); T[:, 0] = T1
        AQ = np.where(KMT > 0, -rng.uniform(0.0, 50.0, KMT.shape) * (rng.random(KMT.shape) < 0.5), 0.0)
        m.set("TRACER", T, tl=1, n=0); m.set("AQICE", AQ)
        S1, PS = m.get("TRACER", 1, 1)[:, 0], m.get("PSURF", 1)
        m.ice_flx_to_coupler()
        a, q, f = ice_ref.flx_to_coupler(T1, S1, PS, KMT, AQ, TH1, tlast, halve, p)
        assert ((AQ < 0) & (KMT > 0)).sum() >= 100 and ((AQ == 0) & (q < 0)).sum() >= 100 and ((AQ == 0) & (q > 0)).sum() >= 100
        assert np.array_equal(m.get("AQICE"), a)
        close(m.get("QICE"), q, "QICE"); close(m.get("QFLUX"), f, "QFLUX") if tlast else None
        if not tlast:
            assert not m.get("QFLUX").any()
    qflux = m.get("QFLUX")
    assert np.abs(qflux).max() > 0.0
    m.ice_export_reset()
    assert m.scalar("tlast_ice") == 0.0 and not m.get("AQICE").any() and not m.get("QICE").any()
    assert np.array_equal(m.get("QFLUX"), qflux)
    m.close()


# ---- 5. restart ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,nml", [(dict(), dict(NML, lfw_as_salt_flx=0)), (dict(tmix_opt=3), NML)], ids=["avgfit-fw", "robert-salt"])
def test_exact_restart_with_ice(pkg, tmp_path, kw, nml):
    cfg = named_config("tiny", **kw)
    nml = dict(nml, ice_freq_opt="coupled", licecesm2=1)
    n1, n2 = 3, 3
    ref, a = start(pkg, cfg, nml), start(pkg, cfg, nml)
    for _ in range(n1 + n2):
        ref.step()
    for _ in range(n1):
        a.step()
    path = str(tmp_path / "restart.bin")
    a.write_restart(path)
    hdr = open(path + ".hdr").read()
    assert "&AQICE" in hdr and "tlast_ice:r8:" in hdr and hdr.index("&FW_FREEZE") < hdr.index("&AQICE") < hdr.index("&UVEL_CUR")
    b = start(pkg, cfg, nml)                                   # a fresh context that made the same init_ice call (and has the same forcing)
    b.read_restart(path)
    assert b.scalar("tlast_ice") == a.scalar("tlast_ice") > 0.0
    for name in ("AQICE", "FW_FREEZE"):
        assert np.array_equal(a.get(name), b.get(name)), name
    assert a.get("AQICE").min() < 0.0 and (nml["lfw_as_salt_flx"] or a.get("FW_FREEZE").min() < 0.0)
    for _ in range(n2):
        b.step()
    same_state(ref, b, "restart")
    for m in (ref, a, b):
        m.close()


PARENT_FIELDS = ["UBTROP_CUR", "UBTROP_OLD", "VBTROP_CUR", "VBTROP_OLD", "PSURF_CUR", "PSURF_OLD", "GRADPX_CUR", "GRADPX_OLD", "GRADPY_CUR",
                 "GRADPY_OLD", "PGUESS", "FW_OLD", "FW_FREEZE", "UVEL_CUR", "UVEL_OLD", "VVEL_CUR", "VVEL_OLD", "TEMP_CUR", "SALT_CUR",
                 "TEMP_OLD", "SALT_OLD"]


def test_restart_file_without_ice_is_unchanged(pkg, tmp_path):
    """A context that never calls init_ice writes the file it always wrote: the sections and attributes of the layout before ice
    formation, FW_FREEZE a record of zeros.  A context that made the call writes the same records, plus AQICE and tlast_ice."""
    cfg = named_config("tiny")
    files = []
    for i, ice in enumerate((False, False, True)):
        m = start(pkg, cfg, dict(NML), ice=ice)                # 'never': nobody forms ice, the three runs are the same run
        m.step(); m.step()
        dtt = m.scalar("dtt")
        path = str(tmp_path / ("r%d.bin" % i))
        m.write_restart(path)
        files.append((open(path, "rb").read(), open(path + ".hdr").read()))
        m.close()
    (d0, h0), (d1, h1), (d2, h2) = files
    assert d0 == d1 and h0 == h1
    names = [ln[1:] for ln in h0.splitlines() if ln.startswith("&")]
    assert names == ["GLOBAL"] + PARENT_FIELDS and "tlast_ice" not in h0 and "AQICE" not in h0
    rec = cfg.nx_global * cfg.ny_global * 8
    assert len(d0) == rec * (13 + 8 * cfg.km) and not any(d0[12 * rec:13 * rec])       # FW_FREEZE: record 13, zeros
    assert len(d2) == len(d0) + rec and d2[:13 * rec] == d0[:13 * rec] and d2[14 * rec:] == d0[13 * rec:] and not any(d2[13 * rec:14 * rec])
    lines0, lines2 = h0.splitlines(), h2.splitlines()
    assert [ln for ln in lines2 if ln.startswith("&")] == ["&GLOBAL"] + ["&" + n for n in PARENT_FIELDS[:13] + ["AQICE"] + PARENT_FIELDS[13:]]
    assert [ln for ln in lines2 if "tlast_ice" in ln] == ["tlast_ice:r8: %.17g" % (dtt * 1.0 + dtt * 0.5)]     # an Euler step and an averaging step
    g0 = lines0[:lines0.index("/")]
    assert [ln for ln in lines2[:lines2.index("/")] if "tlast_ice" not in ln] == g0
