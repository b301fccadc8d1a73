"""Passive tracers (nt = 3 .. 8) and ideal age on the GPU.

A1  phase by phase against the CPU oracle where it runs the all-tracer branch (lpressure_avg = 0): every scheme, nt = 3 .. 8.
A2  properties that need no oracle, bitwise after 4 steps: T, S, U, V, PSURF, RHO and the iteration counts are those of the nt = 2 run;
    tracer 5 (the launch of one) is tracer 3 (a slot of the pair launch); tracer 4, started at twice tracer 3, stays twice tracer 3.
A3  pressure averaging, the branch the oracle lacks: on a leapfrog step the stored right-hand side and the corrected tracer of a model
    with lpressure_avg = 1 are bitwise those of a model with lpressure_avg = 0 given the same PSURF(new) (baroclinic.F90:1303-1321
    against :1328-1344 with mixtime = oldtime).
A4  ideal age against the oracle with the module's source and reset emulated by the test between the oracle's phase calls.
A5  ideal age after the first step against a closed form (dense backward-Euler solve per column), independent of the oracle.
A6  restart: exact continuation, the names of the passive records, a file without them refused.
A7  refusals of pop_init_iage and of a tracer index >= nt.
Every case is the `tiny` configuration (48 x 40 in 16 blocks of 12 x 10), km = 16, 24 with KPP, 60 once for the register Thomas kernels."""
import numpy as np
import pytest

from common import TOL_LOCAL, TOL_SOLVE, interior
from orclib import Oracle
from parity import force_kpp_case
from popcfg import named_config
from passive_common import (DEL4, KPP, IageEmulation, NoDevice, SECONDS_IN_YEAR, closed_form_worst, copy_state, passive_field, passive_fields,
                            run_phases_nt, set_passive)

pytestmark = pytest.mark.gpu


def cfg_of(pkg, kw, **more):
    kw = dict(kw, **more)
    submeso = kw.pop("submeso", False)
    cfg = named_config("tiny", **kw)
    return pkg.submeso_config(cfg, submeso_diag=1) if submeso else cfg


def passive_stf(tlat, n):
    return 1.0e-2 * np.cos(tlat) * (2.0 if n == 3 else 1.0)


def start(pkg, cfg, orc, models, iage=()):
    """the oracle's state (force_kpp_case with KPP) and the passive fields A, 2 A, A, ... on the oracle and on every device model; with
    KPP a surface flux for every passive tracer that is not ideal age"""
    nt = cfg.nt
    if cfg.vmix_choice == 3:
        force_kpp_case(NoDevice(), orc)
    A = passive_field(orc.f3("TRACER", 1, 0).copy(), orc.i2("KMT"))
    F = {n: f for n, f in passive_fields(A, nt).items() if n + 1 not in iage}
    for m in models:
        copy_state(orc, m)
        for n in iage:
            m.init_iage(n)
    set_passive([orc] + list(models), F)
    if cfg.vmix_choice == 3:
        for n in F:
            s = passive_stf(orc.f2("TLAT"), n)
            orc.f2("STF", 1, n)[...] = s
            for m in models:
                m.set("STF", s, n=n)
    return A


A1 = [
    ("default", {}, 5, 4),
    ("upwind3", {"tadvect": 2}, 5, 4),
    ("lw_lim", {"tadvect": 3}, 5, 4),
    ("del4", DEL4, 5, 4),
    ("kpp", KPP, 5, 5),
    ("gm", {"hmix_tracer": 3}, 5, 4),
    ("gm-submeso-kpp", dict(KPP, hmix_tracer=3, submeso=True), 5, 4),
    ("robert", {"tmix_opt": 3}, 5, 5),
    ("avg", {"tmix_opt": 1, "time_mix_freq": 3}, 5, 4),
    ("stepped", {"stepped_bathymetry": 1}, 5, 4),
    ("pbc-del2", {"partial_bottom_cells": 1, "stepped_bathymetry": 1}, 5, 4),
    ("one-block", {"block_size_x": 48, "block_size_y": 40}, 5, 3),
    ("km60-stepped", {"km": 60, "stepped_bathymetry": 1}, 5, 3),
    ("nt3", {}, 3, 3),
    ("nt4", {}, 4, 3),
    ("nt8", {}, 8, 3),
    ("nt6", {}, 6, 3),                                                   # pair, pair
    ("nt7", {}, 7, 3),                                                   # pair, pair, the launch of one
    # without cancellation of the skew-flux terms the reference forms TZ of the tracers n > 2 inside hdifft_gm (hmix_gm.F90:1851-1852)
    ("gm-no-cancellation", {"hmix_tracer": 3, "ah_bolus": 0.4e7}, 5, 4),
]


@pytest.mark.parametrize("name,kw,nt,nsteps", A1, ids=[a[0] for a in A1])
def test_a1_all_tracer_branch_matches_oracle(pkg, orclib_built, name, kw, nt, nsteps):
    cfg = cfg_of(pkg, kw, nt=nt, lpressure_avg=0)
    gpu, orc = pkg.PopModel(cfg), Oracle(cfg)
    for n in range(2, nt):
        assert not gpu.get("TRACER", 1, n).any() and not gpu.get("STF", n=n).any() and not gpu.get("TFW", n=n).any()
    start(pkg, cfg, orc, [gpu])
    tol = TOL_LOCAL
    for s in range(1, nsteps + 1):
        run_phases_nt(gpu, orc, s, tol, nt)
        tol = TOL_SOLVE
    if cfg.hmix_tracer == 3:                                   # the per-tracer diagnostic tendencies are reachable by tracer index
        for n in range(2, nt):
            assert np.isfinite(gpu.get("GM_GTK", n=n)).all() and gpu.get("GM_GTK", n=n).any()
            if getattr(cfg, "lsubmesoscale_mixing", 0):
                assert np.isfinite(gpu.get("SUBM_ADV_TEND", n=n)).all()
    gpu.close(); orc.close()


A2 = [
    ("default", {}),
    ("upwind3", {"tadvect": 2}),
    ("lw_lim", {"tadvect": 3}),
    ("del4", DEL4),
    ("kpp", KPP),
    ("gm-kpp-upwind3", dict(KPP, hmix_tracer=3, tadvect=2)),
    ("robert", {"tmix_opt": 3}),
    ("avg", {"tmix_opt": 1, "time_mix_freq": 3}),
    # Gent-McWilliams without cancellation of the skew-flux terms (k_gm_flux_tile<R, false, false> / the stored stream function; with the
    # submeso scheme k_submeso_flux<false>)
    ("gm-no-cancellation", {"hmix_tracer": 3, "ah_bolus": 0.4e7}),
    ("gm-transition-layer-kpp-submeso", dict(KPP, hmix_tracer=3, gm_transition_layer=1, stepped_bathymetry=1, submeso=True)),
]


@pytest.mark.parametrize("name,kw", A2, ids=[a[0] for a in A2])
def test_a2_passive_linear_and_slot_independent(pkg, orclib_built, name, kw):
    """pressure averaging on (the default).  Zero exceptions: every comparison is np.array_equal."""
    cfg5, cfg2 = cfg_of(pkg, kw, nt=5), cfg_of(pkg, kw, nt=2)
    m5, m2, orc = pkg.PopModel(cfg5), pkg.PopModel(cfg2), Oracle(cfg5)     # the oracle only supplies the initial state
    assert cfg5.lpressure_avg == 1
    A = start(pkg, cfg5, orc, [m5])
    copy_state(orc, m2)
    orc.close()
    iters = {5: [], 2: []}
    for _ in range(4):
        for nt, m in ((5, m5), (2, m2)):
            m.step()
            iters[nt].append(m.solver_diagnostics()[0])
    assert iters[5] == iters[2]
    for tl in (0, 1):
        for f in ("UVEL", "VVEL", "RHO", "PSURF"):
            assert np.array_equal(m5.get(f, tl), m2.get(f, tl)), (f, tl)                      # P1
        for n in (0, 1):
            assert np.array_equal(m5.get("TRACER", tl, n), m2.get("TRACER", tl, n)), (n, tl)  # P1
        t3, t4, t5 = (m5.get("TRACER", tl, n) for n in (2, 3, 4))
        assert np.array_equal(t5, t3), tl                                                     # P2
        assert np.array_equal(t4, 2.0 * t3), tl                                               # P3
        assert np.isfinite(t3).all()
        assert not np.array_equal(interior(t3), interior(A)) and np.abs(interior(t3) - interior(A)).max() > 1e-6
        assert np.ptp(interior(t3)[:, 1]) > 0.0
    m5.close(); m2.close()


@pytest.mark.parametrize("pavg", [0, 1], ids=["all-tracer", "pavg"])
def test_a2_seven_tracers_slots_are_independent(pkg, orclib_built, pavg):
    """nt = 7, KPP + Gent-McWilliams: tracers 3, 5, 7 hold A (slot 0 of a pair, slot 0 of a pair, the launch of one) and stay equal to
    each other; tracers 4, 6 hold 2 A (slot 1 of either pair) and stay twice tracer 3.  Bitwise after 4 steps."""
    cfg = cfg_of(pkg, dict(KPP, hmix_tracer=3), nt=7, lpressure_avg=pavg)
    m, orc = pkg.PopModel(cfg), Oracle(cfg)
    A = start(pkg, cfg, orc, [m])
    mult = {2: 1.0, 3: 2.0, 4: 1.0, 5: 2.0, 6: 1.0}
    set_passive([m], {n: f * A for n, f in mult.items()})
    stf = passive_stf(orc.f2("TLAT"), 2)
    for n, f in mult.items():
        m.set("STF", f * stf, n=n)
    orc.close()
    for _ in range(4):
        m.step()
    for tl in (0, 1):
        t = {n: m.get("TRACER", tl, n) for n in mult}
        assert np.array_equal(t[4], t[2]) and np.array_equal(t[6], t[2]), tl
        assert np.array_equal(t[3], 2.0 * t[2]) and np.array_equal(t[5], 2.0 * t[2]), tl
        assert np.isfinite(t[2]).all() and np.abs(interior(t[2]) - interior(A)).max() > 1e-6 and np.ptp(interior(t[2])[:, 1]) > 0.0
    src = [m.get("KPP_SRC", n=n) for n in (2, 4, 6)]
    assert src[0].any() and np.array_equal(src[1], src[0]) and np.array_equal(src[2], src[0])
    m.close()


@pytest.mark.parametrize("name,kw", [("default", {}), ("kpp", KPP), ("gm", {"hmix_tracer": 3})], ids=["default", "kpp", "gm"])
def test_a3_pressure_averaging_branch_is_the_all_tracer_arithmetic(pkg, orclib_built, name, kw):
    cfg1, cfg0 = cfg_of(pkg, kw, nt=5, tmix_opt=0, lpressure_avg=1), cfg_of(pkg, kw, nt=5, tmix_opt=0, lpressure_avg=0)
    M1, M0, orc = pkg.PopModel(cfg1), pkg.PopModel(cfg0), Oracle(cfg0)
    start(pkg, cfg0, orc, [M1, M0])
    orc.close()
    passive = lambda m, tl: [m.get("TRACER", tl, n) for n in (2, 3, 4)]
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    M1.step(); M0.step()                                        # forward Euler: no pressure averaging in either
    for tl in (0, 1):
        assert same(passive(M1, tl), passive(M0, tl)), "Euler step, tl %d" % tl
    rhs = []
    for m in (M1, M0):
        m.time_manager(); m.dhdt(); m.baroclinic_driver()
        assert m.dim("leapfrogts") == 1
        rhs.append(passive(m, 2))
    assert same(rhs[0], rhs[1]), "the stored right-hand side carries the surface-pressure term of the predictor"
    assert not np.array_equal(M1.get("TRACER", 2, 0), M0.get("TRACER", 2, 0))      # T does differ: M1 has run the predictor
    M1.barotropic_driver()
    M0.set("PSURF", M1.get("PSURF", 2), tl=2)
    assert np.abs(M1.get("PSURF", 2) - M1.get("PSURF", 0)).max() > 0.0
    M1.baroclinic_correct_adjust(); M0.baroclinic_correct_adjust()
    new1, new0 = passive(M1, 2), passive(M0, 2)
    assert same(new1, new0)
    assert not any(np.array_equal(a, b) for a, b in zip(new1, rhs[0]))
    M1.close(); M0.close()


A4 = [("default", {}), ("kpp", KPP), ("upwind3", {"tadvect": 2}), ("robert", {"tmix_opt": 3})]


@pytest.mark.parametrize("name,kw", A4, ids=[a[0] for a in A4])
def test_a4_ideal_age_matches_oracle_with_the_module_emulated(pkg, orclib_built, name, kw):
    """tracer 3 ideal age, tracer 4 plain and started at 0: it must stay exactly 0 (neither the source nor the reset reaches the
    neighbour slot of the pair).  Adding the source to the finished right-hand side instead of into FT differs in the last bit:
    TOL_LOCAL * 10 for tracer 3 before the first solve, the factor run_phases uses elsewhere."""
    cfg = cfg_of(pkg, kw, nt=4, lpressure_avg=0)
    gpu, orc = pkg.PopModel(cfg), Oracle(cfg)
    start(pkg, cfg, orc, [gpu], iage=(3,))
    z = np.zeros_like(orc.f3("TRACER", 1, 3))
    set_passive([orc, gpu], {3: z})
    if cfg.vmix_choice == 3:
        orc.f2("STF", 1, 3)[...] = 0.0
        gpu.set("STF", np.zeros_like(orc.f2("STF", 1, 3)), n=3)
    em = IageEmulation(orc, 2, robert=(cfg.tmix_opt == 3))
    tol = TOL_LOCAL
    for s in range(1, 6):
        run_phases_nt(gpu, orc, s, tol, 4, emul=[em], tol_passive=tol * 10 if s == 1 else None)
        for tl in (0, 1):
            assert not gpu.get("TRACER", tl, 3).any(), "step %d: tracer 4 is no longer 0" % s
            assert not gpu.get("TRACER", tl, 2)[:, 0].any(), "step %d: ideal age at the surface" % s
        tol = TOL_SOLVE
    age = interior(gpu.get("TRACER", 1, 2))
    assert age.max() > 4.0 * 3600.0 / SECONDS_IN_YEAR           # five hourly steps below the surface level
    gpu.close(); orc.close()


@pytest.mark.parametrize("kpp", [False, True], ids=["const", "kpp"])
@pytest.mark.parametrize("pavg", [0, 1])
def test_a5_first_step_of_ideal_age_is_the_closed_form(pkg, orclib_built, kpp, pavg):
    """every interior ocean column of `tiny` with stepped bathymetry, levels 2 .. KMT, 1e-13 of the column's maximum"""
    cfg = cfg_of(pkg, KPP if kpp else {}, nt=3, tmix_opt=0, stepped_bathymetry=1, lpressure_avg=pavg)
    gpu, orc = pkg.PopModel(cfg), Oracle(cfg)                   # the oracle supplies force_kpp_case's state and the level thicknesses
    start(pkg, cfg, orc, [gpu], iage=(3,))
    gpu.time_manager(); gpu.dhdt(); gpu.baroclinic_driver(); gpu.barotropic_driver(); gpu.baroclinic_correct_adjust()
    age = gpu.get("TRACER", 2, 2)
    assert not age[:, 0].any()                                   # the reset
    worst, ncol = closed_form_worst(age, gpu.geti("KMT"), orc.v1("dz"), orc.v1("dzw"), gpu.get("VDC", n=1 if kpp else 0), gpu.get("PSURF", 2),
                                    float(orc.v1("dt")[1]))
    assert float(orc.v1("dt")[1]) == 86400.0 / cfg.steps_per_day
    print("columns %d, worst relative difference %.2e" % (ncol, worst))
    assert ncol > 1000 and worst <= 1e-13
    gpu.close(); orc.close()


@pytest.mark.parametrize("kw", [{}, {"tmix_opt": 3}], ids=["default", "robert"])
def test_a6_restart_continues_exactly(pkg, orclib_built, tmp_path, kw):
    cfg = cfg_of(pkg, kw, nt=4)

    def model():
        m, orc = pkg.PopModel(cfg), Oracle(cfg)
        start(pkg, cfg, orc, [m], iage=(3,))
        orc.close()
        return m
    a, b = model(), model()
    for _ in range(3):
        a.step()
    path = str(tmp_path / "r.bin")
    a.write_restart(path)
    sec, ids = None, {}
    for line in open(path + ".hdr"):
        line = line.strip()
        if line.startswith("&"):
            sec = line[1:]
        elif line.startswith("id:"):
            ids[sec] = int(line.split(":")[2])
    order = ["SALT_OLD", "IAGE_CUR", "TRACER04_CUR", "IAGE_OLD", "TRACER04_OLD"]
    assert [ids[n] for n in order] == [ids["SALT_OLD"] + k * cfg.km for k in range(5)], ids
    b.read_restart(path)
    for _ in range(3):
        a.step(); b.step()
    for tl in (0, 1):
        for n in range(4):
            assert np.array_equal(a.get("TRACER", tl, n), b.get("TRACER", tl, n)), (tl, n)
        for f in ("UVEL", "VVEL", "PSURF"):
            assert np.array_equal(a.get(f, tl), b.get(f, tl)), (tl, f)
    assert interior(a.get("TRACER", 1, 2)).max() > 0.0 and np.ptp(interior(a.get("TRACER", 1, 3))) > 0.0
    a.close(); b.close()
    # an nt = 2 file read into an nt = 4 context
    two = pkg.PopModel(cfg_of(pkg, kw, nt=2))
    two.step()
    p2 = str(tmp_path / "two.bin")
    two.write_restart(p2)
    two.close()
    four = pkg.PopModel(cfg)
    four.init_iage(3)
    with pytest.raises(pkg.PopError, match="could not find field in binary header file: IAGE_CUR"):
        four.read_restart(p2)
    four.close()


def test_a6_nt2_restart_file_has_no_new_records(pkg, tmp_path):
    """the header of an nt = 2 file ends with SALT_OLD as before, and its data file has the size of the 13 2-D and 8 3-D records"""
    import os
    cfg = named_config("tiny")
    m = pkg.PopModel(cfg)
    m.step()
    path = str(tmp_path / "r.bin")
    m.write_restart(path)
    m.close()
    secs = [l.strip()[1:] for l in open(path + ".hdr") if l.startswith("&")]
    assert secs[-1] == "SALT_OLD" and not any(s.startswith(("IAGE", "TRACER0")) for s in secs)
    assert os.path.getsize(path) == (13 + 8 * cfg.km) * cfg.nx_global * cfg.ny_global * 8


def test_a7_refusals_leave_the_context_usable(pkg):
    m = pkg.PopModel(named_config("tiny", nt=4))
    for bad in (2, 5):
        with pytest.raises(pkg.PopError, match="pop_init_iage: n is the 1-based number of a passive tracer, 3 .. nt = 4"):
            m.init_iage(bad)
    m.init_iage(3)
    with pytest.raises(pkg.PopError, match="tracer 3 is ideal age already"):
        m.init_iage(3)
    for f in ("TRACER", "STF", "TFW", "KPP_SRC"):
        with pytest.raises(pkg.PopError, match=f + ": tracer index 4 is outside 0 .. nt-1 = 3"):
            m.get(f, n=4)
        m.get(f, n=3)
    with pytest.raises(pkg.PopError, match="tracer index 4"):
        m.set("TRACER", m.get("TRACER", 1, 3), n=4)
    m.step()
    with pytest.raises(pkg.PopError, match="a step or a phase has already run"):
        m.init_iage(4)
    m.step()
    assert np.isfinite(m.get("TRACER", 1, 2)).all() and interior(m.get("TRACER", 1, 2)).max() > 0.0
    m.close()


def test_kpp_look_ahead_carries_the_passive_sources(pkg, orclib_built):
    """With the KPP look-ahead the coefficients of a step are formed beside the previous step's solver, into the second set of outputs;
    the bracket of the non-local source travels with that set and the passive sources are formed from it after the swap.  Whole steps
    with nothing read in between (a field access drops a look-ahead in flight): bitwise the run without the look-ahead, and the
    library's own count says steps did take their coefficients from it."""
    cfg = cfg_of(pkg, KPP, nt=5)
    runs = {}
    for ahead in (1, 0):
        m, orc = pkg.PopModel(cfg, tuning={"kpp_ahead": ahead}), Oracle(cfg)
        start(pkg, cfg, orc, [m])
        orc.close()
        for _ in range(5):
            m.step()
        used = m.dim("kpp_ahead_used")
        assert (used >= 2) if ahead else (used == 0), used
        runs[ahead] = [m.get("TRACER", 1, n) for n in range(5)] + [m.get("KPP_SRC", n=n) for n in range(5)]
        m.close()
    for a, b in zip(runs[1], runs[0]):
        assert np.array_equal(a, b)
    assert runs[1][7].any()                                      # KPP_SRC of tracer 3: the flux given in start() reaches it


GM_PATHS = [
    ("cancellation", {}, True),
    ("cancellation-submeso-kpp", dict(KPP, submeso=True), True),
    ("no-cancellation", {"ah_bolus": 0.4e7}, False),
    ("no-cancellation-submeso", {"ah_bolus": 0.4e7, "submeso": True}, False),
    ("transition-layer-kpp-submeso", dict(KPP, gm_transition_layer=1, stepped_bathymetry=1, submeso=True), False),
]


@pytest.mark.parametrize("name,kw,cancel", GM_PATHS, ids=[g[0] for g in GM_PATHS])
def test_gm_and_submeso_tendencies_of_a_passive_tracer_that_holds_temperature(pkg, orclib_built, name, kw, cancel):
    """Tracer 3 and tracer 5 hold T, tracer 4 holds 2 T.  On the first step (mixtime = curtime) the Gent-McWilliams tendency of a passive
    tracer, formed by the launches without the addition to VDC, is then bitwise that of T, in the cancellation branch, without cancellation
    and with the transition layer; so is the submeso tendency wherever the reference forms TZ of n > 2.  With cancellation it does not
    (hmix_gm.F90:1851-1852 lies in the other branch), TZ stays 0, the horizontal submeso fluxes of n > 2 vanish and the tendency differs
    from T's -- k_submeso_flux<TZ0 = true>; that it is the reference's number is what A1 'gm-submeso-kpp' checks against the oracle."""
    cfg = cfg_of(pkg, dict(kw, hmix_tracer=3), nt=5)
    m, orc = pkg.PopModel(cfg), Oracle(cfg)
    start(pkg, cfg, orc, [m])
    orc.close()
    for tl in (0, 1, 2):
        T = m.get("TRACER", tl, 0)
        for n, f in ((2, 1.0), (3, 2.0), (4, 1.0)):
            m.set("TRACER", f * T, tl=tl, n=n)
    m.time_manager(); m.dhdt(); m.baroclinic_driver()
    subm = bool(getattr(cfg, "lsubmesoscale_mixing", 0))
    g = [m.get("GM_GTK", n=n) for n in range(5)]
    assert g[0].any() and np.isfinite(g[0]).all()
    assert np.array_equal(g[4], g[2]) and np.array_equal(g[3], 2.0 * g[2])
    if subm:
        t = [m.get("SUBM_ADV_TEND", n=n) for n in range(5)]
        assert t[0].any() and np.array_equal(t[4], t[2]) and np.array_equal(t[3], 2.0 * t[2])
        if cancel:
            assert t[2].any() and not np.array_equal(t[2], t[0])
            # GM_GTK holds the sum of the two tendencies: taking the submeso part out again leaves the Gent-McWilliams part with the rounding
            # of the sum and of the difference on either side, four roundings of 2^-53 relative to the largest term at most
            scale = max(np.abs(x).max() for x in (g[0], g[2], t[0], t[2]))
            assert np.abs((g[2] - t[2]) - (g[0] - t[0])).max() <= 4.0 * 2.0 ** -53 * scale
        else:
            assert np.array_equal(t[2], t[0])
    if not (subm and cancel):
        assert np.array_equal(g[2], g[0])
    m.close()
