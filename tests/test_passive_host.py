"""Passive tracers and ideal age without a GPU: pop_init_iage on a host-only context (existence, argument refusals), the restart
names of the passive tracers, and the two CPU experiments on the oracle that the GPU tests of tests/test_gpu_passive.py lean on -- they
test the yardstick itself:

  1. with nt = 5 and the passive fields A, 2 A, A the oracle's all-tracer branch (lpressure_avg = 0) leaves T, S, U, V, PSURF, RHO and the
     solver's iteration counts bitwise what they are with nt = 2, tracer 5 bitwise tracer 3, and tracer 4 bitwise twice tracer 3;
  2. with the ideal-age source and reset emulated between the oracle's phase calls (passive_common.IageEmulation), the first step of
     every interior ocean column is the backward-Euler solve of passive_common.age_closed_form to 1e-13 of the column's maximum."""
import numpy as np
import pytest

from common import physical
from orclib import AsModel, Oracle
from parity import force_kpp_case
from popcfg import named_config
from passive_common import (IageEmulation, NoDevice, SCHEMES, TWINS, WITHOUT_LAST_PART, TWIN_IDS, TWIN_ROWS, assert_neighbour, assert_twin,
                            closed_form_worst, passive_field, passive_fields, set_passive, twin_row, twin_start)


def test_init_iage_on_a_host_only_context(pkg):
    """pop_init_iage is exported, works without a device, and refuses n outside 3 .. nt, a second call for the same n, and a call
    after a step has begun; the context stays usable after each refusal"""
    m = pkg.PopModel(named_config("tiny", nt=4), host_only=True)
    assert m.dim("nt") == 4
    for bad in (2, 5, 0, -1):
        with pytest.raises(pkg.PopError, match="pop_init_iage: n is the 1-based number of a passive tracer, 3 .. nt = 4"):
            m.init_iage(bad)
    m.init_iage(3)
    with pytest.raises(pkg.PopError, match="tracer 3 is ideal age already"):
        m.init_iage(3)
    m.init_iage(4)                                   # several tracers may each be ideal age
    assert m.dim("nt") == 4
    m.close()
    m = pkg.PopModel(named_config("tiny", nt=3), host_only=True)
    m.time_manager()
    with pytest.raises(pkg.PopError, match="a step or a phase has already run"):
        m.init_iage(3)
    m.close()
    m = pkg.PopModel(named_config("tiny"), host_only=True)          # nt = 2: there is no passive tracer
    with pytest.raises(pkg.PopError, match="3 .. nt = 2"):
        m.init_iage(3)
    m.close()


def test_nt_outside_2_to_8_is_refused(pkg):
    for nt in (1, 9):
        with pytest.raises(Exception, match=r"nt must be in \[2,8\]"):
            pkg.PopModel(named_config("tiny", nt=nt), host_only=True)


EXP1 = [
    ("default", {}),
    ("upwind3", {"tadvect": 2}),
    ("lw_lim", {"tadvect": 3}),
    ("del4", {"hmix_tracer": 4, "ah": -1.0e21}),
    ("kpp", {"vmix_choice": 3, "km": 24}),
    ("gm", {"hmix_tracer": 3}),
    ("robert", {"tmix_opt": 3}),
    ("avg", {"tmix_opt": 1, "time_mix_freq": 3}),
    ("gm-upwind3-kpp", {"hmix_tracer": 3, "tadvect": 2, "vmix_choice": 3, "km": 24}),
]


def _kpp_state(orc):
    force_kpp_case(NoDevice(), orc)
    stf = 1.0e-2 * np.cos(orc.f2("TLAT"))
    for n in range(2, orc.nt):
        orc.f2("STF", 1, n)[...] = stf * (2.0 if n == 3 else 1.0)


@pytest.mark.parametrize("name,kw", EXP1, ids=[e[0] for e in EXP1])
def test_oracle_passive_tracers_are_passive_linear_and_slot_independent(orclib_built, name, kw):
    """experiment 1"""
    runs = {}
    for nt in (5, 2):
        orc = Oracle(named_config("tiny", nt=nt, lpressure_avg=0, **kw))
        if nt == 5:
            A = passive_field(orc.f3("TRACER", 1, 0).copy(), orc.i2("KMT"))
        if kw.get("vmix_choice") == 3:
            _kpp_state(orc)
        if nt == 5:
            set_passive([orc], passive_fields(A, 5))
        iters = [orc.step() for _ in range(4)]
        runs[nt] = dict(iters=iters, PSURF=orc.f2("PSURF", 1).copy(),
                        **{f: orc.f3(f, 1).copy() for f in ("UVEL", "VVEL", "RHO")},
                        **{"T%d" % n: orc.f3("TRACER", 1, n).copy() for n in range(nt)})
        orc.close()
    a, b = runs[5], runs[2]
    assert a["iters"] == b["iters"]
    for f in ("PSURF", "UVEL", "VVEL", "RHO", "T0", "T1"):
        assert np.array_equal(a[f], b[f]), f                            # P1
    assert np.array_equal(a["T4"], a["T2"])                             # P2
    assert np.array_equal(a["T3"], 2.0 * a["T2"])                       # P3
    assert not np.array_equal(a["T2"][:, :, 2:-2, 2:-2], A[:, :, 2:-2, 2:-2])
    assert np.ptp(a["T2"][:, 1, 2:-2, 2:-2]) > 0.0


@pytest.mark.parametrize("kpp", [False, True], ids=["const", "kpp"])
@pytest.mark.parametrize("pavg", [0, 1])
def test_oracle_first_step_of_ideal_age_is_the_closed_form(orclib_built, kpp, pavg):
    """experiment 2"""
    kw = dict(vmix_choice=3, km=24) if kpp else {}
    orc = Oracle(named_config("tiny", nt=3, tmix_opt=0, stepped_bathymetry=1, lpressure_avg=pavg, **kw))
    if kpp:
        _kpp_state(orc)
        orc.f2("STF", 1, 2)[...] = 0.0                  # ideal age has no surface flux
    em = IageEmulation(orc, 2, robert=False)
    L = orc.L
    L.orc_time_manager(orc.h); L.orc_dhdt(orc.h); L.orc_baroclinic_driver(orc.h)
    em.after_driver()
    assert L.orc_barotropic_driver(orc.h) == 0
    L.orc_baroclinic_correct_adjust(orc.h)
    age = orc.f3("TRACER", 2, 2).copy()
    worst, ncol = closed_form_worst(age, orc.i2("KMT"), orc.v1("dz"), orc.v1("dzw"), orc.vdc(1 if kpp else 0), orc.f2("PSURF", 2),
                                    float(orc.v1("dt")[1]))
    assert float(orc.v1("dt")[1]) == 86400.0 / orc.cfg.steps_per_day
    print("columns %d, worst relative difference %.2e" % (ncol, worst))
    assert ncol > 1000 and worst <= 1e-13
    orc.close()


_S_WITHOUT = {}


def _twin_oracle_run(pkg, topology, scheme, nt, without_scheme, tidal_off=False):
    """five steps of a row on the oracle; returns S(cur) at the start and after 4 steps and the mask of the physical ocean cells.
    tidal_off: the row's configuration without the two init calls"""
    cfg, grid, tidal = twin_row(pkg, topology, scheme, nt=nt, without_scheme=without_scheme)
    orc = Oracle(cfg, grid=grid)
    twin_start(orc, [], scheme, tidal and not tidal_off)
    k = np.arange(orc.km)[None, :, None, None]
    ocean = physical(AsModel(orc))[:, None] & (k < orc.i2("KMT")[:, None])
    S0 = orc.f3("TRACER", 1, 1).copy()
    for s in range(1, 6):
        orc.step()
        if nt == 5:
            for n in TWINS:
                assert_twin(orc, n, "%s %s step %d" % (topology, scheme, s))
        if s == 4:
            S4 = orc.f3("TRACER", 1, 1).copy()
            if nt == 2:
                break
    if nt == 5:
        assert_neighbour(orc, "%s %s" % (topology, scheme))
    orc.close()
    return S0, S4, ocean


@pytest.mark.parametrize("topology,scheme", TWIN_ROWS, ids=TWIN_IDS)
def test_oracle_salinity_twin_stays_salinity(pkg, orclib_built, topology, scheme):
    """The yardstick of tests/test_gpu_passive_matrix.py B1, row by row: with lpressure_avg = 0 a passive tracer that starts as salinity
    and carries its STF and TFW stays salinity bit for bit on every cell, in a slot of the pair (tracer 3) and as the launch of one
    (tracer 5), over five steps.  So that this is not an equality of untouched fields: (a) every physical ocean cell of S has changed
    after four steps, and (b) where the row names a scheme, S after four steps differs from S of the same row without the scheme -- and,
    where the scheme has several parts, from S of the row without the last of them (passive_common.WITHOUT_LAST_PART)."""
    S0, S4, ocean = _twin_oracle_run(pkg, topology, scheme, 5, False)
    assert ocean.sum() > 1000
    same = (S4 == S0) & ocean
    assert not same.any(), "(a): %d of %d ocean cells of S unchanged after 4 steps" % (same.sum(), ocean.sum())
    if scheme != "default":
        key = (topology, SCHEMES[scheme].get("km"), SCHEMES[scheme].get("vmix_choice") == 3)
        if key not in _S_WITHOUT:
            _S_WITHOUT[key] = _twin_oracle_run(pkg, topology, scheme, 2, True)[1]
        assert not np.array_equal(S4, _S_WITHOUT[key]), "(b): the scheme leaves S as it is without it"
    if scheme in WITHOUT_LAST_PART:                  # (b) for the last part of a combined scheme: KPP + del4 against KPP, ...
        key = (topology, WITHOUT_LAST_PART[scheme])
        if key not in _S_WITHOUT:
            _S_WITHOUT[key] = _twin_oracle_run(pkg, topology, WITHOUT_LAST_PART[scheme], 2, False)[1]
        assert not np.array_equal(S4, _S_WITHOUT[key]), "(b): S is what it is with %s alone" % WITHOUT_LAST_PART[scheme]
    if scheme == "tidal-bckgrnd":                    # (b) against KPP with the uniform background of the same bckgrnd_vdc1 as well
        assert not np.array_equal(S4, _twin_oracle_run(pkg, topology, scheme, 2, False, tidal_off=True)[1])
