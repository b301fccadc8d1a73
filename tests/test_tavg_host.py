"""Time-averaged output, host side: the tavg_sum bookkeeping of pop_time_manager on a host-only context for every time-mixing
option, the table of entries (rank, method, levels; the names left out), the refusals that need no device, and the reset / normalise
rules of the NumPy restatement (tests/tavg_ref.py) against small arrays written by hand."""
import numpy as np
import pytest

import tavg_ref
from popcfg import named_config


def host(pkg, **kw):
    return pkg.PopModel(named_config("tiny", **kw), host_only=True)


# tmix_opt: 0 leapfrog, 1 avg, 2 avgfit, 3 robert.  Steps 1 .. 8: which are averaging steps (time_management.F90:2139-2234)
@pytest.mark.parametrize("name,kw,avg_steps", [
    ("avgfit", dict(), {2}),                                     # tiny: time_mix_freq 17, the second step of the interval averages
    ("avgfit4", dict(time_mix_freq=4), {2, 4, 8}),
    ("avg", dict(tmix_opt=1, time_mix_freq=3), {3, 6}),
    ("leapfrog", dict(tmix_opt=0), set()),
    ("robert", dict(tmix_opt=3), set()),
])
def test_tavg_sum_bookkeeping(pkg, name, kw, avg_steps):
    m = host(pkg, **kw)
    dtt = m.scalar("dtt")
    m.tavg_request(1, ["TEMP", "SSH"])
    m.tavg_request(2, "TEMP_2")
    want = {1: 0.0, 2: 0.0, 3: 0.0}
    for step in range(1, 9):
        if step == 4:
            m.tavg_on(2, False)
        if step == 7:
            m.tavg_on(2, True)
        m.time_manager()
        w = 0.5 * dtt if step in avg_steps else dtt
        want[1] = want[1] + w
        if not 4 <= step < 7:
            want[2] = want[2] + w
        for ns in (1, 2, 3):
            assert m.tavg_sums(ns) == (want[ns], 0.0), (name, step, ns)
    m.tavg_reset(1)
    assert m.tavg_sums(1) == (0.0, 0.0) and m.tavg_sums(2)[0] == want[2]
    m.close()


def test_entry_table(pkg):
    m = host(pkg, nt=4)
    m.init_iage(3)
    km = m.km
    tab = tavg_ref.table(km, passive=("IAGE", "TRACER04"))
    assert len(tab) >= 80
    for name, (site, ndims, method, kmax, f) in tab.items():
        inf = m.tavg_info(name)
        assert inf == {"stream": 0, "ndims": ndims, "nlevels": kmax if ndims == 3 else 1, "method": method}, name
    for name in ("UVEL", "TEMP", "KE", "RHO", "VDC_T", "UISOP", "dTEMP_POS_3D", "IAGE", "TRACER04_SQR"):
        assert m.tavg_info(name)["ndims"] == 3 and m.tavg_info(name)["nlevels"] == km
    for name in ("SSH", "HBLT", "SST", "U1_8", "T1_8", "U1_1", "RHO_VINT", "dTEMP_NEG_2D", "IAGE_SURF", "SU", "QFLUX"):
        assert m.tavg_info(name)["ndims"] == 2 and m.tavg_info(name)["nlevels"] == 1
    assert [m.tavg_info(n)["method"] for n in ("TEMP_MAX", "TEMP_MIN", "XBLT", "TBLT", "XMXL", "TMXL_DR", "QFLUX")] == \
        ["max", "min", "max", "min", "max", "min", "qflux"]
    for name in tavg_ref.LEFT_OUT:
        with pytest.raises(pkg.PopError, match="known to the reference, not built"):
            m.tavg_info(name)
        with pytest.raises(pkg.PopError, match="known to the reference, not built"):
            m.tavg_request(1, name)
    m.tavg_request(3, "TEMP")
    assert m.tavg_info("TEMP")["stream"] == 3 and m.tavg_info("TEMP_2")["stream"] == 0
    m.close()


def test_refusals_without_a_device(pkg):
    m = host(pkg)
    for call, text in [
        (lambda: m.tavg_request(1, "NO_SUCH_FIELD"), "unknown tavg field NO_SUCH_FIELD"),
        (lambda: m.tavg_request(0, "TEMP"), "stream 0 is outside 1 .. 9"),
        (lambda: m.tavg_request(10, "TEMP"), "stream 10 is outside 1 .. 9"),
        (lambda: m.tavg_request(1, "HBLT"), "HBLT needs vmix_choice = 3 (kpp)"),
        (lambda: m.tavg_request(1, "HMXL"), "HMXL needs vmix_choice = 3 (kpp) with kpp_ml_diagnostics = 1"),
        (lambda: m.tavg_request(1, "KVMIX"), "KVMIX needs pop_init_tidal_mixing with ltidal_mixing and tidal_diag"),
        (lambda: m.tavg_request(1, "UISOP"), "UISOP needs hmix_tracer = 3 (gm) with gm_diag_bolus = 1"),
        (lambda: m.tavg_request(1, "USUBM"), "USUBM needs lsubmesoscale_mixing with submeso_diag = 1"),
        (lambda: m.tavg_request(1, "QFLUX"), "QFLUX needs pop_init_ice"),
        (lambda: m.tavg_request(1, "IAGE"), "unknown tavg field IAGE"),          # nt = 2: no passive tracer
        (lambda: m.tavg_request(1, "UET"), "UET is known to the reference, not built"),
        (lambda: m.tavg_on(12, True), "stream 12 is outside 1 .. 9"),
        (lambda: m.tavg_sums(0), "stream 0 is outside 1 .. 9"),
        (lambda: m.tavg_get("TEMP"), "host-only"),
    ]:
        with pytest.raises(pkg.PopError) as e:
            call()
        assert text in str(e.value), str(e.value)
    m.tavg_request(1, "TEMP")
    with pytest.raises(pkg.PopError, match="TEMP is already requested, in stream 1"):
        m.tavg_request(2, "TEMP")
    m.tavg_request(2, "TEMP_2")                               # the duplicate name is how a second stream holds the same quantity
    m.close()


def test_the_65th_entry_is_refused(pkg):
    m = host(pkg, nt=8)
    tab = tavg_ref.table(m.km, passive=["TRACER%02d" % n for n in range(3, 9)])
    names = [n for n, e in tab.items() if e[0] in ("forcing", "state", "tracer", "btrop") or n in ("VDC_T", "VDC_S", "VVC")]
    assert len(names) >= 65
    m.tavg_request(1, names[:64])
    with pytest.raises(pkg.PopError, match="more than POP_TAVG_MAX_FIELDS = 64 entries"):
        m.tavg_request(1, names[64])
    m.close()


def test_restatement_rules_by_hand():
    a = np.array([1.0, -2.0, 0.0, 3.0])
    assert tavg_ref.reset_value("avg") == 0.0 and tavg_ref.reset_value("qflux") == 0.0 and tavg_ref.reset_value("constant") == 0.0
    assert tavg_ref.reset_value("min") == 1.0e30 and tavg_ref.reset_value("max") == -1.0e30
    b = tavg_ref.accumulate(np.zeros(4), a, "avg", 3600.0)
    assert np.array_equal(b, [3600.0, -7200.0, 0.0, 10800.0])
    b = tavg_ref.accumulate(b, a, "avg", 1800.0)
    assert np.array_equal(b, [5400.0, -10800.0, 0.0, 16200.0])
    assert np.array_equal(tavg_ref.normalise(b, "avg", 5400.0), b * (1.0 / 5400.0))
    lo = tavg_ref.accumulate(np.full(4, 1.0e30), a, "min", 3600.0)
    hi = tavg_ref.accumulate(np.full(4, -1.0e30), a, "max", 3600.0)
    assert np.array_equal(lo, a) and np.array_equal(hi, a)
    lo = tavg_ref.accumulate(lo, np.array([2.0, -2.0, -1.0, 3.0]), "min", 3600.0)       # ties keep the buffer
    hi = tavg_ref.accumulate(hi, np.array([2.0, -2.0, -1.0, 3.0]), "max", 3600.0)
    assert np.array_equal(lo, [1.0, -2.0, -1.0, 3.0]) and np.array_equal(hi, [2.0, -2.0, 0.0, 3.0])
    assert np.array_equal(tavg_ref.normalise(lo, "min", 0.0), lo) and np.array_equal(tavg_ref.normalise(hi, "max", 0.0), hi)
    q = tavg_ref.accumulate(np.zeros(4), a, "qflux", 3600.0, const=7200.0)
    assert np.array_equal(q, [7200.0, 0.0, 0.0, 21600.0])
    assert np.array_equal(tavg_ref.normalise(q, "qflux", 1.0, 7200.0), q * (1.0 / 7200.0))
    assert np.array_equal(tavg_ref.accumulate(b, a, "constant", 3600.0), a)
    with pytest.raises(ZeroDivisionError):
        tavg_ref.normalise(b, "avg", 0.0)
    with pytest.raises(ZeroDivisionError):
        tavg_ref.normalise(q, "qflux", 5.0, 0.0)
