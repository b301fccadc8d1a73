"""The MOC accumulated on the device (pop_moc_*) against the NumPy restatement tests/moc_ref.py.  Base config 'tiny' (48 x 40 x 16 in
16 blocks of 12 x 10, land) on moc_ref.bent_grid: ULAT bent north of the equator, so that a row feeds several bins and a bin is fed
from several rows and blocks; region 2 is a sector with a boundary row, and a marginal sea belongs to neither region.

Against the restatement: U, V, DH and the stored bolus and submesoscale velocities are read after each pop_baroclinic_driver, every
term is formed in the reference's order of operations, the terms of a bin are added exactly, and pop_moc_get must lie within
(N + 8) 2^-53 sum|term| of that, N the number of non-zero terms of the entry over cells, bins up to n and steps (the boundary row of
region 2 included): the first-order bound of ANY order of summation, the bound of tests/test_gpu_diag.py; the 8 covers the rounded
weight of a step, 1 / tavg_sum and the scaling, dz * s and the addition of the boundary transport, the unit factor and the
restatement's own correctly rounded sums.  It is derived, not measured."""
import numpy as np
import pytest

import moc_ref
from common import STATE
from moc_ref import CASES, REG2
from popcfg import named_config

pytestmark = pytest.mark.gpu


def make(pkg, case, request=1, tuning=None):
    kw, sub, gkw, nml, two = CASES[case]
    cfg = named_config("tiny", **kw)
    if sub is not None:
        cfg = pkg.submeso_config(cfg, **sub)
    m = pkg.PopModel(cfg, grid=moc_ref.bent_grid(cfg, **gkw), tuning=tuning)
    wet = np.arange(1, m.km + 1)[None, :, None, None] <= m.geti("KMT")[:, None]
    rng = np.random.default_rng(5)                   # a seeded perturbation of the temperature, so that the flow starts at once
    for tl in (0, 1):
        T = m.get("TRACER", tl, 0)
        m.set("TRACER", np.where(wet, T + 0.05 * rng.standard_normal(T.shape), 0.0), tl=tl, n=0)
        m.halo_update("TRACER", tl, 0)
    T, U, KMT = moc_ref.latitudes(m)
    R = moc_ref.region_mask(KMT) if two else None
    m.init_transports(R, REG2 if two else (), **nml)
    if request:
        m.moc_request(request)
    edge, _ = m.lat_aux_grid()
    RM = moc_ref.region_masks(R if two else (KMT > 0).astype(np.int32), 2 if two else 1, REG2 if two else ())
    ref = dict(g=moc_ref.geometry(m), BIN=moc_ref.bin_map(T, edge), RM=RM, start=moc_ref.region_start(RM, T), KMT=KMT,
               n_lat=edge.size - 1, ncomp=moc_ref.n_moc_comp(cfg), steps=[], weights=[])
    return m, ref


def step(m, ref=None):
    """one step phase by phase; ref: the restatement reads its sources where the site is, at the end of pop_baroclinic_driver"""
    m.time_manager(); m.dhdt(); m.baroclinic_driver()
    if ref is not None:
        ref["steps"].append(moc_ref.step_terms(m, ref["g"], moc_ref.read_step(m), ref["ncomp"]))
        ref["weights"].append(m.scalar("dtt") * m.scalar("time_weight"))          # dtavg of tavg_set_flag: dtt, half of it when averaging
    m.barotropic_driver(); m.baroclinic_correct_adjust(); m.step_tail()


def restated(m, ref, stream=1):
    return moc_ref.entries(ref["steps"], ref["weights"], m.tavg_sums(stream)[0], ref["BIN"], ref["RM"], ref["start"], ref["g"]["dz"], ref["n_lat"])


def check(got, val, mag, cnt, what, factor=1):
    b = moc_ref.bound(mag, cnt) * factor
    err = np.abs(got.astype(np.longdouble) - val)
    w = np.unravel_index(np.argmax(np.where(b > 0, err / np.where(b > 0, b, 1), 0)), err.shape)        # the entry nearest its bound
    print("%-18s max|MOC| %.6e Sv  entry %s: MOC %.17e  |diff| %.3e  bound %.3e  terms %d  |diff| / bound %.3f" %
          (what, np.abs(got).max(), tuple(int(x) for x in w), got[w], err[w], b[w], cnt[w], float(err[w] / b[w])))
    assert np.all(err <= b), (what, w, got[w], val[w], err[w], b[w])
    assert np.all(got[mag == 0] == 0.0)              # nothing to add: exactly 0 (the first latitude of region 1, level km + 1, dry bins)
    assert np.all(got[:, -1] == 0.0) and np.all(got[0, :, :, 0] == 0.0)


# ---- 1. against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_matches_restatement(pkg, case):
    m, ref = make(pkg, case)
    for _ in range(3):
        step(m, ref)
    got = m.moc_get()
    inf = m.moc_info()
    assert got.shape == (inf["n_lat_aux_grid"] + 1, m.km + 1, ref["ncomp"], ref["RM"].shape[0]) and inf["n_moc_comp"] == ref["ncomp"]
    val, mag, cnt = restated(m, ref)
    check(got, val, mag, cnt, case)
    for c in range(ref["ncomp"]):                    # the errors above are not zero by construction: every component that is fed moves
        fed = not (case == "submeso_no_bolus" and c == 1)
        assert (np.abs(got[:, :, c, 0]).max() > 0.0) == fed, (case, c)     # region 1 holds the W terms alone
    if ref["RM"].shape[0] > 1:                       # region 2 carries its southern-boundary transport at every latitude
        assert np.abs(got[0, :-1, 0, 1]).max() > 0.0
    if case == "gm_bolus":
        assert np.any((ref["BIN"] == 0) & (ref["KMT"] > 0))
    m.close()


def test_land_elimination_active(pkg, monkeypatch):
    """the site runs beside kernels that skip land tiles: five steps with the stream off, then three that count"""
    monkeypatch.setenv("POP_LAND_SKIP", "1"); monkeypatch.setenv("POP_LAND_FULL_STEPS", "4")
    m, ref = make(pkg, "avgfit")
    m.tavg_on(1, False)
    for _ in range(5):
        m.step()
    assert m.tavg_sums(1)[0] == 0.0 and not m.moc_sums().any()
    m.tavg_on(1, True)
    for _ in range(3):
        step(m, ref)
        assert m.dim("land_skip_active") == 1
    check(m.moc_get(), *restated(m, ref), what="land elimination")
    m.close()


# ---- 2. the stream switched on for one step of three gives that step's MOC; the surface row closes --------------------------------
def test_one_step_of_three(pkg):
    m, ref = make(pkg, "avgfit")
    m.tavg_on(1, False); step(m)
    m.tavg_on(1, True); step(m, ref)
    DH = moc_ref.to_global(m, m.get("DH") * ref["g"]["TAREA"])         # DH stays as pop_dhdt left it until the next step
    m.tavg_on(1, False); step(m)
    assert m.tavg_sums(1)[0] == ref["weights"][0]
    got = m.moc_get()
    val, mag, cnt = restated(m, ref)
    check(got, val, mag, cnt, "one step of three")
    # closed boundaries: at the northern end the surface value of region 1 is the sum of DH * TAREA over its cells, all of them binned
    import math
    sel = (ref["RM"][0] == 1) & (ref["KMT"] > 0)
    assert np.all(ref["BIN"][sel] > 0)
    t = DH[sel]
    want, tol = math.fsum(t) * 1.0e-12, (np.count_nonzero(t) + 8) * moc_ref.U53 * math.fsum(np.abs(t)) * 1.0e-12
    print("surface closure: MOC %.17e  sum DH TAREA %.17e  |diff| %.3e  bound %.3e" % (got[-1, 0, 0, 0], want, abs(got[-1, 0, 0, 0] - want), tol))
    assert abs(got[-1, 0, 0, 0] - want) <= tol and want != 0.0
    m.close()


# ---- 3. bit-equal comparisons ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["avgfit", "gm_submeso"])
def test_step_equals_phases(pkg, case):
    a, _ = make(pkg, case)
    b, _ = make(pkg, case)
    for _ in range(3):
        a.step(); step(b)
        assert np.array_equal(a.moc_get(), b.moc_get()) and np.array_equal(a.moc_sums(), b.moc_sums())
    c, _ = make(pkg, case)                           # the site on its own: pop_run_phase
    for _ in range(3):
        c.tavg_on(1, False)
        c.time_manager(); c.dhdt(); c.baroclinic_driver()
        c.run_phase("tavg_moc")                      # the stream is off: nothing happens
        assert not c.moc_sums().any()
        c.barotropic_driver(); c.baroclinic_correct_adjust(); c.step_tail()
    m, _ = make(pkg, case, request=0)
    with pytest.raises(pkg.PopError, match="tavg_moc: pop_moc_request has not been called"):
        m.run_phase("tavg_moc")
    for x in (a, b, c, m):
        x.close()


def test_request_leaves_the_model_alone(pkg):
    a, _ = make(pkg, "gm_submeso")
    b, _ = make(pkg, "gm_submeso", request=0)
    for s in range(10):
        a.step(); b.step()
        assert a.solver_diagnostics() == b.solver_diagnostics(), s
    for name, n in STATE:
        for tl in (0, 1, 2):
            assert np.array_equal(a.get(name, tl, n), b.get(name, tl, n)), (name, tl)
    assert np.abs(a.moc_get()).max() > 0.0
    a.close(); b.close()


# ---- 4. properties -----------------------------------------------------------------------------------------------------------------
def test_no_flow_no_moc(pkg):
    m, _ = make(pkg, "avgfit")
    m.time_manager()
    for name in ("UVEL", "VVEL"):
        m.set(name, np.zeros((m.nblocks, m.km, m.nyb, m.nxb)), tl=1)
    m.set("DH", np.zeros((m.nblocks, m.nyb, m.nxb)))
    m.run_phase("tavg_moc")
    assert m.tavg_sums(1)[0] > 0.0 and not m.moc_get().any() and not m.moc_sums().any()
    m.close()


# ---- 5. stream and restart handling -------------------------------------------------------------------------------------------------
def test_reset_and_snapshot(pkg, tmp_path):
    m, _ = make(pkg, "avgfit")
    m.tavg_request(1, "SSH")                         # a slab entry in the same stream, so that the stream can be written
    with pytest.raises(pkg.PopError, match="MOC is not a slab field: it is requested with pop_moc_request"):
        m.tavg_request(1, "MOC")
    m.step(); m.step()
    with pytest.raises(pkg.PopError, match="pop_moc_get: no snapshot yet"):
        m.moc_get(snapshot=True)
    want = m.moc_get()
    assert np.abs(want).max() > 0.0 and m.moc_sums().any()
    m.tavg_write(1, str(tmp_path / "t.bin"))         # normalise, write, reset
    assert np.array_equal(m.moc_get(snapshot=True), want)
    assert m.tavg_sums(1)[0] == 0.0 and not m.moc_sums().any() and not m.moc_get(normalize=False).any()
    with pytest.raises(pkg.PopError, match="moc: cannot normalise: tavg_sum of stream 1 is 0"):
        m.moc_get()
    m.step()
    one = m.moc_get()
    assert np.abs(one).max() > 0.0 and np.array_equal(m.moc_get(snapshot=True), want)
    m.tavg_reset(1)
    assert not m.moc_sums().any()
    m.time_manager()
    for call in (lambda: m.tavg_reset(1), lambda: m.moc_sums(np.zeros(m.moc_sums().size))):
        with pytest.raises(pkg.PopError, match="refused between pop_time_manager and pop_step_tail"):
            call()
    m.close()


def test_sums_carried_over(pkg):
    """pop_moc_sums_get / _set: a run that hands its sums over after two steps stays within twice the bound of the restatement"""
    a, ref = make(pkg, "gm_submeso")
    b, _ = make(pkg, "gm_submeso")
    for _ in range(2):
        step(a, ref); b.step()
    s = b.moc_sums()
    assert np.array_equal(s, a.moc_sums())
    b.moc_sums(s)                                    # the device sums start from 0 again; the vector is added last
    assert np.array_equal(b.moc_sums(), s)
    step(a, ref); b.step()
    val, mag, cnt = restated(a, ref)
    check(a.moc_get(), val, mag, cnt, "uninterrupted")
    check(b.moc_get(), val, mag, cnt, "continued", factor=2)
    a.close(); b.close()
