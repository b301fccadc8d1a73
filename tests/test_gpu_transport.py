"""The northward heat and salt transports accumulated on the device (pop_transport_*) against the NumPy restatement
tests/transport_ref.py.  Base config 'tiny' (48 x 40 x 16 in 16 blocks of 12 x 10, land) on moc_ref.bent_grid with the cases of
moc_ref.CASES: ULAT bent north of the equator, region 2 a sector with a boundary row, a marginal sea in neither region.  Both tracers
carry a seeded perturbation.

1. the per-column fields against the restatement of the reference's formulas, every physical cell, within a first-order rounding
   bound whose operation count is written beside each formula of transport_ref.py;
2. binning and finish against exact sums of the device's own column fields, within moc_ref.bound; masked entries exactly undefined_nf;
3. what a northward transport is: on the 'full' grid the advective and diffusive components are the fluxes through the north faces;
4. closure: flux forms with closed boundaries sum to nothing, for every advection and mixing scheme and for a closed region 2;
5. the house rules of tests/test_gpu_moc.py."""
import math

import numpy as np
import pytest

import moc_ref
import transport_ref as tr
from common import STATE
from moc_ref import CASES, U53, to_global
from transport_ref import UNDEFINED_NF, check, make, step

pytestmark = pytest.mark.gpu
GM = dict(hmix_tracer=3, ah=0.8e7, gm_diag_bolus=1)


def both(m, **kw):
    return [m.transport_get(t, **kw) for t in (1, 2)]


def drive(m):
    """the first half of a step: the column fields of the site are those of this step afterwards"""
    m.time_manager(); m.dhdt(); m.baroclinic_driver()


def finish(m):
    m.barotropic_driver(); m.baroclinic_correct_adjust(); m.step_tail()


# ---- 1. column fields against the restatement ------------------------------------------------------------------------------------
def column_check(m, name, n, want, scale, ops, what):
    """every physical cell within ops 2^-53 scale: ops the rounding operations on the longest path of the formula (counted beside each
    formula of transport_ref.py), scale the sum of the magnitudes of the terms the formula adds"""
    got, want, scale = to_global(m, m.get(name, 1, n)), to_global(m, want), to_global(m, scale)
    err, b = np.abs(got - want), ops * U53 * scale
    w = np.unravel_index(np.argmax(np.where(b > 0, err / np.where(b > 0, b, 1), 0)), err.shape)
    print("%-12s %-14s n %d  max|x| %.6e  cell %s: x %.17e  |diff| %.3e  bound %.3e  |diff| / bound %.3f  (sum|terms| / |x| there %.1e)" %
          (what, name, n, np.abs(got).max(), tuple(int(x) for x in w), got[w], err[w], b[w], float(err[w] / b[w]) if b[w] > 0 else 0.0,
           scale[w] / max(abs(got[w]), 1e-300)))
    assert np.all(err <= b), (what, name, n, w, got[w], want[w], err[w], b[w])
    assert np.all(got[scale == 0] == 0.0)
    return np.abs(got).max()


@pytest.mark.parametrize("case", ["avgfit", "kpp_robert"])
def test_columns_centred_del2(pkg, case):
    m, _ = make(pkg, case)
    g, km = tr.geometry(m), m.km
    for s in range(3):                               # Euler, averaging / leapfrog, leapfrog: the mix time moves
        drive(m)
        st = tr.read_step(m)
        for n in (0, 1):
            (ADV, VNF), (aA, aV) = tr.centered_column(g, st, n, km), tr.centered_column(g, st, n, km, mag=True)
            HD, aH = tr.del2_column(g, st, n, km, m.cfg.ah), tr.del2_column(g, st, n, km, m.cfg.ah, mag=True)
            big = [column_check(m, "TRN_ADV", n, ADV, aA, 14 + 2 * km, case), column_check(m, "TRN_VNF", n, VNF, aV, 6 + km, case),
                   column_check(m, "TRN_HDIF", n, HD, aH, 10 + km, case)]
            assert big[2] > 0.0 and (s == 0 or min(big) > 0.0)       # not a comparison of zeros (the first step starts from rest)
        finish(m)
    with pytest.raises(pkg.PopError, match="unknown field TRN_ADV_ISOP"):
        m.get("TRN_ADV_ISOP", 1, 0)
    m.close()


@pytest.mark.parametrize("case", ["gm_bolus", "gm_submeso"])
def test_columns_eddy_and_submeso(pkg, case):
    m, _ = make(pkg, case)
    g, km = tr.geometry(m), m.km
    big = {}
    for s in range(3):
        drive(m)
        st = tr.read_step(m)
        for kind in ("ISOP",) + (("SUBM",) if case == "gm_submeso" else ()):
            U, V = st["U" + kind], st["V" + kind]
            for n in (0, 1):
                (A, F), (aA, aF) = tr.eddy_column(g, U, V, st["TMIX"][n], km), tr.eddy_column(g, U, V, st["TMIX"][n], km, mag=True)
                big[kind, n] = (column_check(m, "TRN_ADV_" + kind, n, A, aA, 8 + km, case), column_check(m, "TRN_VNF_" + kind, n, F, aF, 6 + km, case))
        finish(m)
    assert all(min(v) > 0.0 for v in big.values()), big       # by the last step every velocity moves
    m.close()


# ---- 2. binning and finish against exact sums of the device's own column fields --------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_binning_and_finish(pkg, case):
    m, ref = make(pkg, case)
    for _ in range(3):
        step(m, ref)
    inf = m.transport_info()
    assert inf["n_transport_comp"] == ref["ncomp"] and inf["n_transport_reg"] == ref["RM"].shape[0]
    masked = tr.masked_entries(ref["MASK"], ref["ncomp"])
    for t, got in zip((1, 2), both(m)):
        check(got, ref, t, m.tavg_sums(1)[0], case)
        for c in range(ref["ncomp"]):                # the errors are not zero by construction: every component that is fed moves
            fed = not (c == 3 and case == "submeso_no_bolus")
            assert (np.abs(np.where(masked, 0, got)[:, c, 0]).max() > 0.0) == fed, (case, t, c)
        if ref["RM"].shape[0] > 1:                   # region 2 carries its southern-boundary transport at its first unmasked latitude
            assert masked[:, 0, 1].all() and masked[:, 2, 1].all() and not masked[:, 1, 1].all()
    assert masked.any() and not masked[:, :, 0].all()
    m.close()


# ---- 3. what a northward transport is ------------------------------------------------------------------------------------------------
def test_full_grid_face_fluxes(pkg):
    """'full' grid, bins = rows, one region (all ocean; with moc_ref.region_mask the marginal sea would be a hole in region 1 through
    whose sides tracer leaves): component 2 at edge n is the advective flux through the north faces of row n - 1, component 3 minus the
    del2 face term there.  Tolerance: 1e-12 of the sum of the magnitudes of the face terms the identity adds -- the transport at edge n
    is the sum of the divergences of every cell of rows 1 .. n - 1, so these are the terms of ALL faces (east, west, north, south, top,
    bottom) of those cells, which cancel pairwise in exact arithmetic, and not the north faces of row n - 1 alone: the rounding error
    of a cancelling pair is relative to the pair, not to what is left.  transport_ref's magnitude mode gives that sum per column."""
    m, ref = make(pkg, "full", two_regions=False)
    g, km = tr.geometry(m), m.km
    assert np.array_equal(ref["BIN"], np.where(ref["BIN"] > 0, np.arange(1, 41)[:, None], 0)) and ref["n_lat"] == 40
    TAREA = ref["TAREA"]
    adv, dif, madv, mdif = np.zeros((2, 41)), np.zeros((2, 41)), np.zeros((2, 41)), np.zeros((2, 41))
    wsum = 0.0
    for s in range(3):
        drive(m)
        st = tr.read_step(m)
        w = m.scalar("dtt") * m.scalar("time_weight")
        wsum += w
        for n in (0, 1):
            _, VNF = tr.centered_column(g, st, n, km)
            aA, _ = tr.centered_column(g, st, n, km, mag=True)
            # del2 north-face term ah CN (T_north - T) dz TAREA, CN = DTN where both cells are wet (hmix_del2.F90:1064)
            TM, face = st["TMIX"][n], np.zeros_like(TAREA)
            for k in range(1, km + 1):
                CN = np.where((k <= g["KMTN"]) & (k <= g["KMT"]), g["DTN"], 0.0)
                face = face + g["dz"][k] * (m.cfg.ah * CN * (moc_ref._sh(TM[:, k - 1], 0, 1) - TM[:, k - 1])) * TAREA
            aH = tr.del2_column(g, st, n, km, m.cfg.ah, mag=True)
            adv[n, 1:] += w * to_global(m, VNF).sum(axis=1); dif[n, 1:] += w * -to_global(m, face).sum(axis=1)
            madv[n, 1:] += w * np.cumsum(to_global(m, aA * TAREA).sum(axis=1)); mdif[n, 1:] += w * np.cumsum(to_global(m, aH * TAREA).sum(axis=1))
        finish(m)
    assert wsum == m.tavg_sums(1)[0]
    masked = tr.masked_entries(ref["MASK"], ref["ncomp"])
    for n, got in enumerate(both(m)):
        f = (1.0e-19 / tr.HFLUX_FACTOR if n == 0 else 1.0) / wsum
        for c, want, mag in ((1, adv[n] * f, madv[n] * f), (2, dif[n] * f, mdif[n] * f)):
            ok = ~masked[:, c, 0]
            err, tol = np.abs(got[ok, c, 0] - want[ok]), 1.0e-12 * mag[ok]
            print("full grid tracer %d component %d: max|TR| %.6e  max |diff| %.3e  max |diff| / (1e-12 sum|face terms|) %.3e" %
                  (n + 1, c + 1, np.abs(got[ok, c, 0]).max(), err.max(), (err / np.where(tol > 0, tol, 1)).max()))
            assert np.all(err <= tol) and np.abs(want[ok]).max() > 0.0 and np.count_nonzero(ok) > 20
    m.close()


# ---- 4. closure ------------------------------------------------------------------------------------------------------------------------
def last_unmasked(masked, c, r):
    return int(np.nonzero(~masked[:, c, r])[0][-1])


def face_scales(m, ref, g, st, n):
    """sum over the cells of each region of TAREA * (the sum of the magnitudes of the centred face-flux terms of the column), per
    advective component 2, 4, 5 (0-based 1, 3, 4); None where the configuration has no such velocity"""
    km = m.km
    cols = {1: tr.centered_column(g, st, n, km, mag=True)}
    if "UISOP" in st:
        cols[3] = tr.eddy_column(g, st["UISOP"], st["VISOP"], st["TMIX"][n], km, mag=True)
    if "USUBM" in st:
        cols[4] = tr.eddy_column(g, st["USUBM"], st["VSUBM"], st["TMIX"][n], km, mag=True)
    out = {}
    for c, (aA, aF) in cols.items():
        A, F = to_global(m, aA * ref["TAREA"]), to_global(m, aF)
        out[c] = [float(A[(ref["RM"][r] == 1) & (ref["BIN"] > 0)].sum()) for r in range(ref["RM"].shape[0])]
        if ref["RM"].shape[0] > 1:
            j = ref["start"][1]
            out[c][1] += float(F[j - 1, ref["RM"][1][j] == 1].sum())
    return out


@pytest.mark.parametrize("name,case,extra", [
    ("centred", "avgfit", {}), ("upwind3", "avgfit", dict(tadvect=2)), ("lw_lim", "avgfit", dict(tadvect=3)),
    ("del4", "avgfit", dict(hmix_tracer=4, ah=-1.0e21)), ("gm", "avgfit", GM), ("gm_submeso", "gm_submeso", {})])
def test_closure_region_1(pkg, name, case, extra):
    """one region = every ocean cell, all of them binned ('southern'), closed boundaries: at the last unmasked edge components 2, 3, 4,
    5 are 0 within 1e-12 of the sum of the magnitudes of the face fluxes.  Advective components: the centred face-flux terms of the
    step's velocities and tracers (transport_ref's magnitude mode; for upwind3 and lw_lim the face values differ from the centred
    means by a tracer difference, which does not change a magnitude).  Component 3: del2's face terms with del2; for del4 and
    Gent-McWilliams, whose face fluxes the restatement does not form, the sum over the cells of |HDIF| TAREA, which is no larger than
    the sum of the face magnitudes, so the check asks no less."""
    m, ref = make(pkg, case, cfg_extra=extra, two_regions=False)
    g, km = tr.geometry(m), m.km
    assert np.all(ref["BIN"][ref["KMT"] > 0] > 0)
    scale = [dict(), dict()]
    wsum = 0.0
    for s in range(3):
        drive(m)
        st = tr.read_step(m)
        w = m.scalar("dtt") * m.scalar("time_weight")
        wsum += w
        for n in (0, 1):
            fs = face_scales(m, ref, g, st, n)
            for c, v in fs.items():
                scale[n][c] = scale[n].get(c, 0.0) + w * v[0]
            if name in ("centred", "upwind3", "lw_lim"):
                h = to_global(m, tr.del2_column(g, st, n, km, m.cfg.ah, mag=True) * ref["TAREA"])
            else:
                h = np.abs(to_global(m, m.get("TRN_HDIF", 1, n) * ref["TAREA"]))
            scale[n][2] = scale[n].get(2, 0.0) + w * float(h[ref["KMT"] > 0].sum())
            if name == "centred" and s == 2:         # the restatement alone stays inside the bound (CPU arithmetic, same data)
                ADV, _ = tr.centered_column(g, st, n, km)
                tot = math.fsum(to_global(m, -(ADV * ref["TAREA"]))[ref["KMT"] > 0])
                print("restatement, centred, tracer %d: sum -ADV TAREA %.3e  1e-12 sum|face terms| %.3e" % (n + 1, tot, 1.0e-12 * fs[1][0]))
                assert abs(tot) <= 1.0e-12 * fs[1][0]
        finish(m)
    masked = tr.masked_entries(ref["MASK"], ref["ncomp"])
    for n, got in enumerate(both(m)):
        f = (1.0e-19 / tr.HFLUX_FACTOR if n == 0 else 1.0) / wsum
        e = last_unmasked(masked, 1, 0)
        for c in range(1, ref["ncomp"]):
            if c not in scale[n]:                    # component 4 without gm_diag_bolus: exactly 0
                assert not got[~masked[:, c, 0], c, 0].any()
                continue
            tol = 1.0e-12 * scale[n][c] * f
            print("closure %-10s tracer %d component %d: last edge %.3e  max|TR| %.3e  1e-12 sum|face fluxes| %.3e  ratio %.3e" %
                  (name, n + 1, c + 1, got[e, c, 0], np.abs(got[~masked[:, c, 0], c, 0]).max(), tol, abs(got[e, c, 0]) / tol))
            assert abs(got[e, c, 0]) <= tol and np.abs(got[~masked[:, c, 0], c, 0]).max() > 1.0e3 * tol
    m.close()


@pytest.mark.parametrize("name,case,extra", [("centred", "avgfit", {}), ("upwind3", "avgfit", dict(tadvect=2)), ("gm_submeso", "gm_submeso", {})])
def test_closure_region_2(pkg, name, case, extra):
    """region 2 closed by land on its west and east sides (transport_ref.make(walls=True), TEST DATA): what enters through the
    southern boundary row (VNF) is what the cells of the region take up (ADV), so the last unmasked edge of components 2, 4, 5 of
    region 2 is 0 within 1e-12 of the sum of the magnitudes of the face fluxes -- the same bound for centred and upwind3"""
    m, ref = make(pkg, case, cfg_extra=extra, walls=True)
    g = tr.geometry(m)
    sector = ref["RM"][1] == 1
    assert sector.any() and not sector[:, 0].any() and not sector[:, 11].any() and not (ref["KMT"][10:, [0, 11]] > 0).any()
    scale = [dict(), dict()]
    wsum = 0.0
    for s in range(3):
        drive(m)
        st = tr.read_step(m)
        w = m.scalar("dtt") * m.scalar("time_weight")
        wsum += w
        for n in (0, 1):
            for c, v in face_scales(m, ref, g, st, n).items():
                scale[n][c] = scale[n].get(c, 0.0) + w * v[1]
        finish(m)
    masked = tr.masked_entries(ref["MASK"], ref["ncomp"])
    for n, got in enumerate(both(m)):
        f = (1.0e-19 / tr.HFLUX_FACTOR if n == 0 else 1.0) / wsum
        for c in sorted(scale[n]):
            e, first = last_unmasked(masked, c, 1), int(np.nonzero(~masked[:, c, 1])[0][0])
            tol = 1.0e-12 * scale[n][c] * f
            print("closure of region 2 %-10s tracer %d component %d: boundary transport %.3e  last edge %.3e  1e-12 sum|face fluxes| %.3e  ratio %.3e" %
                  (name, n + 1, c + 1, got[first, c, 1], got[e, c, 1], tol, abs(got[e, c, 1]) / tol))
            assert abs(got[e, c, 1]) <= tol and abs(got[first, c, 1]) > 1.0e3 * tol
    m.close()


# ---- 5. house rules ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["avgfit", "gm_submeso"])
def test_step_equals_phases(pkg, case):
    a, _ = make(pkg, case)
    b, _ = make(pkg, case)
    for _ in range(3):
        a.step(); step(b)
        assert all(np.array_equal(x, y) for x, y in zip(both(a), both(b))) and np.array_equal(a.transport_sums(), b.transport_sums())
    assert a.transport_sums().any()
    c, _ = make(pkg, case)                           # the site on its own: pop_run_phase
    c.tavg_on(1, False)
    drive(c)
    c.run_phase("tavg_transport")                    # the stream is off: nothing happens
    assert not c.transport_sums().any()
    finish(c)
    c.tavg_on(1, True)
    drive(c)
    one = c.transport_sums()
    c.run_phase("tavg_transport")                    # the same step once more: the same sums added again
    assert one.any() and np.array_equal(c.transport_sums(), one + one)
    with pytest.raises(pkg.PopError, match="pop_transport_request: refused between pop_time_manager and pop_step_tail"):
        c.transport_request(2)
    finish(c)
    m, _ = make(pkg, case, request=0)
    with pytest.raises(pkg.PopError, match="tavg_transport: pop_transport_request has not been called"):
        m.run_phase("tavg_transport")
    with pytest.raises(pkg.PopError, match="pop_transport_get: pop_transport_request has not been called"):
        m.transport_get(1)
    for x in (a, b, c, m):
        x.close()


@pytest.mark.parametrize("tuning", [None, {"tracer_lds": 0}])
def test_request_leaves_the_model_alone(pkg, tuning):
    """default plan (the LDS tracer kernel runs the step, the generic kernel the diagnostic) and the generic kernel for both"""
    a, _ = make(pkg, "avgfit", tuning=tuning)
    b, _ = make(pkg, "avgfit", request=0, tuning=tuning)
    assert a.dim("form_tracer_lds_rows") == (4 if tuning is None else 0)
    for s in range(10):
        a.step(); b.step()
        assert a.solver_diagnostics() == b.solver_diagnostics(), s
    for name, n in STATE:
        for tl in (0, 1, 2):
            assert np.array_equal(a.get(name, tl, n), b.get(name, tl, n)), (name, tl)
    masked = a.transport_get(1) == UNDEFINED_NF
    assert np.abs(np.where(masked, 0, a.transport_get(1))).max() > 0.0
    a.close(); b.close()


def test_generic_and_lds_steps_give_the_same_transports(pkg):
    """the diagnostic launch takes the arguments of the step's kernel, whichever form ran"""
    a, _ = make(pkg, "avgfit")
    b, _ = make(pkg, "avgfit", tuning={"tracer_lds": 0})
    for _ in range(3):
        a.step(); b.step()
    assert all(np.array_equal(x, y) for x, y in zip(both(a), both(b))) and np.array_equal(a.transport_sums(), b.transport_sums())
    a.close(); b.close()


def test_one_step_of_three_and_one_tracer(pkg):
    m, ref = make(pkg, "avgfit", heat=False)
    m.tavg_on(1, False); step(m)
    m.tavg_on(1, True); step(m, ref)
    m.tavg_on(1, False); step(m)
    assert m.tavg_sums(1)[0] == ref["weights"][0]
    check(m.transport_get("salt"), ref, 2, m.tavg_sums(1)[0], "one step of three")
    with pytest.raises(pkg.PopError, match="pop_transport_get: tracer 1 \\(heat\\) or 2 \\(salt\\), as pop_transport_request asked for"):
        m.transport_get("heat")
    s = m.transport_sums().reshape(-1)
    nb = ref["n_lat"] * 2 * 4 * 2
    assert not s[:nb].reshape(ref["n_lat"], 2, 8)[:, 0].any() and s[:nb].reshape(ref["n_lat"], 2, 8)[:, 1].any() and not s[nb:nb + 3].any()
    m.close()


def test_no_flow_uniform_tracers(pkg):
    """no flow: the advective terms and the boundary fluxes are exactly 0, whatever the tracers.  The mixing of a uniform tracer is 0
    only to rounding, in the reference as here: del2 forms CC T + CN T_n + ... with CC = -(CN + CS + CE + CW) rounded, so the column
    term stays within the rounding bound of the formula, (10 + km) 2^-53 of the sum of the magnitudes of its terms."""
    m, ref = make(pkg, "avgfit")
    m.time_manager()
    for name in ("UVEL", "VVEL"):
        m.set(name, np.zeros((m.nblocks, m.km, m.nyb, m.nxb)), tl=1)
    m.set("DH", np.zeros((m.nblocks, m.nyb, m.nxb)))
    wet = np.arange(1, m.km + 1)[None, :, None, None] <= m.geti("KMT")[:, None]
    for n, v in ((0, 4.0), (1, 0.035)):
        for tl in (0, 1):
            m.set("TRACER", np.where(wet, v, 0.0), tl=tl, n=n)
    m.run_phase("tavg_transport")
    assert m.tavg_sums(1)[0] > 0.0
    g, st = tr.geometry(m), tr.read_step(m)
    for n in (0, 1):
        for name in ("TRN_ADV", "TRN_VNF"):
            assert not m.get(name, 1, n).any()
        aH = tr.del2_column(g, st, n, m.km, m.cfg.ah, mag=True)
        assert np.all(np.abs(m.get("TRN_HDIF", 1, n)) <= (10 + m.km) * U53 * aH)
    nb = ref["n_lat"] * 2 * 4 * 2
    s = m.transport_sums()
    bins = s[:nb].reshape(ref["n_lat"], 2, 4, 2)
    assert not bins[:, :, 0].any() and not bins[:, :, 2:].any() and not s[nb:].any()
    # the getter: component 2 exactly 0; component 3 (and the total, 2 + 3) within the bound of its terms: per cell and step the
    # formula's (10 + km) 2^-53 TAREA sum|terms|, added over the bins up to the edge (+ 8 as moc_ref.bound), scaled as the getter does
    masked = tr.masked_entries(ref["MASK"], ref["ncomp"])
    for n, got in enumerate(both(m)):                # one step: tavg_sum is its weight, so the normalised value is the plain sum
        assert not got[:, 1][~masked[:, 1]].any()
        aH = to_global(m, tr.del2_column(g, st, n, m.km, m.cfg.ah, mag=True) * ref["TAREA"])
        f = (1.0e-19 / tr.HFLUX_FACTOR if n == 0 else 1.0)
        for r in range(ref["RM"].shape[0]):
            per_bin = np.array([aH[(ref["BIN"] == b) & (ref["RM"][r] == 1)].sum() for b in range(1, ref["n_lat"] + 1)])
            bound = np.concatenate(([0.0], np.cumsum(per_bin))) * (10 + m.km + 8) * U53 * f
            for c in (0, 2):
                ok = ~masked[:, c, r]
                assert np.all(np.abs(got[ok, c, r]) <= bound[ok]), (n, c, r)
    m.close()


def test_reset_and_snapshot(pkg, tmp_path):
    m, _ = make(pkg, "avgfit")
    m.tavg_request(1, "SSH")                         # a slab entry in the same stream, so that the stream can be written
    m.step(); m.step()
    with pytest.raises(pkg.PopError, match="pop_transport_get: no snapshot yet"):
        m.transport_get(1, snapshot=True)
    want = both(m)
    assert m.transport_sums().any()
    m.tavg_write(1, str(tmp_path / "t.bin"))         # normalise, write, reset
    assert all(np.array_equal(x, y) for x, y in zip(both(m, snapshot=True), want))
    assert m.tavg_sums(1)[0] == 0.0 and not m.transport_sums().any()
    z = m.transport_get(2, normalize=False)
    assert not z[z != UNDEFINED_NF].any()
    with pytest.raises(pkg.PopError, match="transport: cannot normalise: tavg_sum of stream 1 is 0"):
        m.transport_get(1)
    m.step()
    assert m.transport_sums().any() and all(np.array_equal(x, y) for x, y in zip(both(m, snapshot=True), want))
    m.tavg_reset(1)
    assert not m.transport_sums().any()
    m.time_manager()
    for call in (lambda: m.tavg_reset(1), lambda: m.transport_sums(np.zeros(m.transport_sums().size))):
        with pytest.raises(pkg.PopError, match="refused between pop_time_manager and pop_step_tail"):
            call()
    m.close()


def test_sums_carried_over(pkg):
    """pop_transport_sums_get / _set: a run that hands its sums over after two steps stays within twice the bound"""
    a, ref = make(pkg, "gm_submeso")
    b, _ = make(pkg, "gm_submeso")
    for _ in range(2):
        step(a, ref); b.step()
    s = b.transport_sums()
    assert np.array_equal(s, a.transport_sums())
    b.transport_sums(s)                              # the device sums start from 0 again; the vector is added last
    assert np.array_equal(b.transport_sums(), s)
    step(a, ref); b.step()
    for t in (1, 2):
        check(a.transport_get(t), ref, t, a.tavg_sums(1)[0], "uninterrupted")
        check(b.transport_get(t), ref, t, a.tavg_sums(1)[0], "continued", factor=2)
    a.close(); b.close()


def test_land_elimination_active(pkg, monkeypatch):
    """the site runs beside kernels that skip land tiles: five steps with the stream off, then three that count"""
    monkeypatch.setenv("POP_LAND_SKIP", "1"); monkeypatch.setenv("POP_LAND_FULL_STEPS", "4")
    m, ref = make(pkg, "avgfit")
    m.tavg_on(1, False)
    for _ in range(5):
        m.step()
    assert m.tavg_sums(1)[0] == 0.0 and not m.transport_sums().any()
    m.tavg_on(1, True)
    for _ in range(3):
        step(m, ref)
        assert m.dim("land_skip_active") == 1
    for t in (1, 2):
        check(m.transport_get(t), ref, t, m.tavg_sums(1)[0], "land elimination")
    land = to_global(m, m.geti("KMT")) == 0
    for name in ("TRN_ADV", "TRN_HDIF", "TRN_VNF"):
        assert not to_global(m, m.get(name, 1, 0))[land].any()
    m.close()


def test_moc_and_transports_in_one_stream(pkg):
    a, _ = make(pkg, "gm_submeso", request=2, moc=2)
    b, _ = make(pkg, "gm_submeso", request=2)
    c, _ = make(pkg, "gm_submeso", request=0, moc=2)
    for _ in range(3):
        a.step(); b.step(); c.step()
    assert a.tavg_sums(2)[0] == b.tavg_sums(2)[0] == c.tavg_sums(2)[0] > 0.0
    assert all(np.array_equal(x, y) for x, y in zip(both(a), both(b))) and np.array_equal(a.moc_get(), c.moc_get())
    a.tavg_reset(2)
    assert not a.transport_sums().any() and not a.moc_sums().any()
    for x in (a, b, c):
        x.close()
