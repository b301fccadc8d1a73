"""Passive tracers across every set-up the (T, S) path is tested on, by a passive tracer that must stay salinity.

With lpressure_avg = 0 the reference updates every tracer by one loop (baroclinic.F90:1328-1344); a passive tracer that starts as S at the
three time levels, carries S's STF and TFW and takes salinity's diffusivity (vertical_mix.F90:1260) must stay S bit for bit.  On the
device S and the twin go through different launches of the same operation -- the LDS or direct (T, S) right-hand side against
k_tracer_rhs<., ., ., NP, true>, the (T, S) corrector against the all-tracer k_impvmixt<0, PRE>, k_kpp_src_passive, k_avg_passive,
k_rf_surface_div, a second pass of the del4 / lw_lim / Gent-McWilliams / submeso kernels into the passive work fields -- which share
work buffers, side streams, the KPP look-ahead and DevGrid::skip.  A wrong index, a stale buffer, a missed halo, a skipped tile or a
crossed slot shows as a bit.  tests/test_passive_host.py pins the property on the CPU oracle for every row of B1.

Layout, nt = 5: tracers 3 and 5 twins (a slot of the pair launch, the launch of one), tracer 4 passive_field(T).

B1  the twin over topology x scheme (passive_common.TWIN_ROWS); the tripole and padded rows once more with lpressure_avg = 1 under the
    properties P1 / P2 / P3 of test_gpu_passive.test_a2_*
B2  the tracer-path fields of pop_tuning are neutral with passive tracers
B3  land elimination is invisible with passive tracers
B5  the 4-D halo update of five tracers; exact restart
B6  gx1v7, the kernel selection the library makes on its own
(B4, the tracer counts 6 and 7, is in tests/test_gpu_passive.py; B7, several ranks, in tests/test_gpu_passive_multirank.py.)
Every comparison is np.array_equal over all cells, except the halo rule on padded blocks (the cells that exist)."""
import numpy as np
import pytest

import land_common
from common import block_masks
from orclib import AsModel, Oracle
from popcfg import named_config, synthetic_grid
from passive_common import (DEL4, KPP, TWINS, TWIN_IDS, TWIN_ROWS, assert_neighbour, assert_twin, make_salinity_twin,
                            passive_field, set_passive, twin_layout, twin_row, twin_start)

pytestmark = pytest.mark.gpu
NSTEPS = 5


# ------------------------------------------------------------------ B1
@pytest.mark.parametrize("topology,scheme", TWIN_ROWS, ids=TWIN_IDS)
def test_b1_twin_stays_salinity(pkg, orclib_built, topology, scheme):
    cfg, grid, tidal = twin_row(pkg, topology, scheme)
    gpu, orc = pkg.PopModel(cfg, grid=grid), Oracle(cfg, grid=grid)      # the oracle only supplies the initial state
    if "padded" in topology:
        assert block_masks(gpu)["short"] > 0
    twin_start(orc, [gpu], scheme, tidal)
    orc.close()
    if cfg.km == 60:                                             # the register Thomas kernels with nlast = 2 and nlast = 1
        assert gpu.dim("thomas_register_tracers") == 1
    for s in range(1, NSTEPS + 1):
        gpu.step()
        for n in TWINS:
            assert_twin(gpu, n, "%s %s step %d" % (topology, scheme, s))
    assert_neighbour(gpu, "%s %s" % (topology, scheme))
    gpu.close()


PAVG_ROWS = [r for r in TWIN_ROWS if "tripole" in r[0] or "padded" in r[0]]


@pytest.mark.parametrize("topology,scheme", PAVG_ROWS, ids=["%s-%s" % r for r in PAVG_ROWS])
def test_b1_pressure_averaging_rows_are_passive_linear_and_slot_independent(pkg, orclib_built, topology, scheme):
    """lpressure_avg = 1, where the twin does not apply: tracers 3, 4, 5 hold A, 2 A, A beside an nt = 2 model; P1, P2, P3 of test_a2_*"""
    cfg5, grid, tidal = twin_row(pkg, topology, scheme, lpressure_avg=1)
    cfg2 = twin_row(pkg, topology, scheme, nt=2, lpressure_avg=1)[0]
    m5, m2, orc = pkg.PopModel(cfg5, grid=grid), pkg.PopModel(cfg2, grid=grid), Oracle(cfg2, grid=grid)
    twin_start(orc, [m5, m2], scheme, tidal)
    A = passive_field(orc.f3("TRACER", 1, 0).copy(), orc.i2("KMT"))
    set_passive([m5], {2: A, 3: 2.0 * A, 4: A})
    if cfg5.vmix_choice == 3:                                    # a surface flux for the passive tracers, in the ratio of their fields
        stf = 1.0e-2 * np.cos(orc.f2("TLAT"))
        for n, f in ((2, 1.0), (3, 2.0), (4, 1.0)):
            m5.set("STF", f * stf, n=n)
    orc.close()
    iters = {5: [], 2: []}
    for _ in range(NSTEPS):
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
        assert np.isfinite(t3).all() and not np.array_equal(t3, A) and np.ptp(t3[:, 1]) > 0.0
    m5.close(); m2.close()


# ------------------------------------------------------------------ B2
KM60 = dict(vmix_choice=3, km=60, stepped_bathymetry=1)
KPP_DEL4 = dict(KPP, **DEL4)
GM = {"hmix_tracer": 3}
AT_LEAST_2 = -2
# (configuration, its keywords, pop_tuning fields of model X, pop_get_dim values that show the form in use on X -- "D:" on D).
# pop_get_tuning returns the request; what ran is the library's plan, one entry per choice, which pop_get_dim("form_<entry>") returns: every row
# names the entry its field governs with the value X must hold (and D's where the row's point is that they differ).  tracer_lds 4, del4_tile 0,
# kpp_col 1 and thomas_pair 0 are also what the rules choose on this grid.
B2 = ([("tiny", {}, {"tracer_lds": v}, {"form_tracer_lds_rows": v}) for v in (0, 4, 8)] +
     [("tiny", KM60, {"reg_thomas_t": v}, {"thomas_register_tracers": v}) for v in (0, 1)] +
     # thomas_pair acts at one site only, the (T, S) corrector under pressure averaging (launch_impvmixt<1, ., .>), with the register kernels and one shared diffusivity array (KPP): these two rows run with lpressure_avg = 1,
     # X against D bitwise and P2 / P3 in place of the twin.  0 is also what the size rule chooses on `tiny`; 1 is k_impvmixt2_reg.
     [("tiny", KM60, {"thomas_pair": v}, {"thomas_register_tracers": 1, "pavg": 1, "form_thomas_pair": v}) for v in (0, 1)] +
     [("tiny", KPP, {"vdc_shared": 0}, {"form_vdc_shared": 0, "D:form_vdc_shared": 1}),
      ("tiny", KPP_DEL4, {"side_stream": 0}, {"kpp_ahead_used": 0, "form_side_stream": 0, "D:form_side_stream": 1}),
      ("tiny", DEL4, {"del4_side": 0}, {"form_del4_side": 0, "D:form_del4_side": 1})] +
     [("tiny", DEL4, {"del4_tile": v}, {"form_del4_tile_rows": v}) for v in (0, 2, 16)] +
     [("tiny", DEL4, {"d2t_fuse": 1}, {"d2t_fused": 1}),
      # the buffers of the first Laplacian formed ahead belong to the side-stream form (pop_create_tuned allocates them under del4_side):
      # asked for together with del4_side = 0 the library keeps k_del4_d2t in line, and says so
      ("tiny", DEL4, {"d2t_fuse": 1, "del4_side": 0}, {"d2t_fused": 0})] +
     [("tiny", KPP, {"kpp_col": v}, {"form_kpp_col": v}) for v in (1, 2, 4, 8, 16, 31)] +
     [("tiny", KPP, {"kpp_src_full": 1}, {"form_kpp_src_full": 1, "D:form_kpp_src_full": 0}),
      # kpp_sparse acts where the column march runs (sparse = march && ...; march needs bits 3 and 4 of kpp_col, which the size rule leaves
      # off here): the march with the streaming boundary-layer kernel, against the defaults
      ("tiny", KPP, {"kpp_col": 31, "kpp_sparse": 0}, {"form_kpp_march": 1, "form_kpp_sparse": 0, "D:form_kpp_march": 0}),
      ("tiny", KPP, {"kpp_side_stream": 0}, {"form_kpp_side": 0, "D:form_kpp_side": 1}),
      # one block: there the size rule switches the look-ahead on (beside the resident solve), so D runs it
      ("tiny", dict(KPP, block_size_x=48, block_size_y=40), {"kpp_ahead": 0}, {"kpp_ahead_used": 0, "D:kpp_ahead_used": AT_LEAST_2}),
      ("tiny", KPP, {"kpp_ahead": 1}, {"kpp_ahead_used": AT_LEAST_2}),     # five steps with nothing read in between: twins through the look-ahead
      ("tiny", GM, {"gm_flux_tile": 0}, {"form_gm_lds": 0, "D:form_gm_lds": 1}),
      ("tiny", {"hmix_tracer": 3, "ah_bolus": 0.4e7}, {"gm_sf_stored": 0}, {"form_gm_sf_stored": 0, "D:form_gm_sf_stored": 1}),
      ("tiny", dict(KPP, hmix_tracer=3, gm_transition_layer=1, stepped_bathymetry=1, submeso=True), {"submeso_all_levels": 1}, {"form_submeso_all_levels": 1, "D:form_submeso_all_levels": 0}),
      ("tiny", KPP_DEL4, {"halo_separate": 1}, {"form_halo_separate": 1, "D:form_halo_separate": 0})])


def _b2_id(row):
    return "%s-%s" % (row[0], "-".join("%s%d" % kv for kv in row[2].items())) + ("-km60" if row[1].get("km") == 60 else "") + \
        ("-one-block" if "block_size_x" in row[1] else "") + ("-pavg" if row[3].get("pavg") else "")


def _own_twins(m):
    """The twin layout from the device model's own state, where no oracle is at hand.  With KPP first what parity.force_kpp_case
    does to an oracle: surface fluxes and a nearly homogeneous upper ocean (eight levels, where sin(3 TLAT) > 0), so that the boundary layer
    spans several levels and the non-local source is at work; the densities of the new state through pop_state_host."""
    if m.cfg.vmix_choice == 3:
        tlat, kmt = m.get("TLAT"), m.geti("KMT")
        m.set("STF", -3.0e-2 * np.sin(tlat) - 1.0e-2, n=0); m.set("STF", 2.0e-6 * np.cos(2.0 * tlat), n=1)
        z = np.arange(m.km)[None, :, None, None]
        shallow = (z < 8) & (z < kmt[:, None]) & (np.sin(3 * tlat)[:, None] > 0)
        for tl in (0, 1, 2):
            X = []
            for n, slope in ((0, 2.0e-4), (1, -2.0e-9)):
                T = m.get("TRACER", tl, n)
                X.append(np.where(shallow, T[:, 0:1] - slope * z, T))
                m.set("TRACER", X[n], tl=tl, n=n)
            if tl < 2:
                m.set("RHO", np.stack([m.state(k + 1, X[0][:, k], X[1][:, k]) for k in range(m.km)], axis=1), tl=tl)
    if m.nt >= 5:
        twin_layout([m], passive_field(m.get("TRACER", 1, 0), m.geti("KMT")))
    else:
        make_salinity_twin([m], 2)


@pytest.mark.parametrize("row", B2, ids=[_b2_id(r) for r in B2])
def test_b2_kernel_forms_are_neutral_with_passive_tracers(pkg, orclib_built, row):
    name, kw, tuning, dims = row
    kw, dims = dict(kw), dict(dims)
    submeso, pavg = kw.pop("submeso", False), dims.pop("pavg", 0)
    cfg = named_config(name, nt=5, lpressure_avg=pavg, **kw)
    if submeso:
        cfg = pkg.submeso_config(cfg)
    X, D = pkg.PopModel(cfg, tuning=tuning), pkg.PopModel(cfg)
    resolved, default = X.tuning(), D.tuning()
    for f, v in tuning.items():
        assert resolved[f] == v, "%s: asked for %d, the library holds %r" % (f, v, resolved[f])      # the request arrived; the outcome: dims
        assert default[f] is None, "%s is set from outside the test (environment): %r" % (f, default[f])
    if name == "tiny":
        orc = Oracle(cfg)
        A = twin_start(orc, [X, D], "kpp" if cfg.vmix_choice == 3 else "default", False)
        if pavg:                                                 # A, 2 A, A and surface fluxes in that ratio, as test_a2_*
            stf = 1.0e-2 * np.cos(orc.f2("TLAT"))
            for n, f in ((2, 1.0), (3, 2.0), (4, 1.0)):
                set_passive([X, D], {n: f * A})
                for m in (X, D):
                    m.set("STF", f * stf, n=n); m.set("TFW", 0.0 * stf, n=n)
        orc.close()
    else:
        for m in (X, D):
            _own_twins(m)
    same = np.array_equal
    iters = {0: [], 1: []}
    for s in range(NSTEPS):
        for i, m in enumerate((X, D)):
            m.step()
            iters[i].append(m.solver_diagnostics()[0])
    for d, v in dims.items():
        got = D.dim(d[2:]) if d.startswith("D:") else X.dim(d)
        assert (got >= 2) if v == AT_LEAST_2 else (got == v), "%s = %d, expected %d" % (d, got, v)
    assert iters[0] == iters[1]
    for tl in (0, 1):
        for n in range(5):
            assert same(X.get("TRACER", tl, n), D.get("TRACER", tl, n)), (tuning, "TRACER", n, tl)
        for f in ("RHO", "PSURF"):
            assert same(X.get(f, tl), D.get(f, tl)), (tuning, f, tl)
    if pavg:
        for tl in (0, 1):
            t3, t4, t5 = (X.get("TRACER", tl, n) for n in (2, 3, 4))
            assert np.array_equal(t5, t3) and np.array_equal(t4, 2.0 * t3), tl                # P2, P3
            assert np.isfinite(t3).all() and not np.array_equal(t3, A) and np.ptp(t3[:, 1]) > 0.0
    else:
        for n in TWINS:
            assert_twin(X, n, str(tuning))
        assert_neighbour(X, str(tuning))
    X.close(); D.close()


# ------------------------------------------------------------------ B3
def _land_cases():
    return [land_common.CASES[0], land_common.CASES[2], land_common.CASES[-2]]


@pytest.mark.parametrize("pavg", [0, 1], ids=["all-tracer", "pavg"])
@pytest.mark.parametrize("case", [0, 1, 2], ids=["kpp-del4-big", "two-blocks-upwind3-avg", "d2t-fuse-tracer-fwd"])
def test_b3_land_elimination_is_invisible_with_passive_tracers(pkg, monkeypatch, case, pavg):
    name, kw, env, nsteps = _land_cases()[case]
    cfg = named_config(name, nt=5, lpressure_avg=pavg, **kw)
    a, b = land_common.model(pkg, monkeypatch, cfg, env, False), land_common.model(pkg, monkeypatch, cfg, env, True)
    assert b.scalar("land_tile_fraction") > 0.05, "the case has no land tiles"
    for m in (a, b):
        _own_twins(m)
    kpp = cfg.vmix_choice == 3
    for s in range(1, nsteps + 1):
        a.step(); b.step()
        assert a.dim("land_skip_active") == 0 and b.dim("land_skip_active") == (1 if s > 4 else 0), s
        assert a.solver_diagnostics() == b.solver_diagnostics(), "step %d" % s
        if s in (5, 6, nsteps):
            for n in range(5):
                for tl in (0, 1, 2):
                    assert np.array_equal(a.get("TRACER", tl, n), b.get("TRACER", tl, n)), "step %d tracer %d tl %d" % (s, n + 1, tl)
                if kpp:
                    assert np.array_equal(a.get("KPP_SRC", n=n), b.get("KPP_SRC", n=n)), "step %d KPP_SRC %d" % (s, n + 1)
            if pavg == 0:
                for n in TWINS:
                    assert_twin(b, n, "step %d, tiles skipped" % s)
    assert b.dim("land_skip_active") == 1 and (not kpp or b.get("KPP_SRC", n=1).any())
    assert_neighbour(b)
    a.close(); b.close()


# ------------------------------------------------------------------ B5
@pytest.mark.parametrize("kw,own_grid", [({"ns_boundary": 2}, True), ({"block_size_x": 20, "block_size_y": 16}, False),
                                         ({"ns_boundary": 2, "block_size_x": 28, "block_size_y": 24}, True)],
                         ids=["tripole", "padded", "tripole-padded"])
def test_b5_halo_update_of_every_tracer_is_the_oracle_rule(pkg, orclib_built, kw, own_grid):
    """halo_update("TRACER", tl, n=-1) with nt = 5: random values on the physical cells, garbage in the ghost cells; afterwards every
    tracer is what the oracle's POP_HaloUpdate (centre, scalar) makes of the same array.  Compared on every cell that exists (non-zero
    global indices): the padding of a short block holds nothing and no rule says what an update leaves there."""
    cfg = named_config("tiny", nt=5, **kw)
    grid = synthetic_grid(cfg) if own_grid else None
    m, ref = pkg.PopModel(cfg, grid=grid), AsModel(Oracle(cfg, grid=grid))
    masks = block_masks(m)
    assert (masks["short"] > 0) == ("block_size_x" in kw)
    exists = np.zeros((m.nblocks, m.nyb, m.nxb), dtype=bool)
    for lb, bid in enumerate(m.local_block_ids()):
        blk = m.get_block(bid)
        exists[lb] = (blk["j_glob"] != 0)[:, None] & (blk["i_glob"] != 0)[None, :]
    sel = np.broadcast_to(exists[:, None], (m.nblocks, m.km, m.nyb, m.nxb))
    rng = np.random.default_rng(21)
    expect = []
    for n in range(5):
        a = np.where(masks["phys"][:, None], rng.standard_normal((m.nblocks, m.km, m.nyb, m.nxb)) * 10.0 + n, -999.0 - n)
        m.set("TRACER", a, tl=2, n=n)
        e = a.copy()
        ref.halo_update_host_loc(e)
        assert not np.array_equal(e, a) and not (e[sel] == -999.0 - n).any()      # the rule fills every ghost cell that exists
        expect.append(e)
    m.halo_update("TRACER", tl=2, n=-1)
    for n in range(5):
        got = m.get("TRACER", tl=2, n=n)
        assert np.array_equal(got[sel], expect[n][sel]), "tracer %d: %d cells that exist differ (%d cells in all)" % (
            n + 1, (got != expect[n])[sel].sum(), (got != expect[n]).sum())
    m.close(); ref.close()


@pytest.mark.parametrize("kw,own_grid", [(KPP_DEL4, False), ({"ns_boundary": 2}, True)], ids=["kpp-del4", "tripole"])
def test_b5_restart_continues_exactly(pkg, orclib_built, tmp_path, kw, own_grid):
    """nt = 5, tracer 3 ideal age, tracer 4 a field, tracer 5 a salinity twin: 3 + 3 steps continued against re-read"""
    cfg = named_config("tiny", nt=5, **kw)
    grid = synthetic_grid(cfg) if own_grid else None

    def model():
        m, orc = pkg.PopModel(cfg, grid=grid), Oracle(cfg, grid=grid)
        twin_start(orc, [m], "kpp" if cfg.vmix_choice == 3 else "default", False)
        orc.close()
        m.init_iage(3)
        if cfg.ns_boundary == 2:                                 # no wind through the fold (tests/test_gpu_restart.py)
            z = np.zeros_like(m.get("SMF", n=0))
            for n in (0, 1):
                m.set("SMF", z, n=n); m.set("SMFT", z, n=n)
        return m
    a, b = model(), model()
    for _ in range(3):
        a.step()
    path = str(tmp_path / "r.bin")
    a.write_restart(path)
    b.read_restart(path)
    for _ in range(3):
        a.step(); b.step()
    for tl in (0, 1):
        for n in range(5):
            assert np.array_equal(a.get("TRACER", tl, n), b.get("TRACER", tl, n)), (tl, n)
        for f in ("UVEL", "VVEL", "PSURF"):
            assert np.array_equal(a.get(f, tl), b.get(f, tl)), (tl, f)
    age = a.get("TRACER", 1, 2)
    assert age.max() > 0.0 and not age[:, 0].any() and np.isfinite(age).all()
    assert_neighbour(a)
    a.close(); b.close()


# ------------------------------------------------------------------ B6
@pytest.mark.parametrize("kw", [{}, {"tadvect": 2, "tmix_opt": 3}], ids=["default", "upwind3-robert"])
def test_b6_gx1v7_twin_with_the_natural_kernel_selection(pkg, kw):
    """BASELINE's gx1v7 (KPP, km = 60, one block of 320 x 384) with nothing forced: tracer 3 is the twin"""
    cfg = named_config("gx1v7", nt=3, lpressure_avg=0, **kw)
    m = pkg.PopModel(cfg)
    assert all(v is None for f, v in m.tuning().items() if f != "struct_bytes"), m.tuning()      # every form is the size rule's
    _own_twins(m)
    S0 = m.get("TRACER", 1, 1)
    for s in range(1, 7):
        m.step()
        if s in (1, 5, 6):
            assert_twin(m, 2, "step %d" % s)
    S = m.get("TRACER", 1, 1)
    assert np.isfinite(S).all() and not np.array_equal(S, S0) and m.get("KPP_SRC", n=1).any()
    m.close()
