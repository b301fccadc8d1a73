"""Coupled surface forcing on the device (pop_set_coupled_forcing, pop_set_surface_forcing) against the NumPy restatement
tests/forcing_ref.py, bit for bit: the restatement performs the same operations in the same order and reads COS_ANGLET / SIN_ANGLET from
the model; the library is built without fused multiply-adds.  Ghost cells are compared too."""
import numpy as np
import pytest

import forcing_ref
import ice_ref
from common import STATE, tripole_expected
from forcing_common import CASES, consts_of, device_fields, liceform_of, make, restate_import

pytestmark = pytest.mark.gpu

IMPORT_CASES = ["fw", "fw-ice", "fw-active-ice", "salt", "fw-pbc", "salt-pbc", "fw-padded", "salt-padded", "fw-nt4", "salt-nt4"]
IMPORTED = [n for n in forcing_ref.IMPORTED if n != "SHF_QSW"]


def check_equal(got, want, names, tag=""):
    for n in names:
        assert got[n].shape == want[n].shape, n
        bad = got[n] != want[n]
        assert not bad.any(), "%s%s: %d cells differ, first at %s: %r != %r" % (
            tag, n, bad.sum(), np.argwhere(bad)[0], got[n][bad][0], want[n][bad][0])


# ---- 1. import and combine ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", IMPORT_CASES)
def test_import_and_combine(pkg, case):
    m = make(pkg, case)
    x = forcing_ref.seeded_x2o(m, 11)
    f, o = restate_import(m, case, x)
    m.set_coupled_forcing(**x)
    names = ["STF1", "SMF1", "SMF2", "SMFT1", "SMFT2", "SHF_QSW", "SHF_QSW_RAW", "SHF_COMP_QSW"]
    if consts_of(case)["lfw_as_salt_flx"]:
        names += ["STF2"]
    else:
        names += ["FW"] + ["TFW%d" % n for n in range(1, m.nt + 1)]
        if liceform_of(case):
            names += ["SFWF_COMP_CPL", "TFW_COMP_CPL1", "TFW_COMP_CPL2"]
    check_equal(device_fields(m, IMPORTED), f, IMPORTED, case + " ")
    check_equal(device_fields(m, names), o, names, case + " ")
    # the inputs did their work: land is masked, meltw = 0 cells exist on ocean, the rotation mixes the components
    kmt = m.geti("KMT")
    assert (kmt == 0).any() and not o["STF1"][kmt == 0].any() and (o["STF1"][kmt > 0] > 0).any() and (o["STF1"][kmt > 0] < 0).any()
    assert ((f["MELT_F"] == 0.0) & (kmt > 0)).any() and ((f["MELT_F"] != 0.0) & (kmt > 0)).any()
    assert np.abs(m.get("SIN_ANGLET")).max() > 0.5
    assert m.coupled_info()["nsteps_this_interval"] == 0
    # a field left out is zero: the heat flux without evaporation
    x2 = dict(x)
    del x2["evap"]
    f2, o2 = restate_import(m, case, x2)
    m.set_coupled_forcing(**x2)
    check_equal(device_fields(m, ["STF1", "EVAP_F", "PREC_F"]), dict(o2, **f2), ["STF1", "EVAP_F", "PREC_F"], case + " no evap ")
    assert not f2["EVAP_F"].any()
    m.close()


# ---- 2. tripole ---------------------------------------------------------------------------------------------------------------------
def test_tripole_vector_halo(pkg):
    case = "fw-tripole"
    m = make(pkg, case)
    x = forcing_ref.seeded_x2o(m, 12)
    f, o = restate_import(m, case, x)
    m.set_coupled_forcing(**x)
    cfg = m.cfg
    for n in (1, 2):
        S = m.get("SMFT", 1, n - 1)
        assert np.array_equal(S, f["SMFT%d" % n])
        # the library's existing vector halo update applied to the interior values
        W = S.copy()
        for lb, bid in enumerate(m.local_block_ids()):
            b = m.get_block(bid)
            keep = np.zeros((m.nyb, m.nxb), dtype=bool)
            keep[b["jb"] - 1:b["je"], b["ib"] - 1:b["ie"]] = True
            W[lb][~keep] = 7.0
        m.set("DH", W)
        m.halo_update_loc("DH", loc="center", kind="vector")
        assert np.array_equal(m.get("DH"), S)
        # ... and the rule itself: beyond the fold the mirrored cell with the sign changed
        G = np.zeros((cfg.ny_global, cfg.nx_global))
        blocks = [m.get_block(bid) for bid in m.local_block_ids()]
        for lb, b in enumerate(blocks):
            for j in range(b["jb"] - 1, b["je"]):
                for i in range(b["ib"] - 1, b["ie"]):
                    G[b["j_glob"][j] - 1, b["i_glob"][i] - 1] = S[lb, j, i]
        seen = 0
        for lb, b in enumerate(blocks):
            if (b["j_glob"] < 0).any():
                want = tripole_expected(G, b["i_glob"], b["j_glob"], cfg.nx_global, cfg.ny_global, "center", "vector")
                rows = b["j_glob"] < 0
                assert np.array_equal(S[lb][rows], want[rows])
                assert np.abs(want[rows]).max() > 0.0
                seen += 1
        assert seen > 0
    m.close()


# ---- 5. the per-step phase ----------------------------------------------------------------------------------------------------------
def test_per_step_phase_two_intervals(pkg):
    case = "fw-ice"
    m = make(pkg, case, cold=True, qsw_distrb_opt="12hr")
    k = consts_of(case)
    inf = m.coupled_info()
    nspi, factor = inf["nsteps_per_interval"], inf["qsw_12hr_factor"]
    assert nspi == 26 and factor.min() == 0.0 and factor.max() > 3.0
    seen_index, froze = [], 0
    for interval in range(2):
        x = forcing_ref.seeded_x2o(m, 20 + interval)
        _, o = restate_import(m, case, x)
        m.set_coupled_forcing(**x)
        nsteps = nspi + 2 if interval == 0 else 3                  # the first interval runs past its end: index_qsw wraps
        for n in range(nsteps):
            assert m.coupled_info()["nsteps_this_interval"] == n   # the import reset it
            FWF, S1 = m.get("FW_FREEZE"), m.get("TRACER", 1, 1)[:, 0]
            want = forcing_ref.surface_step(o, k, factor, n, FWF, S1)
            m.step()
            check_equal(device_fields(m, ["SHF_QSW", "FW", "TFW1", "TFW2"]), want, ["SHF_QSW", "FW", "TFW1", "TFW2"], "step %d " % n)
            seen_index.append(want["index_qsw"])
            froze += int((FWF != 0.0).any())
    assert seen_index[:nspi] == list(range(1, nspi + 1)) and seen_index[nspi:nspi + 2] == [1, 2] and seen_index[nspi + 2:] == [1, 2, 3]
    assert froze > 5                                               # FW_FREEZE took part
    m.close()


def test_per_step_phase_is_idle_where_nothing_changes(pkg):
    m = make(pkg, "salt")                                          # 'const', the virtual salt flux: the head of a step changes nothing
    x = forcing_ref.seeded_x2o(m, 30)
    m.set_coupled_forcing(**x)
    Q = m.get("SHF_QSW")
    m.set("SHF_QSW", Q + 1.0)
    m.set_surface_forcing()
    assert np.array_equal(m.get("SHF_QSW"), Q + 1.0)
    m.time_manager()
    with pytest.raises(pkg.PopError, match="between pop_time_manager and pop_step_tail"):
        m.set_coupled_forcing(**x)
    m.close()


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------
def _push(m, o, r=None):
    """the path INTEGRATION.md describes for a caller that owns the surface forcing: the six fields through pop_set_field"""
    for n in (1, 2):
        m.set("SMF", o["SMF%d" % n], n=n - 1)
        m.set("SMFT", o["SMFT%d" % n], n=n - 1)
    m.set("STF", o["STF1"], n=0)
    if "STF2" in o:
        m.set("STF", o["STF2"], n=1)
    else:
        src = r if (r is not None and "FW" in r) else o
        m.set("FW", src["FW"])
        m.set("TFW", src["TFW1"], n=0)
        m.set("TFW", src["TFW2"], n=1)
    m.set("SHF_QSW", (r if r is not None else o)["SHF_QSW"])


@pytest.mark.parametrize("case,qsw", [("fw-ice", "const"), ("salt", "const"), ("fw-ice", "12hr")])
def test_end_to_end_against_the_manual_path(pkg, case, qsw):
    from forcing_common import angle_grid
    from ice_common import cold_start
    cfgkw, pbc, ice = CASES[case]
    k = consts_of(case)
    # 'const': six steps, an import every three.  '12hr': eighteen steps, an import every nine, so that index_qsw reaches 8 and 9 --
    # seven and eight o'clock, where the factor is no longer 0 -- and a wrong index would show
    period = 9 if qsw == "12hr" else 3
    nml = dict(qsw_distrb_opt=qsw) if qsw == "12hr" else dict(qsw_distrb_opt=qsw, nsteps_per_interval=period)
    A, C = make(pkg, case, cold=True, **nml), make(pkg, case, cold=True, **nml)
    B = pkg.PopModel(A.cfg, grid=angle_grid(A.cfg, pbc))            # the caller owns the forcing: no pop_init_coupled_forcing
    B.init_ice(**ice)
    cold_start(B)
    factor = A.coupled_info()["qsw_12hr_factor"]
    fw_ice = liceform_of(case) and not k["lfw_as_salt_flx"]
    lit = 0
    for step in range(2 * period):
        if step % period == 0:
            x = forcing_ref.seeded_x2o(A, 40 + step)
            _, o = restate_import(B, case, x)
            A.set_coupled_forcing(**x)
            C.set_coupled_forcing(**x)
        r = forcing_ref.surface_step(o, k, factor, step % period, B.get("FW_FREEZE") if fw_ice else None, B.get("TRACER", 1, 1)[:, 0])
        lit += int(r["SHF_QSW"].any())
        _push(B, o, r)
        A.step()
        B.step()
        C.set_surface_forcing(); C.time_manager(); C.dhdt(); C.baroclinic_driver(); C.barotropic_driver()
        C.baroclinic_correct_adjust(); C.step_tail()
        assert np.array_equal(A.get("SHF_QSW"), r["SHF_QSW"]), step
    assert lit == (4 if qsw == "12hr" else 2 * period)               # '12hr': indices 8 and 9 of both intervals are in daylight
    for name, n in STATE:
        for tl in (0, 1):
            a = A.get(name, tl, n)
            assert np.array_equal(a, B.get(name, tl, n)), (name, n, tl, "manual path")
            assert np.array_equal(a, C.get(name, tl, n)), (name, n, tl, "phase by phase")
    assert np.isfinite(A.get("TRACER", 1, 0)).all() and A.get("UVEL", 1, 0).any()
    for m in (A, B, C):
        m.close()


# ---- 3, 4. marginal seas -------------------------------------------------------------------------------------------------------------
def _ms_model(pkg, **cfgkw):
    from forcing_common import SALT_ICE, angle_grid, ms_setup
    from popcfg import named_config
    cfg = named_config("tiny", **cfgkw)
    m = pkg.PopModel(cfg, grid=angle_grid(cfg))
    m.init_ice(**SALT_ICE)
    regions, R = ms_setup(m)
    m.init_ms_balance(regions, R)
    m.init_coupled_forcing(lms_balance=1)
    return m, regions, R


@pytest.mark.parametrize("cfgkw", [dict(), dict(block_size_x=11, block_size_y=9)], ids=["tiny", "padded"])
def test_marginal_sea_transport_cells_and_conservation(pkg, cfgkw):
    import math
    from forcing_common import SALT_ICE
    m, regions, R = _ms_model(pkg, **cfgkw)
    ice = ice_ref.params(**{k: v for k, v in SALT_ICE.items() if k != "ice_freq_opt"})
    k, c = forcing_ref.consts(ice), forcing_ref.ms_consts(ice)
    seas = forcing_ref.init_ms_balance(m, regions, R)
    assert len(seas) == 2 and m.coupled_info()["n_marginal_seas"] == 2
    rng = np.random.default_rng(5)
    Q = np.where(m.geti("KMT") > 0, 40.0 * rng.standard_normal((m.nblocks, m.nyb, m.nxb)), 0.0)   # QFLUX of both signs [W/m^2]
    m.set("QFLUX", Q)
    x = forcing_ref.seeded_x2o(m, 71)
    f = forcing_ref.import_fields(m, x, k)
    o = forcing_ref.combine(m, f, k, m.get("TRACER", 1, 0)[:, 0], m.get("TRACER", 1, 1)[:, 0], True, nt=m.nt)
    terms, over = forcing_ref.ms_terms(m, f, seas, c, Q)
    m.set_coupled_forcing(**x)
    info = m.ms_balance_info()
    from common import physical
    phys = physical(m)
    DXT, DYT = m.get("DXT"), m.get("DYT")
    got_T = m.get("MS_TRANSPORT_TERM")
    assert np.array_equal(got_T, terms[0] + terms[1])                # a cell lies in at most one sea
    for s, T, inf in zip(seas, terms, info):
        t = T[phys]                                                  # the global sum runs over the physical cells
        t = t[t != 0.0]
        assert t.size >= 6 and (t > 0).any() and (t < 0).any()
        want, mag = math.fsum(t), math.fsum(np.abs(t))
        # test 3: the rule of tests/test_gpu_diag.py -- N terms added in some order: N * 2^-53 * sum |term|
        assert abs(inf["transport"] - want) <= t.size * 2.0 ** -53 * mag, (s["number"], inf["transport"], want)
        assert inf["transport"] != 0.0
    # test 4: the cell values with the device's transports, bit for bit, ghost cells included
    want_stf2 = forcing_ref.ms_apply(m, o["STF2"], seas, c, over, [inf["transport"] for inf in info])
    got = m.get("STF", 1, 1)
    bad = got != want_stf2
    assert not bad.any(), (bad.sum(), np.argwhere(bad)[:3])
    assert not np.array_equal(got, o["STF2"])
    # conservation: what the overwrite takes out of a sea, as fresh water in kg/s, equals what its points receive.  The restatement
    # alone must satisfy the bound: evaluate both sides from it, with its own fsum transport
    for s, T, inf in zip(seas, terms, info):
        for tr in (inf["transport"], math.fsum(T[phys])):
            added = s["MASK_FRAC"] * tr * c["c_t"] / (DXT * DYT)     # what the points receive, in the units of STF2
            back = (added * DXT * DYT / c["c_t"])[phys & (s["MASK_FRAC"] != 0.0)]   # ... as kg/s again
            n = back.size
            assert n == len(s["ipts"])
            # each term carries the rounding of four operations and of its fraction; the fractions sum to 1 within n * 2^-53
            assert abs(math.fsum(back) - tr) <= (n + 6) * 2.0 ** -53 * math.fsum(np.abs(back)) + n * 2.0 ** -53 * abs(tr)
    m.close()


# ---- 7. tavg ------------------------------------------------------------------------------------------------------------------------
TAVG_SRC = {"EVAP_F": "EVAP_F", "PREC_F": "PREC_F", "SNOW_F": "SNOW_F", "MELT_F": "MELT_F", "ROFF_F": "ROFF_F", "IOFF_F": "IOFF_F",
            "SALT_F": "SALT_F", "SENH_F": "SENH_F", "LWUP_F": "LWUP_F", "LWDN_F": "LWDN_F", "MELTH_F": "MELTH_F", "IFRAC": "IFRAC",
            "U10_SQR": "U10_SQR"}


def test_tavg_entries_over_five_steps(pkg):
    import tavg_ref
    case = "fw-ice"
    m = make(pkg, case, cold=True)                                          # 'const': at the first steps of a day '12hr' leaves SHF_QSW = 0
    p = ice_ref.params(tfreeze_option=1, lfw_as_salt_flx=0)
    names = list(TAVG_SRC) + ["TFW_T", "TFW_S", "TAUX", "SHF_QSW"]          # with two entries the site had before: both launches of the site run
    for i, n in enumerate(names):
        m.tavg_request(1 + i % 2, n)
        assert m.tavg_info(n) == {"stream": 1 + i % 2, "ndims": 2, "nlevels": 1, "method": "avg"}
    buf = {n: np.zeros((m.nblocks, m.nyb, m.nxb)) for n in names}
    kmt = m.geti("KMT")
    for step in range(5):
        if step in (0, 3):
            m.set_coupled_forcing(**forcing_ref.seeded_x2o(m, 60 + step))
        m.set_surface_forcing(); m.time_manager()
        dtavg = m.scalar("dtt") * m.scalar("time_weight")
        val = {n: m.get(s) for n, s in TAVG_SRC.items()}
        val["TFW_T"] = m.get("TFW", 1, 0) / p["hflux_factor"]                 # forcing.F90:578
        val["TFW_S"] = m.get("TFW", 1, 1) * p["rho_sw"] * 10.0                # :579
        val["TAUX"] = m.get("SMF", 1, 0)
        val["SHF_QSW"] = np.where(kmt > 0, m.get("SHF_QSW") / p["hflux_factor"], 0.0)
        for n in names:
            buf[n] = tavg_ref.accumulate(buf[n], val[n], "avg", dtavg)
        m.dhdt(); m.baroclinic_driver(); m.barotropic_driver(); m.baroclinic_correct_adjust(); m.step_tail()
    got = {n: m.tavg_get(n, normalize=False) for n in names}
    check_equal(got, buf, names, "tavg ")
    assert all(got[n].any() for n in names)
    m.close()
