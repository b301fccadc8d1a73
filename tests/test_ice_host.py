"""Frazil ice formation, host side (pop_init_ice, pop_tfreez_host): the namelist defaults, every refusal of the entry point with its
message, the freezing point against its three closed forms, and properties of the NumPy restatement (tests/ice_ref.py) that involve no
second implementation: the column heat and salt budgets, the freezing floor and the land columns."""
import ctypes as C

import numpy as np
import pytest

import ice_ref
from popcfg import named_config


def host(pkg, **kw):
    return pkg.PopModel(named_config("tiny", **kw), host_only=True)


def test_nml_defaults(pkg):
    n = pkg.ice_nml()
    assert n.struct_bytes == C.sizeof(pkg.PopIceNml)
    want = dict(ice_ref.DEFAULTS)
    assert want["ice_freq_opt"] == 0 and want["kmxice"] == 1 and want["lactive_ice"] == 0 and want["licecesm2"] == 0
    assert want["lfw_as_salt_flx"] == 0 and want["tfreeze_option"] == 0
    for k, v in want.items():
        assert getattr(n, k) == v, k
    assert (n.sea_ice_salinity, n.ocn_ref_salinity, n.latent_heat_fusion, n.cp_sw, n.rho_sw, n.rho_fw) == \
        (4.0, 34.7, 3.34e9, 3.996e7, 4.1 / 3.996, 1.0)
    assert pkg.ice_nml(ice_freq_opt="coupled", tfreeze_option="mushy").tfreeze_option == 2
    with pytest.raises(AttributeError):
        pkg.ice_nml(no_such_member=1)


@pytest.mark.parametrize("cfgkw,nml,text", [
    ({}, dict(kmxice=0), "kmxice = 0 is outside 1 .. km = 16"),
    ({}, dict(kmxice=17), "kmxice = 17 is outside 1 .. km = 16"),
    ({}, dict(sea_ice_salinity=-1.0), "negative constant"),
    ({}, dict(ocn_ref_salinity=-34.7), "negative constant"),
    ({}, dict(latent_heat_fusion=-1.0), "negative constant"),
    ({}, dict(cp_sw=-1.0), "negative constant"),
    ({}, dict(rho_sw=-1.0), "negative constant"),
    ({}, dict(rho_fw=-1.0), "negative constant"),
    ({}, dict(struct_bytes=8), "struct_bytes is not sizeof(pop_ice_nml)"),
    (dict(tmix_opt=0), dict(ice_freq_opt="coupled"), "'coupled' with licecesm2 = 0 needs tmix_opt robert or avgfit"),
    (dict(tmix_opt=1), dict(ice_freq_opt="coupled"), "'coupled' with licecesm2 = 0 needs tmix_opt robert or avgfit"),
    ({}, dict(ice_freq_opt="nyear"), "'nyear' .. 'nstep' (2 .. 7) is not built"),
    ({}, dict(ice_freq_opt="nmonth"), "'nyear' .. 'nstep' (2 .. 7) is not built"),
    ({}, dict(ice_freq_opt="nday"), "'nyear' .. 'nstep' (2 .. 7) is not built"),
    ({}, dict(ice_freq_opt="nhour"), "'nyear' .. 'nstep' (2 .. 7) is not built"),
    ({}, dict(ice_freq_opt="nsecond"), "'nyear' .. 'nstep' (2 .. 7) is not built"),
    ({}, dict(ice_freq_opt="nstep"), "'nyear' .. 'nstep' (2 .. 7) is not built"),
    ({}, dict(ice_freq_opt=8), "ice_freq_opt: 0 'never', 1 'coupled'"),
    ({}, dict(tfreeze_option=3), "tfreeze_option: 0 'minus1p8', 1 'linear_salt', 2 'mushy'"),
])
def test_refusals(pkg, cfgkw, nml, text):
    m = host(pkg, **cfgkw)
    with pytest.raises(pkg.PopError) as e:
        m.init_ice(**nml)
    assert text in str(e.value) and str(e.value).startswith("pop_init_ice: ")
    m.init_ice()                                   # a refused call leaves the context as it was: the call can still be made
    m.close()


def test_accepted_and_once_only(pkg):
    for cfgkw, nml in (({}, dict(ice_freq_opt="coupled")),                          # avgfit (tiny's tmix_opt)
                       (dict(tmix_opt=3), dict(ice_freq_opt="coupled")),            # robert
                       (dict(tmix_opt=0), dict(ice_freq_opt="coupled", licecesm2=1)),
                       (dict(tmix_opt=1), dict(ice_freq_opt="coupled", licecesm2=1, kmxice=16, lfw_as_salt_flx=1, lactive_ice=1))):
        m = host(pkg, **cfgkw)
        m.init_ice(**nml)
        assert m.scalar("tlast_ice") == 0.0 and m.scalar("time_weight") == 1.0
        p = ice_ref.params()
        assert m.scalar("cp_over_lhfusion") == p["cp_over_lhfusion"]
        with pytest.raises(pkg.PopError, match="called a second time"):
            m.init_ice(**nml)
        m.close()
    m = host(pkg)
    assert np.isnan(m.scalar("tlast_ice"))         # no ice formation without the call
    m.time_manager()
    with pytest.raises(pkg.PopError, match="a step or a phase has already run"):
        m.init_ice()
    with pytest.raises(pkg.PopError, match="needs pop_init_ice"):
        m.tfreez(np.zeros(3))
    m.close()


def test_compute_entries_need_a_device(pkg):
    m = host(pkg)
    m.init_ice()
    for call in (lambda: m.ice_formation(1), m.ice_flx_to_coupler, m.ice_export_reset):
        with pytest.raises(pkg.PopError, match="host-only"):
            call()
    m.close()


@pytest.mark.parametrize("option", [0, 1, 2])
def test_tfreez_host_closed_forms(pkg, option):
    m = host(pkg)
    m.init_ice(tfreeze_option=option)
    # negative salinity counts as 0; 36.77 psu is where the linear form reaches -2, 37.7 psu where the mushy form does
    S = np.array([-0.010, -0.0, 0.0, 1.0e-6, 0.010, 0.030, 0.0347, 0.0367, 0.0368, 0.0376, 0.0378, 0.040, 0.100, 0.5])
    got = m.tfreez(S)
    psu = np.maximum(S * 1000.0, 0.0)
    want = {0: np.full_like(S, -1.8), 1: -0.0544 * psu, 2: psu / (-18.48 + 0.01848 * psu)}[option]
    want = np.maximum(want, -2.0)
    assert np.array_equal(got, want)
    assert np.array_equal(got, ice_ref.tfreez(S, option))
    assert got.min() >= -2.0 and (option == 0 or got.min() == -2.0)
    if option:
        assert got[0] == 0.0 and got[2] == 0.0 and got[4] < 0.0
        assert got[-1] == -2.0 and got[5] > -2.0
    assert m.tfreez(np.zeros((2, 3))).shape == (2, 3)
    m.close()


# ---- properties of the restatement ---------------------------------------------------------------------------------------------
def _columns(seed, km=16, ny=24, nx=32):
    rng = np.random.default_rng(seed)
    KMT = rng.choice(np.array([0, 0, 1, 2, 3, 5, km], dtype=np.int32), size=(2, ny, nx))
    wet = np.arange(1, km + 1)[None, :, None, None] <= KMT[:, None]
    T = np.where(wet, rng.uniform(-2.6, -1.0, wet.shape), 0.0)
    S = np.where(wet, rng.uniform(0.030, 0.037, wet.shape), 0.0)
    PS = np.where(KMT > 0, ice_ref.GRAV * rng.uniform(-60.0, 60.0, KMT.shape), 0.0)
    AQ = np.where(KMT > 0, -rng.uniform(0.0, 40.0, KMT.shape) * (rng.random(KMT.shape) < 0.6), 0.0)
    DZBC = np.where(KMT > 0, rng.uniform(0.3, 1.0, KMT.shape) * ice_ref.thickness(km, KMT)[0, np.clip(KMT, 1, km) - 1, 0, 0], 0.0)
    return KMT, wet, T, S, PS, AQ, DZBC


CASES = [(o, s, k, pbc, tw) for o in (0, 1, 2) for s in (0, 1) for k, pbc, tw in ((1, False, 1.0), (3, False, 0.5), (4, True, 1.0))]


@pytest.mark.parametrize("option,salt,kmxice,pbc,tw", CASES)
def test_restatement_budgets(option, salt, kmxice, pbc, tw):
    KMT, wet, T, S, PS, AQ, DZBC = _columns(3 + option)
    km = T.shape[1]
    p = ice_ref.params(tfreeze_option=option, lfw_as_salt_flx=salt, kmxice=kmxice)
    TH = ice_ref.thickness(km, KMT, DZBC if pbc else None)
    r = ice_ref.formation(T, S, PS, KMT, AQ, TH, p, tw, 3600.0)
    THW = TH.copy()
    THW[:, 0] = r["W"]
    # heat: sum_k thickness (T_after - T_before) = -(AQICE_after - AQICE_before) / time_weight
    heat_terms = THW * (r["T"] - T)
    heat, debt = heat_terms.sum(axis=1), -(r["AQICE"] - AQ) / tw
    # the sum of magnitudes is that of the terms the two sides are differences of: thickness x T before and after (a cell that freezes
    # and then melts in the offset pass ends near where it began, with the rounding of both passes), and the two AQICE
    scale = (THW * (np.abs(r["T"]) + np.abs(T))).sum(axis=1) + np.abs(r["AQICE"]) / tw + np.abs(AQ) / tw
    assert np.all(np.abs(heat - debt) <= 1.0e-12 * scale)
    assert np.abs(heat).max() > 1.0                      # the columns do freeze and melt
    if salt:
        # salt: sum_k thickness (S_after - S_before) = (salref - salice) cp_over_lhfusion x the heat change
        salt_terms = THW * (r["S"] - S)
        f = (p["salref"] - p["salice"]) * p["cp_over_lhfusion"]
        # each term is a difference of two salinities of 0.03 that agree to two or three digits, so its rounding error is that of
        # the salinities themselves: the sum of magnitudes is that of thickness x S before and after
        mag = (THW * (np.abs(r["S"]) + np.abs(S))).sum(axis=1) + abs(f) * scale
        assert np.all(np.abs(salt_terms.sum(axis=1) - f * heat) <= 1.0e-12 * mag)
        assert r["FW_FREEZE"] is None
    else:
        assert r["FW_FREEZE"] is not None and np.all(r["FW_FREEZE"] <= 0.0) and r["FW_FREEZE"].min() < 0.0
    # nothing changes below kmxice
    assert np.array_equal(r["T"][:, kmxice:], T[:, kmxice:]) and np.array_equal(r["S"][:, kmxice:], S[:, kmxice:])
    if option == 0:                                      # no ocean cell of the levels 1 .. kmxice ends below freezing
        top = wet[:, :kmxice]
        assert r["T"][:, :kmxice][top].min() >= -1.8 - 1.0e-13
        assert T[:, :kmxice][top].min() < -2.5
    # land columns stay exactly 0
    land = KMT == 0
    for a in (r["T"], r["S"]):
        assert not a[np.broadcast_to(land[:, None], a.shape)].any()
    for a in (r["QICE"], r["AQICE"]) + (() if salt else (r["FW_FREEZE"],)):
        assert not a[land].any()
    assert (r["QICE"] <= 0.0).all() and r["QICE"].min() < 0.0


def test_restatement_flx_to_coupler():
    KMT, wet, T, S, PS, AQ, DZBC = _columns(9)
    p = ice_ref.params(tfreeze_option=1)
    TH1 = ice_ref.thickness(T.shape[1], KMT)[:, 0]
    a, q, f = ice_ref.flx_to_coupler(T[:, 0], S[:, 0], PS, KMT, AQ, TH1, 0.0, True, p)
    assert np.array_equal(a, 0.5 * AQ) and not f.any()
    assert np.array_equal(q[AQ < 0], -0.5 * AQ[AQ < 0]) and not q[KMT == 0].any()
    a, q, f = ice_ref.flx_to_coupler(T[:, 0], S[:, 0], PS, KMT, AQ, TH1, 7200.0, False, p)
    assert np.array_equal(a, AQ) and np.array_equal(f, q / 7200.0 / p["hflux_factor"])
    melt = (AQ == 0) & (KMT > 0)
    W = TH1 + PS / ice_ref.GRAV + ice_ref.EPS2
    assert np.array_equal(q[melt], ((ice_ref.tfreez(S[:, 0], 1) - T[:, 0]) * W)[melt])
