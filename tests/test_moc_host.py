"""The MOC's host side (pop_init_transports on host-only contexts) against the NumPy restatement tests/moc_ref.py: the auxiliary
latitude grid bit for bit for the three grid types and both branches of the 'southern' remainder, every cell's bin, MASK_LAT_DEPTH,
lat_aux_region_start, n_moc_comp, every refusal of init_lat_aux_grid / init_moc_ts_transport_arrays with the reference's reason, and
the refusals of pop_moc_request.  The test grid is popcfg.synthetic_grid of 'tiny' (48 x 40 x 16 in blocks of 12 x 10) with ULAT bent
north of the equator (moc_ref.bent_grid)."""
import numpy as np
import pytest

import moc_ref
from popcfg import named_config

REG2 = (6,)


def host(pkg, bend=True, lat_span=160.0, cfg=None, north_only=False, bend_south=False, one_longitude=False, **kw):
    cfg = cfg if cfg is not None else named_config("tiny", **kw)
    g = moc_ref.bent_grid(cfg, bend, 80.0 if north_only else lat_span, one_longitude)
    if north_only:                                     # 1 .. 81 degrees north
        g["ULAT"] = g["ULAT"] + 41.0 / moc_ref.RADIAN
    if bend_south:                                     # the southern rows wander by a few hundredths of a degree
        i = np.arange(cfg.nx_global)[None, :]
        g["ULAT"] = np.where(g["ULAT"] < -0.1, g["ULAT"] + 1.0e-3 * np.sin(2.0 * np.pi * i / cfg.nx_global), g["ULAT"])
    return pkg.PopModel(cfg, host_only=True, grid=g)


def restated(m, nml, region_mask=None, reg2=()):
    T, U, KMT = moc_ref.latitudes(m)
    edge, center = moc_ref.lat_aux_grid(T, U, partial_bottom_cells=bool(m.cfg.partial_bottom_cells), **nml)
    nreg = 2 if len(reg2) else 1
    R = region_mask if region_mask is not None else (KMT > 0).astype(np.int32)
    RM = moc_ref.region_masks(R, nreg, reg2)
    start = moc_ref.region_start(RM, T)
    BIN = moc_ref.bin_map(T, edge)
    return dict(T=T, KMT=KMT, edge=edge, center=center, RM=RM, start=start, BIN=BIN)


def check_against(m, r):
    edge, center = m.lat_aux_grid()
    assert np.array_equal(edge, r["edge"]) and np.array_equal(center, r["center"])          # bit for bit
    inf = m.moc_info()
    assert inf["n_lat_aux_grid"] == center.size and inf["km1"] == m.km + 1 and inf["n_transport_reg"] == r["RM"].shape[0]
    assert inf["lat_aux_region_start"] == r["start"][-1] * (r["RM"].shape[0] > 1)
    assert np.array_equal(m.moc_bin_map(), r["BIN"])
    assert np.array_equal(m.moc_mask(), moc_ref.mask_lat_depth(r["BIN"], r["KMT"], r["RM"], center.size, m.km))


# ---- the test data has what the device tests rely on (NumPy side only) -------------------------------------------------------------
def test_the_test_grid_is_a_hard_one(pkg):
    m = host(pkg)
    R = moc_ref.region_mask(moc_ref.latitudes(m)[2])
    r = restated(m, dict(lat_aux_grid_type="southern"), R, REG2)
    BIN, ocean = r["BIN"], r["KMT"] > 0
    assert any(np.unique(BIN[j][ocean[j]]).size >= 2 for j in range(BIN.shape[0]))           # a row with cells in two bins
    blk = moc_ref.block_of(m)
    rows = np.arange(BIN.shape[0])[:, None] + 0 * BIN
    assert any(np.unique(rows[(BIN == b) & ocean]).size >= 2 and np.unique(blk[(BIN == b) & ocean]).size >= 2 for b in range(1, BIN.max() + 1))
    assert np.all(BIN[ocean] > 0)                                                            # 'southern': every ocean cell lies in a bin
    u = restated(m, dict(lat_aux_grid_type="user-specified", lat_aux_begin=-60.0, lat_aux_end=60.0, n_lat_aux_grid=24))
    assert np.any((u["BIN"] == 0) & ocean)                                                   # 'user-specified': some ocean cell in none
    assert r["RM"][1].sum() > 0 and r["start"][1] + 1 >= 3 and np.any(R < 0)                 # region 2, j_southern >= 3, a marginal sea
    m.close()


# ---- init_lat_aux_grid and init_moc_ts_transport_arrays ------------------------------------------------------------------------
@pytest.mark.parametrize("name,model,nml,two", [
    ("southern", dict(), dict(lat_aux_grid_type="southern"), True),                          # 90 + southern_edge >= dlat / 2: padded to 90
    ("southern_one", dict(), dict(lat_aux_grid_type="southern"), False),
    ("southern_to_pole", dict(lat_span=178.0), dict(lat_aux_grid_type="southern"), False),   # the other branch: the last edge is 90
    ("user", dict(), dict(lat_aux_grid_type="user-specified", lat_aux_begin=-60.0, lat_aux_end=60.0, n_lat_aux_grid=24), True),
    ("user_default", dict(), dict(lat_aux_grid_type="user"), False),                         # -90 .. 90 in 180 bins
    # 'full' asks for TLATD_G(:, j) == TLATD_G(1, j) exactly (:483), and TLAT comes out of a Cartesian average whose rounding follows
    # the longitude: the unbent grid with every ULON the same number (the metrics are records of their own) passes it
    ("full", dict(bend=False, one_longitude=True), dict(lat_aux_grid_type="full"), True),
])
def test_grid_bins_and_masks_match_restatement(pkg, name, model, nml, two):
    m = host(pkg, **model)
    T, U, KMT = moc_ref.latitudes(m)
    R = moc_ref.region_mask(KMT) if two else None
    m.init_transports(R, REG2 if two else (), **nml)
    r = restated(m, nml, R, REG2 if two else ())
    check_against(m, r)
    if name == "southern":
        assert r["edge"][-1] < 90.0 + 1e-9 and r["center"].size > 2 * np.count_nonzero(T[:, 0] < 0)
    if name == "southern_to_pole":
        assert r["edge"][-1] == 90.0 and r["center"].size == 2 * np.count_nonzero(T[:, 0] < 0)
    m.close()


@pytest.mark.parametrize("kw,sub,want", [
    (dict(), None, 1),
    (dict(hmix_tracer=3, ah=0.8e7, gm_diag_bolus=1), None, 2),
    (dict(hmix_tracer=3, ah=0.8e7, gm_diag_bolus=1), dict(submeso_diag=1), 3),
    (dict(hmix_tracer=3, ah=0.8e7), dict(submeso_diag=1), 3),                                # component 2 stays 0, as in the reference
])
def test_n_moc_comp(pkg, kw, sub, want):
    cfg = named_config("tiny", **kw)
    if sub is not None:
        cfg = pkg.submeso_config(cfg, **sub)
    m = host(pkg, cfg=cfg)
    m.init_transports()
    assert m.moc_info()["n_moc_comp"] == want == moc_ref.n_moc_comp(cfg)
    m.close()


def test_refusals_of_the_initialisation(pkg):
    def refused(match, model=None, region=None, reg2=(), cfg=None, **nml):
        m = host(pkg, cfg=cfg, **(model or {}))
        T, U, KMT = moc_ref.latitudes(m)
        R = region(KMT) if region else None
        with pytest.raises(pkg.PopError, match=match):
            m.init_transports(R, reg2, **nml)
        with pytest.raises(pkg.PopError, match="pop_init_transports has not been called"):   # and nothing is left half built
            m.moc_info()
        if not match.startswith("pop_"):                                                      # the reference's own refusals: restated too
            with pytest.raises(moc_ref.Refused, match=match):
                n = dict(nml)
                nreg = n.pop("n_transport_reg", 2 if len(reg2) else 1)
                moc_ref.lat_aux_grid(T, U, partial_bottom_cells=bool(m.cfg.partial_bottom_cells), **n)
                RM = moc_ref.region_masks(R if R is not None else (KMT > 0).astype(np.int32), nreg, reg2)
                moc_ref.region_start(RM, T)
        m.close()

    refused("unknown auxilary latitudinal grid choice", lat_aux_grid_type="northern")
    refused("there are no Southern Hemisphere grid points", model=dict(north_only=True))
    refused("SH is not a regular at-lon grid", model=dict(bend_south=True))
    refused("The model grid is not a regular lat-lon grid", lat_aux_grid_type="full")        # the bent grid
    refused("lat_aux_end should be > lat_aux_begin", lat_aux_grid_type="user-specified", lat_aux_begin=10.0, lat_aux_end=10.0)
    from ice_common import ice_grid
    cfg = named_config("tiny", partial_bottom_cells=1)
    m = pkg.PopModel(cfg, host_only=True, grid=ice_grid(cfg, pbc=True))
    with pytest.raises(pkg.PopError, match=r"if \(partial_bottom_cells\), then 1st modify"):
        m.init_transports()
    m.close()
    refused("n_transport_reg must be > 0", n_transport_reg=0)
    refused("n_transport_reg must be < 3", n_transport_reg=3)
    refused("no transport regions have been detected", region=moc_ref.region_mask, n_transport_reg=2)
    refused("pop_init_transports: n_transport_reg = 2 needs REGION_MASK", reg2=REG2)
    refused("The southern boundary for region 2", region=lambda K: moc_ref.region_mask(K, j_southern=24), reg2=REG2)   # a bent row
    refused("pop_init_transports: region 2 starts in row j = 1", region=lambda K: np.full(K.shape, 6, dtype=np.int32), reg2=REG2)
    cfg = pkg.submeso_config(named_config("tiny", hmix_tracer=3, ah=0.8e7, gm_diag_bolus=1), submeso_diag=0)
    refused("pop_init_transports: the submesoscale component of the MOC .* needs submeso_diag = 1", cfg=cfg)


def test_request_time_refusals(pkg):
    m = host(pkg)
    with pytest.raises(pkg.PopError, match="pop_moc_request: pop_init_transports has not been called"):
        m.moc_request(1)
    m.init_transports()
    with pytest.raises(pkg.PopError, match="pop_init_transports: called twice"):
        m.init_transports()
    for ns in (0, 10):
        with pytest.raises(pkg.PopError, match="pop_moc_request: stream %d is outside 1 .. 9" % ns):
            m.moc_request(ns)
    m.time_manager()
    with pytest.raises(pkg.PopError, match="there is no CPU fallback"):
        m.moc_get()
    m.moc_request(3)                                   # a host-only context is never inside a step
    assert m.dim("moc_stream") == 3
    with pytest.raises(pkg.PopError, match="pop_moc_request: MOC is already requested, in stream 3"):
        m.moc_request(4)
    dtt = m.scalar("dtt")
    m.time_manager()                                   # the stream was switched on by the request: tavg_sum follows it
    assert m.tavg_sums(3)[0] > 0.0 and m.tavg_sums(3)[0] <= dtt
    for call in (lambda: m.tavg_request(1, "MOC"), lambda: m.tavg_info("MOC")):
        with pytest.raises(pkg.PopError, match="MOC is not a slab field: it is requested with pop_moc_request"):
            call()
    for name in ("N_HEAT", "N_SALT"):
        with pytest.raises(pkg.PopError, match=name + " is known to the reference, not built"):
            m.tavg_request(1, name)
    m.close()
    late = host(pkg)
    late.time_manager()
    with pytest.raises(pkg.PopError, match="pop_init_transports: call it before the first step or phase"):
        late.init_transports()
    late.close()
