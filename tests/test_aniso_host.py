"""Anisotropic horizontal viscosity (hmix_momentum = 3, pop_config layout 6): the create-time refusals and version handling, and
the time-independent set-up of init_aniso / compute_ccsm_var_viscosity (hmix_aniso.F90:372-533, 1069-1296) in host-only
contexts against the NumPy restatement of tests/aniso_ref.py.  No GPU."""
import numpy as np
import pytest

import aniso_ref
from popcfg import named_config, synthetic_grid

GEOM = ("H1E", "H1W", "H2N", "H2S", "K1E", "K1W", "K2N", "K2S", "AMAX_CFL")
# CESM's gx3v7 hmix_aniso_nml (bld/namelist_files/namelist_defaults_pop.xml): east-aligned, variable viscosity
GX3V7 = dict(aniso_alignment="east", lvariable_hmix_aniso=1, vconst_1=1.0e7, vconst_2=24.5, vconst_3=0.2, vconst_4=2.0e-8,
             vconst_5=3, vconst_6=1.0e7, vconst_7=45.0)


def ulps(a, b):
    """largest distance in units in the last place between two arrays of finite doubles"""
    ia, ib = a.view(np.int64), b.view(np.int64)
    ia = np.where(ia < 0, np.int64(-2 ** 63) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2 ** 63) - ib, ib)
    return int(np.abs(ia - ib).max())


def _model(pkg, cfg, grid=None, rank=0, nranks=1):
    return pkg.PopModel(cfg, rank=rank, nranks=nranks, host_only=True, grid=grid)


def test_layout6_anis_host_only_create(pkg):
    m = _model(pkg, pkg.anisotropic_config(named_config("tiny"), visc_para=1.0e9, visc_perp=0.5e9))
    for n in GEOM + ("ANGLE",):
        assert np.isfinite(m.get(n)).all()
    m.close()


@pytest.mark.parametrize("kw", [{}, {"hmix_momentum": 4, "am": -1.0e22, "lvariable_hmix": 1}])
def test_layout6_del2_del4_equal_layout5(pkg, kw):
    """version 6 with hmix_momentum 2 or 4 builds the same host fields, bit for bit, as version 5"""
    c5 = named_config("tiny", **kw)
    c6 = pkg.anisotropic_config(c5, hmix_momentum=c5.hmix_momentum)
    assert c6.struct_version == 6 and c6.hmix_momentum == c5.hmix_momentum
    a, b = _model(pkg, c5), _model(pkg, c6)
    for n in ("DXU", "DYU", "HTN", "HTE", "UAREA", "DUC", "DUN", "DMC", "DUM", "AMF", "btropWgtNE", "centerWgt"):
        assert np.array_equal(a.get(n), b.get(n)), n
    assert np.array_equal(a.geti("KMU"), b.geti("KMU"))
    a.close(); b.close()


@pytest.mark.parametrize("kw,word", [({"aniso_alignment": "flow"}, "aniso_alignment"),
                                     ({"lsmag_aniso": 1, "c_para": 1.0, "c_perp": 1.0}, "smag_lat_fact"),
                                     ({"aniso_alignment": 3}, "aniso_alignment")])
def test_refused_options_name_themselves(pkg, kw, word):
    cfg = pkg.anisotropic_config(named_config("tiny"), **kw)
    with pytest.raises(pkg.PopError, match=word):
        _model(pkg, cfg)


def test_layout5_cannot_select_anis(pkg):
    with pytest.raises(pkg.PopError, match="struct_version 6"):
        _model(pkg, named_config("tiny", hmix_momentum=3))


def test_partial_bottom_cells_accepted(pkg):
    _model(pkg, pkg.anisotropic_config(named_config("tiny", partial_bottom_cells=1), visc_para=1.0e9, visc_perp=1.0e9)).close()


def _check_setup(pkg, cfg, grid=None):
    m = _model(pkg, cfg, grid)
    ref = aniso_ref.geometry(m.get("HTN"), m.get("HTE"), m.get("DXUR"), m.get("DYUR"), m.scalar("dtu"))
    for n in GEOM:
        assert np.array_equal(m.get(n), ref[n]), n
    if cfg.lsmag_aniso:
        ds, fps = aniso_ref.smag_fields(m.get("DXU"), m.get("DYU"), m.get("ULAT"), cfg)
        assert np.array_equal(m.get("DSMIN"), ds)
        assert ulps(m.get("F_PERP_SMAG"), fps) <= 2
    if cfg.lvariable_hmix_aniso:
        fpa, fpe = aniso_ref.var_viscosity(m, cfg, m.get("AMAX_CFL"))
        a, b = m.get("F_PARA"), m.get("F_PERP")
        assert a.shape == fpa.shape
        assert ulps(a, fpa) <= 2 and ulps(b, fpe) <= 2
    m.close()
    return m


@pytest.mark.parametrize("name,kw", [("tiny", {}), ("test", {}), ("tiny", {"ew_boundary": 0}), ("gx3v7", {})],
                         ids=["tiny", "test-96-blocks", "tiny-closed-ew", "gx3v7"])
def test_setup_matches_restatement(pkg, name, kw):
    cfg = pkg.anisotropic_config(named_config(name, **kw), **GX3V7)
    _check_setup(pkg, cfg)


def test_smagorinsky_fields_match_restatement(pkg):
    _check_setup(pkg, pkg.anisotropic_config(named_config("tiny"), lsmag_aniso=1, lvariable_hmix_aniso=1, c_para=8.0, c_perp=4.0,
                                             smag_lat_fact=0.98, smag_lat=15.0))


def test_library_distance_on_a_row_with_one_boundary(pkg):
    """the library's F_PARA on a row whose only western boundary is at ig = 6 (KMU = 0 at 5, 6): with vconst_6 negligible and
    Smagorinsky on (no taper) F_PARA = bv0 exp(-(vconst_4 DIST)^2); DIST = 0 for 6 <= ig <= 6 + vconst_5 and then grows by HTN
    point by point (compute_ccsm_var_viscosity :1207-1240)"""
    c5 = named_config("tiny", block_size_x=48, block_size_y=40)
    g = synthetic_grid(c5, stepped=False)
    jg = 20
    k = np.full_like(g["KMT"], c5.km)
    k[jg, 5] = 0                                  # KMT(6, jg + 1), 1-based: KMU = 0 at ig = 5, 6 of rows jg, jg + 1
    g["KMT"] = k
    cfg = pkg.anisotropic_config(c5, lvariable_hmix_aniso=1, lsmag_aniso=1, smag_lat_fact=0.98, vconst_6=1.0e-300, vconst_4=2.0e-8)
    m = _model(pkg, cfg, g)
    b = m.get_block(m.local_block_ids()[0])
    j = list(b["j_glob"]).index(jg)               # 0-based block row of global row jg (1-based)
    i0 = list(b["i_glob"]).index(1)
    f = m.get("F_PARA")[0, 0, j, i0:i0 + 48]
    htn, ulat, dxu = (m.get(n)[0, j, i0:i0 + 48] for n in ("HTN", "ULAT", "DXU"))
    bv0 = 0.2 * (2.0 * aniso_ref.OMEGA * np.cos(ulat) / aniso_ref.RADIUS) * (dxu * dxu * dxu)
    dist = np.zeros(48)
    for ig in range(10, 49):
        dist[ig - 1] = htn[ig - 1] + dist[ig - 2]
    d = 0.0
    for ii in range(10, 49):
        d = htn[ii - 1] + d
    dist[0] = htn[0] + d
    for ig in range(2, 6):
        dist[ig - 1] = htn[ig - 1] + dist[ig - 2]
    want = bv0 * np.exp(-((2.0e-8 * dist) * (2.0e-8 * dist)))
    assert (dist[5:9] == 0.0).all()
    assert np.abs(f - want).max() <= 1.0e-14 * np.abs(want).max()
    m.close()


def test_setup_matches_restatement_tripole(pkg):
    c5 = named_config("tiny", ns_boundary=2, block_size_x=48, block_size_y=10)
    g = synthetic_grid(c5)
    g["ANGLE"] = 0.3 * np.sin(2.0 * np.pi * np.arange(c5.nx_global) / c5.nx_global)[None, :] + 0.0 * g["ULAT"]
    cfg = pkg.anisotropic_config(c5, **GX3V7)
    _check_setup(pkg, cfg, g)
    m = _model(pkg, cfg, g)   # ANGLE is scattered as an NE-corner field: ghost rows beyond the fold read the mirrored address
    ang = m.get("ANGLE")
    assert np.array_equal(ang, aniso_ref.scatter_necorner(m, g["ANGLE"], c5.nx_global, c5.ny_global))
    m.close()


def test_row_without_western_boundary(pkg):
    """a row with no western boundary: DIST = dist_max, so F_PARA = vconst_6 and F_PERP = bu (before the taper)"""
    cfg = pkg.anisotropic_config(named_config("tiny"), lvariable_hmix_aniso=1, lsmag_aniso=1, smag_lat_fact=0.98)   # no taper with lsmag
    m = _model(pkg, cfg)
    fpa, fpe, ulat, kmu = m.get("F_PARA"), m.get("F_PERP"), m.get("ULAT"), m.geti("KMU")
    # all-ocean rows of the internal topography: no land anywhere along the row (|lat| < 75, outside the continents' latitudes)
    KG = aniso_ref.to_global(m, kmu, cfg.nx_global, cfg.ny_global)
    rows = [jg for jg in range(cfg.ny_global) if (KG[jg] >= 1).all()]
    assert rows
    bv = np.minimum(np.abs(ulat * aniso_ref.RADIAN), 45.0) * 90.0 / 45.0 / aniso_ref.RADIAN
    bu = 1.0e7 * (1.0 + 24.5 * (1.0 - np.cos(2.0 * bv)))
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        for j in range(b["jb"] - 1, b["je"]):
            if b["j_glob"][j] - 1 in rows:
                sl = slice(b["ib"] - 1, b["ie"])
                assert (fpa[lb, 0, j, sl] == 1.0e7).all()
                assert np.array_equal(fpe[lb, 0, j, sl], bu[lb, j, sl])
    m.close()


def test_two_ranks_hold_the_single_rank_values(pkg):
    cfg = pkg.anisotropic_config(named_config("tiny"), **GX3V7)
    one = _model(pkg, cfg)
    ids1 = one.local_block_ids()
    full = {n: one.get(n) for n in ("F_PARA", "F_PERP", "AMAX_CFL", "K1W", "K2S")}
    for r in range(2):
        m = _model(pkg, cfg, rank=r, nranks=2)
        for lb, bid in enumerate(m.local_block_ids()):
            for n, a in full.items():
                assert np.array_equal(m.get(n)[lb], a[ids1.index(bid)]), (r, bid, n)
        m.close()
    one.close()
