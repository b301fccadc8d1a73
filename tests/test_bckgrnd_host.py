"""The latitude-varying KPP background diffusivity, host side (pop_init_kpp_bckgrnd): the NumPy restatement (tests/bckgrnd_ref.py) pinned
at single points, the host fields BCKGRND_VDC, BCKGRND_VVC and TLON against it on a grid where every branch holds ocean, the refusals
of the entry point, the no-op call and the order of the two init calls."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import bckgrnd_ref
from bckgrnd_common import banda_arctic_grid
from bckgrnd_ref import CESM, RADIAN
from common import TOL_LOCAL, physical
from popcfg import named_config
from tidal_common import KPP, smooth_flux

EPS = np.finfo(float).eps


def rad(deg):
    """radians x with x * RADIAN == deg exactly where such a value exists near deg / RADIAN (the restatement forms TLATD = TLAT *
    radian), else the nearest"""
    x = deg / RADIAN
    for _ in range(8):
        for c in (x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)):
            if c * RADIAN == deg:
                return c
        x = np.nextafter(x, np.inf)
    return deg / RADIAN


def at(lat_deg, lon_deg, **kw):
    b, m = bckgrnd_ref.field(np.array([rad(lat_deg)]), np.array([rad(lon_deg)]), 0.16, **dict(CESM, **kw))
    return float(b[0]), {n: bool(v[0]) for n, v in m.items()}


def psi(lat):
    return 0.13 * math.exp(-(0.4 * (lat - 28.9)) ** 2), 0.13 * math.exp(-(0.4 * (lat + 28.9)) ** 2)      # psin, psis


def test_restatement_pinned_at_single_points():
    for d in (10.0, -10.0, -1.0, -4.0, -7.0, 103.0, 134.0, 70.0):      # the comparisons below sit exactly on these
        assert rad(d) * RADIAN == d, d
    # the equator: the Gregg minimum; the two maxima contribute 0.13 exp(-133.6) each, which 0.01 absorbs
    b, m = at(0.0, 200.0)
    assert b == 0.01 and m["band"] and not (m["south"] or m["north"])
    # the MacKinnon maxima: one exponential is 1, the other 0.13 exp(-534) is absorbed
    for lat, name in ((28.9, "north"), (-28.9, "south")):
        b, m = at(lat, 200.0)
        assert b == (0.01 + 0.13) + 0.16 and m[name] and not m["band"]
    # exactly +-10: .lt. -10 is false and .le. 10 is true, so both belong to the band, where (lat / 10)**2 = 1: the neighbouring formula's value
    for lat in (10.0, -10.0):
        b, m = at(lat, 200.0)
        pn, ps = psi(lat)
        assert m["band"] and not (m["south"] or m["north"])
        assert abs(b - ((0.01 + pn + ps) + 0.16)) <= 4 * EPS * b
        outside, mo = at(lat * 1.0000001, 200.0)
        assert (mo["north"] or mo["south"]) and abs(outside - b) <= 1.0e-6
    # the Banda Sea boxes: -4 belongs to the middle box and -7 to the south box because of the .le.; -1 and -8.3 are outside
    b, m = at(-4.0, 120.0)
    assert b == 1.0 and m["banda_middle"] and not m["banda_north"] and not m["banda_south"]
    b, m = at(-7.0, 120.0)
    assert b == 1.0 and m["banda_south"] and not m["banda_middle"]
    b, m = at(-2.0, 120.0)
    assert b == 1.0 and m["banda_north"]
    for lat in (-1.0, -8.3):
        b, m = at(lat, 120.0)
        assert b < 0.2 and not (m["banda_north"] or m["banda_middle"] or m["banda_south"])
    # the longitudes 103 and 134 are outside (.gt., .lt.); just inside them the value is the Banda one
    for lon in (103.0, 134.0):
        b, m = at(-2.0, lon)
        assert not m["banda_north"] and not m["banda_middle"] and b < 0.2
    assert at(-2.0, 103.0000001)[0] == 1.0 and at(-2.0, 133.9999999)[0] == 1.0
    # the Arctic: .ge. 70 with larctic_bckgrnd_vdc only
    pn, ps = psi(70.0)
    b, m = at(70.0, 10.0)
    assert abs(b - ((0.01 + pn + ps) + 0.16)) <= 4 * EPS * b and not m["arctic"] and m["north"]
    b, m = at(70.0, 10.0, larctic_bckgrnd_vdc=True)
    assert b == 0.01 and m["arctic"]
    assert not at(69.9999999, 10.0, larctic_bckgrnd_vdc=True)[1]["arctic"]


def first_rows(m):
    out = []
    for bid in m.local_block_ids():
        b = m.get_block(bid)
        out.append(b["jb"] - 1 if b["j_glob"][b["jb"] - 1] == 1 else None)
    return out


DECOMP = [("blocks-12x10", {}), ("padded-20x16", dict(block_size_x=20, block_size_y=16)),
          ("tripole-48x10", dict(ns_boundary=2, block_size_x=48, block_size_y=10))]


@pytest.mark.parametrize("name,kw5", DECOMP, ids=[d[0] for d in DECOMP])
def test_host_fields_match_restatement(pkg, name, kw5):
    cfg = named_config("tiny", **dict(KPP, **kw5))
    m = pkg.PopModel(cfg, host_only=True, grid=banda_arctic_grid(cfg))
    nml = m.init_kpp_bckgrnd(larctic_bckgrnd_vdc=1, **CESM)
    TLAT, TLON = m.get("TLAT"), m.get("TLON")
    ref, masks = bckgrnd_ref.from_nml(TLAT, TLON, cfg.bckgrnd_vdc1, nml)
    ocean = physical(m) & (m.geti("KMT") > 0)
    counts = {n: int((masks[n] & ocean).sum()) for n in bckgrnd_ref.MASKS}
    print(name, "physical ocean cells per branch:", counts)
    for n in ("banda_north", "banda_middle", "banda_south", "arctic"):
        assert counts[n] >= 4, counts
    for n in ("south", "band", "north"):
        assert counts[n] >= 20, counts
    # every cell of every block, ghost cells included; the C library's exp and NumPy's may differ in the last place
    for got, want, what in ((m.get("BCKGRND_VDC"), ref, "BCKGRND_VDC"), (m.get("BCKGRND_VVC"), cfg.Prandtl * ref, "BCKGRND_VVC")):
        assert got.shape == want.shape and np.isfinite(got).all()
        err = np.abs(got - want).max() / np.abs(want).max()
        print("%s: max |library - restatement| / max = %.3e" % (what, err))
        assert err <= TOL_LOCAL, what
    assert np.array_equal(m.get("BCKGRND_VDC") == 1.0, masks["banda_north"] | masks["banda_middle"] | masks["banda_south"])
    # TLON: the physical cells from the block's own U points; the ghost cells carry their source cells' values (checked through the
    # field above, which is compared on them)
    t = bckgrnd_ref.tlon(m.get("ULAT"), m.get("ULON"), first_rows(m))
    phys = physical(m)
    err = np.abs(TLON - t)[phys].max() / np.abs(t[phys]).max()
    print("TLON: max |library - restatement| / max = %.3e" % err)
    assert err <= TOL_LOCAL
    assert TLON.min() >= 0.0 and TLON.max() < 2.0 * np.pi
    m.close()


def _call(pkg, m, nml):
    if m.L.pop_init_kpp_bckgrnd(m.h, C.byref(nml)):
        raise pkg.PopError(m.L.pop_last_error(m.h).decode())


@pytest.mark.parametrize("kw5,kwn,msg", [
    (dict(vmix_choice=1), {}, "lhoriz_varying_bckgrnd needs vmix_choice = 3"),
    (dict(vmix_choice=2), {}, "lhoriz_varying_bckgrnd needs vmix_choice = 3"),
    (dict(vmix_choice=3, bckgrnd_vdc2=0.1), {}, "lhoriz_varying_bckgrnd needs bckgrnd_vdc2 = 0 (vmix_kpp.F90:518)"),
    (KPP, dict(bckgrnd_vdc_eq=-0.01), "negative parameter"),
    (KPP, dict(bckgrnd_vdc_psim=-0.13), "negative parameter"),
    (KPP, dict(bckgrnd_vdc_ban=-1.0), "negative parameter"),
    (KPP, dict(struct_bytes=8), "struct_bytes is not sizeof(pop_kpp_bckgrnd_nml)"),
])
def test_refusals(pkg, kw5, kwn, msg):
    m = pkg.PopModel(named_config("tiny", **kw5), host_only=True)
    with pytest.raises(pkg.PopError, match=re.escape(msg)):
        _call(pkg, m, pkg.kpp_bckgrnd_nml(**kwn))
    m.close()


def test_refusals_of_the_call_itself(pkg):
    cfg = named_config("tiny", **KPP)
    m = pkg.PopModel(cfg, host_only=True)
    _call(pkg, m, pkg.kpp_bckgrnd_nml())
    with pytest.raises(pkg.PopError, match="called a second time"):
        _call(pkg, m, pkg.kpp_bckgrnd_nml())
    m.close()
    m = pkg.PopModel(cfg, host_only=True)
    m.time_manager()
    with pytest.raises(pkg.PopError, match="a step or a phase has already run"):
        _call(pkg, m, pkg.kpp_bckgrnd_nml())
    m.close()
    n = pkg.kpp_bckgrnd_nml()
    assert C.sizeof(pkg.PopKppBckgrndNml) == 3 * 4 + 4 + 3 * 8 and n.struct_bytes == C.sizeof(pkg.PopKppBckgrndNml)   # one pad of 4 bytes before the doubles
    d = pkg.PopKppBckgrndNml()
    pkg.lib().pop_kpp_bckgrnd_nml_init(C.byref(d))
    assert (d.lhoriz_varying_bckgrnd, d.larctic_bckgrnd_vdc, d.bckgrnd_vdc_eq, d.bckgrnd_vdc_psim, d.bckgrnd_vdc_ban) == (0, 0, 0.01, 0.13, 1.0)


def test_zero_is_a_value(pkg):
    """the doubles are taken literally: psim = ban = 0 and bckgrnd_vdc1 = 0 leave eq everywhere but in the boxes, which hold 0"""
    cfg = named_config("tiny", **dict(KPP, bckgrnd_vdc1=0.0))
    m = pkg.PopModel(cfg, host_only=True, grid=banda_arctic_grid(cfg))
    nml = m.init_kpp_bckgrnd(bckgrnd_vdc_eq=0.25, bckgrnd_vdc_psim=0.0, bckgrnd_vdc_ban=0.0)
    _, masks = bckgrnd_ref.from_nml(m.get("TLAT"), m.get("TLON"), 0.0, nml)
    box = masks["banda_north"] | masks["banda_middle"] | masks["banda_south"]
    B = m.get("BCKGRND_VDC")
    assert box.any() and np.all(B[box] == 0.0) and np.all(B[~box] == 0.25)
    m.close()


def test_off_builds_nothing(pkg):
    cfg = named_config("tiny", **KPP)
    m = pkg.PopModel(cfg, host_only=True)
    m.init_kpp_bckgrnd(lhoriz_varying_bckgrnd=0)
    for n in ("BCKGRND_VDC", "BCKGRND_VVC"):
        with pytest.raises(pkg.PopError, match=n + " exists after pop_init_kpp_bckgrnd"):
            m.get(n)
    with pytest.raises(pkg.PopError, match="called a second time"):
        m.init_kpp_bckgrnd()
    m.close()
    # off needs neither KPP nor bckgrnd_vdc2 = 0: nothing is built
    m = pkg.PopModel(named_config("tiny", vmix_choice=1), host_only=True)
    m.init_kpp_bckgrnd(lhoriz_varying_bckgrnd=0)
    m.close()


def test_call_order_with_tidal_mixing(pkg):
    cfg = named_config("tiny", **KPP)
    grid = banda_arctic_grid(cfg)
    out = []
    for first in ("bckgrnd", "tidal"):
        m = pkg.PopModel(cfg, host_only=True, grid=grid)
        F = smooth_flux(m, 0.02)
        if first == "bckgrnd":
            m.init_kpp_bckgrnd(**CESM); m.init_tidal_mixing(F)
        else:
            m.init_tidal_mixing(F); m.init_kpp_bckgrnd(**CESM)
        out.append({n: m.get(n) for n in ("BCKGRND_VDC", "BCKGRND_VVC", "TLON", "TIDAL_COEF_3D", "TIDAL_ENERGY_FLUX")})
        m.close()
    for n in out[0]:
        assert np.array_equal(out[0][n], out[1][n]), n
    assert out[0]["BCKGRND_VDC"].max() == 1.0
