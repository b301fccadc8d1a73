"""Jayne tidal mixing, host side: the init-time fields of pop_init_tidal_mixing against the NumPy restatement (tests/tidal_ref.py), the
normalisation of the vertical function, the refusals of the entry point, and the restatement's recurrence pinned against two
hand-written columns."""
import ctypes as C
import re

import numpy as np
import pytest

import tidal_ref
from common import physical
from popcfg import named_config
from tidal_common import BOXES, KPP, smooth_flux, stepped_grid

EPS = np.finfo(float).eps


def test_host_fields_match_restatement(pkg):
    cfg = named_config("tiny", **KPP)
    grid = stepped_grid(cfg)
    assert set(np.unique(grid["KMT"])) == {0, 3, 4, 5, cfg.km}
    m = pkg.PopModel(cfg, host_only=True, grid=grid)
    F = smooth_flux(m, 0.02)
    nml = m.init_tidal_mixing(F, regions=BOXES, tidal_diag=1)
    m.halo_update_host_loc(F)                     # what the call does to its copy of the record
    r = tidal_ref.host_from_model(m, nml, F)
    assert np.array_equal(m.get("TIDAL_ENERGY_FLUX"), r["EF"])
    box = m.geti("TIDAL_REGION_BOX2D")
    assert np.array_equal(box, r["BOX"])
    phys = physical(m) & (r["KMT"] > 0)
    counts = [int(((box == q + 1) & phys).sum()) for q in range(3)]
    print("ocean columns per box:", counts)
    assert min(counts) > 10, counts
    # exp() of the C library and of NumPy may differ in the last place or two; WORK is a sum of positive terms added in the same
    # order, so the quotient differs by a few units in the last place: 16 eps relative, every cell, ghost cells included
    coef = m.get("TIDAL_COEF_3D")
    assert coef.shape == r["COEF"].shape and np.isfinite(coef).all()
    err = np.abs(coef - r["COEF"]).max() / np.abs(r["COEF"]).max()
    rel = (np.abs(coef - r["COEF"]) / np.where(r["COEF"] != 0.0, np.abs(r["COEF"]), 1.0)).max()
    print("TIDAL_COEF_3D: max error / max %.3e, max relative error %.3e" % (err, rel))
    assert rel <= 16 * EPS
    assert np.array_equal(coef == 0.0, r["COEF"] == 0.0)
    lev = np.arange(1, m.km + 1)[None, :, None, None]
    assert np.all(coef[np.broadcast_to(lev > r["KMT"][:, None], coef.shape)] == 0.0)
    assert np.all(coef[np.broadcast_to(r["KMT"][:, None] <= 1, coef.shape)] == 0.0)
    with pytest.raises(pkg.PopError, match="context was created host-only"):
        m.get("TIDAL_DIFF")
    m.close()


def test_vertical_function_integrates_to_one(pkg):
    """flat bottom: sum over k < KMT of VERTICAL_FUNC(k) dzw(k) = 1.  Each term carries two roundings and the sum of n positive terms
    n - 1 more, the factors of TIDAL_COEF_2D three: (km + 4) half-units in the last place at most; the bound below is twice that"""
    cfg = named_config("tiny", **KPP)
    m = pkg.PopModel(cfg, host_only=True)
    F = np.ones((m.nblocks, m.nyb, m.nxb))
    nml = m.init_tidal_mixing(F)
    KMT = m.geti("KMT")
    vg = tidal_ref.submeso_ref.vertical(m.km)
    VF, _ = tidal_ref.vertical_func(KMT, m.get("HT"), vg, 500.0e2)
    coef = m.get("TIDAL_COEF_3D")
    flat = KMT == m.km
    assert flat.sum() > 100
    s_ref, s_lib = np.zeros(KMT.shape), np.zeros(KMT.shape)
    for k in range(1, m.km):
        s_ref += VF[:, k - 1] * vg["dzw"][k]
        s_lib += coef[:, k - 1] * vg["dzw"][k]
    c2 = (nml.tidal_mixing_efficiency / 1.0) * 1.0 * (nml.tidal_local_mixing_fraction * 1000.0)
    e_ref, e_lib = np.abs(s_ref[flat] - 1.0).max(), np.abs(s_lib[flat] / c2 - 1.0).max()
    print("sum VERTICAL_FUNC dzw - 1: restatement %.3e, library %.3e" % (e_ref, e_lib))
    assert e_ref <= (m.km + 4) * EPS and e_lib <= (m.km + 4) * EPS
    m.close()


def _nml(pkg, **kw):
    return pkg.tidal_nml(**kw)


def _call(pkg, m, nml, F=None, count=None):
    F = np.zeros((m.nblocks, m.nyb, m.nxb)) if F is None else F
    e = m.L.pop_init_tidal_mixing(m.h, C.byref(nml), F.ctypes.data_as(C.POINTER(C.c_double)), F.size if count is None else count)
    if e:
        raise pkg.PopError(m.L.pop_last_error(m.h).decode())


@pytest.mark.parametrize("kw5,kwn,msg", [
    (dict(vmix_choice=1), {}, "tidal mixing needs vmix_choice = 3"),
    (dict(vmix_choice=2), {}, "tidal mixing needs vmix_choice = 3"),
    (dict(vmix_choice=3, bckgrnd_vdc2=0.1), {}, "tidal mixing needs bckgrnd_vdc2 = 0"),
    (KPP, dict(tidal_mixing_method="schmittner"), "tidal_mixing_method 0 'jayne' only"),
    (KPP, dict(tidal_mixing_method="polzin"), "tidal_mixing_method 0 'jayne' only"),
    (KPP, dict(tidal_local_mixing_fraction=-0.33), "negative parameter"),
    (KPP, dict(tidal_mixing_efficiency=-0.2), "negative parameter"),
    (KPP, dict(vertical_decay_scale=-500.0e2), "negative parameter"),
    (KPP, dict(tidal_mix_max=-100.0), "negative parameter"),
    (KPP, dict(num_tidal_min_regions=10), "num_tidal_min_regions out of range"),
    (KPP, dict(num_tidal_min_regions=-1), "num_tidal_min_regions out of range"),
    (KPP, dict(struct_bytes=8), "struct_bytes is not sizeof(pop_tidal_nml)"),
])
def test_refusals(pkg, kw5, kwn, msg):
    m = pkg.PopModel(named_config("tiny", **kw5), host_only=True)
    with pytest.raises(pkg.PopError, match=re.escape(msg)):
        _call(pkg, m, _nml(pkg, **kwn))
    m.close()


def test_refusals_of_the_call_itself(pkg):
    cfg = named_config("tiny", **KPP)
    m = pkg.PopModel(cfg, host_only=True)
    with pytest.raises(pkg.PopError, match="count mismatch for the energy flux"):
        _call(pkg, m, _nml(pkg), count=m.nxb * m.nyb)
    _call(pkg, m, _nml(pkg))
    with pytest.raises(pkg.PopError, match="called a second time"):
        _call(pkg, m, _nml(pkg))
    m.close()
    m = pkg.PopModel(cfg, host_only=True)
    _call(pkg, m, _nml(pkg, ltidal_mixing=0))          # succeeds, builds nothing
    with pytest.raises(pkg.PopError, match="TIDAL_COEF_3D exists after pop_init_tidal_mixing"):
        m.get("TIDAL_COEF_3D")
    with pytest.raises(pkg.PopError, match="called a second time"):
        _call(pkg, m, _nml(pkg))
    m.close()
    m = pkg.PopModel(cfg, host_only=True)
    m.time_manager()
    with pytest.raises(pkg.PopError, match="a step or a phase has already run"):
        _call(pkg, m, _nml(pkg))
    m.close()
    assert C.sizeof(pkg.PopTidalNml) == 9 * 4 + 4 + 4 * 8 + 5 * 9 * 8 + 9 * 4 + 4   # two pads of 4 bytes (before the doubles, at the end)


HOST_FIELDS = ("HT", "HU", "TLAT", "ULAT", "ULON", "HTE", "HTN", "DXU", "DYU", "TAREA", "UAREA", "RCALCT", "FCOR", "FCORT", "AU0")


def test_no_effect_when_off_or_zero(pkg):
    cfg = named_config("tiny", **KPP)
    plain = pkg.PopModel(cfg, host_only=True)
    off = pkg.PopModel(cfg, host_only=True)
    off.init_tidal_mixing(np.ones((off.nblocks, off.nyb, off.nxb)), ltidal_mixing=0)
    zero = pkg.PopModel(cfg, host_only=True)
    zero.init_tidal_mixing(np.zeros((zero.nblocks, zero.nyb, zero.nxb)))
    for n in HOST_FIELDS:
        assert np.array_equal(plain.get(n), off.get(n)) and np.array_equal(plain.get(n), zero.get(n)), n
    for n in ("KMT", "KMU"):
        assert np.array_equal(plain.geti(n), off.geti(n)) and np.array_equal(plain.geti(n), zero.geti(n)), n
    assert np.all(zero.get("TIDAL_COEF_3D") == 0.0) and np.all(zero.geti("TIDAL_REGION_BOX2D") == 0)
    for m in (plain, off, zero):
        m.close()


def test_restatement_pinned_against_hand_written_columns():
    """km = 8; column A has KMT = 6 and takes N2 <= 0 (k = 2), the cap (k = 1), the stability control raising (k = 4 = KMT - 2) and
    not raising (k = 5 = KMT - 1); column B has KMT = 4, where k = 2 = KMT - 2 is excluded by k > 2 and k = 3 = KMT - 1 is raised.
    Every level is 2 cm thick here, so the quotients are exact."""
    km = 8
    KMT = np.array([[[6, 4]]], dtype=np.int32)
    DBLOC, COEF = np.zeros((1, km, 1, 2)), np.zeros((1, km, 1, 2))
    DBLOC[0, :5, 0, 0] = [4.0, -2.0, 0.5, 2.0, 2.0]
    COEF[0, :6, 0, 0] = [1024.0, 7.0, 12.5, 10.0, 70.0, 9.0]      # the values at k = 2 and at k = KMT are never used
    DBLOC[0, :3, 0, 1] = [4.0, 2.0, 2.0]
    COEF[0, :4, 0, 1] = [80.0, 5.0, 3.0, 9.0]
    P = dict(mix_max=100.0, lmax=True, stabc=True, lregions=False, regions=[])
    bvdc = np.full(km + 2, 0.16)
    r = tidal_ref.recurrence(DBLOC, COEF, KMT, np.zeros((1, 1, 2), dtype=np.int32), lambda k: 2.0, bvdc, 10.0, P)
    n2_a, td_a = [2.0, -1.0, 0.25, 1.0, 1.0, 0, 0, 0], [100.0, 0.0, 50.0, 50.0, 70.0, 0, 0, 0]
    n2_b, td_b = [2.0, 1.0, 1.0, 0, 0, 0, 0, 0], [40.0, 5.0, 5.0, 0, 0, 0, 0, 0]
    assert r["N2"][0, :, 0, 0].tolist() == n2_a and r["N2"][0, :, 0, 1].tolist() == n2_b
    assert r["DIFF"][0, :, 0, 0].tolist() == td_a and r["DIFF"][0, :, 0, 1].tolist() == td_b
    for col, td, kmt in ((0, td_a, 6), (1, td_b, 4)):
        kv = [min(0.16 + t, 100.0) if k + 1 < kmt else 0.0 for k, t in enumerate(td)]
        kvm = [10.0 * min((10.0 * 0.16) / 10.0 + t, 100.0) if k + 1 < kmt else 0.0 for k, t in enumerate(td)]
        assert r["KVMIX"][0, :, 0, col].tolist() == kv and r["KVMIX_M"][0, :, 0, col].tolist() == kvm
    assert r["KVMIX"][0, 0, 0, 0] == 100.0 and r["KVMIX_M"][0, 0, 0, 0] == 1000.0     # the second cap, on the sum
    # the switches one at a time: without the cap k = 1 keeps 512 (KVMIX is still limited), without the stability control k = 4 keeps 10
    r = tidal_ref.recurrence(DBLOC, COEF, KMT, np.zeros((1, 1, 2), dtype=np.int32), lambda k: 2.0, bvdc, 10.0, dict(P, lmax=False))
    assert r["DIFF"][0, :5, 0, 0].tolist() == [512.0, 0.0, 50.0, 50.0, 70.0] and r["KVMIX"][0, 0, 0, 0] == 100.0
    r = tidal_ref.recurrence(DBLOC, COEF, KMT, np.zeros((1, 1, 2), dtype=np.int32), lambda k: 2.0, bvdc, 10.0, dict(P, stabc=False))
    assert r["DIFF"][0, :5, 0, 0].tolist() == [100.0, 0.0, 50.0, 10.0, 70.0] and r["DIFF"][0, :3, 0, 1].tolist() == [40.0, 5.0, 3.0]
    # a region box with klevels = 2 and a floor of 60 raises k = 4, 5 of column A (k > 2, KMT - 2 .. KMT - 1) and k = 3 of column B
    PB = dict(P, lregions=True, regions=[dict(min_value=60.0, klevels=2)])
    r = tidal_ref.recurrence(DBLOC, COEF, KMT, np.ones((1, 1, 2), dtype=np.int32), lambda k: 2.0, bvdc, 10.0, PB)
    assert r["DIFF"][0, :5, 0, 0].tolist() == [100.0, 0.0, 50.0, 60.0, 70.0] and r["DIFF"][0, :3, 0, 1].tolist() == [40.0, 5.0, 60.0]
