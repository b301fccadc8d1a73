"""Submesoscale mixed-layer eddy scheme, host side: pop_config layout 7 through submeso_config, the refusals of pop_create, TIME_SCALE of
the host set-up, and the NumPy restatement (tests/submeso_ref.py) pinned against a closed form of its own."""
import ctypes as C

import numpy as np
import pytest

import submeso_ref
from popcfg import named_config
from submeso_common import CLOSED_FORM_ULPS, GM, closed_form, linear_state, open_ocean


def test_layout7_round_trip(pkg):
    c5 = named_config("tiny", **GM)
    c7 = pkg.submeso_config(c5, efficiency_factor=0.05, submeso_diag=1)
    assert c7.struct_version == 7 and c7.lsubmesoscale_mixing == 1 and c7.submeso_diag == 1 and c7.efficiency_factor == 0.05
    assert c7.nx_global == c5.nx_global and c7.ah == c5.ah and c7.hmix_tracer == 3 and c7.aniso_alignment == 0
    # a layout-6 base keeps its members, and a layout-7 base is copied, not extended again
    c6 = pkg.anisotropic_config(c5, aniso_alignment="east", visc_para=2.0e9)
    d7 = pkg.submeso_config(c6, time_scale_constant=8.64e4)
    assert d7.hmix_momentum == 3 and d7.aniso_alignment == 1 and d7.visc_para == 2.0e9 and d7.time_scale_constant == 8.64e4
    e7 = pkg.submeso_config(d7, lsubmesoscale_mixing=0)
    assert type(e7) is type(d7) and C.sizeof(e7) == C.sizeof(d7) and e7.lsubmesoscale_mixing == 0 and e7.time_scale_constant == 8.64e4
    assert C.sizeof(c7) == C.sizeof(d7) == C.sizeof(c6) + 3 * 4 + 4 + 3 * 8
    for cfg in (c7, d7, e7):
        pkg.PopModel(cfg, host_only=True).close()
    with pytest.raises(AttributeError):
        pkg.submeso_config(c5, no_such_member=1)


def test_layout5_and_layout6_are_still_read(pkg):
    c5 = named_config("tiny", **GM)
    a = pkg.PopModel(c5, host_only=True)
    b = pkg.PopModel(pkg.submeso_config(c5, lsubmesoscale_mixing=0), host_only=True)
    for n in ("HTE", "FCORT", "gmHYX"):
        assert np.array_equal(a.get(n), b.get(n)), n
    with pytest.raises(pkg.PopError):
        a.get("SUBM_TIME_SCALE")
    a.close(); b.close()
    pkg.PopModel(pkg.anisotropic_config(c5, visc_para=1.0e9), host_only=True).close()
    bad = pkg.submeso_config(c5)
    bad.struct_version = 8
    with pytest.raises(pkg.PopError, match="struct_version is 8, this library reads 5, 6 and 7"):
        pkg.PopModel(bad, host_only=True)


@pytest.mark.parametrize("kw5,kw7,msg", [
    (dict(hmix_tracer=2), {}, "lsubmesoscale_mixing with hmix_tracer = 2 | 4 is not built"),
    (dict(hmix_tracer=4, ah=-1.0e21), {}, "lsubmesoscale_mixing with hmix_tracer = 2 | 4 is not built"),
    (dict(hmix_tracer=3, partial_bottom_cells=1), {}, "partial_bottom_cells"),
    (GM, dict(efficiency_factor=-0.07), "efficiency_factor: >= 0"),
    (GM, dict(time_scale_constant=-1.0), "time_scale_constant: >= 0"),
    (GM, dict(hor_length_scale=-5.0e5), "hor_length_scale: >= 0"),
    (GM, dict(lsubmesoscale_mixing=2), "lsubmesoscale_mixing: 0 or 1"),
    (GM, dict(luse_const_horiz_len_scale=2), "luse_const_horiz_len_scale: 0 or 1"),
    (GM, dict(submeso_diag=-1), "submeso_diag: 0 or 1"),
])
def test_refusals(pkg, kw5, kw7, msg):
    import re
    with pytest.raises(pkg.PopError, match=re.escape(msg)):
        pkg.PopModel(pkg.submeso_config(named_config("tiny", **kw5), **kw7), host_only=True)


def test_a_layout6_struct_cannot_carry_the_switch(pkg):
    """the members beyond a struct's own layout are not read: a layout-7 image announced as layout 6 builds no submeso set-up"""
    c7 = pkg.submeso_config(named_config("tiny", **GM))
    c7.struct_version = 6
    m = pkg.PopModel(c7, host_only=True)
    with pytest.raises(pkg.PopError):
        m.get("SUBM_TIME_SCALE")
    m.close()


@pytest.mark.parametrize("tsc", [0.0, 8.64e4])
def test_time_scale(pkg, tsc):
    """TIME_SCALE = 1 / sqrt(FCORT**2 + 1 / time_scale_constant**2) on every cell, ghost cells included; 0 = 3.456e5 s"""
    m = pkg.PopModel(pkg.submeso_config(named_config("tiny", **GM), time_scale_constant=tsc), host_only=True)
    ts, f = m.get("SUBM_TIME_SCALE"), m.get("FCORT")
    want = 1.0 / np.sqrt(f * f + 1.0 / ((tsc or 3.456e5) ** 2))
    assert ts.shape == f.shape and np.abs(ts / want - 1.0).max() <= 4 * np.finfo(float).eps
    assert ts.max() <= (tsc or 3.456e5) and ts.min() > 0.0
    m.close()


def test_restatement_against_closed_form(pkg):
    a, c, b, eff, hls0 = 2.0 ** -6, -2.0 ** -5, -2.0 ** -3, 0.07, 5.0e5   # powers of two: T and its differences are exact in binary64
    cfg = pkg.submeso_config(named_config("tiny", **GM), luse_const_horiz_len_scale=1)
    m = pkg.PopModel(cfg, host_only=True)
    T, S, lin = linear_state(m, a=a, c=c, b=b)
    # a host-only model has no equation of state to call: a linear one stands in (the pin is on the algebra of the restatement; the
    # device test repeats it with the model's own DRDT)
    r = submeso_ref.from_model(m, cfg, T, S, drd=(-2.0e-4 * (1.0 + 0.02 * T), np.full_like(T, 0.78)))
    ok = open_ocean(r) & lin
    assert ok.sum() > 100
    # only the two half cells of level 1 carry a stream function
    assert np.all(r["SFX"][:, :, :, 1:] == 0.0) and np.all(r["SFY"][:, :, :, 1:] == 0.0)
    assert np.abs(r["SFX"][:, 0, 0, 0][ok]).min() > 0.0
    assert np.array_equal(r["SFX"][:, :, 0, 0], r["SFX"][:, :, 1, 0])
    g1, g2, big = closed_form(r, a, c, b, eff, hls0)
    tol = CLOSED_FORM_ULPS * np.finfo(float).eps
    t = r["TEND"]
    assert np.abs(t[:, 0, 0][ok]).max() > 0.0
    assert (np.abs(t[:, 0, 0] - g1)[ok] <= tol * big[ok]).all()
    assert (np.abs(t[:, 0, 1] - g2)[ok] <= tol * big[ok]).all()
    assert np.all(t[:, 0, 2:][np.broadcast_to(ok[:, None], t[:, 0, 2:].shape)] == 0.0)
    assert np.all(t[:, 1][np.broadcast_to(ok[:, None], t[:, 1].shape)] == 0.0)   # uniform S
    m.close()
