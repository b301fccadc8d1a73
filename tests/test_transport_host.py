"""The host side of the northward heat and salt transports (pop_transport_request / pop_transport_info on host-only contexts):
n_transport_comp in the four configurations, the rules of the request and every refusal, the stream it switches on, and the getter's
answer where there is no device.  The grid is that of tests/test_moc_host.py (moc_ref.bent_grid of 'tiny')."""
import numpy as np
import pytest

import moc_ref
import transport_ref
from popcfg import named_config

REG2 = (6,)
GM = dict(hmix_tracer=3, ah=0.8e7)


def host(pkg, cfg=None, **kw):
    cfg = cfg if cfg is not None else named_config("tiny", **kw)
    return pkg.PopModel(cfg, host_only=True, grid=moc_ref.bent_grid(cfg))


def two_regions(m):
    m.init_transports(moc_ref.region_mask(moc_ref.latitudes(m)[2]), REG2)


@pytest.mark.parametrize("kw,sub,want", [
    (dict(), None, 3),
    (dict(GM, gm_diag_bolus=1), None, 4),
    (dict(GM, gm_diag_bolus=1), dict(submeso_diag=1), 5),
    (dict(GM), dict(submeso_diag=1), 5),                                                     # component 4 stays 0, as in the reference
])
def test_n_transport_comp(pkg, kw, sub, want):
    cfg = named_config("tiny", **kw)
    if sub is not None:
        cfg = pkg.submeso_config(cfg, **sub)
    m = host(pkg, cfg=cfg)
    assert m.dim("n_transport_comp") == 0                                                    # before pop_init_transports
    m.init_transports()
    inf = m.transport_info()
    assert inf["n_transport_comp"] == want == transport_ref.n_transport_comp(cfg) == m.dim("n_transport_comp")
    assert inf["n_lat_aux_grid"] == m.moc_info()["n_lat_aux_grid"] and inf["n_transport_reg"] == 1
    assert (inf["stream"], inf["heat"], inf["salt"]) == (0, False, False) and m.dim("transport_stream") == 0
    m.close()


def test_request_rules_and_refusals(pkg):
    m = host(pkg)
    for call in (lambda: m.transport_request(1), m.transport_info):
        with pytest.raises(pkg.PopError, match="pop_init_transports has not been called"):
            call()
    two_regions(m)
    for ns in (0, 10):
        with pytest.raises(pkg.PopError, match="pop_transport_request: stream %d is outside 1 .. 9" % ns):
            m.transport_request(ns)
    with pytest.raises(pkg.PopError, match="pop_transport_request: neither heat nor salt is asked for"):
        m.transport_request(2, heat=False, salt=False)
    assert m.tavg_sums(4)[0] == 0.0
    m.time_manager()                                                                         # the stream is not on yet
    assert m.tavg_sums(4)[0] == 0.0
    m.transport_request(4, heat=True, salt=False)                                            # a host-only context is never inside a step
    inf = m.transport_info()
    assert (inf["stream"], inf["heat"], inf["salt"], inf["n_transport_reg"]) == (4, True, False, 2) and m.dim("transport_stream") == 4
    with pytest.raises(pkg.PopError, match="pop_transport_request: the transports are already requested, in stream 4"):
        m.transport_request(5)
    dtt = m.scalar("dtt")
    m.time_manager()                                                                         # switched on by the request: tavg_sum follows it
    assert 0.0 < m.tavg_sums(4)[0] <= dtt
    m.tavg_on(4, False)
    s = m.tavg_sums(4)[0]
    m.time_manager()
    assert m.tavg_sums(4)[0] == s
    for call in (lambda: m.transport_get("heat"), m.transport_sums):
        with pytest.raises(pkg.PopError, match="there is no CPU fallback"):
            call()
    # the slab entries stay left out, in the words the MOC's tests pin; N_HEAT / N_SALT name the new request
    for name in ("N_HEAT", "N_SALT"):
        for call in (lambda: m.tavg_request(1, name), lambda: m.tavg_info(name)):
            with pytest.raises(pkg.PopError, match=name + r" is known to the reference, not built \(DESIGN.md section 14\).*pop_transport_request"):
                call()
    for name in ("ADVT", "ADVS", "HDIFT", "HDIFS", "VNT", "VNS"):
        with pytest.raises(pkg.PopError, match=name + r" is known to the reference, not built \(DESIGN.md section 14\)$"):
            m.tavg_request(1, name)
    m.close()


def test_moc_and_transports_share_a_stream(pkg):
    m = host(pkg)
    m.init_transports()
    m.moc_request(2)
    m.transport_request(2)
    assert m.dim("moc_stream") == 2 == m.dim("transport_stream")
    m.time_manager()
    assert m.tavg_sums(2)[0] > 0.0
    m.close()


def test_lw_lim_needs_one_region(pkg):
    m = host(pkg, tadvect=3)
    two_regions(m)
    with pytest.raises(pkg.PopError, match="lw_lim.*n_transport_reg = 2: the north-face value of lw_lim is not kept"):
        m.transport_request(1)
    assert m.transport_info()["stream"] == 0
    m.close()
    one = host(pkg, tadvect=3)
    one.init_transports()
    one.transport_request(1)                                                                 # built from LTK
    assert one.transport_info()["stream"] == 1
    one.close()


def test_submeso_needs_submeso_diag(pkg):
    """n_transport_comp = 5 needs USUBM, VSUBM: pop_init_transports refuses the configuration, naming the switch, so no request follows"""
    cfg = pkg.submeso_config(named_config("tiny", **dict(GM, gm_diag_bolus=1)), submeso_diag=0)
    m = host(pkg, cfg=cfg)
    with pytest.raises(pkg.PopError, match="needs submeso_diag = 1"):
        m.init_transports()
    with pytest.raises(pkg.PopError, match="pop_transport_request: pop_init_transports has not been called"):
        m.transport_request(1)
    m.close()


def test_entry_points_check_their_arguments(pkg):
    """a host-only context is never inside a step (pop_time_manager sets the flag on device contexts only), so the refusal of a
    request between pop_time_manager and pop_step_tail is checked in tests/test_gpu_transport.py; here the C entry points themselves"""
    import ctypes
    m = host(pkg)
    m.init_transports()
    assert m.L.pop_transport_request(None, 1, 1, 1) == 1                                     # no context
    assert m.L.pop_transport_sums_count(m.h) == m.transport_info()["n_lat_aux_grid"] * 2 * 4
    assert m.L.pop_transport_get(m.h, 3, 1, 0, ctypes.POINTER(ctypes.c_double)(), 0) == 1
    m.close()


def test_masked_entries_of_the_restatement():
    """NumPy side only: :1563-1578 on a small mask"""
    MASK = np.zeros((5, 2, 2), dtype=bool)
    MASK[0, 0, :] = True; MASK[1, 0, 0] = True; MASK[4, 0, 1] = True; MASK[3, 1, 0] = True   # level 2 is not looked at
    got = transport_ref.masked_entries(MASK, 3)
    assert got[:, :, 0].all(axis=1).tolist() == [True, True, False, False, False, False]
    assert got[:, 1, 1].tolist() == [True, False, False, False, False, True]
    assert got[:, 0, 1].all() and got[:, 2, 1].all()
