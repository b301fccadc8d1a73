"""The latitude-varying KPP background diffusivity on the GPU (pop_init_kpp_bckgrnd; k_kpp_bckgrnd, k_kpp_tidal<., true>): row by row
against the unchanged CPU oracle, the coefficients below the boundary layer against a run with a uniform background, a uniform field
bit for bit against the per-level background, the tidal diagnostics, every KPP kernel form, the look-ahead, and two ranks."""
import os

import numpy as np
import pytest

import tidal_ref
from bckgrnd_common import FIELDS, ORACLE_CASES, STEPPED, banda_arctic_grid, feed_oracle, restated, set_flux
from bckgrnd_ref import CESM
from common import TOL_LOCAL, physical
from mr_launch import ROOT, run_check
from orclib import Oracle
from popcfg import named_config
from tidal_common import KPP, amplitude, noisy_state, set_state, unit_flux

pytestmark = pytest.mark.gpu


def outputs(m, diag=False):
    out = {n: m.get(*a) for n, a in FIELDS}
    if diag:
        out.update({n: m.get(n) for n in ("TIDAL_DIFF", "KVMIX", "KVMIX_M")})
    return out


def run(pkg, cfg, grid=None, tuning=None, bck=CESM, tidal=None, tidal_first=False, **tidal_kw):
    """a model with the noisy state set, the varying background initialised (bck: keywords of kpp_bckgrnd_nml, None: no call), tidal
    mixing too (tidal: flux amplitude [W/m^2], None: no call; before or after the other call) and the "vmix" phase run once"""
    m = pkg.PopModel(cfg, grid=grid, tuning=tuning)
    T, S = set_state(m)
    set_flux(m)
    F = None if tidal is None else tidal * unit_flux(m)
    nml = None
    if tidal_first and F is not None:
        nml = m.init_tidal_mixing(F, **tidal_kw)
    if bck is not None:
        m.init_kpp_bckgrnd(**bck)
    if not tidal_first and F is not None:
        nml = m.init_tidal_mixing(F, **tidal_kw)
    m.time_manager()
    m.run_phase("vmix")
    return m, T, S, F, nml


@pytest.mark.parametrize("name,kw5,own_grid", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_rows_match_oracle(pkg, orclib_built, name, kw5, own_grid):
    """KPP depends on the background column by column (only the average to VVC mixes rows), and on a lat-lon grid the field takes few
    distinct values: for each value v the oracle runs with the uniform bckgrnd_vdc1 = v, and the device's varying run is compared
    with it on the physical ocean columns where the restated field equals v.  Every physical ocean column is compared."""
    cfg = named_config("tiny", **dict(KPP, **kw5))
    grid = banda_arctic_grid(cfg) if own_grid else None
    gpu = pkg.PopModel(cfg, grid=grid)
    T, S = noisy_state(gpu)
    for k in range(gpu.km):      # ghost cells from their source cells
        for X in (T, S):
            x = np.ascontiguousarray(X[:, k]); gpu.halo_update_host_loc(x); X[:, k] = x
    o0 = Oracle(cfg, grid=grid)
    R = feed_oracle(o0, T, S)
    o0.close()
    for tl in (0, 1, 2):
        gpu.set("TRACER", T, tl=tl, n=0); gpu.set("TRACER", S, tl=tl, n=1)
    for tl in (0, 1):
        gpu.set("RHO", R, tl=tl)
    gpu.init_kpp_bckgrnd(**CESM)
    gpu.time_manager(); gpu.run_phase("vmix")
    KMT = gpu.geti("KMT")
    ocean = physical(gpu) & (KMT > 0)
    D = tidal_ref.dbloc(gpu, T, S, KMT)
    wet = (np.arange(1, gpu.km + 1)[None, :, None, None] < KMT[:, None]) & ocean[:, None]
    print("interfaces: %d stable, %d unstable" % ((D[wet] > 0).sum(), (D[wet] < 0).sum()))
    assert (D[wet] > 0).sum() > 20 and (D[wet] < 0).sum() > 20
    ref, masks = restated(gpu, cfg)
    assert relmax(gpu.get("BCKGRND_VDC"), ref) <= TOL_LOCAL
    if own_grid:
        assert min(int((masks[n] & ocean).sum()) for n in ("banda_north", "banda_middle", "banda_south")) >= 4
    values = np.unique(ref[ocean])
    print("%s: %d distinct values of the field, %.4f .. %.4f" % (name, len(values), values.min(), values.max()))
    assert 3 <= len(values) <= cfg.ny_global + 1
    got = {"VDC0": gpu.get("VDC", 1, 0), "VDC1": gpu.get("VDC", 1, 1), "SRC0": gpu.get("KPP_SRC", 1, 0), "SRC1": gpu.get("KPP_SRC", 1, 1),
           "HBLT": gpu.get("HBLT")}
    diff, scale, seen = {n: 0.0 for n in got}, {n: 0.0 for n in got}, np.zeros(ocean.shape, dtype=bool)
    for v in values:
        orc = Oracle(named_config("tiny", **dict(KPP, **dict(kw5, bckgrnd_vdc1=float(v)))), grid=grid)
        feed_oracle(orc, T, S)
        orc.L.orc_time_manager(orc.h); orc.run_phase("tracer_rhs")
        want = {"VDC0": orc.vdc(0), "VDC1": orc.vdc(1), "SRC0": orc.f3("KPP_SRC", 1, 0), "SRC1": orc.f3("KPP_SRC", 1, 1), "HBLT": orc.f2("HBLT")}
        sel = ocean & (ref == v)
        assert sel.any() and not (sel & seen).any()
        seen |= sel
        for n in got:
            s = sel if got[n].ndim == 3 else np.broadcast_to(sel[:, None], got[n].shape)
            diff[n] = max(diff[n], np.abs(got[n] - want[n])[s].max())
            scale[n] = max(scale[n], np.abs(want[n][s]).max())
        orc.close()
    assert np.array_equal(seen, ocean)
    # common.relerr's rule.  The state is fed as the issue says, without a surface flux, so KPP_SRC is 0 on both sides here;
    # the tests below set a flux (set_flux) and compare a non-zero KPP_SRC bit for bit.  With this noisy state AND a flux the device's
    # HBLT differs from the oracle's by 5e-13 whatever the background is (measured: the same figure with lrich = 0 and with ldbl_diff),
    # which is the boundary-layer-depth interpolation on an unsmooth profile and nothing this comparison is about.
    errs = {n: diff[n] / scale[n] if scale[n] > 0 else diff[n] for n in got}
    print("%s against the oracle, row by row:" % name, {n: "%.3e" % e for n, e in errs.items()})
    assert got["VDC0"].max() > 1.0 or kw5.get("lrich") == 0
    for n, e in errs.items():
        assert e <= TOL_LOCAL, (n, e)
    gpu.close()


def relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


QUIET = 1.0


def quiet(off, n=0):
    """levels whose interior VDC of the run without the call is below QUIET = 1 cm^2/s, i.e. of the order of the background (at most
    0.3): no shear-driven, convective or boundary-layer mixing.  VDC_on and VDC_off are each a rounded sum (b + x, c + x), so their
    difference equals b - c to one unit in the last place of the operands and no better, whatever forms them, the reference's own
    sums included; where convection has added convect_diff = 1000 that is 1e-13, against |b - c| <= 0.15.  Below 1 cm^2/s it is 2e-16
    (VISC there is below Prandtl 0.3 + 1 = 4 and the eight roundings of each run's VVC average amount to 7e-15), so the identities of
    the issue can hold at TOL_LOCAL relative to max |b - c| on these cells, and are asserted on them without any allowance."""
    return np.abs(off.get("VDC", 1, n)[:, 1:-1]) < QUIET


def test_below_the_boundary_layer(pkg):
    """the varying background on and off (uniform bckgrnd_vdc1 = c) on the same state: HBLT bitwise equal, and below both boundary
    layers and above the bottom VDC_on - VDC_off = b - c, VVC_on - VVC_off = the U-point average of Prandtl (b - c) where all four
    columns qualify.  Asserted on the cells that quiet() selects (see there why)."""
    cfg = named_config("tiny", **STEPPED)
    c = cfg.bckgrnd_vdc1
    on, *_ = run(pkg, cfg)
    off, *_ = run(pkg, cfg, bck=None)
    assert np.array_equal(on.get("HBLT"), off.get("HBLT"))
    b, _ = restated(on, cfg)
    kbl = np.maximum(on.geti("KBL"), off.geti("KBL"))[:, None]
    KMT = on.geti("KMT")[:, None]
    lev = np.arange(1, on.km + 1)[None, :, None, None]
    phys = physical(on)
    ok = (lev > kbl) & (lev < KMT) & quiet(off)
    sel = ok & phys[:, None]
    print("quiet cells below both boundary layers: %d" % sel.sum())
    assert sel.sum() > 100
    dk = np.broadcast_to((b - c)[:, None], ok.shape)
    for n in (0, 1):
        d = on.get("VDC", 1, n)[:, 1:-1] - off.get("VDC", 1, n)[:, 1:-1]
        err = np.abs(d - dk)[sel].max() / np.abs(dk[sel]).max()
        print("VDC(%d) on - off against b - c: %.3e" % (n, err))
        assert err <= TOL_LOCAL
    dm = np.where(ok, cfg.Prandtl * dk, 0.0)
    au = [on.get(n)[:, None] for n in ("AU0", "AUN", "AUE", "AUNE")]
    avg, ok4 = np.zeros(dm.shape), np.zeros(dm.shape, dtype=bool)
    avg[..., :-1, :-1] = au[0][..., :-1, :-1] * dm[..., :-1, :-1] + au[1][..., :-1, :-1] * dm[..., 1:, :-1] + \
        au[2][..., :-1, :-1] * dm[..., :-1, 1:] + au[3][..., :-1, :-1] * dm[..., 1:, 1:]
    ok4[..., :-1, :-1] = ok[..., :-1, :-1] & ok[..., 1:, :-1] & ok[..., :-1, 1:] & ok[..., 1:, 1:]
    sel4 = ok4 & phys[:, None]
    print("U cells whose four columns lie below both boundary layers: %d" % sel4.sum())
    assert sel4.sum() > 100
    d = on.get("VVC") - off.get("VVC")
    err = np.abs(d - avg)[sel4].max() / np.abs(avg[sel4]).max()
    print("VVC on - off against the average of Prandtl (b - c): %.3e" % err)
    assert err <= TOL_LOCAL
    on.close(); off.close()


@pytest.mark.parametrize("tidal", [None, 1.0e3], ids=["no-tidal", "tidal"])
def test_uniform_field_bitwise(pkg, tidal):
    """bckgrnd_vdc1 = 0, psim = 0, eq = ban = E: the field is exactly E everywhere, and the run equals, bit for bit, the run that never
    makes the call and has bckgrnd_vdc1 = E"""
    E = 0.16
    a, *_ = run(pkg, named_config("tiny", **dict(STEPPED, bckgrnd_vdc1=0.0)), tidal=tidal,
                bck=dict(bckgrnd_vdc_eq=E, bckgrnd_vdc_psim=0.0, bckgrnd_vdc_ban=E))
    b, *_ = run(pkg, named_config("tiny", **dict(STEPPED, bckgrnd_vdc1=E)), tidal=tidal, bck=None)
    assert np.all(a.get("BCKGRND_VDC") == E)
    oa, ob = outputs(a), outputs(b)
    assert oa["VDC0"].max() > 1.0 and np.abs(oa["SRC0"]).max() > 0.0 and np.abs(oa["SRC1"]).max() > 0.0
    for n in oa:
        assert np.isfinite(oa[n]).all() and np.array_equal(oa[n], ob[n]), n
    for _ in range(3):
        a.step(); b.step()
    for n, args in (("TRACER0", ("TRACER", 1, 0)), ("TRACER1", ("TRACER", 1, 1)), ("UVEL", ("UVEL", 1, 0)), ("PSURF", ("PSURF", 1, 0))):
        x, y = a.get(*args), b.get(*args)
        assert np.isfinite(x).all() and np.array_equal(x, y), n
    a.close(); b.close()


def test_with_tidal_mixing(pkg):
    """KVMIX = min(b + TIDAL_DIFF, tidal_mix_max), KVMIX_M = Prandtl min((Prandtl b) / Prandtl + TIDAL_DIFF, tidal_mix_max) with
    TIDAL_DIFF of tests/tidal_ref.py (it does not depend on the background); both orders of the two init calls give the same bits"""
    cfg = named_config("tiny", **STEPPED)
    probe = pkg.PopModel(cfg)
    T, S = set_state(probe)
    amp = amplitude(pkg, probe, cfg, unit_flux(probe), T, S)
    probe.close()
    m, T, S, F, nml = run(pkg, cfg, tidal=amp, tidal_diag=1)
    r = tidal_ref.from_model(m, cfg, nml, F, T, S)
    b, _ = restated(m, cfg)
    b = b[:, None]
    Pr, mx = cfg.Prandtl, nml.tidal_mix_max
    wet = (np.arange(1, m.km + 1)[None, :, None, None] < r["KMT"][:, None]) & physical(m)[:, None]
    kv = np.where(wet, np.minimum(b + r["DIFF"], mx), 0.0)
    kvm = np.where(wet, Pr * np.minimum((Pr * b) / Pr + r["DIFF"], mx), 0.0)
    above, below = int(((b + r["DIFF"] > mx) & wet).sum()), int(((b + r["DIFF"] < mx) & wet).sum())
    print("flux amplitude %.3e W/m^2; cells limited by tidal_mix_max: %d, below it: %d" % (amp, above, below))
    assert above > 20 and below > 20
    for name, want in (("TIDAL_DIFF", r["DIFF"]), ("KVMIX", kv), ("KVMIX_M", kvm)):
        got = m.get(name)
        err = np.abs(got - want)[wet].max() / np.abs(want[wet]).max()
        print("%s: max |device - restatement| / max |restatement| = %.3e" % (name, err))
        assert np.isfinite(got).all() and err <= TOL_LOCAL, name
    # the uniform background would give something else
    assert np.abs(m.get("KVMIX") - r["KVMIX"])[wet].max() > 0.1
    m2, *_ = run(pkg, cfg, tidal=amp, tidal_first=True, tidal_diag=1)
    o1, o2 = outputs(m, True), outputs(m2, True)
    for n in o1:
        assert np.array_equal(o1[n], o2[n]), n
    m.close(); m2.close()


def _flux(tidal):
    return dict(tidal=1.0e3, tidal_diag=1) if tidal else {}


@pytest.fixture(scope="module")
def base_outputs(pkg):
    out = {}
    for tidal in (False, True):
        m, *_ = run(pkg, named_config("tiny", **KPP), tuning={"kpp_col": 0}, **_flux(tidal))
        out[tidal] = outputs(m, tidal)
        m.close()
    return out


@pytest.mark.parametrize("tidal", [False, True], ids=["no-tidal", "tidal"])
@pytest.mark.parametrize("tuning", [{"kpp_col": 3}, {"kpp_col": 4}, {"kpp_col": 8}, {"kpp_col": 25}, {"kpp_interior_generic": 1}],
                         ids=["col3", "col4", "col8", "col25", "interior-generic"])
def test_every_kernel_form(pkg, base_outputs, tuning, tidal):
    """the interior forms are bitwise equal to each other (kernels_kpp.hpp), so the sums k_kpp_bckgrnd and k_kpp_tidal form are too"""
    m, *_ = run(pkg, named_config("tiny", **KPP), tuning=tuning, **_flux(tidal))
    out = outputs(m, tidal)
    m.close()
    assert out["VDC0"].max() > 1.0 and np.abs(out["SRC0"]).max() > 0.0
    for n, a in out.items():
        assert np.isfinite(a).all() and np.array_equal(a, base_outputs[tidal][n]), n


FORM_CONFIGS = [("km60-register", dict(nx_global=24, ny_global=20, km=60), {"kpp_interior_generic": 1}),
                ("partial-bottom-cells", dict(partial_bottom_cells=1, stepped_bathymetry=1), {"kpp_col": 0}),
                ("padded-blocks", dict(block_size_x=20, block_size_y=16), {"kpp_col": 0})]


@pytest.mark.parametrize("tidal", [False, True], ids=["no-tidal", "tidal"])
@pytest.mark.parametrize("name,kw5,other", FORM_CONFIGS, ids=[c[0] for c in FORM_CONFIGS])
def test_form_configurations(pkg, name, kw5, other, tidal):
    """the default selection of a configuration (the register interior form at km = 60, the partial-bottom-cell instantiations, padded
    blocks) against the kpp_col = 0 / generic-interior run of the same configuration, bit for bit; and the added background itself
    below the boundary layer against the run without the call"""
    cfg = named_config("tiny", **dict(KPP, **kw5))
    a, *_ = run(pkg, cfg, **_flux(tidal))
    b, *_ = run(pkg, cfg, tuning=other, **_flux(tidal))
    if name == "km60-register":
        c, *_ = run(pkg, cfg, tuning={"kpp_col": 0}, **_flux(tidal))
    else:
        c = b
    oa, ob, oc = outputs(a, tidal), outputs(b, tidal), outputs(c, tidal)
    for n in oa:
        assert np.isfinite(oa[n]).all() and np.array_equal(oa[n], ob[n]) and np.array_equal(oa[n], oc[n]), n
    if not tidal:      # the form adds the restated field: below the boundary layer VDC - (run without the call) = b - bckgrnd_vdc1
        off, *_ = run(pkg, cfg, bck=None)
        ref, _ = restated(a, cfg)
        lev = np.arange(1, a.km + 1)[None, :, None, None]
        sel = (lev > np.maximum(a.geti("KBL"), off.geti("KBL"))[:, None]) & (lev < a.geti("KMT")[:, None]) & physical(a)[:, None] & quiet(off)
        assert sel.sum() > 100
        dk = np.broadcast_to((ref - cfg.bckgrnd_vdc1)[:, None], sel.shape)
        d = oa["VDC0"][:, 1:-1] - off.get("VDC", 1, 0)[:, 1:-1]
        err = np.abs(d - dk)[sel].max() / np.abs(dk[sel]).max()
        print("%s VDC on - off against b - c: %.3e" % (name, err))
        assert err <= TOL_LOCAL
        off.close()
    a.close(); b.close()
    if c is not b:
        c.close()


def _three_steps(pkg, cfg, tuning, call=True):
    m = pkg.PopModel(cfg, tuning=tuning)
    if call:
        m.init_kpp_bckgrnd(**CESM)
    for _ in range(3):
        m.step()
    out = {n: m.get(*a) for n, a in (("T", ("TRACER", 1, 0)), ("S", ("TRACER", 1, 1)), ("U", ("UVEL", 1, 0)), ("P", ("PSURF", 1, 0)),
                                     ("VVC", ("VVC", 1, 0)), ("VDC", ("VDC", 1, 0)), ("HBLT", ("HBLT", 1, 0)), ("SRC", ("KPP_SRC", 1, 0)))}
    m.close()
    return out


def test_look_ahead_on_and_off(pkg):
    cfg = named_config("tiny", **STEPPED)
    a = _three_steps(pkg, cfg, {"kpp_ahead": 1})
    b = _three_steps(pkg, cfg, {"kpp_ahead": 0})
    plain = _three_steps(pkg, cfg, {"kpp_ahead": 0}, call=False)
    for n in a:
        assert np.isfinite(a[n]).all() and np.array_equal(a[n], b[n]), n
    assert not np.array_equal(a["T"], plain["T"]) and not np.array_equal(a["VDC"], plain["VDC"])


@pytest.mark.parametrize("opt", ["", "tidal=1.0e3"], ids=["no-tidal", "tidal"])
def test_two_ranks_equal_single_rank(opt):
    run_check(["--nproc-per-node", "2", os.path.join(ROOT, "tests", "mr_gpu_bckgrnd.py"), "--bckgrnd", opt,
                "--config", "tiny", "--steps", "2", "--no-restart", "--kw", "vmix_choice=3,bckgrnd_vdc1=0.16,stepped_bathymetry=1"], 300)
