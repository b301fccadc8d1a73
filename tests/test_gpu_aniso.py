"""Anisotropic horizontal viscosity on the GPU (hmix_momentum = 3): the friction phase k_hdiffu_aniso against the NumPy restatement
of hdiffu_aniso (tests/aniso_ref.py, hmix_aniso.F90:557-1062), the precomputed-friction mode of the momentum kernels bitwise against
del2 with am = 0, and whole steps."""
import numpy as np
import pytest

from aniso_common import CASES, angle_grid, reference, state
from common import TOL_LOCAL, physical
from mr_launch import ROOT, run_check
from popcfg import named_config, synthetic_dzbc

pytestmark = pytest.mark.gpu


def _friction(pkg, cfg, grid=None, seed=5, tuning=None):
    m = pkg.PopModel(cfg, grid=grid, tuning=tuning)
    U, V = state(m, seed)
    m.time_manager()
    m.run_phase("hmix_momentum")
    return m, U, V, m.get("HDU"), m.get("HDV")


@pytest.mark.parametrize("name,cname,kw5,kw6,angle", CASES, ids=[c[0] for c in CASES])
def test_friction_phase_matches_restatement(pkg, name, cname, kw5, kw6, angle):
    c5 = named_config(cname, **kw5)
    grid = angle_grid(c5) if angle else None
    if grid is not None and c5.partial_bottom_cells:
        grid["DZBC"] = synthetic_dzbc(c5, grid["KMT"])
    cfg = pkg.anisotropic_config(c5, **kw6)
    m, U, V, hdu, hdv = _friction(pkg, cfg, grid)
    ru, rv = reference(m, cfg, U, V)
    phys = physical(m)[:, None] & np.ones((1, m.km, 1, 1), dtype=bool)
    for a, b in ((hdu, ru), (hdv, rv)):
        assert np.isfinite(a).all()
        s = np.abs(b[phys]).max()
        assert s > 0
        assert np.abs(a[phys] - b[phys]).max() / s <= TOL_LOCAL
    m.close()


def test_east_equals_grid_bitwise(pkg):
    """'east' with ANGLE = 0 is 'grid'; with visc_para = visc_perp 'east' is 'grid' for any ANGLE"""
    c5 = named_config("tiny")
    kw = dict(visc_para=2.0e9, visc_perp=0.5e9)
    _, _, _, gu, gv = _friction(pkg, pkg.anisotropic_config(c5, **kw))
    _, _, _, eu, ev = _friction(pkg, pkg.anisotropic_config(c5, aniso_alignment="east", **kw))
    assert np.array_equal(gu, eu) and np.array_equal(gv, ev)
    g = angle_grid(c5)
    iso = dict(visc_para=1.0e9, visc_perp=1.0e9)
    _, _, _, gu, gv = _friction(pkg, pkg.anisotropic_config(c5, **iso), g)
    _, _, _, eu, ev = _friction(pkg, pkg.anisotropic_config(c5, aniso_alignment="east", **iso), g)
    assert np.array_equal(gu, eu) and np.array_equal(gv, ev)


@pytest.mark.parametrize("rows", [8, 4, 0])
def test_zero_friction_momentum_equals_del2_with_am_zero(pkg, rows):
    """with HDU = HDV = 0 after the friction phase the momentum right-hand side of 'anis' (the precomputed-friction kernels) equals
    that of del2 with am = 0, bit for bit: LDS tiles of 8 and 4 rows and the direct-load kernel"""
    tun = {"momentum_lds": rows}
    c5 = named_config("tiny", am=0.0, stepped_bathymetry=1)
    a, _, _, hdu, _ = _friction(pkg, pkg.anisotropic_config(c5, visc_para=2.0e9, visc_perp=0.5e9), tuning=tun)
    z = np.zeros_like(hdu)
    a.set("HDU", z); a.set("HDV", z)
    a.run_phase("momentum_rhs")
    d = pkg.PopModel(c5, tuning=tun)
    state(d, 5)
    d.time_manager()
    d.run_phase("momentum_rhs")
    for n, tl in (("UVEL", 2), ("VVEL", 2), ("ZX", 1), ("ZY", 1)):
        assert np.array_equal(a.get(n, tl), d.get(n, tl)), n
    a.close(); d.close()


def test_steps_gx3v7_bounded(pkg):
    """gx3v7 with 'grid' alignment and the variable viscosity: ten whole steps, kinetic energy finite and bounded"""
    cfg = pkg.anisotropic_config(named_config("gx3v7"), lvariable_hmix_aniso=1)
    m = pkg.PopModel(cfg)
    ke = []
    for _ in range(10):
        m.step()
        u, v = m.get("UVEL", 1), m.get("VVEL", 1)
        ke.append(float((u * u + v * v).sum()))
    assert np.isfinite(ke).all() and max(ke) < 1.0e12
    m.close()


def test_restart_is_exact(pkg, tmp_path):
    """pop_step on 'anis' equals its own restart: 3 steps, restart, 2 steps = 5 steps, bit for bit"""
    cfg = pkg.anisotropic_config(named_config("tiny"), aniso_alignment="east", lvariable_hmix_aniso=1)
    a = pkg.PopModel(cfg)
    for _ in range(3):
        a.step()
    path = str(tmp_path / "r")
    a.write_restart(path)
    for _ in range(2):
        a.step()
    b = pkg.PopModel(cfg)
    b.read_restart(path)
    for _ in range(2):
        b.step()
    for n in ("UVEL", "VVEL", "TRACER"):
        assert np.array_equal(a.get(n, 1), b.get(n, 1)), n
    a.close(); b.close()


# ---- closed forms on a uniform Cartesian grid (pop_create_with_grid with constant HTN, HTE, HUS, HUW: every K = 0)
def _cartesian(pkg, ring=0, **kw6):
    """48 x 40 closed basin of 16 levels with dx = dy = 1e6 cm; KMT = km inside, 0 on `ring` outer rows / columns"""
    c5 = named_config("tiny", ew_boundary=0, **{k: v for k, v in kw6.items() if k in ("block_size_x", "block_size_y")})
    nx, ny, d = c5.nx_global, c5.ny_global, 1.0e6
    one = np.ones((ny, nx))
    kmt = np.full((ny, nx), c5.km, dtype=np.int32)
    if ring:
        kmt[:ring, :] = 0; kmt[-ring:, :] = 0; kmt[:, :ring] = 0; kmt[:, -ring:] = 0
    g = {"ULAT": 0.0 * one, "ULON": 0.0 * one, "HTN": d * one, "HTE": d * one, "HUS": d * one, "HUW": d * one, "KMT": kmt,
         "ANGLE": kw6.pop("ANGLE", 0.0 * one)}
    cfg = pkg.anisotropic_config(c5, **{k: v for k, v in kw6.items() if k not in ("block_size_x", "block_size_y")})
    return pkg.PopModel(cfg, grid=g), d


def _coords(m, d):
    """x, y [cm] of every U point of the local blocks (global index times the spacing, centred on the basin)"""
    X = np.zeros((m.nblocks, m.nyb, m.nxb)); Y = np.zeros_like(X)
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        X[lb] = (np.asarray(b["i_glob"], dtype=np.float64)[None, :] - 24.0) * d
        Y[lb] = (np.asarray(b["j_glob"], dtype=np.float64)[:, None] - 20.0) * d
    return X, Y


def _set_uv(m, U, V):
    for tl in (0, 1):
        m.set("UVEL", U, tl); m.set("VVEL", V, tl)


def _inner(m, margin):
    """physical cells at least `margin` cells from the basin's edge (the closed boundary's ghost cells hold 0)"""
    mask = np.zeros((m.nblocks, m.nyb, m.nxb), dtype=bool)
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        ig, jg = np.asarray(b["i_glob"]), np.asarray(b["j_glob"])
        ok_i = (ig > margin) & (ig <= 48 - margin)
        ok_j = (jg > margin) & (jg <= 40 - margin)
        mask[lb, b["jb"] - 1:b["je"], b["ib"] - 1:b["ie"]] = (ok_j[:, None] & ok_i[None, :])[b["jb"] - 1:b["je"], b["ib"] - 1:b["ie"]]
    return mask


@pytest.mark.parametrize("align", ["grid", "east"])
def test_linear_velocity_has_no_friction(pkg, align):
    m, d = _cartesian(pkg, aniso_alignment=align, visc_para=3.0e9, visc_perp=1.0e9, ANGLE=np.full((40, 48), 0.3))   # uniform stress
    X, Y = _coords(m, d)
    U = np.repeat((10.0 + 2.0e-6 * X - 3.0e-6 * Y)[:, None], m.km, axis=1)
    V = np.repeat((-5.0 + 1.0e-6 * X + 4.0e-6 * Y)[:, None], m.km, axis=1)
    _set_uv(m, U, V)
    m.time_manager(); m.run_phase("hmix_momentum")
    inner = _inner(m, 3)[:, None] & np.ones((1, m.km, 1, 1), dtype=bool)
    scale = 3.0e9 * 4.0e-6 / d                    # nu |grad u| / dx: what one term of the divergence is made of
    for n in ("HDU", "HDV"):
        assert np.abs(m.get(n)[inner]).max() <= 1.0e-9 * scale, n
    m.close()


def test_isotropic_quadratic_gives_the_laplacian(pkg):
    """visc_para = visc_perp = nu, u = a x^2 + b y^2, v = 0: HDU = 2 nu (a + b), HDV = 0"""
    nu, al, be = 2.0e9, 3.0e-13, -1.0e-13
    m, d = _cartesian(pkg, visc_para=nu, visc_perp=nu)
    X, Y = _coords(m, d)
    U = np.repeat((al * X * X + be * Y * Y)[:, None], m.km, axis=1)
    _set_uv(m, U, np.zeros_like(U))
    m.time_manager(); m.run_phase("hmix_momentum")
    inner = _inner(m, 3)[:, None] & np.ones((1, m.km, 1, 1), dtype=bool)
    want = 2.0 * nu * (al + be)
    assert np.abs(m.get("HDU")[inner] - want).max() <= 1.0e-9 * abs(want)
    assert np.abs(m.get("HDV")[inner]).max() <= 1.0e-9 * abs(want)
    m.close()


@pytest.mark.parametrize("align", ["grid", "east"])
def test_friction_dissipates_energy(pkg, align):
    """flat-bottom closed basin (two land rows / columns round it), nu_para >= nu_perp, random U, V and ANGLE: the work of the friction
    sum UAREA dz (U HDU + V HDV) is <= 0 on every level (hmix_aniso.F90:565-569: positive-definite dissipation)"""
    rng = np.random.default_rng(11)
    m, d = _cartesian(pkg, ring=2, aniso_alignment=align, visc_para=4.0e9, visc_perp=1.0e9, ANGLE=rng.uniform(-np.pi, np.pi, (40, 48)))
    U, V = state(m, 17)
    m.time_manager(); m.run_phase("hmix_momentum")
    hdu, hdv, area = m.get("HDU"), m.get("HDV"), m.get("UAREA")
    phys = physical(m)
    for k in range(m.km):
        w = (area * (U[:, k] * hdu[:, k] + V[:, k] * hdv[:, k]))[phys].sum()
        e = (area * (U[:, k] ** 2 + V[:, k] ** 2))[phys].sum()
        assert w <= 1.0e-12 * e * 4.0e9 / d ** 2, (k, w)
    m.close()


# ---- schedule: the friction beside the vertical-mixing coefficients (pop_tuning.aniso_side) and the whole step
def _steps(pkg, cfg, n, tuning=None, phases=False):
    m = pkg.PopModel(cfg, tuning=tuning)
    for _ in range(n):
        if phases:   # step_mod.F90:126-832 as the reference's drivers call it
            m.time_manager(); m.dhdt(); m.baroclinic_driver(); m.barotropic_driver(); m.baroclinic_correct_adjust(); m.step_tail()
        else:
            m.step()
    out = {(nm, tl): m.get(nm, tl).copy() for nm in ("UVEL", "VVEL", "TRACER") for tl in (0, 1)}
    m.close()
    return out


@pytest.mark.parametrize("kw5", [{}, {"hmix_tracer": 4, "ah": -1.0e21, "lvariable_hmix": 1}], ids=["del2-tracers", "del4-tracers"])
def test_side_stream_equals_in_line(pkg, kw5):
    cfg = pkg.anisotropic_config(named_config("tiny", stepped_bathymetry=1, **kw5), aniso_alignment="east", lvariable_hmix_aniso=1)
    a = _steps(pkg, cfg, 4)
    for tun in ({"aniso_side": 0}, {"side_stream": 0}):
        b = _steps(pkg, cfg, 4, tuning=tun)
        for key in a:
            assert np.array_equal(a[key], b[key]), (tun, key)


def test_step_equals_phase_sequence(pkg):
    cfg = pkg.anisotropic_config(named_config("tiny", stepped_bathymetry=1), aniso_alignment="east", lvariable_hmix_aniso=1)
    a, b = _steps(pkg, cfg, 4), _steps(pkg, cfg, 4, phases=True)
    for key in a:
        assert np.array_equal(a[key], b[key]), key


def test_gx1v7_cesm_setup_steps(pkg):
    """the gx1v7 CESM set-up with 'anis': east + variable viscosity, Gent-McWilliams with the transition layer and the once-a-day
    'bfre' kappa, upwind3, Robert filter, P-CSI -- three finite steps"""
    c5 = named_config("gx1v7", hmix_tracer=3, gm_transition_layer=1, gm_kappa_type=1, gm_kappa_freq=2, tadvect=2, tmix_opt=3, solver_choice=3)
    m = pkg.PopModel(pkg.anisotropic_config(c5, aniso_alignment="east", lvariable_hmix_aniso=1))
    for _ in range(3):
        m.step()
    for n in ("UVEL", "VVEL", "TRACER"):
        assert np.isfinite(m.get(n, 1)).all(), n
    m.close()


# ---- several ranks (tests/mr_gpu_aniso.py: mr_gpu_check.py on layout-6 configurations)
@pytest.mark.parametrize("nranks,aniso,kw,grid", [
    (2, "aniso_alignment='east',lvariable_hmix_aniso=1", "", 0),
    (3, "lvariable_hmix_aniso=1,visc_para=1.0e9", "block_size_x=20,block_size_y=16", 0),
    (2, "aniso_alignment='east',lvariable_hmix_aniso=1", "ns_boundary=2", 1),
])
def test_multirank_equals_single_rank(nranks, aniso, kw, grid):
    import os
    run_check(["--nproc-per-node", str(nranks), os.path.join(ROOT, "tests", "mr_gpu_aniso.py"), "--aniso", aniso, "--config", "tiny",
                "--steps", "3", "--grid", str(grid), "--kw", kw], 300)
