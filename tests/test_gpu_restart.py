"""POP binary restart files (restart.F90, io_binary.F90) through the C ABI: exact restart, the file layout the
reference defines, and reading a file produced by an independent writer of that layout."""
import os

import numpy as np
import pytest

import restart_ref
from common import STATE
from popcfg import named_config, synthetic_grid
from restart_ref import parse_hdr

pytestmark = pytest.mark.gpu

FIELDS_2D = ["UBTROP_CUR", "UBTROP_OLD", "VBTROP_CUR", "VBTROP_OLD", "PSURF_CUR", "PSURF_OLD", "GRADPX_CUR", "GRADPX_OLD",
             "GRADPY_CUR", "GRADPY_OLD", "PGUESS", "FW_OLD", "FW_FREEZE"]
FIELDS_3D = ["UVEL_CUR", "UVEL_OLD", "VVEL_CUR", "VVEL_OLD", "TEMP_CUR", "SALT_CUR", "TEMP_OLD", "SALT_OLD"]


@pytest.mark.parametrize("kw,n1,n2", [
    ({}, 5, 4),                                           # avgfit: restart inside an averaging interval
    ({"tmix_opt": 1, "time_mix_freq": 3}, 4, 5),          # avg
    ({"vmix_choice": 3, "km": 24, "hmix_momentum": 4, "hmix_tracer": 4, "am": -1.0e22, "ah": -1.0e21, "solver_choice": 2}, 3, 3),
    ({"tmix_opt": 3}, 4, 4),                              # Robert filter: rf_S_prev travels in the header
    ({"block_size_x": 48, "block_size_y": 40}, 3, 3),     # one block
    ({"ns_boundary": 2, "grid": 1}, 4, 4),                # tripole fold on a caller-supplied grid: U-grid fields re-read as NE-corner vectors
    ({"ns_boundary": 0, "grid": 1, "vmix_choice": 3, "km": 24}, 3, 3),
    # Gent-McWilliams with the transition layer: everything it uses is formed from the restart fields each step (kappa every step)
    ({"hmix_tracer": 3, "ah": 0.8e7, "ah_bolus": 0.5e7, "gm_transition_layer": 1, "gm_kappa_type": 1, "gm_kappa_freq": 1, "vmix_choice": 3, "km": 24}, 4, 4),
    # ... with 'bfre' kappa recomputed once a day (the CESM namelist default, `bench.py --gm cesm`): KAPPA_VERTICAL is module state that no restart
    # file carries (1 after init_gm); the file carries eod (restart.F90:345, 467), which the next time_manager copies to eod_last
    # (time_management.F90:1809), so a restart written at the END OF A DAY -- when CESM writes them -- recomputes the profile in its first step
    # exactly as the uninterrupted run does.  (A restart in the middle of a day runs with
    # KAPPA_VERTICAL = 1 until the day ends, in the reference as here: not an exact restart, and not claimed.)
    ({"hmix_tracer": 3, "ah": 0.8e7, "gm_kappa_type": 1, "gm_kappa_freq": 2, "tmix_opt": 0, "steps_per_day": 6, "stepped_bathymetry": 1}, 6, 4),
    ({"hmix_tracer": 3, "ah": 0.8e7, "gm_transition_layer": 1, "gm_kappa_type": 1, "gm_kappa_freq": 2, "vmix_choice": 3, "km": 24, "steps_per_day": 4, "time_mix_freq": 5}, 6, 4),     # avgfit: the fit interval (4 + 2 calls) is the day
])
def test_exact_restart(pkg, tmp_path, kw, n1, n2):
    """The reference's restart contract (CESM ERS test): n1 steps + write + read into a fresh context + n2 steps is
    bit for bit the uninterrupted n1 + n2 steps."""
    kw = dict(kw)
    with_grid = kw.pop("grid", 0)
    cfg = named_config("tiny", **kw)
    grid = synthetic_grid(cfg) if with_grid else None
    def model():
        m = pkg.PopModel(cfg, grid=grid)
        if cfg.ns_boundary == 2:
            # The degenerate top row of a U-grid vector holds every point twice (i and nx - i, opposite orientation); the
            # halo update keeps the pair consistent only if the forcing is (mpi/POP_HaloMod.F90:1936-2050 averages the
            # magnitudes and takes each sign from the partner).  The analytic zonal wind is the same at both copies, i.e.
            # NOT antisymmetric, so the update is not idempotent on it and re-reading would not be exact: no wind here.
            z = np.zeros_like(m.get("SMF", n=0))
            for n in (0, 1):
                m.set("SMF", z, n=n); m.set("SMFT", z, n=n)
        return m
    a, b = model(), model()
    for _ in range(n1):
        a.step(); b.step()
    path = str(tmp_path / "restart.bin")
    b.write_restart(path)
    b.close()
    if cfg.gm_kappa_freq == 2:
        g = parse_hdr(path)["GLOBAL"]
        assert g["eod"] == ("log", "T") and g["eod_last"] == ("log", "F"), "the case must restart at the end of a day"
    b = model()
    b.step(); b.step()                # reading into a context that has already stepped: its GM module state must not survive
    b.read_restart(path)
    assert b.dim("nsteps_total") == n1
    for _ in range(n2):
        a.step(); b.step()
        assert a.solver_diagnostics() == b.solver_diagnostics()
    for name, n in STATE:
        for tl in (0, 1):
            assert np.array_equal(a.get(name, tl, n), b.get(name, tl, n)), (name, tl, n)
    a.close(); b.close()


def test_restart_file_layout(pkg, tmp_path):
    """Data file = nx_global*ny_global r8 records in the order write_restart defines the fields (3-D: km records),
    header ids point at the first record; physical cells only, global (i,j) order."""
    cfg = named_config("tiny")
    m = pkg.PopModel(cfg)
    for _ in range(3):
        m.step()
    path = str(tmp_path / "r.bin")
    m.write_restart(path)
    nx, ny, km = cfg.nx_global, cfg.ny_global, cfg.km
    sec = parse_hdr(path)
    assert list(sec)[0] == "GLOBAL" and list(sec)[1:] == FIELDS_2D + FIELDS_3D
    assert int(sec["GLOBAL"]["nsteps_total"][1]) == 3 and sec["GLOBAL"]["nsteps_total"][0] == "int"
    rec = 1
    for f in FIELDS_2D + FIELDS_3D:
        assert int(sec[f]["id"][1]) == rec and int(sec[f]["nfield_dims"][1]) == (2 if f in FIELDS_2D else 3)
        rec += 1 if f in FIELDS_2D else km
    assert sec["UVEL_CUR"]["grid_loc"][1] == "3221" and sec["TEMP_OLD"]["units"][1] == "degC"
    data = np.fromfile(path, dtype="<f8")
    assert data.size == (rec - 1) * nx * ny
    data = data.reshape(rec - 1, ny, nx)

    def glob(field):      # (nblocks, [km,] nyb, nxb) -> global, physical cells
        out = np.zeros(field.shape[1:-2] + (ny, nx))
        for b in range(m.nblocks):
            blk = m.get_block(b + 1)
            js, is_ = blk["j_glob"][2] - 1, blk["i_glob"][2] - 1
            out[..., js:js + m.nyb - 4, is_:is_ + m.nxb - 4] = field[b][..., 2:-2, 2:-2]
        return out
    assert np.array_equal(data[int(sec["PSURF_CUR"]["id"][1]) - 1], glob(m.get("PSURF", 1)))
    assert np.array_equal(data[int(sec["PSURF_OLD"]["id"][1]) - 1], glob(m.get("PSURF", 0)))
    r0 = int(sec["SALT_CUR"]["id"][1]) - 1
    assert np.array_equal(data[r0:r0 + km], glob(m.get("TRACER", 1, 1)))
    r0 = int(sec["UVEL_OLD"]["id"][1]) - 1
    assert np.array_equal(data[r0:r0 + km], glob(m.get("UVEL", 0)))
    assert not data[int(sec["FW_FREEZE"]["id"][1]) - 1].any()
    m.close()


@pytest.mark.parametrize("byteswap", [False, True])
@pytest.mark.parametrize("style", ["gfortran", "compact"])
def test_reads_a_file_from_an_independent_writer(pkg, tmp_path, byteswap, style):
    """A restart written the way the reference writes it (tests/restart_ref.py) -- every attribute of restart.F90:1281-1376 grouped by
    type, the damaged conventions line, 80-column header lines with list-directed values in either style, no "/" after the global
    attributes (gfortran style: as open_binary leaves it), fields in another order, attributes this library does not know, a char value
    with colons, values on land -- is read into the right places: land masked (read_restart :881-935), ghosts filled by the halo update,
    RHO recomputed, leapfrog on.  What lies past column 80 does not count, and a section is the first one whose name BEGINS with the
    field's (io_binary.F90:979-989)."""
    cfg = named_config("tiny")
    m = pkg.PopModel(cfg)
    nx, ny, km = cfg.nx_global, cfg.ny_global, cfg.km
    rng = np.random.default_rng(23)
    order = FIELDS_3D[::-1] + [f for f in FIELDS_2D[::-1] if f != "FW_FREEZE"]
    ids, recs, rec = {}, [], 1
    for f in order:
        n = km if f in FIELDS_3D else 1
        ids[f] = rec; rec += n
        base = {"TEMP": 10.0, "SALT": 0.035}.get(f[:4], 0.0)
        recs.append(base + (1e-3 if base else 1.0) * rng.standard_normal((n, ny, nx)))
    data = np.concatenate(recs)
    path = str(tmp_path / "ref.bin")
    data.astype(">f8" if byteswap else "<f8").tofile(path)
    attrs = restart_ref.reference_globals(nsteps_total=123, eod=not byteswap, eod_last=byteswap, tlast_ice=0.0, lcoupled_ts=False, dtt=3600.0,
                                          km=km, runid="b.e21.test")
    attrs += [("start_time", "char", "0007-01-01 12:30:00 UTC: a value with colons"), ("tidal_ts_data_ind_low", "int", 5),
              ("some_factor", "r8", -2.5e-7), ("some_switch", "log", True), ("some_real", "r4", 0.5)]
    fields = [dict(name=f, id=ids[f], ndims=3 if f in FIELDS_3D else 2, long_name="whatever: " + "w" * 100) for f in order]
    # a section whose name begins with VVEL_CUR, ahead of it and pointing at UVEL_CUR's records: the one the reference takes
    k = [f["name"] for f in fields].index("VVEL_CUR")
    fields.insert(k, dict(name="VVEL_CURL", id=ids["UVEL_CUR"], ndims=3))
    restart_ref.write_header(path, attrs, fields, style=style, title="some run: 12:00", end_global=style == "compact")
    text = open(path + ".hdr").read().splitlines()
    k = [ln.split(":")[0] for ln in text].index("nsteps_total")
    text[k] = "nsteps_total:int:" + " " * 60 + "123999"                 # the reference sees 80 columns: 123
    open(path + ".hdr", "w").write("\n".join(text) + "\n")
    hd = restart_ref.read_header(path, fields=order)
    assert hd.problems == [] and hd.attrs["nsteps_total"] == ("int", 123) and hd.fields["VVEL_CUR"]["id"] == ids["UVEL_CUR"]
    assert hd.attrs["start_time"] == ("char", "0007-01-01 12:30:00 UTC: a value with colons") and hd.title == "some run: 12:00"
    m.read_restart(path, byteswap=byteswap)
    assert m.dim("nsteps_total") == 123 and m.dim("eod") == int(not byteswap) and m.dim("eod_last") == int(byteswap)
    kmt, kmu = m.geti("KMT"), m.geti("KMU")

    def expect(f, mask3=None, mask2=None):
        g = data[ids[f] - 1: ids[f] - 1 + (km if f in FIELDS_3D else 1)]
        out = np.zeros((m.nblocks,) + g.shape[:1] + (m.nyb, m.nxb))
        for b in range(m.nblocks):
            blk = m.get_block(b + 1)
            jj = np.array(blk["j_glob"]); ii = np.array(blk["i_glob"])
            ok = (jj[:, None] >= 1) & (ii[None, :] >= 1)
            out[b] = np.where(ok, g[:, np.clip(jj, 1, ny) - 1][:, :, np.clip(ii, 1, nx) - 1], 0.0)
        return out
    k = np.arange(1, km + 1)[None, :, None, None]
    t = m.get("TRACER", 1, 0)
    assert np.array_equal(t, np.where(k <= kmt[:, None], expect("TEMP_CUR"), 0.0))
    u = m.get("UVEL", 0)
    assert np.array_equal(u, np.where(k <= kmu[:, None], expect("UVEL_OLD"), 0.0))
    p = m.get("PSURF", 1)
    assert np.array_equal(p, np.where(kmt >= 1, expect("PSURF_CUR")[:, 0], 0.0))
    gx = m.get("GRADPX", 0)
    assert np.array_equal(gx, np.where(kmu >= 1, expect("GRADPX_OLD")[:, 0], 0.0))
    assert np.array_equal(m.get("VVEL", 1), np.where(k <= kmu[:, None], expect("UVEL_CUR"), 0.0))      # through the section VVEL_CURL
    # density recomputed from the tracers read; the next step is a leapfrog step
    import ctypes as C
    rho = m.get("RHO", 1)
    s = m.get("TRACER", 1, 1)
    assert np.isfinite(rho).all() and rho[kmt[:, None] * np.ones_like(k) >= k].min() > 1.0
    m.time_manager()
    assert m.dim("leapfrogts") == 1
    m.close()
