"""Time-averaged output accumulated on the device (pop_tavg_*): every call site against the NumPy restatement tests/tavg_ref.py over
whole blocks, ghost and land cells included; pop_step against the phase-by-phase run; requests leave the model alone; stream control;
refusals; the 'bin' file and the exact restart; the two kernels alone on seeded fields.  Base config 'tiny' (48 x 40 x 16, blocks
12 x 10: 16 blocks, land, an averaging step at step 2).

Entries formed without a division are compared with np.array_equal.  The entries with a division (tavg_ref.DIVISION) come out
equal bit for bit too -- fp64 division is correctly rounded on both sides -- and are asserted so, which is stricter than the bound
steps * 2^-52 * max|buffer| the rounding of a quotient would allow."""
import numpy as np
import pytest

import restart_ref
import tavg_ref
from common import STATE
from popcfg import named_config
from tavg_common import CASES, buffers, make, request

pytestmark = pytest.mark.gpu


def table_kw(m, case):
    extra = CASES[case][1]
    kw = dict(passive=("IAGE", "TRACER04")) if m.nt == 4 else {}
    if extra.get("ice"):
        kw["fw_as_salt"] = True
    return kw


def supported(m, case):
    """every entry the configuration produces the source of, from the configuration alone; at most 64: the forcing entries, which
    every other case holds, go first where there are more"""
    cfg, extra = m.cfg, CASES[case][1]
    kpp, gm = cfg.vmix_choice == 3, cfg.hmix_tracer == 3
    names = []
    for name, (site, ndims, method, kmax, f) in tavg_ref.table(m.km, **table_kw(m, case)).items():
        if name in ("HBLT", "XBLT", "TBLT", "KPP_SRC_TEMP", "KPP_SRC_SALT") and not kpp:
            continue
        if "MXL" in name and not (kpp and cfg.kpp_ml_diagnostics):
            continue
        if name in ("KVMIX", "KVMIX_M") and not extra.get("tidal"):
            continue
        if name in ("UISOP", "VISOP", "WISOP") and not (gm and cfg.gm_diag_bolus):
            continue
        if name in ("USUBM", "VSUBM", "WSUBM") and not extra.get("submeso"):
            continue
        if name == "QFLUX" and not extra.get("ice"):
            continue
        if name in ("VDC_T", "VDC_S") and gm:      # the restatement reads VDC after the driver, when Gent-McWilliams has added K33 to it
            continue
        names.append(name)
    forcing = [n for n in names if tavg_ref.table(m.km)[n][0] == "forcing"] if len(names) > 64 else []
    while len(names) > 64:
        names.remove(forcing.pop())
    return names


def step_by_phases(m, ref=None, coupler=False):
    """one step phase by phase; ref: the restatement takes every site where the reference has it"""
    robert = m.cfg.tmix_opt == 3
    m.time_manager()
    avg = m.scalar("time_weight") == 0.5
    if ref:
        ref.set_flag(avg)
        ref.site("forcing")
    m.dhdt()
    if ref:
        ref.site("state")
        if not robert:
            ref.site("tracer")
    m.baroclinic_driver()
    if ref:
        ref.site("vmix")
        ref.site("hmix")
    m.barotropic_driver()
    if ref:
        ref.site("btrop")
    m.baroclinic_correct_adjust()
    m.step_tail()
    if ref and robert:
        ref.site("tracer", robert_tail=True)
    if coupler:
        tl = m.scalar("tlast_ice")
        m.ice_flx_to_coupler()
        if ref:
            for ns in (1, 2):
                if ref.on.get(ns) and any(s == ns and n == "QFLUX" for n, s in ref.req.items()):
                    ref.sum_qflux[ns] = ref.sum_qflux[ns] + tl
            ref.site("qflux", const=tl)
        m.ice_export_reset()
    return avg


# ---- 1. site by site against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_sites_match_restatement(pkg, case):
    m = make(pkg, case)
    names = supported(m, case)
    assert len(names) >= 50 and len(names) <= 64
    req = request(m, names)
    ref = tavg_ref.TavgRef(m, req, pbc=bool(CASES[case][1].get("pbc")), **table_kw(m, case))
    steps, navg = 5, 0
    for _ in range(steps):
        navg += step_by_phases(m, ref, coupler=(case == "ice"))
    dtt = m.scalar("dtt")
    for ns in (1, 2):
        assert m.tavg_sums(ns)[0] == ref.sum[ns] and ref.sum[ns] == (steps - navg) * dtt + navg * 0.5 * dtt
        assert m.tavg_sums(ns)[1] == ref.sum_qflux[ns]
    if m.cfg.tmix_opt in (1, 2):
        assert navg >= 1
    # the case exercises min and max: on the restatement alone first
    wet = np.arange(1, m.km + 1)[None, :, None, None] <= m.geti("KMT")[:, None]
    assert (ref.buf["TEMP_MAX"] > ref.buf["TEMP_MIN"])[wet].mean() > 0.5
    assert ref.buf["dTEMP_POS_2D"].max() > 0.0 and ref.buf["dTEMP_NEG_2D"].min() < 0.0
    if case == "ice":
        assert ref.buf["QFLUX"].max() > 0.0 and ref.sum_qflux[ref.req["QFLUX"]] > 0.0
    got = buffers(m, req)
    bad = []
    for n in req:
        eq = np.array_equal(got[n], ref.buf[n])
        if n in tavg_ref.DIVISION:
            err, bound = np.abs(got[n] - ref.buf[n]).max(), steps * 2.0 ** -52 * np.abs(ref.buf[n]).max()
            print("%s %s: max |diff| %g, bound %g, bit for bit %s" % (case, n, err, bound, eq))
        if not eq:
            bad.append(n)
    assert not bad, bad
    m.close()


# ---- 2. pop_step equals the phase-by-phase run; 3. requests do not change the model --------------------------------------------
@pytest.mark.parametrize("case,tuning", [("avgfit", None), ("robert", None), ("kpp", dict(kpp_ahead=1)), ("nt4", None)])
def test_step_equals_phases_and_model_unchanged(pkg, case, tuning):
    cfgkw = dict(tmix_opt=0) if case == "kpp" else None          # leapfrog: every step after the first takes the look-ahead
    A, B, P = make(pkg, case, tuning, cfgkw), make(pkg, case, tuning, cfgkw), make(pkg, case, tuning, cfgkw)   # A: step(); B: phases; P: no requests
    names = supported(A, case)
    req = request(A, names)
    request(B, names)
    for _ in range(5):
        A.step()
        P.step()
        step_by_phases(B)
    if case == "kpp":
        assert A.dim("kpp_ahead_used") >= 2 and B.dim("kpp_ahead_used") == 0
    for ns in (1, 2):
        assert A.tavg_sums(ns) == B.tavg_sums(ns) and A.tavg_sums(ns)[0] > 0.0
    a, b = buffers(A, req), buffers(B, req)
    assert not [n for n in req if not np.array_equal(a[n], b[n])]
    for name, n in STATE:
        for tl in (0, 1):
            assert np.array_equal(A.get(name, tl, n), P.get(name, tl, n)), (name, tl)
    for n in range(2, A.nt):
        assert np.array_equal(A.get("TRACER", 1, n), P.get("TRACER", 1, n))
    A.close(); B.close(); P.close()


# ---- 4. stream control ---------------------------------------------------------------------------------------------------------
def test_stream_control(pkg):
    m = make(pkg, "avgfit")
    req = {"TEMP": 1, "TEMP_MAX": 1, "SSH": 1, "RHO_VINT": 1, "TEMP_2": 2, "TEMP_MIN": 2, "SSH_2": 2, "U1_8": 2}
    for n, ns in req.items():
        m.tavg_request(ns, n)
    # reset values by method, and an error -- not a crash -- from normalising with tavg_sum = 0
    for n, v in (("TEMP", 0.0), ("TEMP_MAX", -1.0e30), ("TEMP_MIN", 1.0e30), ("SSH", 0.0), ("U1_8", 0.0)):
        assert (m.tavg_get(n, normalize=False) == v).all()
    with pytest.raises(pkg.PopError, match="cannot normalise TEMP: tavg_sum of stream 1 is 0"):
        m.tavg_get("TEMP")
    assert (m.tavg_get("TEMP_MAX") == -1.0e30).all()            # min / max need no sum
    dtt = m.scalar("dtt")
    for step in range(1, 6):
        if step == 3:
            m.tavg_on(2, False)
            held = buffers(m, req)
            sum2 = m.tavg_sums(2)
        if step == 5:
            m.tavg_on(2, True)
        m.step()
        if step in (3, 4):                                       # the stream that is off gains nothing, the other goes on
            now = buffers(m, req)
            assert all(np.array_equal(now[n], held[n]) for n, ns in req.items() if ns == 2) and m.tavg_sums(2) == sum2
            assert not np.array_equal(now["TEMP"], held["TEMP"])
    assert m.tavg_sums(1)[0] == 4.5 * dtt and m.tavg_sums(2)[0] == 2.5 * dtt
    # normalisation: buffer * (1 / tavg_sum), bit for bit, and the buffer stays as it was
    raw = buffers(m, req)
    for n, ns in req.items():
        want = raw[n] if n in ("TEMP_MAX", "TEMP_MIN") else raw[n] * (1.0 / m.tavg_sums(ns)[0])
        assert np.array_equal(m.tavg_get(n), want), n
        assert np.array_equal(m.tavg_get(n, normalize=False), raw[n]), n
    m.tavg_reset(2)
    assert m.tavg_sums(2) == (0.0, 0.0) and m.tavg_sums(1)[0] == 4.5 * dtt
    assert (m.tavg_get("TEMP_MIN", normalize=False) == 1.0e30).all() and not m.tavg_get("TEMP_2", normalize=False).any()
    assert np.array_equal(m.tavg_get("TEMP", normalize=False), raw["TEMP"])
    m.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    m = make(pkg, "avgfit")
    m.tavg_request(1, "TEMP")
    for call, text in [
        (lambda: m.tavg_request(1, "NO_SUCH_FIELD"), "unknown tavg field NO_SUCH_FIELD"),
        (lambda: m.tavg_request(2, "TEMP"), "TEMP is already requested, in stream 1"),
        (lambda: m.tavg_request(1, "HBLT"), "HBLT needs vmix_choice = 3 (kpp)"),
        (lambda: m.tavg_request(1, "UET"), "UET is known to the reference, not built"),
        (lambda: m.tavg_get("SALT"), "not a requested tavg field: SALT"),
    ]:
        with pytest.raises(pkg.PopError) as e:
            call()
        assert text in str(e.value), str(e.value)
    names = [n for n in supported(m, "avgfit") if n != "TEMP"]
    m.tavg_request(1, names[:54])                                # 55 entries: all this configuration has
    k = pkg.PopModel(named_config("tiny", nt=8))
    tab = tavg_ref.table(k.km, passive=["TRACER%02d" % n for n in range(3, 9)])
    more = [n for n, e in tab.items() if e[0] in ("forcing", "state", "tracer")]
    assert len(more) >= 65
    k.tavg_request(1, more[:64])
    with pytest.raises(pkg.PopError, match="more than POP_TAVG_MAX_FIELDS = 64 entries"):
        k.tavg_request(1, more[64])
    k.close()
    m.time_manager()                                             # inside a step: requests, on / off and resets are refused
    for call in (lambda: m.tavg_request(2, "SALT_2"), lambda: m.tavg_on(1, False), lambda: m.tavg_reset(1)):
        with pytest.raises(pkg.PopError, match="refused between pop_time_manager and pop_step_tail"):
            call()
    m.dhdt(); m.baroclinic_driver(); m.barotropic_driver(); m.baroclinic_correct_adjust(); m.step_tail()
    m.tavg_on(1, False)
    m.close()


# ---- 6. files ------------------------------------------------------------------------------------------------------------------
def to_global(m, a):
    """local blocks (nblocks, [nz,] ny_block, nx_block) -> (nz, ny_global, nx_global), physical cells only"""
    a = a if a.ndim == 4 else a[:, None]
    out = np.full((a.shape[1], m.cfg.ny_global, m.cfg.nx_global), np.nan)
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        for j in range(b["jb"] - 1, b["je"]):
            for i in range(b["ib"] - 1, b["ie"]):
                if b["j_glob"][j] > 0 and b["i_glob"][i] > 0:
                    out[:, b["j_glob"][j] - 1, b["i_glob"][i] - 1] = a[lb, :, j, i]
    return out


def domain_cells(m):
    """(nblocks, ny_block, nx_block): the cell is a cell of the domain (global indices > 0), physical or a ghost copy of one"""
    out = np.zeros((m.nblocks, m.nyb, m.nxb), dtype=bool)
    for lb, bid in enumerate(m.local_block_ids()):
        b = m.get_block(bid)
        out[lb] = (np.asarray(b["j_glob"]) > 0)[:, None] & (np.asarray(b["i_glob"]) > 0)[None, :]
    return out


FILE_NAMES = ["TEMP", "SSH", "KE", "TEMP2", "TEMP_MAX", "RHO_VINT", "U1_8"]     # a name before the names it begins (header search from the top)


def test_write_normalised_file(pkg, tmp_path):
    m = make(pkg, "avgfit")
    m.tavg_request(1, FILE_NAMES)
    m.tavg_request(2, "SALT")
    for _ in range(4):
        m.step()
    want = {n: m.tavg_get(n) for n in FILE_NAMES}
    sums, salt = m.tavg_sums(1), m.tavg_get("SALT", normalize=False)
    path = str(tmp_path / "tavg.bin")
    m.tavg_write(1, path)
    hd = restart_ref.read_header(path, fields=FILE_NAMES)
    assert not hd.problems, hd.problems
    assert hd.attrs["tavg_sum"] == ("r8", sums[0]) and hd.attrs["tavg_sum_qflux"] == ("r8", 0.0) and hd.attrs["nsteps_total"] == ("int", 4)
    nx, ny = m.cfg.nx_global, m.cfg.ny_global
    data = np.fromfile(path, dtype=np.float64).reshape(-1, ny, nx)
    rec = 1
    for n in FILE_NAMES:
        f, g = hd.fields[n], to_global(m, want[n])
        assert f["section"] == n and f["id"] == rec and f["nfield_dims"] == (3 if want[n].ndim == 4 else 2)
        assert not np.isnan(g).any() and np.array_equal(data[rec - 1:rec - 1 + g.shape[0]], g), n
        rec += g.shape[0]
    assert data.shape[0] == rec - 1
    # the stream is reset afterwards, the other one is not
    assert m.tavg_sums(1) == (0.0, 0.0) and not m.tavg_get("TEMP", normalize=False).any() and (m.tavg_get("TEMP_MAX", normalize=False) == -1.0e30).all()
    assert m.tavg_sums(2)[0] > 0.0 and np.array_equal(m.tavg_get("SALT", normalize=False), salt)
    with pytest.raises(pkg.PopError, match="tavg_sum of stream 1 is 0"):
        m.tavg_write(1, path)
    m.close()


@pytest.mark.parametrize("case", ["avgfit", "robert"])
def test_exact_restart(pkg, case, tmp_path):
    A = make(pkg, case)
    names = supported(A, case)
    req = request(A, names)
    for _ in range(6):
        A.step()
    B = make(pkg, case)
    request(B, names)
    for _ in range(3):
        B.step()
    rpath, t1, t2 = str(tmp_path / "restart.bin"), str(tmp_path / "tavg1.bin"), str(tmp_path / "tavg2.bin")
    B.write_restart(rpath); B.tavg_write(1, t1, restart=True); B.tavg_write(2, t2, restart=True)
    before = buffers(B, req)
    assert all(np.array_equal(before[n], B.tavg_get(n, normalize=False)) for n in req)      # restart=True resets nothing
    B.close()
    D = make(pkg, case)
    request(D, names)
    D.read_restart(rpath); D.tavg_read(1, t1); D.tavg_read(2, t2)
    for _ in range(3):
        D.step()
    for ns in (1, 2):
        assert D.tavg_sums(ns) == A.tavg_sums(ns)
    # a record holds the nx_global x ny_global cells of the domain, so that is what a file can carry: every cell of every block that
    # is a cell of the domain, the ghost cells that are copies of one included (tavg_read updates the halo).  The ghost cells beyond
    # a closed boundary belong to no record; the fill value of the update stands there, where the uninterrupted run has summed
    # whatever the sources hold outside the domain (the density of T = S = 0, const_vdc ...)
    dom = domain_cells(A)
    a, d = buffers(A, req), buffers(D, req)
    on = lambda x: np.moveaxis(x, 1, 0)[:, dom] if x.ndim == 4 else x[dom]
    assert not [n for n in req if not np.array_equal(on(a[n]), on(d[n]))]
    whole = [n for n in req if np.array_equal(a[n], d[n])]
    assert len(whole) >= len(req) - 8 and "TEMP" in whole and "KE" in whole and "SSH" in whole and "TEMP_MAX" in whole
    E = make(pkg, case)
    here, absent = [n for n, ns in req.items() if ns == 1][0], [n for n, ns in req.items() if ns == 2][0]
    E.tavg_request(1, [here, absent])                            # a field the file lacks is named
    with pytest.raises(pkg.PopError, match="could not find field in binary header file: %s$" % absent):
        E.tavg_read(1, t1)
    A.close(); D.close(); E.close()


# ---- 7. the kernels alone ------------------------------------------------------------------------------------------------------
KERNEL_NAMES = ["UVEL", "UVEL2", "VVEL_2", "KE", "UV", "U1_8", "V1_8", "U1_1", "V1_1", "TEMP", "SALT_2", "TEMP_MAX", "TEMP_MIN", "SALT_MAX",
                "SALT_MIN", "TEMP2", "ST", "RHO", "T1_8", "S1_8", "SST", "SST2", "SSS", "SSS2", "dTEMP_POS_3D", "dTEMP_NEG_3D", "dTEMP_POS_2D",
                "dTEMP_NEG_2D", "RHO_VINT"]


@pytest.mark.parametrize("blocks", [(12, 10), (48, 40), (11, 9)], ids=["16-blocks", "one-block", "odd-plane"])
def test_kernels_alone(pkg, blocks):
    cfg = named_config("tiny", block_size_x=blocks[0], block_size_y=blocks[1])
    m = pkg.PopModel(cfg)
    assert m.km == 16
    req = request(m, KERNEL_NAMES)
    ref = tavg_ref.TavgRef(m, req)
    rng = np.random.default_rng(11)
    shp3, shp2 = (m.nblocks, m.km, m.nyb, m.nxb), (m.nblocks, m.nyb, m.nxb)
    f = {n: rng.standard_normal(shp3) for n in ("U", "V", "T", "S", "TOLD", "RHO")}
    PS = 980.6 * rng.uniform(-50.0, 50.0, shp2)
    for call, avg in enumerate((False, True)):
        if call:                    # second call: half of the cells keep their value (exact ties for min / max), the others move either way
            keep = rng.random(shp3) < 0.5
            for n in ("U", "V", "T", "S", "RHO"):
                f[n] = np.where(keep, f[n], f[n] + rng.standard_normal(shp3))
        m.set("UVEL", f["U"], 1); m.set("VVEL", f["V"], 1); m.set("TRACER", f["T"], 1, 0); m.set("TRACER", f["S"], 1, 1)
        m.set("TRACER", f["TOLD"], 0, 0); m.set("RHO", f["RHO"], 1); m.set("PSURF", PS, 1)
        m.time_manager()            # tiny: step 1 has the weight dtt, step 2 is an averaging step with 0.5 dtt
        assert (m.scalar("time_weight") == 0.5) == avg
        ref.set_flag(avg)
        m.run_phase("tavg_state"); m.run_phase("tavg_tracer")
        ref.site("state"); ref.site("tracer")
    assert ref.dtavg == 0.5 * m.scalar("dtt") and m.tavg_sums(1)[0] == 1.5 * m.scalar("dtt")
    assert (f["T"] < 0).any() and (ref.buf["TEMP_MAX"] == ref.buf["TEMP_MIN"]).mean() > 0.3 and (ref.buf["TEMP_MAX"] > ref.buf["TEMP_MIN"]).mean() > 0.3
    got = buffers(m, req)
    assert got["U1_8"].shape == shp2 and got["UVEL"].shape == shp3
    assert not [n for n in req if not np.array_equal(got[n], ref.buf[n])]
    m.close()
