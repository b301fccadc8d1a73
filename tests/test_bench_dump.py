"""bench.py --dump-outputs: which cells it writes (host-only contexts, no GPU) and that a plain run writes the state its last timed
step left (GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_cells_are_the_ocean_cells_in_global_order(pkg):
    """tiny = 16 blocks: every ocean cell once, in global (j, i, k) order, whatever block holds it; a smaller budget draws the same
    sample of them every time"""
    import bench
    from popcfg import named_config, synthetic_grid
    cfg = named_config("tiny")
    g = synthetic_grid(cfg)
    m = pkg.PopModel(cfg, host_only=True, grid=g)
    try:
        sel = bench.dump_cells(m, cfg, 10 ** 9)
        n2, km = m.nyb * m.nxb, m.km
        ulat, kmt, kmu = m.get("ULAT").ravel(), g["KMT"], m.geti("KMU").ravel()
        ocean = kmt > 0
        assert np.array_equal(ulat[sel["t2"]], g["ULAT"][ocean])
        col, k = sel["t3"] // (km * n2) * n2 + sel["t3"] % n2, sel["t3"] // n2 % km
        assert np.array_equal(ulat[col], np.repeat(g["ULAT"][ocean], kmt[ocean]))
        assert np.array_equal(k, np.concatenate([np.arange(d) for d in kmt[ocean]]))
        col_u = sel["u3"] // (km * n2) * n2 + sel["u3"] % n2
        assert np.array_equal(np.unique(sel["u2"]), np.unique(col_u)) and (sel["u3"] // n2 % km < kmu[col_u]).all()
        assert len(sel["u3"]) == kmu[sel["u2"]].sum() and (kmu[sel["u2"]] > 0).all()
        a, b = bench.dump_cells(m, cfg, 500), bench.dump_cells(m, cfg, 500)
        for grid in sel:
            assert np.array_equal(a[grid], b[grid]) and len(np.unique(a[grid])) == 500
            assert np.isin(a[grid], sel[grid]).all()
    finally:
        m.close()


@pytest.mark.gpu
def test_plain_run_dumps_its_last_timed_step(pkg, tmp_path):
    """`bench.py --gpus 1 --steps 3 --warmup 2 --dump-outputs DIR`: one result line without the --full measurements, and DIR holds
    the state after the 2 + 3 steps, equal to the same steps taken here"""
    import bench
    from popcfg import named_config
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--workload", "tiny",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 2 and rec["ms_per_step"] > 0 and rec["dtype"] == "f64"
    assert not {"roofline", "kpp_deep_state", "cpu_baseline"} & set(rec)
    cfg = named_config("tiny")
    names = bench.dump_names(cfg)
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in names)
    assert sum(os.path.getsize(os.path.join(tmp_path, n + ".npy")) for n in names) < 64e6
    m = pkg.PopModel(cfg)
    try:
        for _ in range(5):
            m.step()
        sel = bench.dump_cells(m, cfg, bench.DUMP_BYTES // 8 // len(names))
        want = {"TEMP": m.get("TRACER", 1, 0).ravel()[sel["t3"]], "SALT": m.get("TRACER", 1, 1).ravel()[sel["t3"]],
                "UVEL": m.get("UVEL").ravel()[sel["u3"]], "VVEL": m.get("VVEL").ravel()[sel["u3"]], "PSURF": m.get("PSURF").ravel()[sel["t2"]],
                "UBTROP": m.get("UBTROP").ravel()[sel["u2"]], "VBTROP": m.get("VBTROP").ravel()[sel["u2"]]}
    finally:
        m.close()
    for n in names:
        got = np.load(os.path.join(tmp_path, n + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, want[n]), n
