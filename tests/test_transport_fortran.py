"""compute_tracer_transports of module diags_on_lat_aux_grid of the Fortran boundary (pop2-cesm_amd/fortran/pop_amd_mods.F90) through
its small program pop_transport_demo: the sizes, tavg_sum, the number of masked entries and the numbers of TAVG_N_HEAT_TRANS_G and
TAVG_N_SALT_TRANS_G it prints equal the Python-driven run's, rounded to r4 as the reference stores them.  Needs amdflang; skipped when
the toolchain is absent."""
import os
import re
import subprocess

import numpy as np
import pytest

from popcfg import named_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "pop2-cesm_amd", "fortran")
EXE = os.path.join(FDIR, "pop_transport_demo")


@pytest.mark.gpu
def test_demo_matches_python(pkg):
    if not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("amdflang not present")
    subprocess.check_call(["make", "-s", "-C", FDIR, "pop_transport_demo"])
    if not os.path.exists(EXE):
        pytest.skip("pop_transport_demo not built")
    nsteps = 3
    out = subprocess.check_output([EXE, str(nsteps)], text=True, timeout=120)
    g = re.search(r"n_lat_aux_grid\s+(\d+)\s+n_transport_comp\s+(\d+)\s+n_transport_reg\s+(\d+)\s+tavg_sum\s+(\S+)\s+masked\s+(\d+)", out).groups()
    m = pkg.PopModel(named_config("tiny"))
    m.init_transports(lat_aux_grid_type="southern")
    m.transport_request(1)
    for _ in range(nsteps):
        m.step()
    n = m.transport_info()["n_lat_aux_grid"]
    assert (int(g[0]), int(g[1]), int(g[2])) == (n, 3, 1) and float(g[3]) == m.tavg_sums(1)[0] == 2.5 * m.scalar("dtt")
    heat = m.transport_get("heat").astype(np.float32)
    assert int(g[4]) == np.count_nonzero(heat == np.float32(pkg.UNDEFINED_NF)) > 0
    for name, tr in (("heat", heat), ("salt", m.transport_get("salt").astype(np.float32))):
        v = [float(x) for x in re.search(name + r"_total_mid\s+(\S+)\s+" + name + r"_adv_mid\s+(\S+)\s+" + name + r"_dif_mid\s+(\S+)", out).groups()]
        want = [float(tr[n // 2 - 1, c, 0]) for c in range(3)]
        assert all(w != 0.0 and abs(w) < 1.0e30 for w in want)
        for a, b in zip(v, want):
            assert abs(a - b) <= 1.0e-8 * abs(b), (name, v, want)                     # es16.8: 9 significant digits of an r4 number
    m.close()
