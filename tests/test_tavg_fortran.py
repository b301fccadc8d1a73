"""Module tavg of the Fortran boundary (pop2-cesm_amd/fortran/pop_amd_mods.F90) through its small program pop_tavg_demo: tavg_sum and
the global sum of the normalised TEMP it prints equal the Python-driven run's.  Needs amdflang; skipped when the toolchain is absent."""
import os
import re
import subprocess

import pytest

from popcfg import named_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "pop2-cesm_amd", "fortran")
EXE = os.path.join(FDIR, "pop_tavg_demo")


@pytest.mark.gpu
def test_demo_matches_python(pkg):
    if not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("amdflang not present")
    subprocess.check_call(["make", "-s", "-C", FDIR, "pop_tavg_demo"])
    if not os.path.exists(EXE):
        pytest.skip("pop_tavg_demo not built")
    nsteps = 4
    out = subprocess.check_output([EXE, str(nsteps)], text=True, timeout=120)
    got = [float(x) for x in re.search(r"tavg_sum\s+(\S+)\s+tavg_sum_off\s+(\S+)\s+sum_TEMP\s+(\S+)", out).groups()]
    m = pkg.PopModel(named_config("tiny"))
    m.tavg_request(1, "TEMP")
    m.tavg_request(2, "SSH")
    m.tavg_on(2, False)
    for _ in range(nsteps):
        m.step()
    T = m.tavg_get("TEMP")
    total = 0.0
    for k in range(m.km):
        total = total + m.global_sum_host(T[:, k])
    assert got[0] == m.tavg_sums(1)[0] == 3.5 * m.scalar("dtt") and got[1] == m.tavg_sums(2)[0] == 0.0
    assert total != 0.0 and abs(got[2] - total) <= 1.0e-14 * abs(total), (got[2], total)      # es23.15: 16 significant digits
    m.close()
