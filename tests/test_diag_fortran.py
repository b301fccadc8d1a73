"""Module diagnostics of the Fortran boundary (pop2-cesm_amd/fortran/pop_amd_mods.F90) through its small program pop_diag_demo:
diag_ke, avg_tracer(1:2), cfl_advt with its address and check_KE(100.) it prints equal the Python-driven run's.  Needs amdflang;
skipped when the toolchain is absent."""
import os
import re
import subprocess

import pytest

from popcfg import named_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "pop2-cesm_amd", "fortran")
EXE = os.path.join(FDIR, "pop_diag_demo")


@pytest.mark.gpu
def test_demo_matches_python(pkg):
    if not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("amdflang not present")
    subprocess.check_call(["make", "-s", "-C", FDIR, "pop_diag_demo"])
    if not os.path.exists(EXE):
        pytest.skip("pop_diag_demo not built")
    nsteps = 4
    out = subprocess.check_output([EXE, str(nsteps)], text=True, timeout=120)
    f = re.search(r"diag_ke\s+(\S+)\s+avg_tracer1\s+(\S+)\s+avg_tracer2\s+(\S+)\s+cfl_advt\s+(\S+)\s+cfladd_advt\s+(\d+)\s+(\d+)\s+(\d+)\s+check_KE\s+(\S)", out)
    assert f, out
    m = pkg.PopModel(named_config("tiny"))
    for n in range(1, nsteps + 1):
        if n == nsteps:
            m.diag_arm()
        m.step()
    d, c = m.diag_global(), m.diag_cfl("advt")
    assert d["nsteps_total_after"] == nsteps and d["diag_ke"] > 0.0 and c["value"] > 0.0
    # es24.16: 17 significant digits, enough to read a double back exactly
    assert [float(x) for x in f.groups()[:4]] == [d["diag_ke"], d["avg_tracer"][0], d["avg_tracer"][1], c["value"]]
    assert tuple(int(x) for x in f.groups()[4:7]) == c["ijk"]
    assert f.group(8) == "F" and not m.check_ke(100.0) and "the run would stop here" not in out
    m.close()
