"""The modules forcing_coupled, forcing, ice and ms_balance of the Fortran boundary (pop2-cesm_amd/fortran/pop_amd_mods.F90) through
their small program pop_forcing_demo, which runs the virtual-salt-flux case with two marginal seas: the seas it prints (points, area,
warnings, transports), the checksums of STF, FW, SMF, SMFT and SHF_QSW and the interval's step count equal the Python-driven run's.  Needs amdflang; skipped when the toolchain is absent."""
import os
import re
import subprocess

import numpy as np
import pytest

from popcfg import named_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "pop2-cesm_amd", "fortran")
EXE = os.path.join(FDIR, "pop_forcing_demo")
X2O = ("taux", "tauy", "snow", "rain", "evap", "meltw", "rofl", "rofi", "salt", "swnet", "sen", "lwup", "lwdn", "melth", "ifrac", "pslv", "duu10n")
AMP = (0.2, 0.2, 2.0e-5, 8.0e-5, 6.0e-5, 3.0e-5, 2.0e-5, 1.0e-5, 1.0e-6, 250.0, 40.0, 400.0, 350.0, 30.0, 0.5, 1.0e5, 60.0)


def demo_x2o(m):
    """amp(f) * (mod(7 i + 13 j + 5 b + 3 f, 17) - 8) / 8 with the demo's 1-based (i, j, block, field): the same bits"""
    b, j, i = np.meshgrid(np.arange(1, m.nblocks + 1), np.arange(1, m.nyb + 1), np.arange(1, m.nxb + 1), indexing="ij")
    return {n: AMP[f] * ((7 * i + 13 * j + 5 * b + 3 * (f + 1)) % 17 - 8).astype(np.float64) / 8.0 for f, n in enumerate(X2O)}


@pytest.mark.gpu
def test_demo_matches_python(pkg):
    from forcing_common import ms_setup
    if not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("amdflang not present")
    subprocess.check_call(["make", "-s", "-C", FDIR, "pop_forcing_demo"])
    if not os.path.exists(EXE):
        pytest.skip("pop_forcing_demo not built")
    nsteps = 2
    out = subprocess.check_output([EXE, str(nsteps)], text=True, timeout=120)
    m = pkg.PopModel(named_config("tiny"))
    m.init_ice(ice_freq_opt="coupled", licecesm2=1, lfw_as_salt_flx=1)
    regions, R = ms_setup(m)
    m.init_ms_balance(regions, R)
    m.init_coupled_forcing(lms_balance=1)
    m.set_coupled_forcing(**demo_x2o(m))
    seas = m.ms_balance_info()
    stf2_import = m.get("STF", 1, 1)

    def checksum(label, A):
        s, sa = (float(x) for x in re.search(r"^\s*" + label + r"\s+sum\s+(\S+)\s+sumabs\s+(\S+)", out, re.M).groups())
        want_abs = float(np.abs(A).sum())
        tol = A.size * 2.0 ** -53 * want_abs            # the same numbers added in another order: the first-order bound of n terms
        assert abs(sa - want_abs) <= tol and abs(s - float(A.sum())) <= tol, (label, s, sa)
        return want_abs

    # module ms_balance: the region table and REGION_MASK the demo built in Fortran select the same points, and the transports of
    # ms_balancing are Python's -- the same library call on the same inputs, so the same bits (es24.16 prints 17 digits)
    got = re.findall(r"^\s*sea\s+(-?\d+)\s+npts\s+(\d+)\s+first\s+(\d+)\s+(\d+)\s+lastfrac\s+(\S+)\s+area\s+(\S+)\s+warnings\s+(\d+)\s+transport\s+(\S+)",
                     out, re.M)
    assert len(got) == len(seas) == 2
    for g, w in zip(got, seas):
        assert (int(g[0]), int(g[1]), int(g[2]), int(g[3]), int(g[6])) == (w["number"], w["npts"], w["ipts"][0], w["jpts"][0], w["warnings"])
        assert float(g[4]) == w["fracs"][-1] and float(g[5]) == w["area"] and float(g[7]) == w["transport"] != 0.0
    assert [w["number"] for w in seas] == [-3, -5] and seas[0]["warnings"] == pkg.MS_WARN_TWO_REGIONS
    assert checksum("stf2_import", stf2_import) > 0.0
    for _ in range(nsteps):
        m.step()
    m.set_surface_forcing()
    inf = m.coupled_info()
    g = re.search(r"nsteps_per_interval\s+(\d+)\s+nsteps_this_interval\s+(\d+)\s+n_marginal_seas\s+(\d+)", out).groups()
    assert (int(g[0]), int(g[1]), int(g[2])) == (inf["nsteps_per_interval"], nsteps, 2) and inf["nsteps_this_interval"] == nsteps
    fields = {"stf1": m.get("STF", 1, 0), "stf2": m.get("STF", 1, 1), "fw": m.get("FW"), "smf1": m.get("SMF", 1, 0), "smf2": m.get("SMF", 1, 1),
              "smft1": m.get("SMFT", 1, 0), "smft2": m.get("SMFT", 1, 1), "shf_qsw": m.get("SHF_QSW")}
    for label, A in fields.items():
        assert (checksum(label, A) > 0.0) == (label != "fw")     # the virtual salt flux: FW stays 0
    m.close()
