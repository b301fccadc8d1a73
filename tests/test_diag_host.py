"""Global and CFL diagnostics, host side: arming and the refusals that need no device on a host-only context, the names left out,
the areas and volumes of grid.F90:1059-1072 against NumPy from the context's own grid fields, check_ke before any armed step."""
import math

import numpy as np
import pytest

import aniso_ref
import diag_ref
from common import physical
from ice_common import ice_grid
from popcfg import named_config


def host(pkg, pbc=False, **kw):
    cfg = named_config("tiny", **kw)
    return pkg.PopModel(cfg, host_only=True, grid=ice_grid(cfg, pbc=True) if pbc else None)


def test_arming_and_refusals_without_a_device(pkg):
    m = host(pkg)
    m.diag_arm()                                              # accepted; pop_time_manager takes it
    m.diag_arm(want_global=True, want_cfl=False)
    m.time_manager()
    m.diag_arm(False, False)
    for call in (m.diag_global, lambda: m.diag_cfl("advt"), lambda: m.diag_value("diag_ke")):
        with pytest.raises(pkg.PopError, match="host-only"):
            call()
    for name in diag_ref.LEFT_OUT:
        with pytest.raises(pkg.PopError, match=name + " is known to the reference, not built"):
            m.diag_value(name)
    with pytest.raises(pkg.PopError, match="pop_check_ke: no armed step has run yet .pop_diag_arm"):
        m.check_ke(100.0)
    m.close()
    p = pkg.PopModel(named_config("tiny"), plan_only=True)
    with pytest.raises(pkg.PopError, match="pop_diag_arm: the context has no fields"):
        p.diag_arm()
    with pytest.raises(pkg.PopError, match="pop_grid_volumes: the context has no fields"):
        p.grid_volumes()
    p.close()


@pytest.mark.parametrize("pbc,kw", [(False, {}), (False, dict(stepped_bathymetry=1)), (True, dict(partial_bottom_cells=1))], ids=["flat", "stepped", "pbc"])
def test_grid_volumes(pkg, pbc, kw):
    """every sum within N 2^-53 sum|term| of the exact sum of the same terms (the first-order bound of any order of summation)"""
    m = host(pkg, pbc=pbc, **kw)
    km, P = m.km, physical(m)
    TAREA, UAREA, HT, HU, KMT, KMU = m.get("TAREA"), m.get("UAREA"), m.get("HT"), m.get("HU"), m.geti("KMT"), m.geti("KMU")
    dz = aniso_ref.vertical_dz(km)
    if pbc:                                                   # grid.F90:1001-1020: HT, HU end with the partial bottom cell
        zw = np.concatenate(([0.0], np.cumsum(dz[1:])))
        ht = np.where(KMT >= 1, zw[np.maximum(KMT, 1) - 1] + m.get("DZBC"), 0.0)
        assert np.array_equal(HT[P], ht[P]) and (m.get("DZBC")[P & (KMT >= 1)] < dz[KMT[P & (KMT >= 1)]]).any()
    v = m.grid_volumes()

    def close(got, terms):
        t = terms[P]
        want, mag, n = math.fsum(t), math.fsum(np.abs(t)), np.count_nonzero(t)
        assert want > 0.0 and abs(got - want) <= n * diag_ref.U53 * mag, (got, want)

    close(v["area_t"], TAREA * (KMT >= 1))
    close(v["volume_t"], TAREA * HT * (KMT >= 1))
    close(v["volume_u"], UAREA * HU * (KMU >= 1))
    assert v["area_t_k"][0] == v["area_t"]
    close(v["volume_t_k"][0], TAREA * dz[1] * (KMT >= 1))
    for k in range(2, km + 1):
        close(v["area_t_k"][k - 1], np.where(k <= KMT, TAREA, 0.0))
        close(v["volume_t_k"][k - 1], np.where(k <= KMT, TAREA * dz[k], 0.0))
    assert (KMT[P] == 0).any() and (np.diff(v["area_t_k"]) <= 0.0).all()                      # the case has land
    if kw.get("stepped_bathymetry"):
        assert v["area_t_k"][-1] < v["area_t_k"][0]
    m.close()
