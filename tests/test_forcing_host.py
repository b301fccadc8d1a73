"""Coupled surface forcing, host side (pop_init_coupled_forcing): ANGLET and its cosine / sine against the restatement of
grid.F90:660-735 (tests/forcing_ref.py), qsw_12hr_factor against the restatement of forcing_coupled.F90:358-408 with its normalisation,
the namelist defaults, every refusal by its message, and that the compute entry points need a device."""
import ctypes as C
import math

import numpy as np
import pytest

import forcing_ref
from popcfg import named_config, synthetic_grid

GRIDS = [("tiny", {}), ("padded", dict(block_size_x=11, block_size_y=9)), ("tripole", dict(ns_boundary=2)),
         ("tripole-bands", dict(ns_boundary=2, block_size_x=48, block_size_y=10))]


def random_angle_grid(cfg, seed):
    """popcfg.synthetic_grid with ANGLE uniform in (-pi, pi): neighbours differ by more than pi all over, so every branch of the
    unwrapping is taken.  TEST DATA."""
    g = synthetic_grid(cfg)
    rng = np.random.default_rng(seed)
    g["ANGLE"] = np.ascontiguousarray(rng.uniform(-math.pi, math.pi, g["ANGLE"].shape))
    return g


@pytest.mark.parametrize("name,kw", GRIDS, ids=[g[0] for g in GRIDS])
def test_anglet_bit_for_bit(pkg, name, kw):
    cfg = named_config("tiny", **kw)
    g = random_angle_grid(cfg, 5)
    m = pkg.PopModel(cfg, host_only=True, grid=g)
    want = forcing_ref.anglet(m, g["ANGLE"])
    got = m.get("ANGLET")                                  # readable before (and without) pop_init_coupled_forcing
    assert np.array_equal(got, want)
    assert np.abs(want).max() > 1.0
    # the unwrapping was exercised: some physical cell has a0 < 0 and a neighbour more than pi away
    A = forcing_ref.scatter_necorner(m, g["ANGLE"])
    assert ((A[:, 1:, 1:] < 0.0) & (np.abs(A[:, 1:, :-1] - A[:, 1:, 1:]) > math.pi)).any()
    for lb, bid in enumerate(m.local_block_ids()):         # row j_glob = 1 is 0
        b = m.get_block(bid)
        for j in np.nonzero(b["j_glob"] == 1)[0]:
            assert not got[lb, j, b["ib"] - 1:b["ie"]].any()
    m.init_coupled_forcing()
    assert np.array_equal(m.get("ANGLET"), want)
    m.close()


def test_cos_sin_anglet_within_one_ulp(pkg):
    cfg = named_config("tiny")
    g = random_angle_grid(cfg, 6)
    m = pkg.PopModel(cfg, host_only=True, grid=g)
    A, c, s = m.get("ANGLET"), m.get("COS_ANGLET"), m.get("SIN_ANGLET")
    assert np.all(np.abs(c - np.cos(A)) <= np.spacing(np.abs(np.cos(A))))      # the libm bound: 1 ulp
    assert np.all(np.abs(s - np.sin(A)) <= np.spacing(np.abs(np.sin(A))))
    m.close()
    m = pkg.PopModel(cfg, host_only=True)                  # the internal lat-lon grid: ANGLE = 0
    assert not m.get("ANGLET").any() and np.all(m.get("COS_ANGLET") == 1.0) and not m.get("SIN_ANGLET").any()
    m.close()


STEPPING = [("leapfrog", dict(tmix_opt=0)), ("avg", dict(tmix_opt=1, time_mix_freq=5)), ("avgfit", dict(tmix_opt=2, time_mix_freq=17)),
            ("robert", dict(tmix_opt=3))]


@pytest.mark.parametrize("name,kw", STEPPING, ids=[s[0] for s in STEPPING])
def test_qsw_12hr_factor(pkg, name, kw):
    cfg = named_config("tiny", **kw)
    m = pkg.PopModel(cfg, host_only=True)
    m.init_coupled_forcing(qsw_distrb_opt="12hr")
    inf = m.coupled_info()
    nspi, dt1 = inf["nsteps_per_interval"], m.scalar("dtt")
    assert inf["initialised"] and inf["qsw_distrb_opt"] == "12hr" and inf["nsteps_this_interval"] == 0 and inf["n_marginal_seas"] == 0
    assert nspi == m.dim("cpl_nsteps_per_interval") and (nspi == cfg.steps_per_day if cfg.tmix_opt != 2 else nspi > cfg.steps_per_day)
    want, w = forcing_ref.qsw_12hr_factor(dt1, nspi, cfg.tmix_opt, cfg.time_mix_freq)
    got = inf["qsw_12hr_factor"]
    assert np.array_equal(got, want)
    assert got.min() == 0.0 and got.max() > 3.0            # night, and a noon peak of about pi
    if cfg.tmix_opt in (1, 2):
        assert 0.5 in w
    # the normalisation of forcing_coupled.F90:385: the weighted sum over the interval is a day, within the first-order rounding
    # bound n * 2^-53 * sum |term| (n terms added, each carrying the rounding of its own products and of the division: 4 more)
    terms = [wn * dt1 * f for wn, f in zip(w, got)]
    assert abs(math.fsum(terms) - 86400.0) <= (nspi + 4) * 2.0 ** -53 * math.fsum(abs(t) for t in terms)
    m.close()
    m = pkg.PopModel(cfg, host_only=True)                  # 'const': ones; an interval of the caller's own length
    m.init_coupled_forcing(nsteps_per_interval=3)
    assert np.array_equal(m.coupled_info()["qsw_12hr_factor"], np.ones(3))
    m.close()


def test_nml_defaults(pkg):
    n = pkg.coupled_nml()
    assert n.struct_bytes == C.sizeof(pkg.PopCoupledNml)
    for k, _ in pkg.PopCoupledNml._fields_[1:]:
        assert getattr(n, k) == 0, k
    assert pkg.coupled_nml(qsw_distrb_opt="12hr").qsw_distrb_opt == 1
    with pytest.raises(AttributeError):
        pkg.coupled_nml(no_such_member=1)
    k = forcing_ref.consts()
    assert (k["lhv"], k["lhf"], k["salinity_factor"]) == (2.501e6, 3.337e5, -34.7 * 1.0e-4)


@pytest.mark.parametrize("nml,text", [
    (dict(qsw_distrb_opt="cosz"), "'cosz' is not built: compute_cosz"),
    (dict(qsw_distrb_opt=3), "qsw_distrb_opt: 0 'const', 1 '12hr'"),
    (dict(shf_formulation="partially-coupled"), "'partially-coupled' shf / sfwf formulations are not built"),
    (dict(sfwf_formulation="partially-coupled"), "'partially-coupled' shf / sfwf formulations are not built"),
    (dict(lestuary_on=1), "lestuary_on / lvsf_river / lebm_on are not built"),
    (dict(lvsf_river=1), "lestuary_on / lvsf_river / lebm_on are not built"),
    (dict(lebm_on=1), "lestuary_on / lvsf_river / lebm_on are not built"),
    (dict(luse_cpl_ifrac=1), "luse_cpl_ifrac is not built: OCN_WGT"),
    (dict(lms_balance=1), "lms_balance needs pop_init_ms_balance first"),
    (dict(lms_balance=2), "lms_balance: 0 or 1"),
    (dict(nsteps_per_interval=-1), "nsteps_per_interval: >= 0"),
    (dict(latent_heat_vapor_mks=-1.0), "negative constant"),
    (dict(struct_bytes=8), "struct_bytes is not sizeof(pop_coupled_nml)"),
])
def test_refusals(pkg, nml, text):
    m = pkg.PopModel(named_config("tiny"), host_only=True)
    with pytest.raises(pkg.PopError) as e:
        m.init_coupled_forcing(**nml)
    assert text in str(e.value) and str(e.value).startswith("pop_init_coupled_forcing: ")
    assert not m.coupled_info()["initialised"]
    m.init_coupled_forcing()                               # a refused call leaves the context as it was
    m.close()


def test_once_only_and_before_the_first_step(pkg):
    m = pkg.PopModel(named_config("tiny"), host_only=True)
    m.init_ice(ice_freq_opt="coupled", lfw_as_salt_flx=1)
    m.init_coupled_forcing()
    with pytest.raises(pkg.PopError, match="called a second time"):
        m.init_coupled_forcing()
    m.set_surface_forcing()                                # the head of a step: nothing to do on a host-only context
    m.time_manager()
    assert m.coupled_info()["nsteps_this_interval"] == 1   # pop_time_manager advances the interval's count
    m.close()
    m = pkg.PopModel(named_config("tiny"), host_only=True)
    m.set_surface_forcing()                                # not initialised: returns 0, does nothing
    m.time_manager()
    assert m.coupled_info()["nsteps_this_interval"] == 0
    with pytest.raises(pkg.PopError, match="a step or a phase has already run"):
        m.init_coupled_forcing()
    m.close()


def test_compute_entries_need_a_device_and_the_init(pkg):
    m = pkg.PopModel(named_config("tiny"), host_only=True)
    z = np.zeros((m.nblocks, m.nyb, m.nxb))
    with pytest.raises(pkg.PopError, match="host-only"):
        m.set_coupled_forcing(taux=z)
    with pytest.raises(AttributeError):
        m.set_coupled_forcing(no_such_field=z)
    with pytest.raises(ValueError):
        m.set_coupled_forcing(taux=z[0])
    with pytest.raises(pkg.PopError, match="unknown field"):
        m.get("EVAP_F")
    m.close()


TAVG_NEW = ("EVAP_F", "PREC_F", "SNOW_F", "MELT_F", "ROFF_F", "IOFF_F", "SALT_F", "SENH_F", "LWUP_F", "LWDN_F", "MELTH_F", "IFRAC", "U10_SQR",
            "TFW_T", "TFW_S")


def test_tavg_entries_name_the_init_call(pkg):
    m = pkg.PopModel(named_config("tiny"), host_only=True)
    for n in TAVG_NEW:
        with pytest.raises(pkg.PopError) as e:
            m.tavg_request(1, n)
        assert "pop_init_coupled_forcing" in str(e.value), n
    with pytest.raises(pkg.PopError, match="known to the reference, not built"):
        m.tavg_request(1, "SFWF_WRST")
    m.init_coupled_forcing()
    for i, n in enumerate(TAVG_NEW):
        m.tavg_request(1 + i % 2, n)
        assert m.tavg_info(n) == {"stream": 1 + i % 2, "ndims": 2, "nlevels": 1, "method": "avg"}
    m.close()


# ---- init_ms_balance ------------------------------------------------------------------------------------------------------------------
def _ms_host(pkg, **cfgkw):
    from forcing_common import angle_grid
    cfg = named_config("tiny", **cfgkw)
    return pkg.PopModel(cfg, host_only=True, grid=angle_grid(cfg))


@pytest.mark.parametrize("cfgkw", [dict(), dict(block_size_x=11, block_size_y=9)], ids=["tiny", "padded"])
def test_init_ms_balance_against_the_restatement(pkg, cfgkw):
    from forcing_common import ms_setup
    m = _ms_host(pkg, **cfgkw)
    regions, R = ms_setup(m)
    m.init_ms_balance(regions, R)
    want = forcing_ref.init_ms_balance(m, regions, R)
    got = m.ms_balance_info(transports=False)
    assert [g["number"] for g in got] == [-3, -5] == [w["number"] for w in want]
    for sea, (g, w) in enumerate(zip(got, want)):
        assert g["npts"] == len(w["ipts"]) >= 7
        assert np.array_equal(g["ipts"], w["ipts"]) and np.array_equal(g["jpts"], w["jpts"])
        assert np.array_equal(g["fracs"], w["fracs"]) and g["area"] == w["area"] >= regions[2 + sea][4]
        total = 0.0
        for f in g["fracs"]:
            total = total + f
        assert total == 1.0                                        # the last fraction absorbed 1 - sum
        assert np.array_equal(m.get("MASK_FRAC", n=sea), w["MASK_FRAC"]) and (w["MASK_FRAC"] != 0.0).sum() >= g["npts"]
        assert (R[g["jpts"] - 1, g["ipts"] - 1] > 0).all()         # no land, no marginal-sea point
        assert bool(g["warnings"] & pkg.MS_WARN_TWO_REGIONS) == w["warn_two_regions"] and not g["warnings"] & pkg.MS_WARN_MAX_POINTS
    assert got[0]["warnings"] == pkg.MS_WARN_TWO_REGIONS and got[1]["warnings"] == 0      # sea -3 sits on the border of regions 1 and 2
    with pytest.raises(pkg.PopError, match="called a second time"):
        m.init_ms_balance(regions, R)
    m.close()


def test_init_ms_balance_warnings_and_errors(pkg):
    from forcing_common import ms_setup
    m = _ms_host(pkg)
    regions, R = ms_setup(m)
    with pytest.raises(pkg.PopError, match="struct_bytes is not sizeof"):
        m.init_ms_balance(regions, R, struct_bytes=8)
    with pytest.raises(pkg.PopError, match="maximum number of marginal seas exceeded: 8 > max_ms = 7"):
        m.init_ms_balance(regions + [(-10 - n, "x", 0.0, 0.0, 1.0) for n in range(6)], R)
    far = [r if r[0] != -5 else (-5, "sea5", -89.0, 180.0, r[4]) for r in regions]     # a search centre over land: 16 growths find nothing
    with pytest.raises(pkg.PopError, match="marginal sea sea5: no points selected for distribution area"):
        m.init_ms_balance(far, R)
    m.init_ms_balance(regions, R, max_points=4)                    # a refused call leaves the context as it was
    got = m.ms_balance_info(transports=False)
    want = forcing_ref.init_ms_balance(m, regions, R, max_points=4)
    for g, w in zip(got, want):
        assert g["npts"] == 4 and g["warnings"] & pkg.MS_WARN_MAX_POINTS and w["warn_max_points"]
        assert np.array_equal(g["ipts"], w["ipts"]) and np.array_equal(g["fracs"], w["fracs"])
    m.close()
    m = _ms_host(pkg)                                              # lms_balance belongs to the virtual-salt-flux branch
    m.init_ms_balance(regions, R)
    with pytest.raises(pkg.PopError, match="lms_balance needs lfw_as_salt_flx"):
        m.init_coupled_forcing(lms_balance=1)
    m.init_coupled_forcing()
    with pytest.raises(pkg.PopError, match="pop_init_ice: after pop_init_coupled_forcing"):
        m.init_ice()
    m.close()


def test_region_mask_is_shared_with_init_transports(pkg):
    from forcing_common import ms_setup
    for first in ("transports", "ms_balance"):
        m = _ms_host(pkg)
        regions, R = ms_setup(m)
        other = R.copy()
        other[20, 30] = 7 if other[20, 30] != 7 else 8
        if first == "transports":
            m.init_transports(np.abs(R) * 0 + R, n_transport_reg=1)
            with pytest.raises(pkg.PopError, match=r"pop_init_ms_balance: REGION_MASK differs .* first at global \(i, j\) = \(31, 21\)"):
                m.init_ms_balance(regions, other)
            m.init_ms_balance(regions, R)                      # the same mask: accepted, one copy kept
        else:
            m.init_ms_balance(regions, R)
            with pytest.raises(pkg.PopError, match=r"pop_init_transports: REGION_MASK differs .* first at global \(i, j\) = \(31, 21\)"):
                m.init_transports(other, n_transport_reg=1)
            m.init_transports(R, n_transport_reg=1)
        assert m.coupled_info()["n_marginal_seas"] == 2
        m.close()
