"""pop2-cesm_amd: host-side mirror of the reference's step interface over libpop_amd.so.

The product is the HIP library (csrc/ -> libpop_amd.so, C ABI in include/pop_amd.h).  This
module is plumbing: a ctypes binding whose method names follow the reference routines
(step_mod.F90 `step`, baroclinic.F90 `baroclinic_driver`, barotropic.F90 `barotropic_driver`,
POP_HaloMod `POP_HaloUpdate`, POP_ReductionsMod `POP_GlobalSum`, POP_SolversMod
`POP_SolversRun` / `POP_SolversGetDiagnostics`, blocks.F90 `get_block`), used by bench.py and
the tests.  There is no CPU fallback: a missing library or GPU raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("POP_AMD_LIB") or os.path.join(_HERE, "libpop_amd.so")   # POP_AMD_LIB: build-variant experiments
POP_CREATE_HOST_ONLY = 1
POP_CREATE_PLAN_ONLY = 2
UNDEFINED_NF = 9.9692099683868690e+36   # POP_UNDEFINED_NF: the fill value of masked transport entries

XCHG_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_longlong),
                      C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong))
ALLRED_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_longlong, C.c_longlong)


def build(verbose=False):
    """Compile libpop_amd.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc")]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise RuntimeError("libpop_amd.so is missing: run __graft_entry__.build() (no CPU fallback exists)")
    L = C.CDLL(_SO)
    vp, ci, cd, cs, ll = C.c_void_p, C.c_int, C.c_double, C.c_char_p, C.c_longlong
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int)
    sig = {
        "pop_create": (ci, [vp, ci, ci, ci, C.POINTER(vp)]), "pop_destroy": (ci, [vp]),
        "pop_create_with_grid": (ci, [vp, vp, ci, ci, ci, C.POINTER(vp)]),
        "pop_create_tuned": (ci, [vp, vp, vp, ci, ci, ci, C.POINTER(vp)]),
        "pop_tuning_init": (None, [vp]), "pop_get_tuning": (ci, [vp, vp]),
        "pop_read_grid_files": (ci, [cs, cs, ci, ci, pd, pi]),
        "pop_last_error": (cs, [vp]), "pop_get_dim": (ci, [vp, cs]), "pop_get_scalar": (cd, [vp, cs]),
        "pop_get_block": (ci, [vp, ci, pi, pi, pi]), "pop_local_block_ids": (ci, [vp, pi]),
        "pop_get_field": (ci, [vp, cs, ci, ci, pd, ll]), "pop_set_field": (ci, [vp, cs, ci, ci, pd, ll]),
        "pop_get_ifield": (ci, [vp, cs, pi, ll]), "pop_field_count": (ll, [vp, cs]),
        "pop_field_device_ptr": (vp, [vp, cs, ci, ci]),
        "pop_time_manager": (ci, [vp]), "pop_dhdt": (ci, [vp]), "pop_baroclinic_driver": (ci, [vp]),
        "pop_barotropic_driver": (ci, [vp]), "pop_barotropic_driver_updated": (ci, [vp]), "pop_baroclinic_correct_adjust": (ci, [vp]),
        "pop_step_tail": (ci, [vp]), "pop_step": (ci, [vp]),
        "pop_halo_update": (ci, [vp, cs, ci, ci]),
        "pop_halo_update_host_r8": (ci, [vp, pd, ci, cd]), "pop_halo_update_host_i4": (ci, [vp, pi, ci, ci]),
        "pop_halo_update_loc": (ci, [vp, cs, ci, ci, ci, ci]),
        "pop_halo_update_host_r8_loc": (ci, [vp, pd, ci, cd, ci, ci]), "pop_halo_update_host_i4_loc": (ci, [vp, pi, ci, ci, ci, ci]),
        "pop_global_sum": (ci, [vp, cs, ci, ci, cs, pd]), "pop_solver_run": (ci, [vp]),
        "pop_global_count": (ci, [vp, cs, ci, ci, ci, C.POINTER(ll)]),
        "pop_global_extreme": (ci, [vp, cs, ci, ci, cs, ci, pd, pi, pi]),
        "pop_global_sum_loc": (ci, [vp, cs, ci, ci, cs, ci, pd]),
        "pop_global_sum_host": (ci, [vp, pd, pd, ci, pd]),
        "pop_global_sum_nfields": (ci, [vp, ci, C.POINTER(cs), pi, pi, cs, pd]),
        "pop_global_sum_prod": (ci, [vp, cs, ci, ci, cs, ci, ci, cs, pd]),
        "pop_global_sum_scalar": (ci, [vp, cd, pd]), "pop_global_sum_i4": (ci, [vp, cs, C.POINTER(ll)]),
        "pop_write_restart": (ci, [vp, cs]), "pop_read_restart": (ci, [vp, cs, ci]),
        "pop_solver_diagonal": (ci, [vp, ci, pd]),
        "pop_solver_preconditioner": (ci, [vp, cs, ci, cs, ci]),
        "pop_operator": (ci, [vp, ci, ci, cs, cs, ci, cs, cs]),
        "pop_operator_host": (ci, [vp, ci, ci, ci, vp, vp, vp, vp]),
        "pop_solver_get_diagnostics": (ci, [vp, pi, pd]),
        "pop_state_host": (ci, [vp, ci, pd, pd, pd, pd, pd, ll]),
        "pop_set_comm": (ci, [vp, vp, vp, vp, ll, XCHG_FN, ALLRED_FN, vp]),
        "pop_comm_buffer_doubles": (ll, [vp]), "pop_set_stream": (ci, [vp, vp]),
        "pop_reduce_buffer_doubles": (ll, [vp]), "pop_set_reduce_buffer": (ci, [vp, vp, ll]),
        "pop_rccl_unique_id": (ci, [C.c_char_p]), "pop_comm_init_rccl": (ci, [vp, C.c_char_p]),
        "pop_comm_selftest": (ci, [vp]), "pop_comm_info": (ci, [vp, pi, C.c_char_p, ci]),
        "pop_halo_plan_counts": (ci, [vp, pi, pi, pi]), "pop_halo_plan_peer": (ci, [vp, ci, pi, pi, pi]),
        "pop_halo_plan_lists": (ci, [vp, ci, pi, pi]), "pop_halo_plan_local": (ci, [vp, pi, pi, pi]),
        "pop_timers_reset": (ci, [vp]), "pop_timer_ms": (ci, [vp, cs, pd, pi]),
        "pop_time_phase": (ci, [vp, cs, ci, pd]), "pop_device_sync": (ci, [vp]), "pop_run_phase": (ci, [vp, cs]),
        "pop_tidal_nml_init": (None, [vp]), "pop_init_tidal_mixing": (ci, [vp, vp, pd, ll]),
        "pop_kpp_bckgrnd_nml_init": (None, [vp]), "pop_init_kpp_bckgrnd": (ci, [vp, vp]),
        "pop_init_iage": (ci, [vp, ci]),
        "pop_ice_nml_init": (None, [vp]), "pop_init_ice": (ci, [vp, vp]), "pop_ice_formation": (ci, [vp, ci]),
        "pop_ice_flx_to_coupler": (ci, [vp]), "pop_ice_export_reset": (ci, [vp]), "pop_tfreez_host": (ci, [vp, pd, pd, ll]),
        "pop_coupled_nml_init": (None, [vp]), "pop_init_coupled_forcing": (ci, [vp, vp]), "pop_coupled_qsw_factor": (ci, [vp, pd, ll]),
        "pop_init_ms_balance": (ci, [vp, vp, pi]), "pop_ms_balance_info": (ci, [vp, ci, pi, pi, pd, pi, pd]),
        "pop_ms_balance_points": (ci, [vp, ci, pi, pi, pd, ll]),
        "pop_set_coupled_forcing": (ci, [vp, vp, ll]), "pop_set_surface_forcing": (ci, [vp]), "pop_coupled_info": (ci, [vp, pi, pi]),
        "pop_tavg_request": (ci, [vp, ci, cs]), "pop_tavg_set_on": (ci, [vp, ci, ci]), "pop_tavg_info": (ci, [vp, cs, pi, pi, pi, pi]),
        "pop_tavg_sums": (ci, [vp, ci, pd, pd]), "pop_tavg_get": (ci, [vp, cs, ci, pd, ll]), "pop_tavg_device_ptr": (vp, [vp, cs]),
        "pop_tavg_reset": (ci, [vp, ci]), "pop_tavg_write": (ci, [vp, ci, cs, ci]), "pop_tavg_read": (ci, [vp, ci, cs]),
        "pop_diag_arm": (ci, [vp, ci, ci]), "pop_diag_global_get": (ci, [vp, vp, pd, ll]), "pop_diag_value": (ci, [vp, cs, ci, pd]),
        "pop_diag_cfl": (ci, [vp, cs, pd, pi, pd, pi, pi]), "pop_check_ke": (ci, [vp, cd, pi]),
        "pop_grid_volumes": (ci, [vp, pd, pd, pd, pd, pd]),
        "pop_transports_nml_init": (None, [vp]), "pop_init_transports": (ci, [vp, vp, pi]),
        "pop_lat_aux_grid": (ci, [vp, pi, pd, pd]), "pop_moc_info": (ci, [vp, pi, pi, pi, pi]),
        "pop_moc_mask": (ci, [vp, pi, ll]), "pop_moc_bin_map": (ci, [vp, pi, ll]), "pop_moc_request": (ci, [vp, ci]),
        "pop_moc_get": (ci, [vp, ci, ci, pd, ll]), "pop_moc_sums_count": (ll, [vp]),
        "pop_moc_sums_get": (ci, [vp, pd, ll]), "pop_moc_sums_set": (ci, [vp, pd, ll]),
        "pop_transport_request": (ci, [vp, ci, ci, ci]), "pop_transport_info": (ci, [vp, pi, pi, pi, pi, pi, pi]),
        "pop_transport_get": (ci, [vp, ci, ci, ci, pd, ll]), "pop_transport_sums_count": (ll, [vp]),
        "pop_transport_sums_get": (ci, [vp, pd, ll]), "pop_transport_sums_set": (ci, [vp, pd, ll]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)       # AttributeError here = the library does not export the ABI
        f.restype, f.argtypes = res, args
    _lib = L
    return L


ABI_SYMBOLS = None


def abi_symbols():
    """Names declared in include/pop_amd.h (parsed), for the export check."""
    import re
    hdr = open(os.path.join(os.path.dirname(_HERE), "include", "pop_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(pop_[a-z0-9_]+)\s*\(", hdr)) - {"pop_exchange_fn", "pop_allreduce_fn"})


class PopError(RuntimeError):
    pass


def tuning_fields():
    """field names of include/pop_amd.h pop_tuning, in declaration order (all int)"""
    import re
    hdr = open(os.path.join(os.path.dirname(_HERE), "include", "pop_amd.h")).read()
    body = hdr[hdr.index("typedef struct pop_tuning {"):hdr.index("} pop_tuning;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in re.findall(r"\bint\s+([^;]+);", body):
        names += [n.strip() for n in decl.split(",")]
    return names


def make_tuning(**kw):
    """pop_tuning with every field unset (pop_tuning_init) except the ones given"""
    names = tuning_fields()
    t = (C.c_int * len(names))()
    lib().pop_tuning_init(C.cast(t, C.c_void_p))
    for k, v in kw.items():
        t[names.index(k)] = int(v)
    return t


ANISO_FIELDS = [("aniso_alignment", C.c_int), ("lvariable_hmix_aniso", C.c_int), ("lsmag_aniso", C.c_int), ("vconst_5", C.c_int)] + \
    [(n, C.c_double) for n in ("visc_para", "visc_perp", "c_para", "c_perp", "u_para", "u_perp", "vconst_1", "vconst_2", "vconst_3",
                               "vconst_4", "vconst_6", "vconst_7", "smag_lat", "smag_lat_fact", "smag_lat_gauss")]
ANISO_ALIGNMENT = {"grid": 0, "east": 1, "flow": 2}
_v6_types = {}


def anisotropic_config(cfg, **hmix_aniso_nml):
    """pop_config layout 6 (include/pop_amd.h): a copy of the caller's layout-5 struct `cfg` (any ctypes mirror, such as
    tests/popcfg.py PopConfig) with the hmix_aniso_nml members appended and hmix_momentum = 3 ('anis').  Keywords: the
    members by name; aniso_alignment may also be 'grid' | 'east' | 'flow'; any other pop_config field (hmix_momentum ...)."""
    base = type(cfg)
    if hasattr(cfg, "aniso_alignment"):
        base = base.__mro__[1]
    v6 = _v6_types.get(base)
    if v6 is None:
        v6 = _v6_types[base] = type(base.__name__ + "V6", (base,), {"_fields_": ANISO_FIELDS})
    out = v6()
    C.memmove(C.addressof(out), C.addressof(cfg), min(C.sizeof(cfg), C.sizeof(out)))
    out.struct_version = 6
    out.hmix_momentum = 3
    for k, v in hmix_aniso_nml.items():
        if k == "aniso_alignment" and isinstance(v, str):
            v = ANISO_ALIGNMENT[v]
        if not hasattr(out, k):
            raise AttributeError("pop_config has no field %r" % k)
        setattr(out, k, v)
    return out


SUBMESO_FIELDS = [("lsubmesoscale_mixing", C.c_int), ("luse_const_horiz_len_scale", C.c_int), ("submeso_diag", C.c_int),
                  ("efficiency_factor", C.c_double), ("time_scale_constant", C.c_double), ("hor_length_scale", C.c_double)]
_v7_types = {}


def submeso_config(cfg, **mix_submeso_nml):
    """pop_config layout 7 (include/pop_amd.h): a copy of the caller's layout-5 or layout-6 struct `cfg` (any ctypes mirror, such as
    tests/popcfg.py PopConfig or what anisotropic_config returns) with the lsubmesoscale_mixing / mix_submeso_nml members appended and
    lsubmesoscale_mixing = 1.  Keywords: the members by name, or any other pop_config field (lsubmesoscale_mixing=0 ...)."""
    if hasattr(cfg, "lsubmesoscale_mixing"):
        v6 = type(cfg).__mro__[1]
    elif hasattr(cfg, "aniso_alignment"):
        v6 = type(cfg)
    else:                           # layout 5: the hmix_aniso_nml members appended, all 0
        base = type(cfg)
        v6 = _v6_types.get(base)
        if v6 is None:
            v6 = _v6_types[base] = type(base.__name__ + "V6", (base,), {"_fields_": ANISO_FIELDS})
    v7 = _v7_types.get(v6)
    if v7 is None:
        v7 = _v7_types[v6] = type(v6.__name__ + "V7", (v6,), {"_fields_": SUBMESO_FIELDS})
    out = v7()
    C.memmove(C.addressof(out), C.addressof(cfg), min(C.sizeof(cfg), C.sizeof(out)))
    out.struct_version = 7
    out.lsubmesoscale_mixing = 1
    for k, v in mix_submeso_nml.items():
        if not hasattr(out, k):
            raise AttributeError("pop_config has no field %r" % k)
        setattr(out, k, v)
    return out


MAX_TIDAL_MIN_REGIONS = 9
TIDAL_METHOD = {"jayne": 0, "schmittner": 1, "polzin": 2}
_TIDAL_REGION_KEYS = {"min_value": "tidal_min_values", "TLATmin": "tidal_TLATmin_regions", "TLATmax": "tidal_TLATmax_regions",
                      "TLONmin": "tidal_TLONmin_regions", "TLONmax": "tidal_TLONmax_regions", "klevels": "tidal_min_regions_klevels"}


class PopTidalNml(C.Structure):
    """include/pop_amd.h pop_tidal_nml"""
    _fields_ = [(n, C.c_int) for n in ("struct_bytes", "ltidal_mixing", "tidal_mixing_method", "ltidal_max", "ltidal_stabc",
                                       "lccsm_control_compatible", "ltidal_min_regions", "num_tidal_min_regions", "tidal_diag")] + \
        [(n, C.c_double) for n in ("tidal_local_mixing_fraction", "tidal_mixing_efficiency", "vertical_decay_scale", "tidal_mix_max")] + \
        [(n, C.c_double * MAX_TIDAL_MIN_REGIONS) for n in ("tidal_min_values", "tidal_TLATmin_regions", "tidal_TLATmax_regions",
                                                           "tidal_TLONmin_regions", "tidal_TLONmax_regions")] + \
        [("tidal_min_regions_klevels", C.c_int * MAX_TIDAL_MIN_REGIONS)]


def tidal_nml(regions=None, **kw):
    """pop_tidal_nml with the code defaults (pop_tidal_nml_init) and ltidal_mixing = 1, then the keywords: the members by name
    (tidal_mixing_method may also be 'jayne' | 'schmittner' | 'polzin').  regions: a list of dicts, one per box of ltidal_min_regions,
    with the keys TLATmin, TLATmax, TLONmin, TLONmax [degrees] and optionally min_value [cm^2/s] and klevels (2 | 6); giving it sets
    ltidal_min_regions = 1 and num_tidal_min_regions unless the keywords say otherwise."""
    n = PopTidalNml()
    lib().pop_tidal_nml_init(C.byref(n))
    n.ltidal_mixing = 1
    if regions is not None:
        if len(regions) > MAX_TIDAL_MIN_REGIONS:
            raise ValueError("at most %d tidal regions" % MAX_TIDAL_MIN_REGIONS)
        n.ltidal_min_regions, n.num_tidal_min_regions = 1, len(regions)
        for r, box in enumerate(regions):
            for k, v in box.items():
                getattr(n, _TIDAL_REGION_KEYS[k])[r] = v
    for k, v in kw.items():
        if k == "tidal_mixing_method" and isinstance(v, str):
            v = TIDAL_METHOD[v]
        if not hasattr(n, k):
            raise AttributeError("pop_tidal_nml has no field %r" % k)
        setattr(n, k, v)
    return n


class PopKppBckgrndNml(C.Structure):
    """include/pop_amd.h pop_kpp_bckgrnd_nml"""
    _fields_ = [(n, C.c_int) for n in ("struct_bytes", "lhoriz_varying_bckgrnd", "larctic_bckgrnd_vdc")] + \
        [(n, C.c_double) for n in ("bckgrnd_vdc_eq", "bckgrnd_vdc_psim", "bckgrnd_vdc_ban")]


def kpp_bckgrnd_nml(**kw):
    """pop_kpp_bckgrnd_nml with the code defaults (pop_kpp_bckgrnd_nml_init: 0.01, 0.13, 1.0) and lhoriz_varying_bckgrnd = 1, then the
    keywords: the members by name.  The doubles are taken literally (0 is a value).  CESM's gx grids: bckgrnd_vdc_eq = 0.01,
    bckgrnd_vdc_psim = 0.13, bckgrnd_vdc_ban = 1.0 with pop_config bckgrnd_vdc1 = 0.16."""
    n = PopKppBckgrndNml()
    lib().pop_kpp_bckgrnd_nml_init(C.byref(n))
    n.lhoriz_varying_bckgrnd = 1
    for k, v in kw.items():
        if not hasattr(n, k):
            raise AttributeError("pop_kpp_bckgrnd_nml has no field %r" % k)
        setattr(n, k, v)
    return n


class PopIceNml(C.Structure):
    """include/pop_amd.h pop_ice_nml"""
    _fields_ = [(n, C.c_int) for n in ("struct_bytes", "ice_freq_opt", "licecesm2", "kmxice", "lactive_ice", "lfw_as_salt_flx",
                                       "tfreeze_option")] + \
        [(n, C.c_double) for n in ("sea_ice_salinity", "ocn_ref_salinity", "latent_heat_fusion", "cp_sw", "rho_sw", "rho_fw")]


ICE_FREQ_OPT = {"never": 0, "coupled": 1, "nyear": 2, "nmonth": 3, "nday": 4, "nhour": 5, "nsecond": 6, "nstep": 7}
TFREEZE_OPTION = {"minus1p8": 0, "linear_salt": 1, "mushy": 2}


def ice_nml(**kw):
    """pop_ice_nml with the code defaults (pop_ice_nml_init: 'never', kmxice 1, fresh-water form, 'minus1p8', 4.0, 34.7, 3.34e9,
    3.996e7, 4.1/3.996, 1.0), then the keywords: the members by name; ice_freq_opt may also be 'never' | 'coupled' | 'nyear' ...,
    tfreeze_option 'minus1p8' | 'linear_salt' | 'mushy'.  CESM: ice_freq_opt='coupled', licecesm2=1, kmxice=1, lactive_ice=1,
    lfw_as_salt_flx=1, tfreeze_option='mushy'."""
    n = PopIceNml()
    lib().pop_ice_nml_init(C.byref(n))
    for k, v in kw.items():
        if k == "ice_freq_opt" and isinstance(v, str):
            v = ICE_FREQ_OPT[v]
        if k == "tfreeze_option" and isinstance(v, str):
            v = TFREEZE_OPTION[v]
        if not hasattr(n, k):
            raise AttributeError("pop_ice_nml has no field %r" % k)
        setattr(n, k, v)
    return n


class PopCoupledNml(C.Structure):
    """include/pop_amd.h pop_coupled_nml"""
    _fields_ = [(n, C.c_int) for n in ("struct_bytes", "qsw_distrb_opt", "nsteps_per_interval", "lms_balance", "shf_formulation",
                                       "sfwf_formulation", "lestuary_on", "lvsf_river", "lebm_on", "luse_cpl_ifrac")] + \
        [(n, C.c_double) for n in ("latent_heat_vapor_mks", "latent_heat_fusion_mks", "sea_ice_salinity", "rho_fw")]


class PopMsRegion(C.Structure):
    """include/pop_amd.h pop_ms_region"""
    _fields_ = [("number", C.c_int), ("name", C.c_char * 36), ("lat", C.c_double), ("lon", C.c_double), ("area", C.c_double)]


class PopMsBalanceNml(C.Structure):
    """include/pop_amd.h pop_ms_balance_nml"""
    _fields_ = [(n, C.c_int) for n in ("struct_bytes", "num_regions", "max_points", "reserved")] + [("regions", C.POINTER(PopMsRegion))]


MS_WARN_TWO_REGIONS, MS_WARN_MAX_POINTS = 1, 2
QSW_DISTRB_OPT = {"const": 0, "12hr": 1, "cosz": 2}
FORMULATION = {"coupled": 0, "partially-coupled": 1}
X2O_FIELDS = ("taux", "tauy", "snow", "rain", "evap", "meltw", "rofl", "rofi", "salt", "swnet", "sen", "lwup", "lwdn", "melth", "ifrac",
              "pslv", "duu10n")


class PopX2o(C.Structure):
    """include/pop_amd.h pop_x2o"""
    _fields_ = [("struct_bytes", C.c_int), ("reserved", C.c_int)] + [(n, C.POINTER(C.c_double)) for n in X2O_FIELDS]


def coupled_nml(**kw):
    """pop_coupled_nml with pop_coupled_nml_init's values ('const', the time manager's interval, the coupled constants), then the
    keywords: the members by name; qsw_distrb_opt may also be 'const' | '12hr' | 'cosz', shf_formulation / sfwf_formulation
    'coupled' | 'partially-coupled'."""
    n = PopCoupledNml()
    lib().pop_coupled_nml_init(C.byref(n))
    for k, v in kw.items():
        if k == "qsw_distrb_opt" and isinstance(v, str):
            v = QSW_DISTRB_OPT[v]
        if k in ("shf_formulation", "sfwf_formulation") and isinstance(v, str):
            v = FORMULATION[v]
        if not hasattr(n, k):
            raise AttributeError("pop_coupled_nml has no field %r" % k)
        setattr(n, k, v)
    return n


MAX_TRANSPORT_REG2 = 16
LAT_AUX_GRID_TYPE = {"sou": 0, "ful": 1, "use": 2}       # the reference looks at the first three letters (diags_on_lat_aux_grid.F90:312)


class PopTransportsNml(C.Structure):
    """include/pop_amd.h pop_transports_nml"""
    _fields_ = [(n, C.c_int) for n in ("struct_bytes", "lat_aux_grid_type", "n_lat_aux_grid", "n_transport_reg", "nreg2")] + \
        [("reg2_numbers", C.c_int * MAX_TRANSPORT_REG2), ("lat_aux_begin", C.c_double), ("lat_aux_end", C.c_double)]


def transports_nml(reg2_numbers=(), **kw):
    """pop_transports_nml with the code defaults (pop_transports_nml_init: 'southern', -90, 90, 180), then the keywords: the members by
    name; lat_aux_grid_type may also be 'southern' | 'full' | 'user-specified' (any other string is the reference's unknown choice).
    reg2_numbers: the REGION_MASK numbers of transport_reg2_names; n_transport_reg defaults to 2 when some are given, else to 1."""
    n = PopTransportsNml()
    lib().pop_transports_nml_init(C.byref(n))
    if len(reg2_numbers) > MAX_TRANSPORT_REG2:
        raise ValueError("at most %d region numbers" % MAX_TRANSPORT_REG2)
    n.nreg2 = len(reg2_numbers)
    for i, r in enumerate(reg2_numbers):
        n.reg2_numbers[i] = int(r)
    n.n_transport_reg = 2 if len(reg2_numbers) else 1
    for k, v in kw.items():
        if k == "lat_aux_grid_type" and isinstance(v, str):
            v = LAT_AUX_GRID_TYPE.get(v[:3], -1)
        if not hasattr(n, k):
            raise AttributeError("pop_transports_nml has no field %r" % k)
        setattr(n, k, v)
    return n


DIAG_MAX_NT = 8


class PopDiagGlobal(C.Structure):
    """include/pop_amd.h pop_diag_global"""
    _fields_ = [(n, C.c_int) for n in ("struct_bytes", "nt", "km", "nsteps_total_pre", "nsteps_total_after", "iterationCount")] + \
        [(n, C.c_double) for n in ("rmsResidual", "diag_sealevel", "diag_ke")] + \
        [(n, C.c_double * DIAG_MAX_NT) for n in ("avg_tracer", "sfc_tracer_flux")] + \
        [(n, C.c_double) for n in ("diag_ws", "diag_press_free", "diag_ke_free", "diag_ke_psfc")] + \
        [(n, C.c_double * DIAG_MAX_NT) for n in ("dtracer_avg", "dtracer_abs")]


class PopGridInput(C.Structure):
    """include/pop_amd.h pop_grid_input"""
    _fields_ = [(n, C.POINTER(C.c_double)) for n in ("ULAT", "ULON", "HTN", "HTE", "HUS", "HUW", "ANGLE")] + [("KMT", C.POINTER(C.c_int)),
                                                                                                               ("DZBC", C.POINTER(C.c_double))]


def grid_input(grid, nx, ny):
    """dict of (ny, nx) arrays -> (PopGridInput, the contiguous arrays it points into)"""
    gin, keep = PopGridInput(), []
    for n in ("ULAT", "ULON", "HTN", "HTE", "HUS", "HUW", "ANGLE", "DZBC"):
        if grid.get(n) is None:
            continue
        a = np.ascontiguousarray(grid[n], dtype=np.float64)
        if a.shape != (ny, nx):
            raise ValueError("grid[%s]: shape %s, expected (ny_global, nx_global) = %s" % (n, a.shape, (ny, nx)))
        keep.append(a)
        setattr(gin, n, a.ctypes.data_as(C.POINTER(C.c_double)))
    if grid.get("KMT") is not None:
        a = np.ascontiguousarray(grid["KMT"], dtype=np.int32)
        if a.shape != (ny, nx):
            raise ValueError("grid[KMT]: shape %s, expected %s" % (a.shape, (ny, nx)))
        keep.append(a)
        gin.KMT = a.ctypes.data_as(C.POINTER(C.c_int))
    return gin, keep


def read_grid_files(horiz_grid_file, topography_file, nx, ny):
    """the reference's direct-access binary files -> the dict PopModel(grid=...) takes"""
    rec = np.empty((7, ny, nx), dtype=np.float64)
    kmt = np.empty((ny, nx), dtype=np.int32)
    e = lib().pop_read_grid_files(horiz_grid_file.encode(), topography_file.encode() if topography_file else None, nx, ny,
                                  rec.ctypes.data_as(C.POINTER(C.c_double)), kmt.ctypes.data_as(C.POINTER(C.c_int)))
    if e:
        raise PopError("pop_read_grid_files: cannot read %s" % (horiz_grid_file if e == 1 else topography_file))
    g = {n: rec[i] for i, n in enumerate(("ULAT", "ULON", "HTN", "HTE", "HUS", "HUW", "ANGLE"))}
    if topography_file:
        g["KMT"] = kmt
    return g


class PopModel:
    """One rank's model instance.  Array views are numpy arrays shaped
    (nblocks_local, [km,] ny_block, nx_block) = the reference layout read in C order."""

    def __init__(self, cfg, rank=0, nranks=1, host_only=False, grid=None, tuning=None, plan_only=False):
        """grid: None (the internal lat-lon grid) or a dict of global (ny_global, nx_global) arrays ULAT, ULON, HTN,
        HTE, HUS, HUW [, ANGLE] [, KMT] -- the records of horiz_grid_file / topography_file (pop_create_with_grid).
        plan_only: block table, distribution and halo plan of this rank only (POP_CREATE_PLAN_ONLY; no fields, no GPU)."""
        self.L = lib()
        self.cfg = cfg
        self.h = C.c_void_p()
        flags = (POP_CREATE_HOST_ONLY if host_only else 0) | (POP_CREATE_PLAN_ONLY if plan_only else 0)
        tun = C.cast(make_tuning(**tuning), C.c_void_p) if tuning else None    # dict of pop_tuning fields (pop_create_tuned)
        if grid is None:
            e = self.L.pop_create_tuned(C.byref(cfg), None, tun, rank, nranks, flags, C.byref(self.h))
        else:
            gin, keep = grid_input(grid, cfg.nx_global, cfg.ny_global)
            e = self.L.pop_create_tuned(C.byref(cfg), C.byref(gin), tun, rank, nranks, flags, C.byref(self.h))
            del keep
        if e:
            msg = self.L.pop_last_error(self.h).decode() if self.h else "pop_create failed"
            raise PopError(msg)
        d = self.dim
        self.nxb, self.nyb, self.km, self.nt = d("nx_block"), d("ny_block"), d("km"), d("nt")
        self.nblocks, self.nblocks_tot = d("nblocks"), d("nblocks_tot")
        self._cb = None

    def close(self):
        if self.h:
            self.L.pop_destroy(self.h)
            self.h = C.c_void_p()

    def _chk(self, e):
        if e:
            raise PopError(self.L.pop_last_error(self.h).decode())

    def dim(self, name):
        return self.L.pop_get_dim(self.h, name.encode())

    def tuning(self):
        """the resolved pop_tuning as a dict (None = the library's size rule applied)"""
        names = tuning_fields()
        t = (C.c_int * len(names))()
        self._chk(self.L.pop_get_tuning(self.h, C.cast(t, C.c_void_p)))
        return {n: (None if t[i] == -2147483648 else t[i]) for i, n in enumerate(names)}

    def scalar(self, name):
        return self.L.pop_get_scalar(self.h, name.encode())

    # ---- blocks.F90 get_block
    def get_block(self, block_id):
        out = (C.c_int * 8)()
        ig, jg = (C.c_int * self.nxb)(), (C.c_int * self.nyb)()
        self._chk(self.L.pop_get_block(self.h, block_id, out, ig, jg))
        keys = ("block_id", "local_id", "ib", "ie", "jb", "je", "iblock", "jblock")
        blk = dict(zip(keys, list(out)))
        blk["i_glob"], blk["j_glob"] = np.array(ig), np.array(jg)
        return blk

    def local_block_ids(self):
        ids = (C.c_int * self.nblocks)()
        self.L.pop_local_block_ids(self.h, ids)
        return list(ids)

    # ---- fields
    def _shape(self, name):
        cnt = self.L.pop_field_count(self.h, name.encode())
        n2 = self.nxb * self.nyb * self.nblocks
        nz = cnt // n2
        return (self.nblocks, self.nyb, self.nxb) if nz == 1 else (self.nblocks, nz, self.nyb, self.nxb)

    def get(self, name, tl=1, n=0):
        shp = self._shape(name)
        a = np.empty(shp, dtype=np.float64)
        self._chk(self.L.pop_get_field(self.h, name.encode(), tl, n, a.ctypes.data_as(C.POINTER(C.c_double)), a.size))
        return a

    def set(self, name, arr, tl=1, n=0):
        a = np.ascontiguousarray(arr, dtype=np.float64)
        self._chk(self.L.pop_set_field(self.h, name.encode(), tl, n, a.ctypes.data_as(C.POINTER(C.c_double)), a.size))

    def geti(self, name):
        a = np.empty((self.nblocks, self.nyb, self.nxb), dtype=np.int32)
        self._chk(self.L.pop_get_ifield(self.h, name.encode(), a.ctypes.data_as(C.POINTER(C.c_int)), a.size))
        return a

    def init_tidal_mixing(self, energy_flux, regions=None, **nml):
        """init_tidal_mixing1 / 2 (tidal_mixing.F90) for the Jayne method: energy_flux = the record of tidal_energy_file [W/m^2] on the
        local blocks (nblocks, ny_block, nx_block); regions and keywords as tidal_nml().  Once, before the first step or phase;
        collective over the ranks.  Returns the pop_tidal_nml that was passed."""
        n = tidal_nml(regions, **nml)
        a = np.ascontiguousarray(energy_flux, dtype=np.float64)
        self._chk(self.L.pop_init_tidal_mixing(self.h, C.byref(n), a.ctypes.data_as(C.POINTER(C.c_double)), a.size))
        return n

    def init_kpp_bckgrnd(self, **nml):
        """The lhoriz_varying_bckgrnd branch of init_vmix_kpp (vmix_kpp.F90:544-611): keywords as kpp_bckgrnd_nml().  Once, before the
        first step or phase, before or after init_tidal_mixing; on every rank.  Afterwards get("BCKGRND_VDC"), get("BCKGRND_VVC") and
        get("TLON") serve the 2-D fields.  Returns the pop_kpp_bckgrnd_nml that was passed."""
        n = kpp_bckgrnd_nml(**nml)
        self._chk(self.L.pop_init_kpp_bckgrnd(self.h, C.byref(n)))
        return n

    def init_iage(self, n):
        """Make the passive tracer n (1-based, 3 .. nt) ideal age (iage_mod.F90): interior source 1 / (365 * 86400) below the surface
        level, surface level reset to 0, 0 at the three time levels now.  Once per tracer, before the first step or phase; on every
        rank; again before read_restart on a fresh context (the file does not carry the marking)."""
        self._chk(self.L.pop_init_iage(self.h, n))

    def init_ice(self, **nml):
        """init_ice (ice.F90:98-317): keywords as ice_nml().  Once, before the first step or phase, in any order with the other
        init_* calls; on every rank.  With ice_freq_opt != 'never' step() forms ice; ice_formation(tl) is legal either way.
        Afterwards get / set serve "QICE", "AQICE", "QFLUX", "FW_FREEZE" and scalar() "tlast_ice", "time_weight",
        "cp_over_lhfusion".  Returns the pop_ice_nml that was passed."""
        n = ice_nml(**nml)
        self._chk(self.L.pop_init_ice(self.h, C.byref(n)))
        return n

    def ice_formation(self, tl=2):
        """ice_formation (ice.F90:357-621) on TRACER(tl), PSURF(tl): tl = 0 old, 1 cur, 2 new"""
        self._chk(self.L.pop_ice_formation(self.h, tl))

    def ice_flx_to_coupler(self):
        """ice_flx_to_coupler (ice.F90:625-717): QICE, QFLUX from AQICE and the melt potential of TRACER(cur)"""
        self._chk(self.L.pop_ice_flx_to_coupler(self.h))

    def ice_export_reset(self):
        """tlast_ice = 0, AQICE = 0, QICE = 0 once the coupler has QFLUX (ocn_import_export.F90:715-717)"""
        self._chk(self.L.pop_ice_export_reset(self.h))

    def tfreez(self, S):
        """freezing point [deg C] of salinity S [g/g] with the tfreeze_option of init_ice (the host twin of the device function)"""
        a = np.ascontiguousarray(S, dtype=np.float64)
        out = np.empty_like(a)
        P = C.POINTER(C.c_double)
        self._chk(self.L.pop_tfreez_host(self.h, a.ctypes.data_as(P), out.ctypes.data_as(P), a.size))
        return out

    # ---- coupled surface forcing (forcing_coupled.F90; include/pop_amd.h pop_init_coupled_forcing ...)
    def init_coupled_forcing(self, **nml):
        """pop_init_coupled (forcing_coupled.F90) for what is built: keywords as coupled_nml().  Once, after init_ice if that is used,
        before the first step or phase.  Afterwards the library owns STF, SMF, SMFT, FW, TFW and SHF_QSW: set_coupled_forcing forms
        them once per coupling interval, step() applies the per-step part.  Returns the pop_coupled_nml that was passed."""
        n = coupled_nml(**nml)
        self._chk(self.L.pop_init_coupled_forcing(self.h, C.byref(n)))
        return n

    def init_ms_balance(self, regions, region_mask, max_points=0, struct_bytes=None):
        """init_ms_balance (ms_balance.F90:61-453): regions = the records of the region_info_file as (number, name, lat, lon, area)
        tuples, a negative number marking a marginal sea; region_mask = REGION_MASK as a global (ny_global, nx_global) integer
        array.  Once, before init_coupled_forcing(lms_balance=1); on every rank."""
        recs = (PopMsRegion * max(len(regions), 1))()
        for r, (number, name, lat, lon, area) in zip(recs, regions):
            r.number, r.name, r.lat, r.lon, r.area = int(number), name.encode(), float(lat), float(lon), float(area)
        n = PopMsBalanceNml()
        n.struct_bytes = C.sizeof(PopMsBalanceNml) if struct_bytes is None else struct_bytes
        n.num_regions, n.max_points, n.regions = len(regions), int(max_points), recs
        rm = np.ascontiguousarray(region_mask, dtype=np.int32)
        if rm.shape != (self.cfg.ny_global, self.cfg.nx_global):
            raise ValueError("region_mask: shape %s, expected (ny_global, nx_global)" % (rm.shape,))
        self._chk(self.L.pop_init_ms_balance(self.h, C.byref(n), rm.ctypes.data_as(C.POINTER(C.c_int))))

    def ms_balance_info(self, transports=True):
        """one dict per marginal sea in region order: number, npts, area, warnings (MS_WARN_* bits), ipts, jpts (1-based global), fracs
        and, with transports (the one call that waits for the device), the transport [kg/s] of the last set_coupled_forcing"""
        out = []
        for sea in range(self.coupled_info()["n_marginal_seas"]):
            num, npts, warn, area, tr = C.c_int(), C.c_int(), C.c_int(), C.c_double(), C.c_double()
            self._chk(self.L.pop_ms_balance_info(self.h, sea, C.byref(num), C.byref(npts), C.byref(area), C.byref(warn),
                                                 C.byref(tr) if transports else None))
            ip, jp, fr = np.empty(npts.value, dtype=np.int32), np.empty(npts.value, dtype=np.int32), np.empty(npts.value, dtype=np.float64)
            self._chk(self.L.pop_ms_balance_points(self.h, sea, ip.ctypes.data_as(C.POINTER(C.c_int)), jp.ctypes.data_as(C.POINTER(C.c_int)),
                                                   fr.ctypes.data_as(C.POINTER(C.c_double)), npts.value))
            out.append({"number": num.value, "npts": npts.value, "area": area.value, "warnings": warn.value, "ipts": ip, "jpts": jp,
                        "fracs": fr, "transport": tr.value if transports else None})
        return out

    def set_coupled_forcing(self, **fields):
        """ocn_import + rotate_wind_stress + pop_set_coupled_forcing on the device: keywords are the x2o fields (X2O_FIELDS: taux, tauy,
        snow, rain, evap, meltw, rofl, rofi, salt, swnet, sen, lwup, lwdn, melth, ifrac, pslv, duu10n) on the local blocks,
        (nblocks, ny_block, nx_block), in the coupler's MKS units; a field left out is zero.  Resets the interval's step count."""
        x, keep = PopX2o(), []
        x.struct_bytes = C.sizeof(PopX2o)
        shape = (self.nblocks, self.nyb, self.nxb)
        for k, v in fields.items():
            if k not in X2O_FIELDS:
                raise AttributeError("pop_x2o has no field %r" % k)
            if v is None:
                continue
            a = np.ascontiguousarray(v, dtype=np.float64)
            if a.shape != shape:
                raise ValueError("x2o field %s: shape %s, expected (nblocks, ny_block, nx_block) = %s" % (k, a.shape, shape))
            keep.append(a)
            setattr(x, k, a.ctypes.data_as(C.POINTER(C.c_double)))
        self._chk(self.L.pop_set_coupled_forcing(self.h, C.byref(x), self.nblocks * self.nyb * self.nxb))
        del keep

    def set_surface_forcing(self):
        """the per-step tail of set_surface_forcing (forcing.F90:379-437); step() calls it at its head, a caller that owns the
        sequence calls it before time_manager()"""
        self._chk(self.L.pop_set_surface_forcing(self.h))

    def coupled_info(self):
        """dict(initialised, qsw_distrb_opt, nsteps_per_interval, nsteps_this_interval, n_marginal_seas, qsw_12hr_factor)"""
        out, nms = (C.c_int * 4)(), C.c_int()
        self._chk(self.L.pop_coupled_info(self.h, out, C.byref(nms)))
        inf = {"initialised": bool(out[0]), "qsw_distrb_opt": {v: k for k, v in QSW_DISTRB_OPT.items()}[out[1]],
               "nsteps_per_interval": out[2], "nsteps_this_interval": out[3], "n_marginal_seas": nms.value, "qsw_12hr_factor": None}
        if out[0]:
            f = np.empty(out[2], dtype=np.float64)
            self._chk(self.L.pop_coupled_qsw_factor(self.h, f.ctypes.data_as(C.POINTER(C.c_double)), f.size))
            inf["qsw_12hr_factor"] = f
        return inf

    # ---- time-averaged output (tavg.F90; include/pop_amd.h pop_tavg_*)
    TAVG_METHOD = {1: "avg", 2: "min", 3: "max", 4: "qflux", 5: "constant"}

    def tavg_request(self, stream, names):
        """request_tavg_field for every name (one name or a list) in stream 1 .. 9; the stream is on from the first request"""
        for name in ([names] if isinstance(names, str) else names):
            self._chk(self.L.pop_tavg_request(self.h, stream, name.encode()))

    def tavg_on(self, stream, flag=True):
        """ltavg_on of the stream"""
        self._chk(self.L.pop_tavg_set_on(self.h, stream, 1 if flag else 0))

    def tavg_info(self, name):
        """dict(stream, ndims, nlevels, method) of an entry this configuration knows; stream 0: not requested"""
        s, d, l, m = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._chk(self.L.pop_tavg_info(self.h, name.encode(), C.byref(s), C.byref(d), C.byref(l), C.byref(m)))
        return {"stream": s.value, "ndims": d.value, "nlevels": l.value, "method": self.TAVG_METHOD[m.value]}

    def tavg_sums(self, stream):
        """(tavg_sum, tavg_sum_qflux) of the stream"""
        a, b = C.c_double(), C.c_double()
        self._chk(self.L.pop_tavg_sums(self.h, stream, C.byref(a), C.byref(b)))
        return a.value, b.value

    def tavg_get(self, name, normalize=True):
        """the buffer of a requested entry, (nblocks, [nlevels,] ny_block, nx_block); normalize: as tavg_norm_field_all would leave it
        (the buffer itself stays untouched)"""
        inf = self.tavg_info(name)
        shp = (self.nblocks, self.nyb, self.nxb) if inf["ndims"] == 2 else (self.nblocks, inf["nlevels"], self.nyb, self.nxb)
        a = np.empty(shp, dtype=np.float64)
        self._chk(self.L.pop_tavg_get(self.h, name.encode(), 1 if normalize else 0, a.ctypes.data_as(C.POINTER(C.c_double)), a.size))
        return a

    def tavg_reset(self, stream):
        self._chk(self.L.pop_tavg_reset(self.h, stream))

    def tavg_write(self, stream, path, restart=False):
        """<path> + <path>.hdr in the format of the restart files.  restart=False: normalise, write, reset the stream; True: the sums as
        they are, for tavg_read"""
        self._chk(self.L.pop_tavg_write(self.h, stream, os.fsencode(path), 1 if restart else 0))

    def tavg_read(self, stream, path):
        self._chk(self.L.pop_tavg_read(self.h, stream, os.fsencode(path)))

    # ---- global and CFL diagnostics (diagnostics.F90; include/pop_amd.h pop_diag_*)
    CFL_NAMES = ("advu", "advv", "advw", "advt", "hdifft", "hdiffu", "vdifft", "vdiffu")

    def diag_arm(self, want_global=True, want_cfl=True):
        """arm the next step (one-shot): global diagnostics and / or CFL numbers"""
        self._chk(self.L.pop_diag_arm(self.h, 1 if want_global else 0, 1 if want_cfl else 0))

    def diag_global(self):
        """the global diagnostics of the last armed step: a dict of the scalars, of (nt,) arrays avg_tracer, sfc_tracer_flux,
        dtracer_avg, dtracer_abs and of avg_tracer_k (km, nt); nsteps_total_pre / _after: the step each site ran in (-1: not yet, NaN)"""
        g = PopDiagGlobal()
        g.struct_bytes = C.sizeof(PopDiagGlobal)
        atk = np.empty((self.nt, self.km), dtype=np.float64)
        self._chk(self.L.pop_diag_global_get(self.h, C.byref(g), atk.ctypes.data_as(C.POINTER(C.c_double)), atk.size))
        out = {}
        for name, typ in PopDiagGlobal._fields_:
            v = getattr(g, name)
            if name != "struct_bytes":
                out[name] = np.array(v[:self.nt]) if hasattr(v, "__len__") else v
        out["avg_tracer_k"] = atk.T.copy()
        return out

    def diag_value(self, name, n=0):
        """one global diagnostic by the reference's name (n: 0-based tracer index where it has one)"""
        r = C.c_double()
        self._chk(self.L.pop_diag_value(self.h, name.encode(), n, C.byref(r)))
        return r.value

    def diag_cfl(self, name):
        """one CFL number of the last armed step: dict(value, ijk = global (i, j, k) of the maximum, value_k (km,), ij_k (km, 2),
        nsteps_total)"""
        v, ijk, step = C.c_double(), (C.c_int * 3)(), C.c_int()
        vk, ijk_k = np.empty(self.km, dtype=np.float64), np.empty((self.km, 2), dtype=np.int32)
        self._chk(self.L.pop_diag_cfl(self.h, name.encode(), C.byref(v), ijk, vk.ctypes.data_as(C.POINTER(C.c_double)),
                                      ijk_k.ctypes.data_as(C.POINTER(C.c_int)), C.byref(step)))
        return {"value": v.value, "ijk": tuple(ijk), "value_k": vk, "ij_k": ijk_k, "nsteps_total": step.value}

    def check_ke(self, ke_thresh):
        """check_KE (diagnostics.F90:3260-3290) on the last diag_ke"""
        r = C.c_int()
        self._chk(self.L.pop_check_ke(self.h, float(ke_thresh), C.byref(r)))
        return bool(r.value)

    def grid_volumes(self):
        """dict(area_t, volume_t, volume_u, area_t_k (km,), volume_t_k (km,)) of grid.F90:1059-1072; a host-only context has them too"""
        a, vt, vu = C.c_double(), C.c_double(), C.c_double()
        ak, vk = np.empty(self.km, dtype=np.float64), np.empty(self.km, dtype=np.float64)
        P = C.POINTER(C.c_double)
        self._chk(self.L.pop_grid_volumes(self.h, C.byref(a), C.byref(vt), C.byref(vu), ak.ctypes.data_as(P), vk.ctypes.data_as(P)))
        return {"area_t": a.value, "volume_t": vt.value, "volume_u": vu.value, "area_t_k": ak, "volume_t_k": vk}

    # ---- meridional overturning circulation (diags_on_lat_aux_grid.F90; include/pop_amd.h pop_init_transports, pop_moc_*)
    def init_transports(self, region_mask=None, reg2_numbers=(), **nml):
        """init_lat_aux_grid and init_moc_ts_transport_arrays: region_mask = REGION_MASK as a global (ny_global, nx_global) integer
        array, or None (1 on ocean cells, one region only); reg2_numbers and keywords as transports_nml().  Once, before the first
        step or phase; on every rank.  Returns the pop_transports_nml that was passed."""
        n = transports_nml(reg2_numbers, **nml)
        rm = None
        if region_mask is not None:
            rm = np.ascontiguousarray(region_mask, dtype=np.int32)
            if rm.shape != (self.cfg.ny_global, self.cfg.nx_global):
                raise ValueError("region_mask: shape %s, expected (ny_global, nx_global)" % (rm.shape,))
        self._chk(self.L.pop_init_transports(self.h, C.byref(n), rm.ctypes.data_as(C.POINTER(C.c_int)) if rm is not None else None))
        return n

    def moc_info(self):
        """dict(n_lat_aux_grid, km1 = km + 1, n_moc_comp, n_transport_reg, lat_aux_region_start)"""
        v = [C.c_int() for _ in range(4)]
        self._chk(self.L.pop_moc_info(self.h, *[C.byref(x) for x in v]))
        out = dict(zip(("n_lat_aux_grid", "km1", "n_moc_comp", "n_transport_reg"), [x.value for x in v]))
        out["lat_aux_region_start"] = self.dim("lat_aux_region_start")
        return out

    def lat_aux_grid(self):
        """(lat_aux_edge (n + 1,), lat_aux_center (n,)) in degrees north"""
        n = self.moc_info()["n_lat_aux_grid"]
        e, c = np.empty(n + 1, dtype=np.float64), np.empty(n, dtype=np.float64)
        P = C.POINTER(C.c_double)
        self._chk(self.L.pop_lat_aux_grid(self.h, None, e.ctypes.data_as(P), c.ctypes.data_as(P)))
        return e, c

    def moc_mask(self):
        """MASK_LAT_DEPTH as a bool array (n_lat_aux_grid, km, n_transport_reg)"""
        inf = self.moc_info()
        a = np.empty((inf["n_lat_aux_grid"], self.km, inf["n_transport_reg"]), dtype=np.int32)
        self._chk(self.L.pop_moc_mask(self.h, a.ctypes.data_as(C.POINTER(C.c_int)), a.size))
        return a != 0

    def moc_bin_map(self):
        """(ny_global, nx_global): the 1-based bin of every cell, 0 = in no bin"""
        a = np.empty((self.cfg.ny_global, self.cfg.nx_global), dtype=np.int32)
        self._chk(self.L.pop_moc_bin_map(self.h, a.ctypes.data_as(C.POINTER(C.c_int)), a.size))
        return a

    def moc_request(self, stream):
        """put the MOC into tavg stream 1 .. 9 (its ltavg_on, tavg_sum and reset)"""
        self._chk(self.L.pop_moc_request(self.h, stream))

    def moc_get(self, normalize=True, snapshot=False):
        """TAVG_MOC_G in Sverdrups as (n_lat_aux_grid + 1, km + 1, n_moc_comp, n_transport_reg); snapshot: the one tavg_write took
        before it reset the stream"""
        inf = self.moc_info()
        a = np.empty((inf["n_lat_aux_grid"] + 1, inf["km1"], inf["n_moc_comp"], inf["n_transport_reg"]), dtype=np.float64)
        self._chk(self.L.pop_moc_get(self.h, 1 if normalize else 0, 1 if snapshot else 0, a.ctypes.data_as(C.POINTER(C.c_double)), a.size))
        return a

    def moc_sums(self, values=None):
        """the reduced unnormalised sums of the running interval as one vector (bins (n, km, comp, reg), then the boundary row of
        region 2 (km, comp)); with `values` such a vector replaces the sums (it is added last when they are next read)"""
        if values is not None:
            v = np.ascontiguousarray(values, dtype=np.float64)
            self._chk(self.L.pop_moc_sums_set(self.h, v.ctypes.data_as(C.POINTER(C.c_double)), v.size))
            return v
        a = np.empty(max(self.L.pop_moc_sums_count(self.h), 0), dtype=np.float64)
        self._chk(self.L.pop_moc_sums_get(self.h, a.ctypes.data_as(C.POINTER(C.c_double)), a.size))
        return a

    # ---- northward heat and salt transports (compute_tracer_transports; include/pop_amd.h pop_transport_*)
    def transport_request(self, stream, heat=True, salt=True):
        """put N_HEAT and / or N_SALT into tavg stream 1 .. 9 (its ltavg_on, tavg_sum and reset); after init_transports"""
        self._chk(self.L.pop_transport_request(self.h, stream, 1 if heat else 0, 1 if salt else 0))

    def transport_info(self):
        """dict(n_lat_aux_grid, n_transport_comp, n_transport_reg, stream (0: not requested), heat, salt)"""
        v = [C.c_int() for _ in range(6)]
        self._chk(self.L.pop_transport_info(self.h, *[C.byref(x) for x in v]))
        out = dict(zip(("n_lat_aux_grid", "n_transport_comp", "n_transport_reg", "stream"), [x.value for x in v[:4]]))
        out["heat"], out["salt"] = bool(v[4].value), bool(v[5].value)
        return out

    def transport_get(self, tracer, normalize=True, snapshot=False):
        """TAVG_N_HEAT_TRANS_G (tracer "heat" or 1, PW) or TAVG_N_SALT_TRANS_G ("salt" or 2) as (n_lat_aux_grid + 1, n_transport_comp,
        n_transport_reg); masked entries are UNDEFINED_NF; snapshot: the one tavg_write took before it reset the stream"""
        t = {"heat": 1, "salt": 2}.get(tracer, tracer)
        inf = self.transport_info()
        a = np.empty((inf["n_lat_aux_grid"] + 1, inf["n_transport_comp"], inf["n_transport_reg"]), dtype=np.float64)
        self._chk(self.L.pop_transport_get(self.h, t, 1 if normalize else 0, 1 if snapshot else 0, a.ctypes.data_as(C.POINTER(C.c_double)), a.size))
        return a

    def transport_sums(self, values=None):
        """the reduced unnormalised sums of the running interval as one vector (bins (n, 2 tracers, 4 terms, reg), then the boundary
        row of region 2 (2 tracers, 3 terms)); with `values` such a vector replaces the sums (it is added last when they are next read)"""
        if values is not None:
            v = np.ascontiguousarray(values, dtype=np.float64)
            self._chk(self.L.pop_transport_sums_set(self.h, v.ctypes.data_as(C.POINTER(C.c_double)), v.size))
            return v
        a = np.empty(max(self.L.pop_transport_sums_count(self.h), 0), dtype=np.float64)
        self._chk(self.L.pop_transport_sums_get(self.h, a.ctypes.data_as(C.POINTER(C.c_double)), a.size))
        return a

    # ---- step_mod.F90 sequence
    def time_manager(self):
        self._chk(self.L.pop_time_manager(self.h))

    def dhdt(self):
        self._chk(self.L.pop_dhdt(self.h))

    def baroclinic_driver(self):
        self._chk(self.L.pop_baroclinic_driver(self.h))

    def barotropic_driver(self, zx_zy_updated=False):
        """zx_zy_updated: the caller has already updated the halos of ZX, ZY (step_mod.F90:405-423)"""
        self._chk((self.L.pop_barotropic_driver_updated if zx_zy_updated else self.L.pop_barotropic_driver)(self.h))

    def baroclinic_correct_adjust(self):
        self._chk(self.L.pop_baroclinic_correct_adjust(self.h))

    def step_tail(self):
        self._chk(self.L.pop_step_tail(self.h))

    def step(self):
        self._chk(self.L.pop_step(self.h))

    def sync(self):
        self._chk(self.L.pop_device_sync(self.h))

    # ---- POP_HaloUpdate / POP_GlobalSum / POP_Solvers*
    def halo_update(self, name, tl=1, n=0):
        self._chk(self.L.pop_halo_update(self.h, name.encode(), tl, n))

    LOC = {"center": 0, "NEcorner": 1, "Nface": 2, "Eface": 3}
    KIND = {"scalar": 0, "vector": 1, "angle": 2}

    def halo_update_loc(self, name, tl=1, n=0, loc="center", kind="scalar"):
        self._chk(self.L.pop_halo_update_loc(self.h, name.encode(), tl, n, self.LOC[loc], self.KIND[kind]))

    def halo_update_host_loc(self, arr, fill=0, loc="center", kind="scalar"):
        a = arr
        nz = a.size // (self.nxb * self.nyb * self.nblocks_tot)
        if a.dtype == np.int32:
            self._chk(self.L.pop_halo_update_host_i4_loc(self.h, a.ctypes.data_as(C.POINTER(C.c_int)), nz, int(fill), self.LOC[loc], self.KIND[kind]))
        else:
            assert a.dtype == np.float64
            self._chk(self.L.pop_halo_update_host_r8_loc(self.h, a.ctypes.data_as(C.POINTER(C.c_double)), nz, float(fill), self.LOC[loc], self.KIND[kind]))

    def halo_update_host(self, arr, fill=0):
        a = arr
        nz = a.size // (self.nxb * self.nyb * self.nblocks_tot)
        if a.dtype == np.int32:
            self._chk(self.L.pop_halo_update_host_i4(self.h, a.ctypes.data_as(C.POINTER(C.c_int)), nz, int(fill)))
        else:
            self._chk(self.L.pop_halo_update_host_r8(self.h, a.ctypes.data_as(C.POINTER(C.c_double)), nz, float(fill)))

    def global_sum(self, name, tl=1, n=0, mask=None):
        r = C.c_double()
        self._chk(self.L.pop_global_sum(self.h, name.encode(), tl, n, mask.encode() if mask else None, C.byref(r)))
        return r.value

    def global_count(self, name, tl=1, n=0, loc="center"):
        r = C.c_longlong()
        self._chk(self.L.pop_global_count(self.h, name.encode(), tl, n, self.LOC[loc], C.byref(r)))
        return r.value

    def global_extreme(self, name, tl=1, n=0, mask=None, want_max=True):
        """(value, iGlobal, jGlobal) of the global maximum / minimum"""
        v, i, j = C.c_double(), C.c_int(), C.c_int()
        self._chk(self.L.pop_global_extreme(self.h, name.encode(), tl, n, mask.encode() if mask else None, 1 if want_max else 0,
                                            C.byref(v), C.byref(i), C.byref(j)))
        return v.value, i.value, j.value

    def global_sum_loc(self, name, tl=1, n=0, mask=None, loc="center"):
        r = C.c_double()
        self._chk(self.L.pop_global_sum_loc(self.h, name.encode(), tl, n, mask.encode() if mask else None, self.LOC[loc], C.byref(r)))
        return r.value

    def global_sum_host(self, arr, mask=None, loc="center"):
        """POP_GlobalSum of a host array of the local blocks (optional multiplicative mask of the same shape)"""
        a = np.ascontiguousarray(arr, dtype=np.float64)
        mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.float64)
        r = C.c_double()
        P = C.POINTER(C.c_double)
        self._chk(self.L.pop_global_sum_host(self.h, a.ctypes.data_as(P), mk.ctypes.data_as(P) if mk is not None else None,
                                             self.LOC[loc], C.byref(r)))
        return r.value

    def global_sum_nfields(self, names, tl=1, n=0, mask=None):
        nf = len(names)
        arr = (C.c_char_p * nf)(*[x.encode() for x in names])
        tls, ns = (C.c_int * nf)(*([tl] * nf)), (C.c_int * nf)(*([n] * nf))
        out = (C.c_double * nf)()
        self._chk(self.L.pop_global_sum_nfields(self.h, nf, arr, tls, ns, mask.encode() if mask else None, out))
        return list(out)

    def global_sum_prod(self, a, b, tl_a=1, n_a=0, tl_b=1, n_b=0, mask=None):
        r = C.c_double()
        self._chk(self.L.pop_global_sum_prod(self.h, a.encode(), tl_a, n_a, b.encode(), tl_b, n_b,
                                             mask.encode() if mask else None, C.byref(r)))
        return r.value

    def global_sum_scalar(self, x):
        r = C.c_double()
        self._chk(self.L.pop_global_sum_scalar(self.h, float(x), C.byref(r)))
        return r.value

    def global_sum_i4(self, name):
        r = C.c_longlong()
        self._chk(self.L.pop_global_sum_i4(self.h, name.encode(), C.byref(r)))
        return r.value

    def solver_diagonal(self, block_local, corr):
        a = np.ascontiguousarray(corr, dtype=np.float64)
        assert a.size == self.nxb * self.nyb
        self._chk(self.L.pop_solver_diagonal(self.h, block_local, a.ctypes.data_as(C.POINTER(C.c_double))))

    def write_restart(self, path):
        """POP binary restart (<path> + <path>.hdr), restart.F90:1095-1715"""
        self._chk(self.L.pop_write_restart(self.h, os.fsencode(path)))

    def read_restart(self, path, byteswap=False):
        self._chk(self.L.pop_read_restart(self.h, os.fsencode(path), 1 if byteswap else 0))

    def solver_preconditioner(self, x_name, px_name, x_tl=1, px_tl=1):
        """PX = M^-1 X on the physical cells (EVP sub-block solves when preconditioner_choice = 1, else the diagonal)"""
        self._chk(self.L.pop_solver_preconditioner(self.h, x_name.encode(), x_tl, px_name.encode(), px_tl))

    def operator(self, op, k, a, b=None, o1="DH", o2="DHU", tl=1):
        """operators.F90 grad / div / zcurl at level k on named device fields (results in o1 [, o2])"""
        self._chk(self.L.pop_operator(self.h, {"grad": 0, "div": 1, "zcurl": 2}[op], k, a.encode(), (b or a).encode(), tl,
                                      o1.encode(), o2.encode()))

    def operator_host(self, op, k, block_local, a, b=None):
        """the reference's argument lists (operators.F90:49, 126, 199) on host arrays (ny_block, nx_block) of ONE local block,
        block_local = this_block%local_id (1-based): grad -> (GRADX, GRADY), div / zcurl -> one array"""
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.shape == (self.nyb, self.nxb)
        bb = np.ascontiguousarray(b if b is not None else a, dtype=np.float64)
        o1, o2 = np.empty_like(a), np.empty_like(a)
        code = {"grad": 0, "div": 1, "zcurl": 2}[op]
        self._chk(self.L.pop_operator_host(self.h, code, k, block_local, a.ctypes.data, bb.ctypes.data if code else None,
                                           o1.ctypes.data, o2.ctypes.data if code == 0 else None))
        return (o1, o2) if code == 0 else o1

    def solver_run(self):
        self._chk(self.L.pop_solver_run(self.h))

    def solver_diagnostics(self):
        it, rms = C.c_int(), C.c_double()
        self.L.pop_solver_get_diagnostics(self.h, C.byref(it), C.byref(rms))
        return it.value, rms.value

    def state(self, kk, T, S, derivs=False):
        T = np.ascontiguousarray(T, dtype=np.float64)
        S = np.ascontiguousarray(S, dtype=np.float64)
        rho = np.empty_like(T)
        dt_ = np.empty_like(T) if derivs else None
        ds_ = np.empty_like(T) if derivs else None
        P = C.POINTER(C.c_double)
        self._chk(self.L.pop_state_host(self.h, kk, T.ctypes.data_as(P), S.ctypes.data_as(P), rho.ctypes.data_as(P),
                                        dt_.ctypes.data_as(P) if derivs else None,
                                        ds_.ctypes.data_as(P) if derivs else None, T.size))
        return (rho, dt_, ds_) if derivs else rho

    # ---- timers / bench support
    def timers_reset(self):
        self.L.pop_timers_reset(self.h)

    def timer(self, name):
        ms, calls = C.c_double(), C.c_int()
        self.L.pop_timer_ms(self.h, name.encode(), C.byref(ms), C.byref(calls))
        return ms.value, calls.value

    def run_phase(self, phase):
        """one phase of baroclinic_driver / baroclinic_correct_adjust on its own (include/pop_amd.h pop_run_phase)"""
        self._chk(self.L.pop_run_phase(self.h, phase.encode()))

    def time_phase(self, phase, reps=10):
        ms = C.c_double()
        self._chk(self.L.pop_time_phase(self.h, phase.encode(), reps, C.byref(ms)))
        return ms.value

    # ---- halo plan introspection
    # ---- in-library RCCL transport (include/pop_amd.h) ----
    @staticmethod
    def rccl_unique_id():
        """128-byte id made on rank 0; broadcast it, then every rank calls comm_init_rccl(id)."""
        buf = C.create_string_buffer(128)
        if lib().pop_rccl_unique_id(buf):
            raise PopError("pop_rccl_unique_id failed (librccl not loadable?)")
        return buf.raw

    def comm_init_rccl(self, id128):
        assert len(id128) == 128
        self._chk(self.L.pop_comm_init_rccl(self.h, C.c_char_p(id128)))

    def comm_selftest(self):
        self._chk(self.L.pop_comm_selftest(self.h))

    def comm_info(self):
        """what the installed transport is (pop_comm_info), as a dict for a run's record"""
        out, path = (C.c_int * 6)(), C.create_string_buffer(256)
        self._chk(self.L.pop_comm_info(self.h, out, path, 256))
        return {"kind": ["none", "host-callbacks", "rccl-native"][out[0]], "ncclCommCount": out[1], "ncclCommUserRank": out[2],
                "ncclCommCount_second_communicator": out[3], "halo_neighbour_ranks": out[4], "midstep_halo_overlap": bool(out[5]),
                "librccl": path.value.decode()}

    def halo_plan(self):
        nl, nf, npeer = C.c_int(), C.c_int(), C.c_int()
        self.L.pop_halo_plan_counts(self.h, C.byref(nl), C.byref(nf), C.byref(npeer))
        dst, src, fill = (C.c_int * max(nl.value, 1))(), (C.c_int * max(nl.value, 1))(), (C.c_int * max(nf.value, 1))()
        self.L.pop_halo_plan_local(self.h, dst, src, fill)
        ia = lambda x: np.array(x, dtype=np.int64)
        plan = {"copy_dst": ia(dst[:nl.value]), "copy_src": ia(src[:nl.value]),
                "fill_dst": ia(fill[:nf.value]), "peers": []}
        for ip in range(npeer.value):
            r, ns, nr = C.c_int(), C.c_int(), C.c_int()
            self.L.pop_halo_plan_peer(self.h, ip, C.byref(r), C.byref(ns), C.byref(nr))
            s, d = (C.c_int * max(ns.value, 1))(), (C.c_int * max(nr.value, 1))()
            self.L.pop_halo_plan_lists(self.h, ip, s, d)
            plan["peers"].append({"rank": r.value, "send_src": ia(s[:ns.value]), "recv_dst": ia(d[:nr.value])})
        return plan
