/*
 * pop_oracle.h -- CPU restatement of the POP2 per-timestep dynamics hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under oracle/ is part of the product:
 * only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load this library, and there only as the checker / reported CPU baseline.
 *
 * It follows the reference (ESCOMP/POP2-CESM, read-only under /root/reference)
 * statement for statement, in the reference's own (i,j,k,block) i-fastest
 * layout and 1-based index conventions; every function cites the file:line it
 * restates.  The reference itself cannot be compiled here, so
 * this restatement is pinned by the reference's own fixtures only:
 *   - MWJF known answer rho(S=35,theta=20,p=200bar)=1.033213242
 *     (source/state_mod.F90:413-414)
 *   - the constructive halo rule of test/unit/halo/POP.F90Dipole:134-147
 *   - the serial-sum rule of test/unit/reduction/POP.F90
 * For advection / hmix / vmix / solvers the reference holds no fixtures:
 * parity for those is "unpinned by reference tests" (see DESIGN.md).
 */
#ifndef POP_ORACLE_H
#define POP_ORACLE_H

#ifdef __cplusplus
extern "C" {
#endif

/* Same field order as include/pop_amd.h's pop_config so one ctypes
 * Structure serves both libraries (declared separately on purpose). */
#define ORC_CONFIG_VERSION 7   /* = POP_CONFIG_VERSION of include/pop_amd.h; orc_create accepts 7, 6 and 5 as the device does: a version-5 struct is
                                 * read up to kappa_depth_scale, a version-6 struct up to smag_lat_gauss, the members beyond stay 0 */
typedef struct {
  int struct_version;         /* 5, 6 or 7 (ORC_CONFIG_VERSION); orc_create returns NULL for any other, the reason in orc_last_error() */
  int nx_global, ny_global, km, nt;
  int block_size_x, block_size_y;
  int ew_boundary;            /* 0 closed, 1 cyclic */
  int ns_boundary;            /* 0 closed, 1 cyclic, 2 tripole (time stepping needs orc_create_with_grid) */
  int hmix_momentum;          /* 2 del2, 4 del4, 3 anis (struct_version >= 6) */
  int hmix_tracer;            /* 2 del2, 4 del4 */
  int lvariable_hmix;         /* variable hmix coefficients */
  int vmix_choice;            /* 1 const, 2 rich, 3 kpp */
  int tadvect;                /* 1 centered, 2 upwind3, 3 lw_lim */
  int solver_choice;          /* 1 pcg, 2 ChronGear, 3 PCSI */
  int max_iterations;
  int convergence_check_freq;
  int tmix_opt;               /* 0 none, 1 avg, 2 avgfit, 3 robert */
  int time_mix_freq;
  int steps_per_day;
  int lbouss_correct, lpressure_avg, impcor, reset_to_freezing;
  int lrich, ldbl_diff, lshort_wave, lcheckekmo, num_v_smooth_Ri; /* kpp */
  int maxlanczosstep, convergence_check_start, preconditioner_choice;   /* solvers_nml */
  int stepped_bathymetry;     /* test extension */
  int distribution_type;
  int kpp_ml_diagnostics;
  int sw_absorption_type, jerlov_water_type, lsw_absorb;
  int partial_bottom_cells;   /* grid.F90:916-1020 */
  int gm_slope_control;       /* hmix_tracer = 3 (gm): 0 notanh, 1 tanh */
  int gm_kappa_type, gm_kappa_freq;   /* 0 constant | 1 bfre; 0 never | 1 every_time_step */
  double am, ah;              /* del2 or del4 coefficients */
  double const_vvc, const_vdc;
  double convect_diff, convect_visc, bottom_drag, aidif;
  double rich_bckgrnd_vvc, rich_bckgrnd_vdc, rich_mix;
  double bckgrnd_vdc1, bckgrnd_vdc2, bckgrnd_vdc_dpth, bckgrnd_vdc_linv;
  double Prandtl, kpp_rich_mix;
  double convergence_criterion;
  double init_ts_perturbation, robert_alpha, robert_nu, lanczos_convergence_criterion;
  double ah_bolus, ah_bkg_srfbl, slm_r, slm_b;   /* hmix_gm_nml; 0 = ah, ah, 0.3, 0.3 */
  int gm_transition_layer;
  int gm_diag_bolus;
  int gm_kappa_bkg_srfbl;
  int reserved_i[1];
  double ah_bkg_bottom;
  double kappa_depth_1, kappa_depth_2, kappa_depth_scale;
  /* struct_version 6: hmix_aniso_nml (hmix_aniso.F90:167-224), read with hmix_momentum = 3; a 0 stands for the code default where the device says so */
  int aniso_alignment;        /* 0 'grid', 1 'east'; 2 'flow' is refused as on the device */
  int lvariable_hmix_aniso;   /* F_PARA / F_PERP of compute_ccsm_var_viscosity, tapered to AMAX_CFL */
  int lsmag_aniso;            /* Smagorinsky viscosities: NOT restated here, refused */
  int vconst_5;               /* 0 = 3 */
  double visc_para, visc_perp;
  double c_para, c_perp;
  double u_para, u_perp;
  double vconst_1, vconst_2, vconst_3, vconst_4, vconst_6, vconst_7;   /* 0 = 1e7, 24.5, 0.2, 1e-8, 1e7, 45 */
  double smag_lat, smag_lat_fact, smag_lat_gauss;
  /* struct_version 7: lsubmesoscale_mixing and mix_submeso_nml (mix_submeso.F90:164-188) */
  int lsubmesoscale_mixing;
  int luse_const_horiz_len_scale;
  int submeso_diag;           /* 1: "SUBM_ADV_TEND" (n = 0, 1) kept for orc_field */
  double efficiency_factor;   /* 0 = 0.07 */
  double time_scale_constant; /* 0 = 3.456e5 */
  double hor_length_scale;    /* 0 = 5e5 */
} orc_config;

typedef struct orc_model orc_model;

/* horiz_grid_opt = 'file' / topography_opt = 'file' (grid.F90:1314-1542 read_horiz_grid, :2025-2107 read_topography):
 * the records of horiz_grid_file (ULAT, ULON, HTN, HTE, HUS, HUW, ANGLE) and of topography_file (KMT) as global
 * (nx_global, ny_global) arrays, i fastest.  KMT = NULL: topography_internal on the supplied ULAT/ULON. */
typedef struct {
  const double *ULAT, *ULON, *HTN, *HTE, *HUS, *HUW, *ANGLE;
  const int *KMT;
  const double *DZBC;   /* partial_bottom_cells: record of bottom_cell_file (grid.F90:2116-2186), or NULL */
} orc_grid_input;

/* tidal_nml and the lhoriz_varying_bckgrnd members of vmix_kpp_nml through entry points of their own, with the layouts of
 * include/pop_amd.h pop_tidal_nml / pop_kpp_bckgrnd_nml (declared separately on purpose, like the config) and the same rules:
 * one call each, after orc_create* and before the first orc_time_manager / orc_step / phase, in either order.  Both return 0,
 * or non-zero with the reason in orc_last_error().  Refused as on the device: vmix_choice != 3, bckgrnd_vdc2 != 0, the
 * Schmittner and Polzin methods, negative parameters.  Refused here only: ltidal_min_regions (not restated). */
#define ORC_MAX_TIDAL_MIN_REGIONS 9
typedef struct {
  int struct_bytes;
  int ltidal_mixing, tidal_mixing_method, ltidal_max, ltidal_stabc, lccsm_control_compatible, ltidal_min_regions, num_tidal_min_regions;
  int tidal_diag;               /* accepted; "TIDAL_DIFF", "TIDAL_N2", "KVMIX", "KVMIX_M" are always kept here */
  double tidal_local_mixing_fraction, tidal_mixing_efficiency, vertical_decay_scale, tidal_mix_max;   /* 0 = 0.33, 0.2, 500e2, 100 */
  double tidal_min_values[ORC_MAX_TIDAL_MIN_REGIONS], tidal_TLATmin_regions[ORC_MAX_TIDAL_MIN_REGIONS], tidal_TLATmax_regions[ORC_MAX_TIDAL_MIN_REGIONS];
  double tidal_TLONmin_regions[ORC_MAX_TIDAL_MIN_REGIONS], tidal_TLONmax_regions[ORC_MAX_TIDAL_MIN_REGIONS];
  int tidal_min_regions_klevels[ORC_MAX_TIDAL_MIN_REGIONS];
} orc_tidal_nml;
typedef struct {
  int struct_bytes;
  int lhoriz_varying_bckgrnd, larctic_bckgrnd_vdc;
  double bckgrnd_vdc_eq, bckgrnd_vdc_psim, bckgrnd_vdc_ban;   /* taken literally */
} orc_kpp_bckgrnd_nml;
const char *orc_last_error(void);   /* why the last orc_create* returned NULL or the last init call failed */

orc_model *orc_create(const orc_config *cfg);
orc_model *orc_create_with_grid(const orc_config *cfg, const orc_grid_input *grid);   /* grid = NULL: orc_create */
void       orc_destroy(orc_model *m);
/* flux: the record of tidal_energy_file [W/m^2], (nx_block, ny_block, nblocks); its ghost cells are filled by a halo update */
int orc_init_tidal_mixing(orc_model *m, const orc_tidal_nml *nml, const double *flux, long long count);
int orc_init_kpp_bckgrnd(orc_model *m, const orc_kpp_bckgrnd_nml *nml);

/* array access by the reference's variable name; tl = 0 old,1 cur,2 new
 * (logical time level, resolved through the rotating indices); n = tracer.
 * Returns pointer to the (nx_block,ny_block[,km],nblocks) array, or NULL. */
/* Under the device's names, once the scheme is on: "HDU", "HDV" (the friction of the last clinic), "F_PARA", "F_PERP", "AMAX_CFL" (anis);
 * "SUBM_ML_DEPTH", "HLS_SUBM", "SUBM_TIME_SCALE", "SUBM_ADV_TEND" (n = 0, 1) (submeso); "TIDAL_ENERGY_FLUX", "TIDAL_COEF_3D",
 * "TIDAL_DIFF", "TIDAL_N2", "KVMIX", "KVMIX_M" (after orc_init_tidal_mixing); "BCKGRND_VDC", "BCKGRND_VVC" (2-D, after
 * orc_init_kpp_bckgrnd); "TLON", "ANGLE" always. */
double *orc_field(orc_model *m, const char *name, int tl, int n);
int    *orc_ifield(orc_model *m, const char *name);
double *orc_vfield(orc_model *m, const char *name);  /* vertical 1-D arrays */
int     orc_dim(orc_model *m, const char *name);
double  orc_scalar(orc_model *m, const char *name);

/* the step_mod.F90 call sequence, one entry per reference routine */
void orc_time_manager(orc_model *m);      /* set step flags for next step */
void orc_dhdt(orc_model *m);
int  orc_baroclinic_driver(orc_model *m);
/* the same in stages (bit mask): 1 vmix_coeffs + tracer_update, 2 impvmixt + halo, 4 state(new), 8 clinic, 16 impvmixu + finish */
int  orc_baroclinic_stages(orc_model *m, int stages);
int  orc_barotropic_driver(orc_model *m);
void orc_baroclinic_correct_adjust(orc_model *m);
void orc_step_tail(orc_model *m);
int  orc_step(orc_model *m);              /* all of the above */

/* pieces exposed for unit parity */
void   orc_state(orc_model *m, int k, int kk, const double *T, const double *S,
                 double *rho, double *drhodt, double *drhods, int npts);
double orc_state_point(double T, double S_msu, double p_bar);
void   orc_halo_update(orc_model *m, double *a, int nz, int fieldloc_unused);
void   orc_halo_update_int(orc_model *m, int *a);
/* POP_HaloUpdate(array, halo, fieldLoc, fieldKind): the ordinary update, plus the tripole pass when ns_boundary = 2 */
enum { ORC_CENTER = 0, ORC_NECORNER = 1, ORC_NFACE = 2, ORC_EFACE = 3 };
enum { ORC_SCALAR = 0, ORC_VECTOR = 1, ORC_ANGLE = 2 };
void   orc_halo(orc_model *m, double *a, int nz, int loc, int kind);
void   orc_halo_int(orc_model *m, int *a, int loc, int kind);
/* tripole northern boundary (mpi/POP_HaloMod.F90:1936-2050); loc 0 centre, 1 NE corner, 2 N face, 3 E face; kind 0 scalar, 1 vector, 2 angle */
void   orc_halo_update_tripole(orc_model *m, double *a, int nz, int loc, int kind);
void   orc_halo_update_tripole_int(orc_model *m, int *a, int loc, int kind);
double orc_global_sum(orc_model *m, const double *a, const double *mask);
double orc_global_sum_tripole(orc_model *m, const double *a, const double *mask, int loc);
int    orc_solver_iterations(orc_model *m);
double orc_solver_rms(orc_model *m);
/* POP_SolversMod.F90:2268-2369 preconditioner on whole arrays (EVP when preconditioner_choice = 1), :2992 partition */
void orc_preconditioner(orc_model *m, const double *X, double *PX);
int orc_evp_info(orc_model *m, int what, int idx);
void orc_btrop_operator(orc_model *m, const double *X, double *AX);   /* POP_SolversMod.F90:2414-2426 */
int orc_solver_run(orc_model *m, double *X, const double *B);
/* operators.F90: 0 grad :126-192, 1 div :49-119, 2 zcurl :199-272 on whole 2-D fields at level k */
void orc_operator(orc_model *m, int op, int k, const double *A, const double *B, double *O1, double *O2);         /* :327-417 */

#ifdef __cplusplus
}
#endif
#endif
