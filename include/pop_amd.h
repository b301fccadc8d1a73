/*
 * pop_amd.h -- C ABI of the MI355X-native POP2 dynamics core (libpop_amd.so).
 *
 * This is the drop-in boundary for the reference's per-timestep hot path.
 * The reference (ESCOMP/POP2-CESM) has no FFI: its seam is the Fortran
 * module-procedure surface that source/step_mod.F90 calls.  Each entry point
 * below names the reference routine it replaces (file:line under
 * /root/reference/); pop2-cesm_amd/fortran/ holds ISO_C_BINDING modules with
 * the reference's names and argument lists that forward here, and
 * INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions:
 *   - plain pointers and sizes only; no torch / HIP types in signatures;
 *   - every function returns int: 0 = POP_Success, nonzero = error, message
 *     via pop_last_error() (mirrors POP_ErrorSet/return, POP_ErrorMod.F90:82);
 *   - one host thread per GPU/rank; all entry points are collective across
 *     ranks (same order on every rank), like the reference's MPI tasks;
 *   - host arrays are Fortran order (nx_block, ny_block[, km], nblocks_local),
 *     i fastest, exactly source/prognostic.F90:47-66 per time level;
 *   - the three time levels are rotated by index, never copied
 *     (step_mod.F90:827-830): tl = 0 old, 1 cur, 2 new (logical).
 */
#ifndef POP_AMD_H
#define POP_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

/* Run-time configuration: the namelist subset this path reads
 * (domain_nml, grid_nml, time_manager_nml, hmix_*_nml, vertical_mix_nml,
 *  vmix_*_nml, advect_nml, pressure_grad_nml, baroclinic_nml, &solvers). */
#define POP_CONFIG_VERSION 7   /* layout of pop_config below (4: gm_transition_layer appended; 5: gm_diag_bolus and gm_kappa_bkg_srfbl out of reserved_i,
                                 * ah_bkg_bottom and kappa_depth_* appended -- added late in round 3 without a new number; 6: the hmix_aniso_nml members appended;
                                 * 7: lsubmesoscale_mixing and the mix_submeso_nml members appended).
                                 * pop_create accepts 7, 6 and 5; a version-5 struct is read up to kappa_depth_scale only (its size) and cannot select
                                 * hmix_momentum = 3, a version-6 struct up to smag_lat_gauss and cannot select lsubmesoscale_mixing.  Any other
                                 * struct_version is refused. */
typedef struct pop_config {
  int struct_version;         /* = POP_CONFIG_VERSION (round 3: every option has its own named field) */
  int nx_global, ny_global, km, nt;   /* domain_size.F90 */
  int block_size_x, block_size_y;     /* domain_size.F90 */
  int ew_boundary;            /* 0 closed, 1 cyclic   (domain.F90 ew_boundary_type) */
  int ns_boundary;            /* 0 closed, 1 cyclic, 2 tripole (time stepping: with pop_create_with_grid) */
  int hmix_momentum;          /* 2 del2, 4 del4       (horizontal_mix.F90:427-472), 3 anis (hmix_momentum_type_anis, horizontal_mix.F90:68,
                               * 194-195, 464-472; struct_version 6: the hmix_aniso_nml members at the end) */
  int hmix_tracer;            /* 2 del2, 4 del4, 3 gm: Gent-McWilliams eddy transport + isopycnal (Redi) diffusion with ah as the isopycnal
                               * diffusivity (hmix_gm.F90:1102-2226 in the code-default hmix_gm_nml: constant kappa, kappa_freq 'never',
                               * no transition layer; see gm_slope_control, ah_bolus ... below) */
  int lvariable_hmix;         /* hmix_del2.F90:223, hmix_del4.F90:200 */
  int vmix_choice;            /* 1 const, 2 rich, 3 kpp (vertical_mix.F90:280-296) */
  int tadvect;                /* 1 centered, 2 upwind3, 3 lw_lim (advection.F90:1667-1729, 2313-2676, 2684-3280) */
  int solver_choice;          /* 1 pcg, 2 ChronGear, 3 PCSI with Lanczos eigenvalue bounds
                               * (POP_SolversMod.F90:442-472, 1510-1835, 2699-2990) */
  int max_iterations;
  int convergence_check_freq;
  int tmix_opt;               /* 0 none, 1 avg, 2 avgfit (time_management.F90:2170-2213), 3 robert
                               * (Robert-Asselin-Williams filter, step_mod.F90:919-1350) */
  int time_mix_freq;
  int steps_per_day;          /* dt_option='steps_per_day', dt_count */
  int lbouss_correct, lpressure_avg, impcor, reset_to_freezing;
  int lrich, ldbl_diff, lshort_wave, lcheckekmo, num_v_smooth_Ri; /* vmix_kpp_nml (lshort_wave reads SHF_QSW: pop_set_field) */
  int maxlanczosstep;         /* solvers_nml, PCSI (POP_SolversMod.F90:626): 0 = 20 */
  int convergence_check_start;/* solvers_nml convergenceCheckStart, PCSI (:636): 0 = 60 */
  int preconditioner_choice;  /* solvers_nml preconditionerChoice (:124, :252-290, :2434-2696): 0 'diagonal', 1 'evp'; any solver_choice */
  int stepped_bathymetry;     /* synthetic topography: 0 the reference's internal flat bottom (grid.F90:880-884, 1957-1985),
                               * 1 stepped bathymetry KMT = 3 ... km (TEST EXTENSION, not in the reference) */
  int distribution_type;      /* domain_nml clinic_distribution_type (domain.F90): 0 contiguous runs of equal block counts
                               * ('cartesian' for one column of blocks), 1 contiguous runs of equal ocean columns
                               * (load-balanced, in the spirit of 'rake' / 'spacecurve', distribution.F90) */
  int kpp_ml_diagnostics;     /* 1: the diagnostic mixed-layer depths of vmix_coeffs_kpp every step (HMXL, HMXL_DR,
                               * vmix_kpp.F90:1310-1418; fields "HMXL", "HMXL_DR"); 0: not computed (nothing on the path reads them) */
  int sw_absorption_type;     /* sw_absorption_nml: 0 'top-layer', 1 'jerlov' (sw_absorption.F90:736-811),
                               * 2 'chlorophyll' (:467-728, 951-1047; the field "CHL", mg/m^3, is 0.25 until set with pop_set_field) */
  int jerlov_water_type;      /* 1..5 (0 = 3, the CESM default) */
  int lsw_absorb;             /* != 0: the penetrating short wave SHF_QSW heats the levels below the first
                               * (add_sw_absorb, sw_absorption.F90:818-947, in tracer_update) with sw_absorption_type */
  int partial_bottom_cells;   /* grid_nml partial_bottom_cells (grid.F90:916-1020): 1 = the bottom T cell of every column has the
                               * thickness DZBC (pop_grid_input.DZBC = the record of bottom_cell_file; NULL with the internal
                               * topography: a synthetic DZBC in (0.25, 1] dz(KMT), TEST EXTENSION), DZT / DZU as the reference forms them */
  int gm_slope_control;       /* hmix_gm_nml slope_control_choice: 0 'notanh' (the default, hmix_gm.F90:1508-1539), 1 'tanh' (:1490-1506),
                               * 2 'clip' (:1541-1573: the slopes themselves are limited), 3 'Gerd' (:1575-1594) */
  int gm_kappa_type;          /* hmix_gm_nml kappa_isop_choice = kappa_thic_choice: 0 'constant', 2 'depth' (kappa_depth_1 + kappa_depth_2 exp(-zt / kappa_depth_scale),
                               * hmix_gm.F90:850-874), 1 'bfre' (buoyancy_frequency_dependent_profile,
                               * hmix_gm.F90:3011-3180: KAPPA_VERTICAL = N^2 / N_ref^2 in [0.1, 1] below the surface diabatic layer; kappa_*_deep = 0.1) */
  int gm_kappa_freq;          /* kappa_freq_choice with gm_kappa_type = 1: 0 'never' (refused with 'bfre' as in the reference, hmix_gm.F90:756-780),
                               * 1 'every_time_step', 2 'once_a_day' (the first step after a day has ended, eod_last; for runs that start at midnight:
                               * with avgfit the fit interval is the day, without averaging steps every steps_per_day-th step ends one) */
  double am, ah;              /* del2 [cm^2/s] or del4 [cm^4/s] */
  double const_vvc, const_vdc;
  double convect_diff, convect_visc, bottom_drag, aidif;
  double rich_bckgrnd_vvc, rich_bckgrnd_vdc, rich_mix;
  double bckgrnd_vdc1, bckgrnd_vdc2, bckgrnd_vdc_dpth, bckgrnd_vdc_linv;
  double Prandtl, kpp_rich_mix;
  double convergence_criterion;
  double init_ts_perturbation;           /* amplitude of the synthetic initial T perturbation (1e-2) */
  double robert_alpha, robert_nu;        /* tmix_opt = 3 (0 = defaults 0.53, 0.20, time_management.F90:461-462) */
  double lanczos_convergence_criterion;  /* PCSI LanczosconvergenceCriterion (0 = 0.1) */
  /* hmix_gm_nml (hmix_gm.F90:364-428); each 0 = the value that makes the default set-up: */
  double ah_bolus;                       /* thickness (bolus) diffusivity, 0 = ah (then the skew-flux terms cancel, 'cancellation_occurs' :970-983) */
  double ah_bkg_srfbl;                   /* horizontal diffusivity inside the surface boundary layer, 0 = ah */
  double slm_r, slm_b;                   /* maximum slope for isopycnal / thickness diffusion, 0 = 0.3 */
  int gm_transition_layer;               /* hmix_gm_nml transition_layer_on (hmix_gm.F90:3183-3848: transition_layer, merged_streamfunction,
                                          * apply_vertical_profile_to_isop_hor_diff); with KPP the diabatic depth is the smoothed HMXL */
  int gm_diag_bolus;                     /* hmix_gm_nml diag_gm_bolus: 1 = the eddy-induced (bolus) velocity of hdifft_gm (hmix_gm.F90:2079-2151) every step:
                                          * fields "UISOP", "VISOP" (east / north face of the T cell) and "WISOP" (top of the T cell); nothing on the path reads them */
  int gm_kappa_bkg_srfbl;                /* 1: hmix_gm_nml use_const_ah_bkg_srfbl = .false. -- the horizontal diffusivity of the surface boundary layer follows
                                          * KAPPA_ISOP instead of ah_bkg_srfbl (hmix_gm.F90:1369-1370, 1602-1631) */
  int reserved_i[1];                     /* must be 0 */
  double ah_bkg_bottom;                  /* hmix_gm_nml ah_bkg_bottom: horizontal diffusivity in the bottom half of the bottom cell (:1757-1761), 0 = none */
  double kappa_depth_1, kappa_depth_2, kappa_depth_scale;   /* gm_kappa_type = 2; scale 0 = 150000 cm */
  /* ---- struct_version 6: hmix_aniso_nml (hmix_aniso.F90:167-224), read with hmix_momentum = 3 only.  A 0 stands for the code default
   *      given last in each comment wherever 0 is not a meaningful value of its own. */
  int aniso_alignment;        /* hmix_alignment_choice: 0 'grid', 1 'east' (NORM1 = cos ANGLE, NORM2 = -sin ANGLE, :777-780); 2 'flow' is refused:
                               * :787-794 resets the whole NORM1 / NORM2 block array whenever one point is slower than eps, and land points have
                               * U = 0, so the result depends on the block's loop order (code default 'flow') */
  int lvariable_hmix_aniso;   /* 1: F_PARA / F_PERP of compute_ccsm_var_viscosity (:1069-1296, var_viscosity_infile 'ccsm-internal'), tapered to
                               * AMAX_CFL without lsmag_aniso (:444-464); pop_set_field("F_PARA" | "F_PERP") replaces them as a var_viscosity_infile
                               * would, the taper applied again (code default .false.) */
  int lsmag_aniso;            /* 1: Smagorinsky viscosities (:807-856); refused with smag_lat_fact = 0 (:512-531 leaves F_PERP_SMAG unset then)
                               * (code default .false.) */
  int vconst_5;               /* points of the western-boundary buffer (:1211), 0 = 3 */
  double visc_para, visc_perp;/* constant viscosities [cm^2/s] (code default 0) */
  double c_para, c_perp;      /* Smagorinsky coefficients (code default 0) */
  double u_para, u_perp;      /* accepted without effect, as in the reference: hdiffu_aniso never reads them (code default 0) */
  double vconst_1;            /* [cm^2/s], 0 = 1e7 */
  double vconst_2;            /* 0 = 24.5 */
  double vconst_3;            /* 0 = 0.2 */
  double vconst_4;            /* [1/cm], 0 = 1e-8 */
  double vconst_6;            /* [cm^2/s], 0 = 1e7 */
  double vconst_7;            /* [degrees], 0 = 45 */
  double smag_lat;            /* [degrees], 0 = 20 */
  double smag_lat_fact;       /* no default: 0 with lsmag_aniso is refused (code default 0.98) */
  double smag_lat_gauss;      /* 0 = 98 */
  /* ---- struct_version 7: the submesoscale mixed-layer eddy scheme of Fox-Kemper, Ferrari and Hallberg (mix_submeso.F90; hmix_nml
   *      lsubmesoscale_mixing and mix_submeso_nml :164-188).  With lsubmesoscale_mixing = 0 nothing below is read. */
  int lsubmesoscale_mixing;   /* 1: the restratification tendency of submeso_sf / submeso_flux added to the Gent-McWilliams tendency
                               * (horizontal_mix.F90:566-581).  Needs hmix_tracer = 3 and no partial_bottom_cells; with KPP the mixed-layer
                               * depth is HMXL (kpp_ml_diagnostics is switched on), zw(1) otherwise (code default .false.; CESM: .true. on gx grids) */
  int luse_const_horiz_len_scale;   /* 1: HLS = hor_length_scale everywhere (code default .false.) */
  int submeso_diag;           /* 1: the diagnostic velocities "USUBM", "VSUBM" (east / north face), "WSUBM" (top of the T cell) (:599-661) and the
                               * tendency "SUBM_ADV_TEND" (n = 0, 1) of each tracer on its own, readable with pop_get_field.  Always readable with
                               * the scheme on: "HLS_SUBM", "SUBM_ML_DEPTH", "SUBM_TIME_SCALE"; "GM_GTK" (n = 0, 1, hmix_tracer = 3) is the whole
                               * mixing tendency the tracer right-hand side reads */
  double efficiency_factor;   /* 0 = 0.07 */
  double time_scale_constant; /* [s], 0 = 3.456e5 (4 days, the code default; CESM's namelist default is 8.64e4) */
  double hor_length_scale;    /* [cm], 0 = 5e5: the floor of the length scale, or the length scale itself with luse_const_horiz_len_scale */
} pop_config;

typedef struct pop_ctx pop_ctx;

/* flags for pop_create */
#define POP_CREATE_HOST_ONLY 1   /* build blocks/grid/plans on the host, touch no GPU */
#define POP_CREATE_PLAN_ONLY 2   /* implies HOST_ONLY: the block table (create_blocks, blocks.F90:100-270), the distribution (domain.F90:379-543)
                                  * and the halo plan (POP_HaloCreate, mpi/POP_HaloMod.F90:142-1640) of this rank only -- no grid fields.  For
                                  * checking a decomposition of any size in milliseconds: pop_get_block, pop_local_block_ids, pop_halo_plan_*,
                                  * pop_halo_update_host_*, pop_get_dim("ocean_columns_local" | "ocean_columns_total") work; field access does not */

/* ---- tuning: kernel-form and schedule choices.  NONE changes a result: every alternative is tested bitwise equal to the
 *      default (tests/test_gpu_parity.py, test_gpu_land.py, test_gpu_land_schemes.py, test_gpu_passive_matrix.py,
 *      test_gpu_multirank.py); they exist for measurement and for those
 *      tests.  Resolved ONCE, at pop_create*, into one plan (csrc/forms.hpp resolve_forms): the library's size rules, overridden by
 *      the caller's pop_tuning (fields left at POP_TUNING_UNSET keep the rule), overridden by the environment variable
 *      POP_<FIELD NAME IN UPPER CASE> (read at create only; nothing in the step reads the environment or the request).
 *      pop_get_tuning returns the REQUEST (struct and environment merged; POP_TUNING_UNSET = the rule applied);
 *      pop_get_dim("form_<entry of the plan>") returns the OUTCOME, on host-only contexts too. ---------------------- */
#define POP_TUNING_UNSET (-2147483647 - 1)
typedef struct pop_tuning {
  int struct_bytes;        /* sizeof(pop_tuning) of the caller */
  int land_skip;           /* 0: every workgroup runs (no land elimination at tile granularity) */
  int land_full_steps;     /* steps after set-up / restart / a new state that run every workgroup (default 4) */
  int xcd_remap;           /* column kernels: workgroup order 0 linear, 1 XCD bands; any other value is refused at create */
  int red_band;            /* 2-D reduction / solver kernels: XCD-banded chunk order */
  int lds_order;           /* LDS-tiled stencil kernels: 1 = XCD patch order */
  int momentum_lds;        /* momentum right-hand side: LDS tile rows 8 | 4, 0 = direct-load kernel */
  int tracer_lds;          /* tracer right-hand side (centred advection): LDS tile rows 8 | 4, 0 = direct-load kernel */
  int generic_thomas;      /* 1: scratch-staged Thomas kernels for U, V even at km = 60 / 62 */
  int reg_thomas_t;        /* tracers: 1 register Thomas kernels (km = 60 / 62), 0 generic */
  int thomas_pair;         /* corrector: both tracers in one thread when they share the diffusivity array */
  int tracer_fwd;          /* predictor: forward elimination inside the tracer right-hand-side kernel */
  int vdc_shared;          /* 0: two diffusivity arrays even without double diffusion */
  int side_stream;         /* 0: no side stream at all (every launch in the reference's order on one stream) */
  int del4_side;           /* 0: del4 first Laplacians in line instead of beside the vertical-mixing coefficients */
  int del4_tile;           /* del4 first Laplacians: patch rows 0 | 2 | 4 | 8 | 16 */
  int d2t_fuse, d2u_fuse;  /* del4: the previous step's tracer / momentum launch forms the first Laplacian */
  int vmixu_defer;         /* implicit vertical mixing of U, V launched after the solve with the barotropic sum */
  int vmixu_inline;        /* 1: implicit vertical mixing of U, V on the launch stream */
  int btrop_inline;        /* 1: barotropic velocity added in the step tail (the reference's order) */
  int kpp_ahead;           /* KPP of the next step beside the barotropic solver */
  int kpp_col;             /* KPP kernel forms, bit mask: 1 ushear column, 4 buoydiff LDS, 8 buoydiff + interior fused, 16 the two as one column march;
                            * 2 is unused and accepted: a mask with it selects what the same mask without it selects */
  int kpp_lazy;            /* 0: surface-layer buoyancy difference at every level */
  int kpp_ushear_hint;     /* 0: shear kernel forms every level */
  int kpp_ushear_margin;   /* levels beyond the previous boundary-layer level (default 3; may be negative) */
  int kpp_side_stream;     /* 0: KPP kernels on one stream */
  int kpp_interior_generic;/* 1: scratch-staged interior kernel even at km = 60 / 62 */
  int kpp_src_full;        /* 1: the tracer kernel reads KPP_SRC at every level */
  int solver_unfused;      /* 1: one kernel per solver operation */
  int solver_nograph;      /* 1: no hipGraph replay of the check intervals */
  int solver_presum;       /* 1: block sums by their own launch even on small grids */
  int solver_distributed;  /* 1: never the replicated barotropic solve */
  int solver_overlap_off;  /* 1: solver halo exchange in line with the all-reduce */
  int fpcg_b2;             /* 0: one cell per thread in step B of the fused pcg */
  int pcsi_step2;          /* fused P-CSI step with two cells per thread */
  int halo_separate;       /* 1: one message per field instead of one per neighbour */
  int halo_overlap_off;    /* 1: mid-step tracer halo in line instead of beside interior tiles */
  int rccl_overlap;        /* second communicator: 0 none, 1 (default) own stream, 2 ... */
  int evp_wave;            /* EVP block preconditioner: 0 one thread per sub-block; 3 (default) anti-diagonal wavefronts (8 lanes per sub-block), the
                            * operands in registers, the coefficients read from their 2-D fields and every load of the front end issued up front
                            * (unconditional at clamped addresses; the conditions select values); any other value is refused at create */
  int fpcg_a_pair;         /* 0: one chunk per workgroup in step A of the fused pcg even on compacted launches */
  int kpp_sparse;          /* 0: KPP boundary-layer kernel streams every level even when the interior kernel formed the convection mask */
  int pbc_generic_thomas;  /* 1: partial bottom cells with the scratch-staged Thomas kernels even at km = 60 / 62 */
  int pbc_generic_kpp;     /* 1: partial bottom cells with the 3-D-parallel / scratch-staged KPP kernels on large grids too */
  int gm_sf_stored;        /* 0: Gent-McWilliams without cancellation: the stream-function terms SF_SLX / SF_SLY re-derived in the flux kernel instead of stored */
  int state3d_levels;      /* density of a whole 3-D array: levels per thread, 4 (default) | 2 | 8 with the per-level EOS coefficients read from
                            * a table, 1 = one cell per thread with the coefficients formed in place */
  int pcg_persist;         /* pcg, ChronGear and P-CSI with the diagonal preconditioner on small 2-D systems (<= 2000 chunks of 256 cells in <= 8 blocks, single rank or the replicated solve):
                            * 1 (the default where it applies) = the whole solve as ONE resident launch, vectors in LDS / registers, workgroups exchanging partials and halo z through
                            * tagged 16-byte memory words (kernels_pcg_persist.hpp); 0 = the two-launch fused iteration; 2 | 4 | 8: measurement only, that many chunks per workgroup */
  int gm_flux_tile;        /* 0: Gent-McWilliams fluxes cell by cell (every horizontal face flux evaluated in both cells that share it); default 1 = once per face in 64 x 8 tiles */
  int pcsi_two_step;       /* fused P-CSI (diagonal preconditioner; one rank or blocks spread over ranks; through a tripole fold whose partners are on the rank): 1 = two iterations per pass over the state where no check follows
                            * (k_pcsi_step_x2; the default on large grids), 0 = one launch per iteration */
  int block_sums_relay;    /* ordered block sums of more than 64 x 256 chunk partials (the fused pcg / ChronGear of large grids): 0 = 256 threads, each adding
                            * its accumulator's terms in batches (two or three memory round trips); default 1 = 1024 threads, four per accumulator, every term
                            * requested at once and the quarters added in turn (k_block_sums_relay: the same additions in the same order); 2 = also below 64 terms (cross-check) */
  int aniso_side;          /* hmix_momentum = 3: 0 = the friction k_hdiffu_aniso in line before the momentum right-hand side; default 1 = on the
                            * side stream beside the vertical-mixing coefficients (it reads only the mix-time U, V and fixed coefficients) */
  int submeso_all_levels;  /* lsubmesoscale_mixing: 1 = k_submeso_flux marches all km levels; default 0 = every tile stops at the last level that
                            * can hold a non-zero tendency (from the largest mixed-layer depth over the tile and a one-cell rim); bitwise equal */
} pop_tuning;
void pop_tuning_init(pop_tuning *t);   /* struct_bytes = sizeof, every field POP_TUNING_UNSET */
int pop_get_tuning(const pop_ctx *ctx, pop_tuning *resolved);   /* the request; fields still POP_TUNING_UNSET: the size rule applied */

/* ---- lifecycle (no reference counterpart: the reference's state is module
 *      global, initial.F90:133-699 builds it) -------------------------------- */
int pop_create(const pop_config *cfg, int rank, int nranks, int flags, pop_ctx **out);
/* horiz_grid_opt = 'file' / topography_opt = 'file' (grid.F90:1314-1542 read_horiz_grid, :2025-2107 read_topography):
 * the seven records of horiz_grid_file and the KMT record of topography_file as global (nx_global, ny_global)
 * arrays, i fastest, scattered with the reference's field locations (mpi/gather_scatter.F90:862-1161, tripole ghost
 * rows mirrored).  KMT = NULL: topography_internal on the supplied ULAT / ULON.  ANGLE is accepted for file-format
 * parity; nothing on this path reads it (the analytic wind stress is not rotated).  The arrays are read during the
 * call only.  A tripole decomposition (ns_boundary = 2) steps only on a grid supplied this way: the internal grid is
 * lat-lon and has no values beyond the fold.  pop_read_grid_files fills the arrays from the reference's direct-access
 * binary files (records of nx_global*ny_global r8 / one record of i4, native byte order). */
typedef struct pop_grid_input {
  const double *ULAT, *ULON, *HTN, *HTE, *HUS, *HUW, *ANGLE;
  const int *KMT;
  const double *DZBC;   /* partial_bottom_cells: the record of bottom_cell_file (read_bottom_cell, grid.F90:2116-2186): thickness of
                         * the bottom T cell of every column [cm], global (nx_global, ny_global), scattered as a centre scalar.
                         * NULL: see pop_config.partial_bottom_cells */
} pop_grid_input;
int pop_create_with_grid(const pop_config *cfg, const pop_grid_input *grid, int rank, int nranks, int flags, pop_ctx **out);
/* the same with the caller's tuning (NULL: none); grid may be NULL */
int pop_create_tuned(const pop_config *cfg, const pop_grid_input *grid, const pop_tuning *tuning, int rank, int nranks, int flags, pop_ctx **out);
int pop_read_grid_files(const char *horiz_grid_file, const char *topography_file, int nx_global, int ny_global,
                        double *seven_records /* 7*nx*ny, or NULL */, int *kmt /* nx*ny, or NULL */);
int pop_destroy(pop_ctx *ctx);
const char *pop_last_error(const pop_ctx *ctx);

/* ---- tidal mixing (tidal_mixing.F90; vmix_kpp.F90:1758-1857): tidal_nml through an entry point of its own, as the
 *      reference's init_tidal_mixing1 / init_tidal_mixing2 are calls separate from init_vmix_kpp.  The native (lcvmix = .false.)
 *      Jayne and St. Laurent (2001) method only; the Schmittner and Polzin methods, ltidal_lunar_cycle, ltidal_schmittner_socn,
 *      lniw_mixing and the CVMix path are not built.  A 0 in a double member stands for the code default. */
#define POP_MAX_TIDAL_MIN_REGIONS 9   /* tidal_mixing.F90:262 max_tidal_min_regions */
typedef struct pop_tidal_nml {
  int struct_bytes;             /* sizeof(pop_tidal_nml) of the caller */
  int ltidal_mixing;            /* 0: the call succeeds and builds nothing */
  int tidal_mixing_method;      /* tidal_mixing_method_choice: 0 'jayne'; 1 'schmittner' and 2 'polzin' are refused */
  int ltidal_max;               /* TIDAL_DIFF limited to tidal_mix_max (code default .true.) */
  int ltidal_stabc;             /* stability control at the two levels above the bottom (code default .true.) */
  int lccsm_control_compatible; /* 1 switches the stability control off (tidal_mixing.F90:3117) */
  int ltidal_min_regions;       /* a floor of the tidal diffusivity near the bottom inside latitude / longitude boxes (code default .false.) */
  int num_tidal_min_regions;    /* 0 .. POP_MAX_TIDAL_MIN_REGIONS */
  int tidal_diag;               /* 1: "TIDAL_DIFF", "TIDAL_N2", "KVMIX", "KVMIX_M" of the last evaluation readable with pop_get_field
                                 * (the KPP look-ahead is then off: the fields belong to the step that has run) */
  double tidal_local_mixing_fraction;   /* 0 = 0.33 */
  double tidal_mixing_efficiency;       /* 0 = 0.2 */
  double vertical_decay_scale;          /* [cm], 0 = 500e2 */
  double tidal_mix_max;                 /* [cm^2/s], 0 = 100 */
  double tidal_min_values[POP_MAX_TIDAL_MIN_REGIONS];        /* [cm^2/s] (code default 20) */
  double tidal_TLATmin_regions[POP_MAX_TIDAL_MIN_REGIONS];   /* degrees */
  double tidal_TLATmax_regions[POP_MAX_TIDAL_MIN_REGIONS];
  double tidal_TLONmin_regions[POP_MAX_TIDAL_MIN_REGIONS];   /* degrees east, 0 .. 360; min > max: the box wraps around 360 */
  double tidal_TLONmax_regions[POP_MAX_TIDAL_MIN_REGIONS];
  int tidal_min_regions_klevels[POP_MAX_TIDAL_MIN_REGIONS];  /* 2 | 6: levels above the bottom the floor applies to (any other value: none; code default 6) */
} pop_tidal_nml;
void pop_tidal_nml_init(pop_tidal_nml *nml);   /* struct_bytes = sizeof, the code defaults of tidal_mixing.F90:670-760 (ltidal_mixing = 0) */
/* init_tidal_mixing1 / 2 (tidal_mixing.F90:542-1340) for the Jayne method.  energy_flux: the record of tidal_energy_file [W/m^2] on the
 * local blocks, (nx_block, ny_block, nblocks) as pop_set_field takes a 2-D field; its ghost cells are filled by a halo update (centre,
 * scalar), so with several ranks the call is collective.  Once per context, before the first pop_time_manager / pop_step / pop_run_phase.
 * Needs vmix_choice = 3 (initial.F90:1962) and bckgrnd_vdc2 = 0 (:1975).  Works on a host-only context (the fields below that
 * need no device).  Afterwards pop_get_field serves "TIDAL_ENERGY_FLUX" [g/s^3], "TIDAL_COEF_3D", "TLON" [radians] and, with tidal_diag,
 * "TIDAL_DIFF", "TIDAL_N2", "KVMIX", "KVMIX_M"; pop_get_ifield serves "TIDAL_REGION_BOX2D".  Restart files carry nothing of it. */
int pop_init_tidal_mixing(pop_ctx *ctx, const pop_tidal_nml *nml, const double *energy_flux, long long count);

/* ---- latitude-varying KPP background diffusivity (lhoriz_varying_bckgrnd of vmix_kpp_nml; vmix_kpp.F90:544-611): the Gregg
 *      equatorial minimum, the MacKinnon maxima at +-28.9 degrees and the Banda Sea value, through an entry point of its own
 *      (pop_config keeps its layout).  bckgrnd_vdc1 and Prandtl are pop_config's.  The three doubles are taken literally: 0 is a
 *      value, not a stand-in for the default.  lniw_mixing and the CVMix path are not built. */
typedef struct pop_kpp_bckgrnd_nml {
  int struct_bytes;              /* sizeof(pop_kpp_bckgrnd_nml) of the caller */
  int lhoriz_varying_bckgrnd;    /* 0: the call succeeds and builds nothing */
  int larctic_bckgrnd_vdc;       /* 1: bckgrnd_vdc_eq at and north of 70 degrees */
  double bckgrnd_vdc_eq;         /* [cm^2/s] equatorial value (code default 0.01) */
  double bckgrnd_vdc_psim;       /* [cm^2/s] amplitude of the maxima at +-28.9 degrees (code default 0.13) */
  double bckgrnd_vdc_ban;        /* [cm^2/s] Banda Sea value (code default 1.0) */
} pop_kpp_bckgrnd_nml;
void pop_kpp_bckgrnd_nml_init(pop_kpp_bckgrnd_nml *nml);   /* struct_bytes = sizeof, the code defaults of vmix_kpp.F90:337-349 (both switches 0) */
/* The lhoriz_varying_bckgrnd branch of init_vmix_kpp (vmix_kpp.F90:544-611): bckgrnd_vdc from TLAT and TLON on every cell of every
 * local block, ghost cells included (a ghost cell carries its source cell's latitude and longitude), bckgrnd_vvc = Prandtl *
 * bckgrnd_vdc.  Once per context, after pop_create* and before the first pop_time_manager / pop_step / pop_run_phase; with several
 * ranks after the transport is installed and on every rank (TLON takes a halo update).  Before or after pop_init_tidal_mixing: both
 * orders give the same bits.  Refused: vmix_choice != 3; bckgrnd_vdc2 != 0 (vmix_kpp.F90:518); a negative bckgrnd_vdc_eq / _psim /
 * _ban; a struct_bytes of another layout; a second call; a call after a step or a phase.  Works on a host-only context.
 * Afterwards pop_get_field serves "BCKGRND_VDC" and "BCKGRND_VVC" (the reference's tavg fields VDC_BCK / VVC_BCK) as 2-D fields --
 * ONE level is stored where the reference stores km identical copies -- and "TLON" [radians].  Restart files carry nothing of it. */
int pop_init_kpp_bckgrnd(pop_ctx *ctx, const pop_kpp_bckgrnd_nml *nml);

/* ---- passive tracers (nt = 3 .. 8) and ideal age (iage_mod.F90).  A tracer n >= 3 is a plain passive tracer unless made ideal age
 *      here: no source, no reset, 0 at the three time levels, STF(n) = TFW(n) = 0 until set with pop_set_field; it is advected and
 *      mixed as T and S are (cfg.tadvect, the (T, S) mixing schemes, salinity's vertical diffusivity) and feeds nothing back.
 * pop_init_iage makes tracer n (1-based, 3 .. nt) ideal age: interior source 1 / (365 * 86400) [years/s] at the levels 1 < k <= KMT
 * (iage_mod.F90:325-355), TRACER(:,:,1) = 0 after the tracer update and after the Robert filter (:386-415), 0 at the three time
 * levels now.  Once per tracer (several tracers may each be ideal age), after pop_create* and -- with several ranks -- the transport,
 * before the first pop_time_manager / pop_step / pop_run_phase, in any order with the other pop_init_* calls.  Refused: n outside
 * 3 .. nt; a second call for the same n; a call after a step or a phase.  Works on a host-only context.
 * Restart files name the tracer IAGE (IAGE_<n> from the second one on; TRACER<nn> for a plain passive tracer) and do not carry the
 * marking: make the call again before pop_read_restart. */
int pop_init_iage(pop_ctx *ctx, int n);

/* ---- frazil ice formation (ice.F90; ice_nml) through an entry point of its own: pop_config keeps its layout, and a context that
 *      never makes the call steps exactly as before.  Wherever a cell of the levels 1 .. kmxice is colder than the freezing point the
 *      cell is warmed to it and salinity adjusted; the heat debt is kept in QICE (this call) and AQICE (accumulated) for the coupler.
 *      The surface layer is the variable-thickness one (dz(1) + PSURF/grav + eps2), as everywhere in this library.  The doubles are
 *      taken literally.  The freezing point (shr_frz_mod of CIME, not part of POP) is restated from memory: DESIGN.md section 13. */
typedef struct pop_ice_nml {
  int struct_bytes;             /* sizeof(pop_ice_nml) of the caller */
  int ice_freq_opt;             /* 0 'never', 1 'coupled'; 2 'nyear' .. 7 'nstep' are refused (ice.F90:211-234 set a flag that ice_formation never reads, :424-428) */
  int licecesm2;                /* 1: ice forms on every step (time_management.F90:1959-1991); 0 with 'coupled' needs tmix_opt robert or avgfit */
  int kmxice;                   /* ice forms in the levels 1 .. kmxice (code default 1) */
  int lactive_ice;              /* accepted for namelist parity: nothing on this path reads it */
  int lfw_as_salt_flx;          /* 1: virtual salt flux (CESM): S += (salref - salice) POTICE cp_over_lhfusion / thickness; 0: the fresh-water form -- the
                                 * volume-replacement formulas of ice.F90:496-504, 555-557 and FW_FREEZE.  Adding FW_FREEZE to FW / TFW (forcing.F90:425-437) stays
                                 * with the caller, who owns the surface forcing */
  int tfreeze_option;           /* 0 'minus1p8', 1 'linear_salt', 2 'mushy' */
  double sea_ice_salinity;      /* [psu] (4.0) */
  double ocn_ref_salinity;      /* [psu] (34.7) */
  double latent_heat_fusion;    /* [erg/g] (3.34e9) */
  double cp_sw;                 /* [erg/g/K] (3.996e7) */
  double rho_sw;                /* [g/cm^3] (4.1 / 3.996) */
  double rho_fw;                /* [g/cm^3] (1.0) */
} pop_ice_nml;
void pop_ice_nml_init(pop_ice_nml *nml);   /* struct_bytes = sizeof, the code defaults of ice.F90:158-162, forcing_sfwf.F90:268, pop_constants.F90:239-250 ('never') */
/* init_ice (ice.F90:98-317).  Once per context, after pop_create* and -- with several ranks -- the transport, before the first
 * pop_time_manager / pop_step / pop_run_phase, in any order with the other pop_init_* calls.  Works on a host-only context.  Allocates
 * QICE, AQICE, QFLUX, FW_FREEZE (zeros) and sets tlast_ice = 0; liceform = (ice_freq_opt != 'never').  After the call
 * pop_baroclinic_correct_adjust adds dtt * time_weight to tlast_ice on every step (increment_tlast_ice, baroclinic.F90:1253: whatever
 * ice_freq_opt says).  With liceform: the corrector's freeze clamp (reset_to_freezing) is off (baroclinic.F90:1418);
 * pop_baroclinic_correct_adjust, without the Robert filter, forms ice on TRACER(new) after the corrector; with the Robert filter
 * pop_step_tail forms ice on TRACER(cur), then TRACER(new), after the filter's conservation adjustment (step_mod.F90:1250-1273).
 * Without the Robert filter QICE, AQICE and FW_FREEZE take part in pop_step_tail's halo update.  Refused: kmxice outside
 * 1 .. km; a negative constant; a struct_bytes of another layout; a second call; a call after a step or a phase; 'coupled' with
 * licecesm2 = 0 unless tmix_opt is robert or avgfit (the pre-CESM2 rule follows the coupler's calendar); ice_freq_opt 'nyear' .. 'nstep'.
 * Afterwards pop_get_field / pop_set_field serve "QICE", "AQICE", "QFLUX", "FW_FREEZE" and pop_get_scalar "tlast_ice", "time_weight",
 * "cp_over_lhfusion".  Restart files then carry the AQICE record, the real FW_FREEZE and the attribute tlast_ice (the reference's
 * QFLUX-instead-of-AQICE record at a coupled time step, restart.F90:680-687, is not built); without the call they are byte for byte
 * what they were. */
int pop_init_ice(pop_ctx *ctx, const pop_ice_nml *nml);
/* ice_formation (ice.F90:357-621) on TRACER(:,:,:,:,tl) and PSURF(:,:,tl), tl = 0 old, 1 cur, 2 new: one kernel launch over every cell
 * of every local block, ghost cells included.  Legal after pop_init_ice even with 'never': a caller who owns the step sequence decides
 * when ice forms.  time_weight is that of the step pop_time_manager last set up (0.5 on an averaging step, otherwise 1; 1 before any
 * step).  QICE is zeroed at the start of the call, AQICE carries over; RHO(tl) is recomputed at the levels 1 .. kmxice. */
int pop_ice_formation(pop_ctx *ctx, int tl);
/* ice_flx_to_coupler (ice.F90:625-717) on TRACER(cur), PSURF(cur): AQICE halved for avg, avgfit and robert, QICE = the merged freeze
 * and melt potential, QFLUX = QICE / tlast_ice / hflux_factor (0 if tlast_ice = 0; hflux_factor = 1000 / (rho_sw cp_sw)) */
int pop_ice_flx_to_coupler(pop_ctx *ctx);
/* ocn_import_export.F90:715-717 after the export: tlast_ice = 0, AQICE = 0, QICE = 0 */
int pop_ice_export_reset(pop_ctx *ctx);
/* tfreez (ice.F90:725-757) on count host values of salinity [g/g]: the host twin of the device function (one definition) */
int pop_tfreez_host(pop_ctx *ctx, const double *S, double *TFRZ, long long count);

/* ---- coupled surface forcing on the device (forcing_coupled.F90, drivers/mct/ocn_import_export.F90:171-239, the tail of
 *      set_surface_forcing forcing.F90:379-437) through entry points of its own: a context that never makes the init call steps
 *      exactly as before, and its caller keeps the surface forcing (pop_set_field of STF, SMF, SMFT, FW, TFW, SHF_QSW).  After the
 *      call the library owns those six fields: pop_set_coupled_forcing forms them from the coupler's x2o fields once per coupling
 *      interval, pop_set_surface_forcing -- the head of pop_step -- applies the per-step part.  The surface layer is the
 *      variable-thickness one ('varthick'), as everywhere in this library.  DESIGN.md section 18 has the rules and what is not built. */
/* ---- marginal-sea balance (ms_balance.F90): the excess or deficit of fresh water of every marginal sea (a region with a negative
 *      number) is moved to or from a patch of the open ocean near it.  pop_init_ms_balance is init_ms_balance (:61-453); the balancing
 *      itself (ms_balancing :461-646) runs inside pop_set_coupled_forcing when pop_coupled_nml.lms_balance = 1. */
#define POP_MAX_MS 7              /* grid.F90:191 max_ms */
#define POP_MS_WARN_TWO_REGIONS 1 /* the distribution points span two regions (ms_balance.F90:351-369) */
#define POP_MS_WARN_MAX_POINTS 2  /* max_points reached: other points of the search area may have been left out (:340-345) */
typedef struct pop_ms_region {    /* one record of the region_info_file (grid.F90:2709-2715) */
  int number;                     /* REGION_MASK value; negative: a marginal sea */
  char name[36];
  double lat, lon, area;          /* marginal seas: centre of the search [degrees north / east, 0 .. 360] and the area asked for, in the units of DXT * DYT [cm^2] */
} pop_ms_region;
typedef struct pop_ms_balance_nml {
  int struct_bytes;               /* sizeof(pop_ms_balance_nml) of the caller */
  int num_regions;
  int max_points;                 /* 0 = 5000 (ms_balance.F90:81) */
  int reserved;                   /* 0 */
  const pop_ms_region *regions;   /* num_regions records, read during the call only */
} pop_ms_balance_nml;
/* Once, after pop_create* (with several ranks on every rank, with the same arguments), before pop_init_coupled_forcing; a host-only
 * context takes it too.  region_mask_global: REGION_MASK as (ny_global, nx_global), i fastest, as pop_init_transports takes it; when
 * both calls are made the masks must be equal: the first call's array is the one copy kept, a second call with another mask is refused with the first differing cell.  For every marginal sea the expanding latitude / longitude box search
 * over active-ocean points (duplicates, marginal-sea and land points rejected; it stops at max_points or when the accumulated area of
 * the T cells reaches the area asked for), fracs = areas / area with the last fraction absorbing 1 - sum, MASK_FRAC scattered as a
 * centre scalar.  Errors, not aborts: a marginal sea without a selected point; more than POP_MAX_MS seas; a second call; a call
 * after pop_init_coupled_forcing or a step.  The monthly / annual depth bookkeeping and all printing are left out. */
int pop_init_ms_balance(pop_ctx *ctx, const pop_ms_balance_nml *nml, const int *region_mask_global);
/* marginal sea `sea` = 0 .. n_marginal_seas - 1 in region order (mask_index - 1): its REGION_MASK number, the number of distribution
 * points, their area, POP_MS_WARN_* bits, and the transport [kg/s of fresh water] of the last pop_set_coupled_forcing (0 before one).
 * Any pointer may be NULL.  Reading the transport waits for the device (the only call of the coupled forcing that does); with several
 * ranks it is the same number on every rank. */
int pop_ms_balance_info(pop_ctx *ctx, int sea, int *number, int *npts, double *area, int *warnings, double *transport);
/* the distribution points of a sea, 1-based global (i, j) in selection order, and their fractions; count = npts */
int pop_ms_balance_points(pop_ctx *ctx, int sea, int *ipts, int *jpts, double *fracs, long long count);

typedef struct pop_coupled_nml {
  int struct_bytes;             /* sizeof(pop_coupled_nml) of the caller */
  int qsw_distrb_opt;           /* 0 'const', 1 '12hr' (any time stepping: the reference's restriction to avgfit / robert, forcing_coupled.F90:335-343, and its
                                 * dttxcel / dtuxcel check :345-349 are not made -- the library has no accelerated time steps); 2 'cosz' is refused:
                                 * compute_cosz needs shr_orb_mod of CIME, which is not part of POP */
  int nsteps_per_interval;      /* steps per coupling interval, the length of qsw_12hr_factor; 0 = the time manager's own
                                 * (steps_per_day, or full + half steps with avgfit) */
  int lms_balance;              /* marginal-sea balancing (ms_balance.F90, forcing_coupled.F90:845-848): needs pop_init_ms_balance before this call and
                                 * lfw_as_salt_flx (the reference balances in the virtual-salt-flux branch only) */
  int shf_formulation;          /* 0 the coupled form; 1 'partially-coupled' is refused (set_combined_forcing is not built) */
  int sfwf_formulation;         /* the same for the fresh-water flux */
  int lestuary_on, lvsf_river, lebm_on;   /* 1 is refused each (MASK_ESTUARY is 0 in what is built) */
  int luse_cpl_ifrac;           /* 1 is refused (OCN_WGT is not built) */
  double latent_heat_vapor_mks; /* [J/kg]  0 = 2.501e6  (the coupled values of pop_constants.F90:283-290) */
  double latent_heat_fusion_mks;/* [J/kg]  0 = 3.337e5 */
  double sea_ice_salinity;      /* [psu]   0 = 4.0; read by the marginal-sea balance */
  double rho_fw;                /* [g/cm^3] 0 = 1.0; likewise */
} pop_coupled_nml;
void pop_coupled_nml_init(pop_coupled_nml *nml);   /* struct_bytes = sizeof, everything else 0 ('const', the time manager's interval) */
/* pop_init_coupled (forcing_coupled.F90:128-470) for what is built.  Once per context, after pop_create* and after pop_init_ice if
 * that is used, before the first pop_time_manager / pop_step / pop_run_phase.  hflux_factor, salinity_factor = -ocn_ref_salinity *
 * fwflux_factor, lfw_as_salt_flx, lactive_ice, tfreeze_option and the sea-ice salinity of the frazil-ice terms are the context's:
 * pop_ice_nml's after pop_init_ice, its code defaults otherwise.  Forms ANGLET, COS_ANGLET = cos(ANGLET), SIN_ANGLET on the host
 * (grid.F90:660-735; readable with pop_get_field on any context, before the call too) and qsw_12hr_factor from the context's
 * time stepping (forcing_coupled.F90:358-408; pop_coupled_qsw_factor reads it back).  Works on a host-only context (no device
 * fields).  Refused, each with its reason: a second call; a call after a step or a phase; a struct_bytes of another layout;
 * everything the struct's comments call refused; nsteps_per_interval < 0; lms_balance without pop_init_ms_balance or without
 * lfw_as_salt_flx.  pop_init_ice is refused after this call (the constants and branches above are taken from it here). */
int pop_init_coupled_forcing(pop_ctx *ctx, const pop_coupled_nml *nml);
/* qsw_12hr_factor(1 : nsteps_per_interval); count = nsteps_per_interval (pop_get_dim "cpl_nsteps_per_interval") */
int pop_coupled_qsw_factor(pop_ctx *ctx, double *factor, long long count);
/* the x2o fields of one coupling interval: host arrays in the local block layout of pop_set_field, (nx_block, ny_block, nblocks);
 * only the physical cells are read for their values (ghost cells are filled by the halo update).  NULL = zeros.  MKS units, as the
 * coupler sends them: taux, tauy [N/m^2] (true zonal / meridional); snow, rain, evap, meltw, rofl, rofi, salt [kg/m^2/s]; swnet,
 * sen, lwup, lwdn, melth [W/m^2]; ifrac [fraction]; pslv [Pa]; duu10n [m^2/s^2]. */
typedef struct pop_x2o {
  int struct_bytes;             /* sizeof(pop_x2o) of the caller */
  int reserved;                 /* 0 */
  const double *taux, *tauy, *snow, *rain, *evap, *meltw, *rofl, *rofi, *salt, *swnet, *sen, *lwup, *lwdn, *melth, *ifrac, *pslv, *duu10n;
} pop_x2o;
/* ocn_import (the fields above), rotate_wind_stress, update_ghost_cells_coupler_fluxes and pop_set_coupled_forcing
 * (forcing_coupled.F90:677-945): one staged upload of the given fields on the context's stream, then k_cpl_import, the halo updates
 * of the imported fields (SMFT as centre-located vectors; three fused batches of at most eight fields, field by field on a tripole grid),
 * k_cpl_combine, and with lms_balance the marginal-sea balance.  Leaves SMFT, SMF, STF(1), SHF_QSW and, with
 * lfw_as_salt_flx = 0, FW and TFW, with lfw_as_salt_flx = 1 STF(2); the imported fields and SHF_QSW_RAW, SHF_COMP_QSW,
 * SFWF_COMP_CPL, TFW_COMP_CPL for pop_get_field.  Resets the interval's step count to 0.  count = nx_block * ny_block * nblocks.
 * The arrays are read during the call only.  Between steps only (refused between pop_time_manager and pop_step_tail).  On one
 * rank nothing in the call waits for the device except the reuse of the staging buffer by a second call. */
int pop_set_coupled_forcing(pop_ctx *ctx, const pop_x2o *x2o, long long count);
/* the per-step tail of set_surface_forcing (forcing.F90:379-437): SHF_QSW = qsw_12hr_factor(index_qsw) * SHF_COMP_QSW with index_qsw =
 * mod(steps of this interval, nsteps_per_interval) + 1; with lfw_as_salt_flx = 0 and ice formation on (pop_init_ice, ice_freq_opt
 * 'coupled') FW = SFWF_COMP_CPL + FW_FREEZE, TFW(1) = TFW_COMP_CPL(1) + FW_FREEZE * tfreez(S(cur)), TFW(2) = TFW_COMP_CPL(2) +
 * FW_FREEZE * salice.  pop_step calls it at its head, before pop_time_manager (step_mod.F90:231); a caller that owns the sequence
 * calls it there.  pop_time_manager advances the interval's step count.  Returns 0 and does nothing while the coupled forcing is not
 * initialised or no pop_set_coupled_forcing has been made. */
int pop_set_surface_forcing(pop_ctx *ctx);
/* out4 = {initialised, qsw_distrb_opt, nsteps_per_interval, steps of this interval so far}; n_marginal_seas: of pop_init_ms_balance */
int pop_coupled_info(pop_ctx *ctx, int *out4, int *n_marginal_seas);

/* ---- blocks.F90:43-63 / get_block (blocks.F90:282-320) ---------------------- */
int pop_get_dim(const pop_ctx *ctx, const char *name);         /* nx_block, ny_block, km, nt,
                                                                  nblocks (local), nblocks_tot,
                                                                  nblocks_x, nblocks_y, ... */
double pop_get_scalar(const pop_ctx *ctx, const char *name);   /* dtt, dtu, dtp, residualNorm ... */
/* block_id is the global 1-based id; out[8] = {block_id, local_id, ib, ie, jb, je, iblock, jblock};
 * i_glob (nx_block) / j_glob (ny_block) may be NULL */
int pop_get_block(const pop_ctx *ctx, int block_id, int *out8, int *i_glob, int *j_glob);
int pop_local_block_ids(const pop_ctx *ctx, int *ids /* nblocks local */);

/* ---- state transfer: host arrays in the reference layout -------------------- */
/* name = the reference's variable name (TRACER, UVEL, VVEL, RHO, PSURF, GRADPX, GRADPY, UBTROP,
 * VBTROP, PGUESS, FW, FW_OLD, SMF, SMFT, STF, TFW, SHF_QSW, ZX, ZY, DH, DHU, VDC, VVC, RHS, grid
 * fields DXU ... ); tl = logical time level; n = tracer / vector component.
 * VDC (levels 0 .. km+1): n = 0 / 1 are KPP's two tracer classes.  Without double diffusion (ldbl_diff = 0) the reference fills
 * both with the same values (vmix_kpp.F90 ri_iwmix / blmix) and the library keeps ONE array for them: n = 0 and n = 1 read and
 * write the same storage.  KPP_SRC: a value written with pop_set_field is used at every level until KPP has run again. */
int pop_get_field(pop_ctx *ctx, const char *name, int tl, int n, double *host, long long count);
int pop_set_field(pop_ctx *ctx, const char *name, int tl, int n, const double *host, long long count);
int pop_get_ifield(pop_ctx *ctx, const char *name, int *host, long long count);
long long pop_field_count(const pop_ctx *ctx, const char *name);
/* device pointer of a field (for zero-copy host frameworks); 0 if unknown.  The call is the library's only notice that the caller
 * may WRITE the field: it drops work computed ahead from the old values (KPP look-ahead, del4 first Laplacians), marks the ghost
 * cells as possibly inconsistent and restarts the full (no land elimination) steps, exactly as pop_set_field does -- once.  A
 * caller that writes through a cached pointer must therefore fetch the pointer again before EVERY write (one call per field per
 * step; the call is cheap: no copy, no synchronisation beyond joining the library's side streams); the time levels rotate by
 * index, so the pointer of (name, tl) changes from step to step anyway. */
void *pop_field_device_ptr(pop_ctx *ctx, const char *name, int tl, int n);

/* ---- restart files: write_restart (restart.F90:1095-1715) / read_restart (:184-1088) in the reference's 'bin'
 * format (io_binary.F90): <path> = direct-access records of nx_global*ny_global r8 (native byte order, a 3-D field
 * = km records), <path>.hdr = text header with the scalars as "&GLOBAL" attributes and one "&NAME ... id:int:<first
 * record> ... /" section per field.  Fields: {UBTROP,VBTROP,PSURF,GRADPX,GRADPY}_{CUR,OLD}, PGUESS, FW_OLD,
 * FW_FREEZE (zeros), {UVEL,VVEL,TEMP,SALT}_{CUR,OLD}.  Every rank writes / reads the rows of its own blocks
 * (shared file system), rank 0 writes the header.  Reading applies the land masks and halo updates of
 * read_restart :881-1040, recomputes RHO at both time levels (initial.F90:1665-1681) and continues with leapfrog
 * steps (first_step = .false., initial.F90:1088).  flags bit 0: the data file is byte-swapped. */
int pop_write_restart(pop_ctx *ctx, const char *path);
int pop_read_restart(pop_ctx *ctx, const char *path, int flags);

/* ---- the step_mod.F90:126-911 call sequence --------------------------------- */
int pop_time_manager(pop_ctx *ctx);              /* time_management.F90:1823-1847, 2139-2234 */
int pop_dhdt(pop_ctx *ctx);                      /* surface_hgt.F90:131   dhdt(DH,DHU) */
int pop_baroclinic_driver(pop_ctx *ctx);         /* baroclinic.F90:578    baroclinic_driver(ZX,ZY,DH,DHU,err) */
int pop_barotropic_driver(pop_ctx *ctx);         /* barotropic.F90:267    barotropic_driver(ZX,ZY,err)
                                                    (includes the ZX,ZY halo of step_mod.F90:405-423) */
int pop_barotropic_driver_updated(pop_ctx *ctx); /* barotropic.F90:267 alone: ZX, ZY already halo-updated by the caller
                                                    (as step_mod.F90:405-423 does before the call) */
int pop_baroclinic_correct_adjust(pop_ctx *ctx); /* baroclinic.F90:1217 */
int pop_step_tail(pop_ctx *ctx);                 /* step_mod.F90:467-832  halos, +barotropic, PGUESS,
                                                    averaging step / time-level rotation */
int pop_step(pop_ctx *ctx);                      /* step_mod.F90:126      step(errorCode) */

/* ---- POP_HaloMod / POP_ReductionsMod / POP_SolversMod surface --------------- */
/* POP_HaloUpdate(array, halo, fieldLoc, fieldKind, errorCode, fillValue)
 * mpi/POP_HaloMod.F90:1732-1773 (2-D), :2766-3211 (3-D), :4122-4585 (4-D: n = -1 updates every
 * tracer of a field with a tracer dimension); on a device-resident field */
int pop_halo_update(pop_ctx *ctx, const char *name, int tl, int n);
/* the same with the reference's fieldLoc / fieldKind arguments (POP_GridHorzMod / POP_FieldMod constants):
 * field_loc 0 centre, 1 NE corner, 2 N face, 3 E face; field_kind 0 scalar, 1 vector, 2 angle.  They matter
 * on a tripole northern boundary only (mpi/POP_HaloMod.F90:1936-2050: mirrored copy with offsets and sign,
 * symmetrised degenerate top row for NE-corner / N-face fields; the top row of blocks on one rank). */
int pop_halo_update_loc(pop_ctx *ctx, const char *name, int tl, int n, int field_loc, int field_kind);
int pop_halo_update_host_r8_loc(pop_ctx *ctx, double *array, int nz, double fill, int field_loc, int field_kind);
int pop_halo_update_host_i4_loc(pop_ctx *ctx, int *array, int nz, int fill, int field_loc, int field_kind);
/* host-array variants used at init time and by the unit-test rule of
 * test/unit/halo/POP.F90Dipole (nz = product of trailing dims).  pop_halo_update_host_r8_loc also serves decompositions
 * over several ranks (the array is then staged through a device work field; 1 <= nz <= km) */
int pop_halo_update_host_r8(pop_ctx *ctx, double *array, int nz, double fill);
int pop_halo_update_host_i4(pop_ctx *ctx, int *array, int nz, int fill);
/* POP_GlobalSum(array, dist, fieldLoc, errorCode, mMask) mpi/POP_ReductionsMod.F90:144-389
 * (b4b formulation :348-383); mask_name may be NULL */
int pop_global_sum(pop_ctx *ctx, const char *name, int tl, int n, const char *mask_name, double *result);
/* the other members of the generic interface (mpi/POP_ReductionsMod.F90:50-64), same b4b rule:
 *   POP_GlobalSumNfields2DR8 :823-1084, POP_GlobalSumProd2DR8 :1395-1618,
 *   POP_GlobalSumScalarR8 :1091-1191 (one value per task), POP_GlobalSum2DI4 :621-816 (integer field) */
/* with fieldLoc: on a tripole grid fields on north faces (2) / NE corners (1) count the redundant half of the
 * top row once (:308-341); otherwise identical to pop_global_sum */
int pop_global_sum_loc(pop_ctx *ctx, const char *name, int tl, int n, const char *mask_name, int field_loc, double *result);
/* POP_GlobalCount :2062-2207 (non-zero physical cells), POP_GlobalMaxval/Minval :2670-3223 and
 * POP_GlobalMaxloc/Minloc :4002-4400 (value and global (i,j) of the first cell attaining it; the optional mask
 * selects cells whose mask value is non-zero; iloc / jloc may be NULL) */
int pop_global_count(pop_ctx *ctx, const char *name, int tl, int n, int field_loc, long long *count);
int pop_global_extreme(pop_ctx *ctx, const char *name, int tl, int n, const char *mask_name, int want_max,
                       double *value, int *iloc, int *jloc);
/* POP_GlobalSum on HOST arrays of the local blocks, array(nx_block, ny_block, nblocks) and an optional multiplicative mask
 * of the same shape (NULL: none) -- the reference's own argument list; staged through device work fields, same b4b rule */
int pop_global_sum_host(pop_ctx *ctx, const double *array, const double *mask, int field_loc, double *result);
int pop_global_sum_nfields(pop_ctx *ctx, int nfields, const char *const *names, const int *tl, const int *n,
                           const char *mask_name, double *results);
int pop_global_sum_prod(pop_ctx *ctx, const char *name_a, int tl_a, int n_a, const char *name_b, int tl_b, int n_b,
                        const char *mask_name, double *result);
int pop_global_sum_scalar(pop_ctx *ctx, double local_value, double *result);
int pop_global_sum_i4(pop_ctx *ctx, const char *int_field_name, long long *result);
/* POP_SolversRun(sfcPressure, rhsClinic, errorCode) POP_SolversMod.F90:327;
 * operates on PSURF(newtime) and RHS in place */
int pop_solver_run(pop_ctx *ctx);
/* POP_SolversDiagonal(diagonalCorrection(nx_block,ny_block), blockIndx, errorCode) :1110-1151:
 * centre weight of local block blockIndx (1-based) = time-independent part - correction (host array) */
int pop_solver_diagonal(pop_ctx *ctx, int block_local, const double *diagonal_correction);
/* preconditioner(PX, X, bid) :2268-2369 on every local block: PX = M^-1 X on the physical cells.  M is the EVP
 * block preconditioner (8x8 sub-block solves, :2434-2696; preconditionerChoice = 'evp') when preconditioner_choice = 1,
 * else the diagonal (current centre weight).  Private in the reference; exported so that parity tests can pin the
 * preconditioner on its own.  x_name / px_name: 2-D device fields (time level tl where it applies). */
int pop_solver_preconditioner(pop_ctx *ctx, const char *x_name, int x_tl, const char *px_name, int px_tl);
/* operators.F90 as stand-alone calls on device fields at level k (the time step has them inlined in its kernels):
 * op 0  grad(k, GRADX, GRADY, F)   :126-192   F at T points  -> o1, o2 at U points (0 where k > KMU)
 * op 1  div(k, DIV, UX, UY)        :49-119    a, b at U points -> o1 at T points, times the cell area (0 where k > KMT)
 * op 2  zcurl(k, CURL, UX, UY)     :199-272   a, b at U points -> o1 at T points, times the cell area
 * A 3-D field name selects its level-k slab; tl applies to names with time levels. */
int pop_operator(pop_ctx *ctx, int op, int k, const char *a_name, const char *b_name, int tl, const char *o1_name, const char *o2_name);
/* The same three operators with the reference's own argument lists -- div(k, DIV_OUT, UX, UY, this_block) operators.F90:49,
 * grad(k, GRADX, GRADY, F, this_block) :126, zcurl(k, CURL, UX, UY, this_block) :199 --: host arrays (nx_block, ny_block) of ONE
 * block, block_local = this_block%local_id (1-based).  a (and b for div / zcurl) in, o1 (and o2 for grad) out; the arrays are
 * staged through the GPU (the kernel is the one pop_operator launches). */
int pop_operator_host(pop_ctx *ctx, int op, int k, int block_local, const double *a, const double *b, double *o1, double *o2);
/* POP_SolversGetDiagnostics(iterationCount, residual, errorCode) :1158 */
int pop_solver_get_diagnostics(const pop_ctx *ctx, int *iterations, double *rms_residual);
/* state(k,kk,TEMPK,SALTK,this_block,RHOOUT,...) state_mod.F90:258 on n device-resident or
 * host points (host variant stages through the GPU) */
int pop_state_host(pop_ctx *ctx, int kk, const double *T, const double *S, double *rho,
                   double *drhodt, double *drhods, long long n);

/* ---- multi-rank transport: the library packs/unpacks on the GPU and asks the
 *      host to move bytes (RCCL via torch.distributed in bench.py, MPI/RCCL from
 *      Fortran).  Buffers are device pointers owned by the host framework. ---- */
typedef int (*pop_exchange_fn)(void *user, int nmsg, const int *peer, const long long *send_off,
                               const long long *send_cnt, const long long *recv_off,
                               const long long *recv_cnt);   /* offsets/counts in doubles */
typedef int (*pop_allreduce_fn)(void *user, long long off, long long cnt);
int pop_set_comm(pop_ctx *ctx, void *dev_sendbuf, void *dev_recvbuf, void *dev_redbuf,
                 long long buf_doubles, pop_exchange_fn xchg, pop_allreduce_fn allred, void *user);
long long pop_comm_buffer_doubles(const pop_ctx *ctx);   /* size the host must provide */
/* reduce buffer (block-sum vectors; in replicated-barotropic mode also the gathered RHS + guess) */
long long pop_reduce_buffer_doubles(const pop_ctx *ctx);
int pop_set_reduce_buffer(pop_ctx *ctx, void *dev_redbuf, long long doubles);
/* in-library RCCL transport (replaces the communicator set-up of mpi/POP_CommMod.F90:70-135 and the
 * MPI calls of mpi/POP_HaloMod.F90:1865-1960, mpi/POP_ReductionsMod.F90:348-383): rank 0 obtains a
 * 128-byte id, the host broadcasts it by whatever means it has (MPI_Bcast, torch.distributed), every
 * rank calls pop_comm_init_rccl.  Halo messages and block-sum all-reduces are then enqueued on the
 * context's stream with no host round trip.  librccl is opened at run time. */
int pop_rccl_unique_id(unsigned char *id128);
int pop_comm_init_rccl(pop_ctx *ctx, const unsigned char *id128);
/* what the installed transport is, for a run's record: out6 = {kind (0 none, 1 host callbacks of pop_set_comm, 2 in-library RCCL),
 * ncclCommCount of the first communicator, its ncclCommUserRank, ncclCommCount of the second communicator (0: none),
 * number of neighbour ranks in the halo plan, 1 if the mid-step halo runs beside interior tiles}; -1 where RCCL does not say.
 * lib_path (may be NULL) receives the name of the librccl that was bound. */
int pop_comm_info(const pop_ctx *ctx, int *out6, char *lib_path, int lib_path_bytes);
/* checks the installed transport (either kind): an all-reduce of known values + a self message */
int pop_comm_selftest(pop_ctx *ctx);
/* halo plan introspection (host logic, testable without a GPU) */
int pop_halo_plan_counts(const pop_ctx *ctx, int *n_local_copies, int *n_fill, int *n_peers);
int pop_halo_plan_peer(const pop_ctx *ctx, int ipeer, int *peer_rank, int *n_send, int *n_recv);
int pop_halo_plan_lists(const pop_ctx *ctx, int ipeer, int *send_src /* n_send */, int *recv_dst /* n_recv */);
int pop_halo_plan_local(const pop_ctx *ctx, int *dst, int *src /* n_local_copies */, int *fill_dst /* n_fill */);

/* ---- timers (timers.F90 phase names STEP/BAROCLINIC/BAROTROPIC/3D-UPDATE) --- */
int pop_timers_reset(pop_ctx *ctx);
int pop_timer_ms(pop_ctx *ctx, const char *name, double *total_ms, int *calls);
/* bench support: time `reps` launches of one named kernel phase with HIP events on the
 * stream it runs on; returns average ms */
int pop_time_phase(pop_ctx *ctx, const char *phase, int reps, double *avg_ms);
/* one phase of baroclinic_driver / baroclinic_correct_adjust on its own (the public routines the reference's drivers
 * call one after the other): "vmix" vmix_coeffs vertical_mix.F90:518, "hmix_tracer" / "hmix_momentum" first Laplacians of
 * hmix_del4.F90:1021 / :730 (no-ops for del2), "tracer_rhs" tracer_update baroclinic.F90:1902 for T and S, "passive_rhs" the
 * same for the tracers n = 3 .. nt (nothing with nt = 2; after "vmix", "hmix_tracer" and "tracer_rhs", whose flux velocities,
 * slopes and stream function it uses: with nt > 2 the two phases together are tracer_update), "impvmixt"
 * vertical_mix.F90:1164, "state" state_mod.F90:258 on the new tracers, "momentum_rhs" clinic baroclinic.F90:1635,
 * "impvmixu" vertical_mix.F90:1679 + baroclinic.F90:1077-1129, "correct" impvmixt_correct :1460 with the surface
 * terms of baroclinic.F90:1261-1475, "add_btrop" step_mod.F90:572-600, "ice" ice_formation ice.F90:357 on the new tracers (after
 * pop_init_ice).  Uses the step parameters of the last
 * pop_time_manager call. */
int pop_run_phase(pop_ctx *ctx, const char *phase);
int pop_device_sync(pop_ctx *ctx);

/* ---- time-averaged output (tavg.F90): accumulation on the device, normalisation, reset, streams and the 'bin' file ------------
 * A tavg entry is one field of the reference's tavg_contents, by its short name ("TEMP", "SSH2", "HBLT" ...; DESIGN.md section 14
 * lists them and where in the step each is taken).  A name belongs to one stream, 1 .. POP_TAVG_MAX_STREAMS (tavg.F90
 * max_avail_tavg_streams); the reference's duplicate names (TEMP_2, SSH_2 ...) let a second stream hold the same quantity.
 * pop_time_manager adds the weight of the step (dtt, 0.5 dtt on an averaging step; tavg_set_flag, tavg.F90:1549-1557) to tavg_sum of
 * every stream that is on -- host state, kept on a host-only context too -- and the phases of the step accumulate the entries of
 * those streams where the reference calls accumulate_tavg_field.  With nothing requested, or every stream off, a step launches,
 * allocates and moves nothing more than before.  All functions return 0 or set pop_last_error.  pop_tavg_request, pop_tavg_set_on
 * and pop_tavg_reset are refused between pop_time_manager and pop_step_tail of a step. */
#define POP_TAVG_MAX_STREAMS 9
#define POP_TAVG_MAX_FIELDS 64
/* methods, numbered as tavg.F90:75-80 */
#define POP_TAVG_METHOD_AVG 1
#define POP_TAVG_METHOD_MIN 2
#define POP_TAVG_METHOD_MAX 3
#define POP_TAVG_METHOD_QFLUX 4
#define POP_TAVG_METHOD_CONSTANT 5
/* request an entry for a stream, before the first step or between steps; the buffer is allocated here and starts reset, and the
 * stream is switched on (tavg_start_opt 'nstep', 0).  Refused with a message: an unknown name, a name the reference knows whose call
 * site is not built, a name already requested in any stream, an entry whose source the configuration does not produce (the
 * message names the missing switch), more than POP_TAVG_MAX_FIELDS entries. */
int pop_tavg_request(pop_ctx *ctx, int stream, const char *name);
int pop_tavg_set_on(pop_ctx *ctx, int stream, int on);                      /* ltavg_on of the stream */
/* any entry this configuration knows, requested or not: stream (0: not requested), ndims (2 | 3), levels of the buffer, method.
 * Any of the four pointers may be NULL. */
int pop_tavg_info(pop_ctx *ctx, const char *name, int *stream, int *ndims, int *nlevels, int *method);
int pop_tavg_sums(pop_ctx *ctx, int stream, double *tavg_sum, double *tavg_sum_qflux);
/* the buffer of a requested entry on the local blocks, in the layout pop_get_field uses: (nx_block, ny_block, [nlevels,] nblocks).
 * normalize = 1: the values tavg_norm_field_all would leave (avg: buffer * (1 / tavg_sum); qflux: buffer * (1 / tavg_sum_qflux); min,
 * max, constant: as they are), formed in a copy -- the buffer stays as it is.  tavg_sum = 0 is an error, not an abort. */
int pop_tavg_get(pop_ctx *ctx, const char *name, int normalize, double *host, long long count);
void *pop_tavg_device_ptr(pop_ctx *ctx, const char *name);
/* tavg_reset_field_stream: avg / qflux / constant buffers 0, min +1e30, max -1e30; tavg_sum = 0 (and tavg_sum_qflux where the stream
 * holds a qflux entry) */
int pop_tavg_reset(pop_ctx *ctx, int stream);
/* the entries of a stream as a 'bin' file, the format of the restart files: <path> is direct-access, one nx_global x ny_global r8
 * record per level of every entry; <path>.hdr holds the global attributes tavg_sum, tavg_sum_qflux, nsteps_total and one section per
 * entry under its short name.  restart_type = 0: normalise, write, reset the stream; 1: write the sums as they are, reset nothing.
 * Collective over the ranks (rank 0 writes the header, every rank its own rows). */
int pop_tavg_write(pop_ctx *ctx, int stream, const char *path, int restart_type);
/* reads a restart_type = 1 file into a context that has made the same requests for the stream: the sums and the physical cells of
 * every buffer, then a halo update of each buffer.  A field missing from the file is an error that names it. */
int pop_tavg_read(pop_ctx *ctx, int stream, const char *path);
/* pop_run_phase / pop_time_phase also know the sites on their own, each run once with the weight of the last pop_time_manager:
 * "tavg_forcing", "tavg_state", "tavg_tracer", "tavg_vmix", "tavg_hmix", "tavg_btrop". */

/* ---- global and CFL diagnostics (diagnostics.F90), computed on the device -------------------------------------------------------
 * The reference decides per step whether to diagnose (ldiag_global, ldiag_cfl of diag_init_sums); here the caller does:
 * pop_diag_arm arms the NEXT step only (one-shot: pop_time_manager takes the arming).  It is refused between pop_time_manager and
 * pop_step_tail of a step.  An armed step runs three more sites, each one launch plus a small second stage, and copies a few
 * numbers to pinned host memory without synchronising:
 *   "diag_global_preupdate"   in pop_step_tail after PGUESS, before the time levels rotate (diag_global_preupdate, step_mod.F90:649)
 *   "diag_global_afterupdate" at the end of pop_step_tail, after the rotation / the Robert filter (diag_global_afterupdate, :860)
 *   "diag_cfl"                at the end of pop_baroclinic_driver (cfl_advect, cfl_hdiff, cfl_check; baroclinic.F90:1203)
 * pop_run_phase / pop_time_phase know the sites by these names: they run when the context is armed or inside an armed step and do
 * nothing otherwise (run on their own they do not use the arming up).  With nothing armed every site is one test of a host flag.
 * Results stay readable until the next armed step overwrites them and carry the nsteps_total they belong to.  A host-only context
 * accepts pop_diag_arm; its getters answer the host-only error.  DESIGN.md section 15 has the rules of summation and the list of
 * the reference's diagnostics that are not built (asking for one by name says so). */
#define POP_DIAG_MAX_NT 8
typedef struct pop_diag_global {
  int struct_bytes;               /* in: sizeof(pop_diag_global) */
  int nt, km;
  int nsteps_total_pre, nsteps_total_after;   /* the step each site last ran in; -1: not yet (its numbers are NaN) */
  int iterationCount;             /* POP_SolversGetDiagnostics of that step */
  double rmsResidual;
  /* afterupdate */
  double diag_sealevel, diag_ke;
  double avg_tracer[POP_DIAG_MAX_NT];        /* [1] in ppt (salt_to_ppt) */
  double sfc_tracer_flux[POP_DIAG_MAX_NT];   /* [0] in W/m^2 (/ hflux_factor), [1] as a fresh-water flux (/ salinity_factor) */
  /* preupdate */
  double diag_ws, diag_press_free, diag_ke_free, diag_ke_psfc;
  double dtracer_avg[POP_DIAG_MAX_NT], dtracer_abs[POP_DIAG_MAX_NT];
} pop_diag_global;
int pop_diag_arm(pop_ctx *ctx, int want_global, int want_cfl);
/* avg_tracer_k: NULL, or km * nt doubles, avg_tracer_k(k, n) at [n * km + k - 1] (count = km * nt) */
int pop_diag_global_get(pop_ctx *ctx, pop_diag_global *out, double *avg_tracer_k, long long count);
/* one global diagnostic by the reference's name ("diag_ke", "avg_tracer", "dtracer_abs" ...; n: 0-based tracer index where the
 * name has one, else 0).  The reference's names whose sources exist only inside the tracer and momentum kernels ("diag_ke_adv",
 * "diag_pe", "diag_tracer_hdiff" ...) answer "known to the reference, not built". */
int pop_diag_value(pop_ctx *ctx, const char *name, int n, double *value);
/* one CFL number: name "advu" | "advv" | "advw" | "advt" | "hdifft" | "hdiffu" | "vdifft" | "vdiffu".  value and ijk[3] = the total
 * and the global (i, j, k) of its maximum; value_k[km] and ij_k[2 * km] ((i, j) of level k at [2 (k - 1)]) = the level maxima; any
 * pointer may be NULL.  The first physical cell in (block id, j, i) order that attains a maximum owns the address, whatever the
 * distribution over ranks.  The vertical-mixing numbers are those of a run with implicit vertical mixing, the only form the
 * library has: cfl_vdiff is never called (vertical_mix.F90:677-678), so they are 0 with the address (0, 0, 1).
 * nsteps_total: the step the numbers belong to. */
int pop_diag_cfl(pop_ctx *ctx, const char *name, double *value, int *ijk, double *value_k, int *ij_k, int *nsteps_total);
/* check_KE (diagnostics.F90:3260-3290) on the last diag_ke: *exceeded = diag_ke > ke_thresh or diag_ke < 0.  An error while no
 * armed step has run. */
int pop_check_ke(pop_ctx *ctx, double ke_thresh, int *exceeded);
/* grid.F90:1059-1072, formed on the host at create (a host-only context has them too): area_t, volume_t, volume_u and, km doubles
 * each, area_t_k, volume_t_k.  Any pointer may be NULL. */
int pop_grid_volumes(pop_ctx *ctx, double *area_t, double *volume_t, double *volume_u, double *area_t_k, double *volume_t_k);

/* ---- meridional overturning circulation (diags_on_lat_aux_grid.F90), accumulated on the device ---------------------------------
 * The reference forms the MOC when it writes a tavg file, from the time means of WVEL, VVEL, WISOP, VISOP, WSUBM, VSUBM
 * (tavg.F90:7204-7224, compute_moc :942-1288).  compute_moc is linear in them, so the library adds every step's binned sums,
 * weighted like any tavg entry, into small accumulators on the device and holds no 3-D WVEL.  DESIGN.md section 16 has the rules.
 *
 * pop_init_transports: init_lat_aux_grid (:121-597) and init_moc_ts_transport_arrays (:603-936).  Once, after pop_create* (with
 * several ranks on every rank, with the same arguments), before the first step or phase; a host-only context takes it too.
 * region_mask_global: REGION_MASK as (ny_global, nx_global), i fastest; NULL = 1 on ocean cells and 0 on land, allowed with
 * n_transport_reg = 1 only.  Region 1 is REGION_MASK > 0; region 2 is abs(REGION_MASK) in reg2_numbers (the caller resolves
 * transport_reg2_names to numbers and leaves marginal seas out).  The reference's refusals come back as errors with its reasons. */
#define POP_MAX_TRANSPORT_REG2 16
typedef struct pop_transports_nml {
  int struct_bytes;              /* in: sizeof(pop_transports_nml) */
  int lat_aux_grid_type;         /* 0 'southern' (default), 1 'full', 2 'user-specified' */
  int n_lat_aux_grid;            /* 'user-specified' only (default 180); the other types derive it */
  int n_transport_reg;           /* 1 or 2 (default 2) */
  int nreg2;                     /* entries of reg2_numbers */
  int reg2_numbers[POP_MAX_TRANSPORT_REG2];
  double lat_aux_begin, lat_aux_end;   /* 'user-specified' only: edge latitudes, degrees north (default -90, 90) */
} pop_transports_nml;
void pop_transports_nml_init(pop_transports_nml *nml);
int pop_init_transports(pop_ctx *ctx, const pop_transports_nml *nml, const int *region_mask_global);
/* lat_aux_edge (n + 1 doubles) and lat_aux_center (n doubles), degrees north; either array may be NULL */
int pop_lat_aux_grid(pop_ctx *ctx, int *n_lat_aux_grid, double *edge, double *center);
/* n_lat_aux_grid, km + 1, n_moc_comp (1 Eulerian; 2 + bolus with hmix_tracer = 3 and gm_diag_bolus; 3 + submesoscale with
 * lsubmesoscale_mixing, which needs submeso_diag = 1) and n_transport_reg.  pop_get_dim "lat_aux_region_start" is the row south of
 * the southernmost row of region 2 (1-based global j; 0 with one region). */
int pop_moc_info(pop_ctx *ctx, int *n_lat_aux_grid, int *km1, int *n_moc_comp, int *n_transport_reg);
/* MASK_LAT_DEPTH(n, k, m) as mask[n - 1][k - 1][m - 1] (m fastest), 1 = .true. = no ocean cell of region m at level k in bin n;
 * count = n_lat_aux_grid * km * n_transport_reg */
int pop_moc_mask(pop_ctx *ctx, int *mask, long long count);
/* the bin of every cell as (ny_global, nx_global): b = 1 .. n_lat_aux_grid when lat_aux_edge(b) <= TLATD < lat_aux_edge(b + 1)
 * (the reference's loop index n = b + 1), 0 when the cell lies in no bin */
int pop_moc_bin_map(pop_ctx *ctx, int *bins, long long count);
/* put the MOC into one tavg stream, 1 .. POP_TAVG_MAX_STREAMS: it follows that stream's ltavg_on, tavg_sum and the weight of the
 * step, and pop_tavg_reset of the stream zeroes its sums.  A stream without an entry is switched on, as by its first
 * pop_tavg_request.  Refused between pop_time_manager and pop_step_tail, before pop_init_transports, and a second time.  The
 * sums are taken at the end of pop_baroclinic_driver (phase "tavg_moc" of pop_run_phase / pop_time_phase). */
int pop_moc_request(pop_ctx *ctx, int stream);
/* TAVG_MOC_G(n, k, comp, reg) in Sverdrups as out[n - 1][k - 1][comp - 1][reg - 1] (reg fastest), count = (n_lat_aux_grid + 1) *
 * (km + 1) * n_moc_comp * n_transport_reg; in r8, where the reference stores r4.  normalize = 1: scaled by 1 / tavg_sum (an error
 * when that is 0); 0: the sums as they are.  which = 0: the running interval; 1: the snapshot pop_tavg_write(stream, path, 0) took
 * just before it reset the stream.  Synchronises; with several ranks collective, and the same on every rank. */
int pop_moc_get(pop_ctx *ctx, int normalize, int which, double *out, long long count);
/* the reduced unnormalised sums of the running interval, for a caller that carries them across a restart: bins as
 * [n_lat_aux_grid][km][n_moc_comp][n_transport_reg], then the southern-boundary rows of region 2 as [km][n_moc_comp] (only with two
 * regions).  pop_moc_sums_set takes such a vector: it replaces the sums of the interval (the device accumulators start from 0) and is
 * added last when the sums are next read, so a continued run equals the uninterrupted one to rounding, not bit for bit.  The
 * caller carries tavg_sum of the stream beside it (pop_tavg_write(.., 1) / pop_tavg_read).  Refused between pop_time_manager and
 * pop_step_tail.  count = pop_moc_sums_count. */
long long pop_moc_sums_count(pop_ctx *ctx);
int pop_moc_sums_get(pop_ctx *ctx, double *sums, long long count);
int pop_moc_sums_set(pop_ctx *ctx, const double *sums, long long count);

/* ---- northward heat and salt transports N_HEAT, N_SALT (compute_tracer_transports, diags_on_lat_aux_grid.F90:1294-1594) ----------
 * The reference forms them when it writes a tavg file, from the time means of ADVT/ADVS, HDIFT/HDIFS, VNT/VNS and their _ISOP and
 * _SUBM companions (tavg.F90:7556-7614).  The routine is linear in them, so, as for the MOC, the library adds every step's binned
 * sums on the device, weighted like a tavg entry, and holds no time-mean field.  The latitude grid, the regions and the masks are
 * those of pop_init_transports.  DESIGN.md section 17 has the rules.
 *
 * undefined_nf, the netCDF default float fill value the reference masks with: entries without an ocean cell, and the total and
 * diffusive components of region 2, whose southern-boundary diffusive transport is not available (:1563-1578). */
#define POP_UNDEFINED_NF 9.9692099683868690e+36
/* put the transports into one tavg stream, 1 .. POP_TAVG_MAX_STREAMS, for heat (tracer 1), salt (tracer 2) or both (non-zero
 * flags; one at least): they follow that stream's ltavg_on, tavg_sum and the weight of the step, and pop_tavg_reset of the stream
 * zeroes their sums.  A stream without an entry is switched on.  Refused between pop_time_manager and pop_step_tail, before
 * pop_init_transports, a second time, and with tadvect = 3 (lw_lim) and two regions: the north-face value of lw_lim is not kept, so
 * the southern-boundary transport of region 2 cannot be formed (with one region it is not needed).  The sums are taken right after
 * the (T, S) right-hand side of a step (phase "tavg_transport" of pop_run_phase / pop_time_phase; pop_run_phase("tracer_rhs")
 * includes the site, as a step does).  Every run of the site adds to the sums: pop_time_phase("tavg_transport", reps) adds the
 * step's terms reps + 1 times, so reset the stream after timing it. */
int pop_transport_request(pop_ctx *ctx, int stream, int heat, int salt);
/* n_lat_aux_grid, n_transport_comp (3; 4 with hmix_tracer = 3 and gm_diag_bolus; 5 with lsubmesoscale_mixing, :886-889),
 * n_transport_reg, and of the request the stream (0: none) and the two flags.  Any pointer may be NULL.  pop_get_dim
 * "transport_stream", "n_transport_comp" give the same. */
int pop_transport_info(pop_ctx *ctx, int *n_lat_aux_grid, int *n_transport_comp, int *n_transport_reg, int *stream, int *heat, int *salt);
/* TAVG_N_HEAT_TRANS_G (tracer = 1, PW) or TAVG_N_SALT_TRANS_G (tracer = 2, unscaled as the reference leaves it) as
 * out[n - 1][comp - 1][reg - 1] (reg fastest), count = (n_lat_aux_grid + 1) * n_transport_comp * n_transport_reg; in r8, where the
 * reference stores r4.  Components: 1 total = 2 + 3, 2 Eulerian-mean advection, 3 horizontal mixing (with Gent-McWilliams: eddy-induced
 * and submesoscale advection plus diffusion), 4 eddy-induced advection (0 without gm_diag_bolus), 5 submesoscale advection.
 * normalize, which: as pop_moc_get.  Masked entries are POP_UNDEFINED_NF.  Synchronises; with several ranks collective, and the
 * same on every rank. */
int pop_transport_get(pop_ctx *ctx, int tracer, int normalize, int which, double *out, long long count);
/* the reduced unnormalised sums of the running interval, carried across a restart as the MOC's: bins as
 * [n_lat_aux_grid][2 tracers][4 terms: -ADV TAREA, -HDIF TAREA, -ADV_ISOP TAREA, -ADV_SUBM TAREA][n_transport_reg], then the
 * southern-boundary row of region 2 as [2 tracers][3 terms: VNF, VNF_ISOP, VNF_SUBM] (only with two regions); a tracer that was
 * not requested and a term the configuration does not form stay 0.  count = pop_transport_sums_count. */
long long pop_transport_sums_count(pop_ctx *ctx);
int pop_transport_sums_get(pop_ctx *ctx, double *sums, long long count);
int pop_transport_sums_set(pop_ctx *ctx, const double *sums, long long count);
/* pop_get_field of the per-column terms of the last accumulated step, n = tracer index 0 | 1, (nx_block, ny_block, nblocks):
 * "TRN_ADV", "TRN_HDIF", "TRN_VNF" and, where the configuration forms them, "TRN_ADV_ISOP", "TRN_VNF_ISOP", "TRN_ADV_SUBM",
 * "TRN_VNF_SUBM". */

/* run all launches on the host framework's HIP stream (e.g. torch.cuda.current_stream().cuda_stream) */
int pop_set_stream(pop_ctx *ctx, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
