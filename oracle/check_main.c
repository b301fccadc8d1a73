/* check_main.c -- memory check of the CPU oracle under AddressSanitizer + UBSan (TEST INFRASTRUCTURE ONLY; `make -C oracle check`).
 *
 * A plain executable: the oracle is compiled into it with -fsanitize=address,undefined, nothing is preloaded.  It creates the
 * configuration with every CESM gx-grid scheme on (tests/cesm_case.py ALL_ON: anis 'east' with the variable viscosities, the
 * submesoscale scheme, Jayne tidal mixing, the latitude-varying KPP background, GM with the transition layer and once-a-day 'bfre'
 * kappa, KPP with double diffusion, upwind3, Robert filter, P-CSI + EVP, stepped bathymetry) on 48 x 40 x 20 in 12 x 10 blocks and
 * in padded 20 x 16 blocks, runs four steps of each and prints a checksum.  The surface fluxes are force_kpp_case's
 * (tests/test_gpu_parity.py); the energy flux is a smooth function of the global indices, 0.5 W/m^2 on average.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pop_oracle.h"

static orc_config all_on(int bx, int by) {
  orc_config c;
  memset(&c, 0, sizeof c);
  c.struct_version = ORC_CONFIG_VERSION;
  c.nx_global = 48; c.ny_global = 40; c.km = 20; c.nt = 2;
  c.block_size_x = bx; c.block_size_y = by;
  c.ew_boundary = 1; c.ns_boundary = 0;
  c.hmix_momentum = 3; c.hmix_tracer = 3; c.vmix_choice = 3; c.tadvect = 2;
  c.solver_choice = 3; c.preconditioner_choice = 1; c.max_iterations = 1000; c.convergence_check_freq = 10;
  c.tmix_opt = 3; c.time_mix_freq = 17; c.steps_per_day = 4;
  c.lpressure_avg = 1; c.impcor = 1; c.reset_to_freezing = 1;
  c.lrich = 1; c.ldbl_diff = 1; c.num_v_smooth_Ri = 1;
  c.stepped_bathymetry = 1;
  c.gm_transition_layer = 1; c.gm_kappa_type = 1; c.gm_kappa_freq = 2;
  c.am = 3.0e9; c.ah = 1.0e7;
  c.const_vvc = 0.25; c.const_vdc = 0.25; c.convect_diff = 1000.0; c.convect_visc = 1000.0; c.bottom_drag = 1.0e-3; c.aidif = 1.0;
  c.rich_bckgrnd_vvc = 1.0; c.rich_bckgrnd_vdc = 0.1; c.rich_mix = 50.0;
  c.bckgrnd_vdc1 = 0.16; c.bckgrnd_vdc_dpth = 2500.0e2; c.bckgrnd_vdc_linv = 4.5e-5;
  c.Prandtl = 10.0; c.kpp_rich_mix = 50.0;
  c.convergence_criterion = 1.0e-12; c.init_ts_perturbation = 1.0e-2;
  c.aniso_alignment = 1; c.lvariable_hmix_aniso = 1;
  c.lsubmesoscale_mixing = 1; c.submeso_diag = 1; c.time_scale_constant = 8.64e4;
  return c;
}

static double run(int bx, int by) {
  const orc_config c = all_on(bx, by);
  orc_model *m = orc_create(&c);
  if (!m) { fprintf(stderr, "orc_create: %s\n", orc_last_error()); exit(1); }
  const int nxb = orc_dim(m, "nx_block"), nyb = orc_dim(m, "ny_block"), km = orc_dim(m, "km"), nb = orc_dim(m, "nblocks");
  const size_t n2 = (size_t)nxb * nyb, a2 = n2 * nb;
  const double pi = 4.0 * atan(1.0);
  const double *TLAT = orc_field(m, "TLAT", 1, 0);
  double *STF_T = orc_field(m, "STF", 1, 0), *STF_S = orc_field(m, "STF", 1, 1);
  const int *ig = orc_ifield(m, "i_glob"), *jg = orc_ifield(m, "j_glob");
  double *flux = (double *)calloc(a2, sizeof(double));
  for (int b = 0; b < nb; b++)
    for (int j = 0; j < nyb; j++) for (int i = 0; i < nxb; i++) {
      const size_t p = (size_t)b * n2 + (size_t)j * nxb + i;
      STF_T[p] = -3.0e-2 * sin(TLAT[p]) - 1.0e-2;
      STF_S[p] = 2.0e-6 * cos(2.0 * TLAT[p]);
      flux[p] = 0.5 * (1.0 + 0.5 * cos(2.0 * pi * (double)ig[b * nxb + i] / (double)c.nx_global) * sin(pi * (double)abs(jg[b * nyb + j]) / (double)c.ny_global));
    }
  orc_tidal_nml tn;
  memset(&tn, 0, sizeof tn);
  tn.struct_bytes = (int)sizeof tn; tn.ltidal_mixing = 1; tn.ltidal_max = 1; tn.ltidal_stabc = 1; tn.tidal_diag = 1;
  orc_kpp_bckgrnd_nml bn;
  memset(&bn, 0, sizeof bn);
  bn.struct_bytes = (int)sizeof bn; bn.lhoriz_varying_bckgrnd = 1; bn.bckgrnd_vdc_eq = 0.01; bn.bckgrnd_vdc_psim = 0.13; bn.bckgrnd_vdc_ban = 1.0;
  if (orc_init_tidal_mixing(m, &tn, flux, (long long)a2) || orc_init_kpp_bckgrnd(m, &bn)) { fprintf(stderr, "init: %s\n", orc_last_error()); exit(1); }
  free(flux);
  for (int s = 0; s < 4; s++)
    if (orc_step(m)) { fprintf(stderr, "step %d: the solver did not converge\n", s + 1); exit(1); }
  /* checksum over the physical cells of every block (padding and ghost cells excluded) */
  const int *ib = orc_ifield(m, "blk_ib"), *ie = orc_ifield(m, "blk_ie"), *jb = orc_ifield(m, "blk_jb"), *je = orc_ifield(m, "blk_je");
  const char *names[] = {"UVEL", "VVEL", "HDU", "HDV", "TIDAL_DIFF", "KVMIX", "KVMIX_M", "VVC"};
  double sum = 0.0;
  for (int t = 0; t < 2; t++) {
    const double *T = orc_field(m, "TRACER", 1, t), *S = orc_field(m, "SUBM_ADV_TEND", 1, t);
    for (int b = 0; b < nb; b++) for (int k = 0; k < km; k++)
      for (int j = jb[b]; j <= je[b]; j++) for (int i = ib[b]; i <= ie[b]; i++) {
        const size_t p = ((size_t)b * km + k) * n2 + (size_t)(j - 1) * nxb + (i - 1);
        sum += fabs(T[p]) + 1.0e6 * fabs(S[p]);
      }
  }
  for (size_t f = 0; f < sizeof(names) / sizeof(names[0]); f++) {
    const double *A = orc_field(m, names[f], 1, 0);
    if (!A) { fprintf(stderr, "no field %s\n", names[f]); exit(1); }
    for (int b = 0; b < nb; b++) for (int k = 0; k < km; k++)
      for (int j = jb[b]; j <= je[b]; j++) for (int i = ib[b]; i <= ie[b]; i++)
        sum += fabs(A[((size_t)b * km + k) * n2 + (size_t)(j - 1) * nxb + (i - 1)]);
  }
  const char *names2[] = {"SUBM_ML_DEPTH", "HLS_SUBM", "BCKGRND_VDC", "TLON", "PSURF", "HBLT"};
  for (size_t f = 0; f < sizeof(names2) / sizeof(names2[0]); f++) {
    const double *A = orc_field(m, names2[f], 1, 0);
    if (!A) { fprintf(stderr, "no field %s\n", names2[f]); exit(1); }
    for (int b = 0; b < nb; b++)
      for (int j = jb[b]; j <= je[b]; j++) for (int i = ib[b]; i <= ie[b]; i++)
        sum += fabs(A[(size_t)b * n2 + (size_t)(j - 1) * nxb + (i - 1)]);
  }
  printf("blocks %2d x %2d: %d solver iterations at step 4, checksum %.17g\n", bx, by, orc_solver_iterations(m), sum);
  orc_destroy(m);
  return sum;
}

int main(void) {
  const double a = run(12, 10), b = run(20, 16);
  if (!(isfinite(a) && isfinite(b))) { fprintf(stderr, "checksum is not finite\n"); return 1; }
  return 0;
}
