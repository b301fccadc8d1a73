/* orc_tidal.inc -- Jayne tidal mixing (tidal_mixing.F90, tidal_mixing_method 'jayne', lcvmix = .false.) and the latitude-varying
 * KPP background diffusivity (lhoriz_varying_bckgrnd, vmix_kpp.F90:544-611), restated for the CPU oracle.  TEST INFRASTRUCTURE ONLY.
 *
 * Not restated, refused at the init call: the Schmittner and Polzin methods, ltidal_lunar_cycle, ltidal_schmittner_socn, lniw_mixing
 * (as the device); ltidal_min_regions (tidal_mixing.F90:880-1003, 3374-3429: the device has it, tests/tidal_ref.py checks it).
 * The per-step part lives where the reference has it, in ri_iwmix (orc_kpp.inc: tidal_compute_diff below is called from there).
 */
typedef struct {
  orc_tidal_nml nml;          /* resolved: a 0 in a double member replaced by the code default (tidal_mixing.F90:670-760) */
  double *FLUX;               /* TIDAL_ENERGY_FLUX_2D [g/s^3] (nx,ny,blocks) */
  double *COEF;               /* TIDAL_COEF_3D (nx,ny,km,blocks) */
  double *DIFF, *N2, *KVMIX, *KVMIX_M;   /* (nx,ny,km,blocks) of the last vmix_coeffs_kpp */
} orc_tidal;
typedef struct {
  orc_kpp_bckgrnd_nml nml;
  double *VDC, *VVC;          /* bckgrnd_vdc(:,:,1,:), bckgrnd_vvc(:,:,1,:): the reference copies level 1 to every level (:608-611) */
} orc_bck;

/* init_tidal_mixing1 / 2 for the Jayne method with the Jayne energy file: tidal_read_energy_jayne (tidal_mixing.F90:2246-2295),
 * tidal_form_qE_2D (:2631-2661), the vertical function (:1281-1306), tidal_form_coef_jayne (:2512-2548) */
int orc_init_tidal_mixing(orc_model *m, const orc_tidal_nml *nml, const double *flux, long long count) {
  DECL_DIMS
  if (!m) return 1;
  if (!nml || nml->struct_bytes != (int)sizeof(orc_tidal_nml)) return ORC_FAIL("orc_init_tidal_mixing: struct_bytes is not sizeof(orc_tidal_nml) (%d)", (int)sizeof(orc_tidal_nml));
  if (m->tidal) return ORC_FAIL("orc_init_tidal_mixing: called a second time (once per model)");
  if (m->ran || m->nsteps_total > 0) return ORC_FAIL("orc_init_tidal_mixing: a step or a phase has already run");
  orc_tidal *T = (orc_tidal *)calloc(1, sizeof(orc_tidal));
  T->nml = *nml;
  if (!nml->ltidal_mixing) { m->tidal = T; return 0; }   /* builds nothing */
  orc_tidal_nml *n = &T->nml;
  const char *why = NULL;
  if (m->c.vmix_choice != 3) why = "tidal mixing needs vmix_choice = 3 (kpp) (initial.F90:1962)";
  else if (m->c.bckgrnd_vdc2 != 0.0) why = "tidal mixing needs bckgrnd_vdc2 = 0 (initial.F90:1975)";
  else if (n->tidal_mixing_method != 0) why = "tidal mixing: tidal_mixing_method 0 'jayne' only";
  else if (n->tidal_local_mixing_fraction < 0.0 || n->tidal_mixing_efficiency < 0.0 || n->vertical_decay_scale < 0.0 || n->tidal_mix_max < 0.0)
    why = "tidal mixing: negative parameter";
  else if (n->ltidal_min_regions) why = "tidal mixing: ltidal_min_regions is not restated in the oracle (DESIGN.md section 5)";
  else if (!flux || count != (long long)(n2 * m->nblocks)) why = "orc_init_tidal_mixing: count mismatch for the energy flux (nx_block * ny_block * nblocks)";
  if (why) { free(T); return ORC_FAIL("%s", why); }
  if (n->tidal_local_mixing_fraction == 0.0) n->tidal_local_mixing_fraction = 0.33;
  if (n->tidal_mixing_efficiency == 0.0) n->tidal_mixing_efficiency = 0.20;
  if (n->vertical_decay_scale == 0.0) n->vertical_decay_scale = 500.0e02;
  if (n->tidal_mix_max == 0.0) n->tidal_mix_max = 100.0;
  const size_t a2 = n2 * m->nblocks, a3 = n3 * m->nblocks;
  T->FLUX = dalloc(a2); T->COEF = dalloc(a3); T->DIFF = dalloc(a3); T->N2 = dalloc(a3); T->KVMIX = dalloc(a3); T->KVMIX_M = dalloc(a3);
  /* the record is read into the physical cells and halo-updated as a centre scalar; W/m^2 -> g/s^3 (:2287) */
  memcpy(T->FLUX, flux, a2 * sizeof(double));
  orc_halo(m, T->FLUX, 1, ORC_CENTER, ORC_SCALAR);
  for (size_t p = 0; p < a2; p++) T->FLUX[p] = 1000.0 * T->FLUX[p];
  const double rho_fw = 1.0;   /* pop_constants.F90:240 */
  const double tidal_gamma_rhor = n->tidal_mixing_efficiency / rho_fw;   /* :1181 */
  double *WORK = dalloc(n2), *VERTICAL_FUNC = dalloc(n3), *TIDAL_COEF_2D = dalloc(n2);
  for (int b = 0; b < m->nblocks; b++) {
    DECL_BLK
    const int *KMT = m->KMT + o2;
    const double *HT = m->HT + o2;
    for (size_t p = 0; p < n2; p++) WORK[p] = 0.0;
    for (size_t p = 0; p < n3; p++) VERTICAL_FUNC[p] = 0.0;
    for (int k = 1; k <= km; k++)
      for (size_t p = 0; p < n2; p++)
        if (k < KMT[p]) WORK[p] = WORK[p] + exp(-(HT[p] - m->zw[k]) / n->vertical_decay_scale) * m->dzw[k];
    /* :1297-1304.  WORK = 0 where KMT <= 1: the reference divides by it at k = KMT = 1; TIDAL_COEF_3D there is never read (TIDAL_DIFF is
     * formed where N2 > 0, and DBLOC(k >= KMT) = 0); 0 is kept, as the device does */
    for (int k = 1; k <= km; k++)
      for (size_t p = 0; p < n2; p++) {
        if (!(KMT[p] > 1)) continue;
        if (k < KMT[p]) VERTICAL_FUNC[(size_t)(k - 1) * n2 + p] = exp(-(HT[p] - m->zw[k]) / n->vertical_decay_scale) / WORK[p];
        if (k == KMT[p]) VERTICAL_FUNC[(size_t)(k - 1) * n2 + p] = 1.0 / WORK[p];
      }
    /* tidal_form_qE_2D and tidal_form_coef_jayne */
    for (size_t p = 0; p < n2; p++) {
      const double TIDAL_QE_2D = n->tidal_local_mixing_fraction * T->FLUX[o2 + p];
      TIDAL_COEF_2D[p] = tidal_gamma_rhor * m->RCALCT[o2 + p] * TIDAL_QE_2D;
    }
    for (int k = 1; k <= km; k++)
      for (size_t p = 0; p < n2; p++)
        if (k <= KMT[p]) T->COEF[o3 + (size_t)(k - 1) * n2 + p] = TIDAL_COEF_2D[p] * VERTICAL_FUNC[(size_t)(k - 1) * n2 + p];
  }
  free(WORK); free(VERTICAL_FUNC); free(TIDAL_COEF_2D);
  m->tidal = T;
  return 0;
}
static orc_tidal *tidal_on(const orc_model *m) {
  orc_tidal *T = (orc_tidal *)m->tidal;
  return (T && T->nml.ltidal_mixing) ? T : NULL;
}

/* tidal_compute_diff (tidal_mixing.F90:3046-3140) at level k of block b for the Jayne method: WORK1 = N^2 at the bottom of level k.
 * TD = TIDAL_DIFF of the block (nx,ny,km), 0 on entry to the k loop (vmix_kpp.F90:1759) */
static void tidal_compute_diff(const orc_model *m, const orc_tidal *T, int b, int k, const double *WORK1, double *TD) {
  DECL_DIMS DECL_BLK
  const orc_tidal_nml *n = &T->nml;
  const int *KMT = m->KMT + o2;
  const double *COEF = T->COEF + o3 + (size_t)(k - 1) * n2;
  double *TDK = TD + (size_t)(k - 1) * n2;
  for (size_t p = 0; p < n2; p++) if (WORK1[p] > 0.0) TDK[p] = COEF[p] / WORK1[p];
  if (n->ltidal_max) for (size_t p = 0; p < n2; p++) TDK[p] = TDK[p] < n->tidal_mix_max ? TDK[p] : n->tidal_mix_max;
  if (n->ltidal_stabc && !n->lccsm_control_compatible && k > 2)
    for (size_t p = 0; p < n2; p++)
      if (k == KMT[p] - 1 || k == KMT[p] - 2) TDK[p] = TDK[p] > TDK[p - n2] ? TDK[p] : TDK[p - n2];
}

/* the lhoriz_varying_bckgrnd branch of init_vmix_kpp (vmix_kpp.F90:544-611) */
int orc_init_kpp_bckgrnd(orc_model *m, const orc_kpp_bckgrnd_nml *nml) {
  DECL_DIMS
  if (!m) return 1;
  if (!nml || nml->struct_bytes != (int)sizeof(orc_kpp_bckgrnd_nml)) return ORC_FAIL("orc_init_kpp_bckgrnd: struct_bytes is not sizeof(orc_kpp_bckgrnd_nml) (%d)", (int)sizeof(orc_kpp_bckgrnd_nml));
  if (m->bck) return ORC_FAIL("orc_init_kpp_bckgrnd: called a second time (once per model)");
  if (m->ran || m->nsteps_total > 0) return ORC_FAIL("orc_init_kpp_bckgrnd: a step or a phase has already run");
  if (nml->lhoriz_varying_bckgrnd) {
    if (m->c.vmix_choice != 3) return ORC_FAIL("lhoriz_varying_bckgrnd needs vmix_choice = 3 (kpp)");
    if (m->c.bckgrnd_vdc2 != 0.0) return ORC_FAIL("lhoriz_varying_bckgrnd needs bckgrnd_vdc2 = 0 (vmix_kpp.F90:518)");
    if (nml->bckgrnd_vdc_eq < 0.0 || nml->bckgrnd_vdc_psim < 0.0 || nml->bckgrnd_vdc_ban < 0.0) return ORC_FAIL("lhoriz_varying_bckgrnd: negative parameter");
  }
  orc_bck *B = (orc_bck *)calloc(1, sizeof(orc_bck));
  B->nml = *nml;
  m->bck = B;
  if (!nml->lhoriz_varying_bckgrnd) return 0;
  const size_t a2 = n2 * m->nblocks;
  const double pi = 4.0 * atan(1.0), radian = 180.0 / pi;
  const double bckgrnd_vdc1 = m->c.bckgrnd_vdc1, bckgrnd_vdc_eq = nml->bckgrnd_vdc_eq, bckgrnd_vdc_psim = nml->bckgrnd_vdc_psim, bckgrnd_vdc_ban = nml->bckgrnd_vdc_ban;
  B->VDC = dalloc(a2); B->VVC = dalloc(a2);
  for (size_t p = 0; p < a2; p++) {
    const double TLATD = m->TLAT[p] * radian, TLOND = m->TLON[p] * radian;   /* grid.F90:3099-3100 */
    const double as = 0.4 * (TLATD + 28.9), an = 0.4 * (TLATD - 28.9);
    const double bckgrnd_vdc_psis = bckgrnd_vdc_psim * exp(-(as * as));
    const double bckgrnd_vdc_psin = bckgrnd_vdc_psim * exp(-(an * an));
    double v = bckgrnd_vdc_eq + bckgrnd_vdc_psin + bckgrnd_vdc_psis;
    if (TLATD < -10.0) v = v + bckgrnd_vdc1;
    else if (TLATD <= 10.0) v = v + bckgrnd_vdc1 * ((TLATD / 10.0) * (TLATD / 10.0));
    else v = v + bckgrnd_vdc1;
    if (TLATD < -1.0 && TLATD > -4.0 && TLOND > 103.0 && TLOND < 134.0) v = bckgrnd_vdc_ban;    /* North Banda Sea */
    if (TLATD <= -4.0 && TLATD > -7.0 && TLOND > 106.0 && TLOND < 140.0) v = bckgrnd_vdc_ban;   /* Middle Banda Sea */
    if (TLATD <= -7.0 && TLATD > -8.3 && TLOND > 111.0 && TLOND < 142.0) v = bckgrnd_vdc_ban;   /* South Banda Sea */
    if (nml->larctic_bckgrnd_vdc && TLATD >= 70.0) v = bckgrnd_vdc_eq;
    B->VDC[p] = v;
    B->VVC[p] = m->c.Prandtl * v;
  }
  return 0;
}
static void free_tidal(orc_model *m) {
  orc_tidal *T = (orc_tidal *)m->tidal;
  if (T) { free(T->FLUX); free(T->COEF); free(T->DIFF); free(T->N2); free(T->KVMIX); free(T->KVMIX_M); free(T); m->tidal = NULL; }
  orc_bck *B = (orc_bck *)m->bck;
  if (B) { free(B->VDC); free(B->VVC); free(B); m->bck = NULL; }
}
static double *orc_tidal_field(orc_model *m, const char *name) {
  const orc_tidal *T = tidal_on(m);
  const orc_bck *B = (const orc_bck *)m->bck;
  if (T) {
    if (!strcmp(name, "TIDAL_ENERGY_FLUX")) return T->FLUX;
    if (!strcmp(name, "TIDAL_COEF_3D")) return T->COEF;
    if (!strcmp(name, "TIDAL_DIFF")) return T->DIFF;
    if (!strcmp(name, "TIDAL_N2")) return T->N2;
    if (!strcmp(name, "KVMIX")) return T->KVMIX;
    if (!strcmp(name, "KVMIX_M")) return T->KVMIX_M;
  }
  if (B && B->VDC) {
    if (!strcmp(name, "BCKGRND_VDC")) return B->VDC;
    if (!strcmp(name, "BCKGRND_VVC")) return B->VVC;
  }
  return NULL;
}
