/* orc_api.inc -- construction, initial state and field registry of the CPU
 * restatement (TEST INFRASTRUCTURE ONLY; included by pop_oracle.c). */

/* Levitus 1992 global-mean profile (published data table;
 * source/initial.F90:964-1005) */
static const double depth_levitus[33] = {0, 10, 20, 30, 50, 75, 100, 125, 150, 200, 250, 300, 400, 500, 600,
  700, 800, 900, 1000, 1100, 1200, 1300, 1400, 1500, 1750, 2000, 2500, 3000, 3500, 4000, 4500, 5000, 5500};
static const double tmean_levitus[33] = {18.27, 18.22, 18.09, 17.87, 17.17, 16.11, 15.07, 14.12, 13.29, 11.87,
  10.78, 9.94, 8.53, 7.35, 6.38, 5.65, 5.06, 4.57, 4.13, 3.80, 3.51, 3.26, 3.05, 2.86, 2.47, 2.19, 1.78, 1.49,
  1.26, 1.05, 0.91, 0.87, 1.00};
static const double smean_levitus[33] = {34.57, 34.67, 34.73, 34.79, 34.89, 34.97, 35.01, 35.03, 35.03, 34.98,
  34.92, 34.86, 34.76, 34.68, 34.63, 34.60, 34.59, 34.60, 34.61, 34.63, 34.65, 34.66, 34.68, 34.70, 34.72, 34.74,
  34.75, 34.74, 34.74, 34.73, 34.73, 34.72, 34.72};

/* initial.F90:1389-1427 ('internal' init) + :1660-1676 (RHO) + the
 * deterministic perturbation of SURVEY.md 8(d) (amplitude init_ts_perturbation) */
static void init_ts(orc_model *m) {
  DECL_DIMS
  double pi = 4.0 * atan(1.0), amp = m->c.init_ts_perturbation;
  for (int b = 0; b < m->nblocks; b++) {
    DECL_BLK
    const int *ig = m->i_glob + (size_t)b * nxb, *jg = m->j_glob + (size_t)b * nyb;
    for (int k = 1; k <= km; k++) {
      double dpth_meters = m->zt[k] * 0.01;
      int kk;
      for (kk = 1; kk <= 32; kk++)
        if (dpth_meters >= depth_levitus[kk - 1] && dpth_meters < depth_levitus[kk]) break;
      if (kk > 32) kk = 33 > 32 ? 32 : kk; /* Fortran exits with kk=33; guard the table */
      double sinterp = (dpth_meters - depth_levitus[kk - 1]) / (depth_levitus[kk] - depth_levitus[kk - 1]);
      double tinit = (1.0 - sinterp) * tmean_levitus[kk - 1] + sinterp * tmean_levitus[kk];
      double sinit = (1.0 - sinterp) * smean_levitus[kk - 1] + sinterp * smean_levitus[kk];
      for (int j = 1; j <= nyb; j++) for (int i = 1; i <= nxb; i++)
        if (k <= m->KMT[o2 + P2(i, j)]) {
          double dT = amp * sin(2.0 * pi * ig[i - 1] / (double)m->c.nx_global) * cos(pi * jg[j - 1] / (double)m->c.ny_global);
          m->TRACER[0][m->curtime][o3 + P3(i, j, k)] = tinit + dT;
          m->TRACER[1][m->curtime][o3 + P3(i, j, k)] = sinit * 1.e-3;
        }
    }
  }
  /* the test perturbation is a function of the global indices, which ghost rows beyond a tripole boundary do not carry */
  if (m->c.ns_boundary == 2) orc_halo(m, m->TRACER[0][m->curtime], km, ORC_CENTER, ORC_SCALAR);
  for (int n = 0; n < m->nt; n++) {
    memcpy(m->TRACER[n][m->newtime], m->TRACER[n][m->curtime], n3 * m->nblocks * sizeof(double));
    memcpy(m->TRACER[n][m->oldtime], m->TRACER[n][m->curtime], n3 * m->nblocks * sizeof(double));
  }
  for (int b = 0; b < m->nblocks; b++) {
    DECL_BLK
    for (int k = 1; k <= km; k++) {
      size_t ok = o3 + (size_t)(k - 1) * n2;
      state_level(m, k, m->TRACER[0][m->curtime] + ok, m->TRACER[1][m->curtime] + ok, m->RHO[m->curtime] + ok, n2);
      state_level(m, k, m->TRACER[0][m->oldtime] + ok, m->TRACER[1][m->oldtime] + ok, m->RHO[m->oldtime] + ok, n2);
    }
  }
}

/* forcing_ws.F90:266-307 analytic zonal wind (ANGLE = 0 on the internal grid) */
static void init_forcing(orc_model *m) {
  size_t a2 = m->n2 * m->nblocks;
  for (size_t p = 0; p < a2; p++) {
    double s = -cos(3.0 * m->ULAT[p]), st = -cos(3.0 * m->TLAT[p]);
    m->SMF[1][p] = -sin(0.0) * s; m->SMFT[1][p] = -sin(0.0) * st;
    m->SMF[0][p] = cos(0.0) * s;  m->SMFT[0][p] = cos(0.0) * st;
  }
}

/* what the device refuses, and what this restatement leaves out (DESIGN.md section 5): NULL = accepted */
static const char *orc_refuse(const orc_config *cfg) {
  if (cfg->hmix_momentum == 3) {
    if (cfg->struct_version < 6) return "hmix_momentum = 3 (anis) needs struct_version 6: the hmix_aniso_nml members";
    if (cfg->aniso_alignment == 2) return "aniso_alignment 'flow' is refused (as on the device)";
    if (cfg->aniso_alignment < 0 || cfg->aniso_alignment > 2) return "aniso_alignment: 0 'grid' or 1 'east'";
    if (cfg->lsmag_aniso) return "lsmag_aniso: the Smagorinsky viscosities are not restated in the oracle (DESIGN.md section 5)";
  }
  if (cfg->lsubmesoscale_mixing) {
    if (cfg->hmix_tracer != 3) return "lsubmesoscale_mixing needs hmix_tracer = 3 (gm): del2 / del4 are refused as on the device";
    if (cfg->partial_bottom_cells) return "lsubmesoscale_mixing with partial_bottom_cells is refused (as on the device)";
  }
  /* init_gm aborts: 'hmix_gm currently incompatible with partial bottom cells' (hmix_gm.F90:782-785); 'depth' profile with
   * kappa_depth_2 = 0 (:724-730); 'bfre' with kappa_freq 'never' and no N^2 file (:756-780) */
  if (cfg->hmix_tracer == 3 && cfg->partial_bottom_cells) return "hmix_tracer = 3 (gm) with partial_bottom_cells is refused (hmix_gm.F90:782-785)";
  if (cfg->hmix_tracer == 3 && cfg->gm_kappa_type == 2 && cfg->kappa_depth_2 == 0.0) return "gm 'depth' kappa profile with kappa_depth_2 = 0 (hmix_gm.F90:724-730)";
  if (cfg->hmix_tracer == 3 && cfg->gm_kappa_type == 1 && cfg->gm_kappa_freq == 0) return "gm 'bfre' kappa with kappa_freq 'never' (hmix_gm.F90:756-780)";
  if (cfg->nt < 2 || cfg->nt > 8) return "nt: 2 to 8 tracers";
  return NULL;
}
orc_model *orc_create(const orc_config *cfg) { return orc_create_with_grid(cfg, NULL); }
orc_model *orc_create_with_grid(const orc_config *cfg, const orc_grid_input *grid) {
  /* layout of orc_config = include/pop_amd.h pop_config of the same version; 5 and 6 are read up to their own size, the rest stays 0 */
  orc_config cfg_full;
  memset(&cfg_full, 0, sizeof cfg_full);
  if (cfg->struct_version == 7) cfg_full = *cfg;
  else if (cfg->struct_version == 6) memcpy(&cfg_full, cfg, offsetof(orc_config, lsubmesoscale_mixing));
  else if (cfg->struct_version == 5) memcpy(&cfg_full, cfg, offsetof(orc_config, aniso_alignment));
  else { ORC_FAIL("orc_config.struct_version is %d, this library reads 5, 6 and 7", cfg->struct_version); return NULL; }
  cfg = &cfg_full;
  {
    const char *why = orc_refuse(cfg);
    if (why) { ORC_FAIL("%s", why); return NULL; }
  }
  orc_model *m = (orc_model *)calloc(1, sizeof(orc_model));
  m->c = *cfg;
  if (cfg->hmix_tracer == 3 && cfg->gm_transition_layer == 1 && cfg->vmix_choice == 3) m->c.kpp_ml_diagnostics = 1;   /* the diabatic depth is the smoothed HMXL */
  if (cfg->lsubmesoscale_mixing && cfg->vmix_choice == 3) m->c.kpp_ml_diagnostics = 1;   /* the mixed-layer depth is HMXL (mix_submeso.F90:425-426) */
  m->gin = grid;
  m->km = cfg->km; m->nt = cfg->nt;
  /* block sizes that do not divide the domain: the last row / column of blocks is padded (blocks.F90:174-265) */
  create_blocks(m);
  int km = m->km;
  size_t a2 = m->n2 * m->nblocks, a3 = m->n3 * m->nblocks;
#define V1(x) m->x = dalloc(km + 3)
  V1(dz); V1(dzw); V1(zt); V1(zw); V1(c2dz); V1(dzr); V1(dz2r); V1(dzwr); V1(pressz); V1(bouss); V1(dt); V1(c2dtt);
  V1(afac_t); V1(afac_u); V1(hfac);
#undef V1
#define A2(x) m->x = dalloc(a2)
  A2(ULAT); A2(ULON); A2(TLAT); A2(TLON); A2(ANGLE); A2(HTN); A2(HTE); A2(HUS); A2(HUW); A2(DXU); A2(DYU); A2(DXT); A2(DYT);
  A2(DXUR); A2(DYUR); A2(DXTR); A2(DYTR); A2(UAREA); A2(TAREA); A2(UAREA_R); A2(TAREA_R);
  A2(AU0); A2(AUN); A2(AUE); A2(AUNE); A2(FCOR); A2(FCORT); A2(HU); A2(HUR); A2(HT); A2(RCALCT); A2(RCALCU);
  A2(AMF); A2(AHF); A2(DTN); A2(DTS); A2(DTE); A2(DTW);
  A2(DUC); A2(DUN); A2(DUS); A2(DUE); A2(DUW); A2(DMC); A2(DMN); A2(DMS); A2(DME); A2(DMW); A2(DUM); A2(KXU); A2(KYU);
  A2(D4_AMF); A2(D4_AHF);
  A2(btropWgtNE); A2(btropWgtEast); A2(btropWgtNorth); A2(centerWgtIndep); A2(centerWgt); A2(mMask);
  A2(CHECKER); A2(CONSTNT); A2(PGUESS); A2(FW); A2(FW_OLD); A2(SHF_QSW); A2(CHL);
  A2(DH); A2(DHU); A2(ZX); A2(ZY); A2(UH); A2(VH); A2(RHS); A2(HBLT); A2(HMXL); A2(HMXL_DR);
#undef A2
  m->KMT = ialloc(a2); m->KMU = ialloc(a2); m->KMTN = ialloc(a2); m->KMTS = ialloc(a2); m->KMTE = ialloc(a2);
  m->KMTW = ialloc(a2); m->KMTEE = ialloc(a2); m->KMTNN = ialloc(a2); m->KBL = ialloc(a2);
  for (int t = 0; t < 3; t++) {
    for (int n = 0; n < m->nt; n++) m->TRACER[n][t] = dalloc(a3);
    m->UVEL[t] = dalloc(a3); m->VVEL[t] = dalloc(a3); m->RHO[t] = dalloc(a3);
    m->PSURF[t] = dalloc(a2); m->GRADPX[t] = dalloc(a2); m->GRADPY[t] = dalloc(a2);
    m->UBTROP[t] = dalloc(a2); m->VBTROP[t] = dalloc(a2);
  }
  for (int n = 0; n < 2; n++) { m->SMF[n] = dalloc(a2); m->SMFT[n] = dalloc(a2); }
  for (int n = 0; n < m->nt; n++) { m->STF[n] = dalloc(a2); m->TFW[n] = dalloc(a2); m->KPP_SRC[n] = dalloc(a3); }
  m->VDC[0] = dalloc((size_t)(km + 2) * a2); m->VDC[1] = dalloc((size_t)(km + 2) * a2);
  m->VVC = dalloc(a3);

  vert_grid(m);
  horiz_grid(m);
  /* init_state state_mod.F90:1036-1038 ; init_pressure_grad pressure_grad.F90:168-175 */
  for (int k = 1; k <= km; k++) m->pressz[k] = pressure_fn(m->zt[k] * 0.01);
  for (int k = 1; k <= km; k++)
    m->bouss[k] = cfg->lbouss_correct
      ? 1.0 / (1.02819 + 4.4004e-5 * m->pressz[k] - 2.93161e-4 * exp(-0.05 * m->pressz[k])) : 1.0;
  /* vertical_mix.F90:444-448 */
  for (int k = 1; k <= km; k++) { m->afac_u[k] = cfg->aidif * m->dzwr[k]; m->afac_t[k] = cfg->aidif * m->dzwr[k]; }
  init_time(m);
  init_del2(m);
  if (cfg->hmix_momentum == 4 || cfg->hmix_tracer == 4) init_del4(m);
  if (cfg->hmix_momentum == 3) init_aniso(m);
  if (cfg->tadvect == 2) init_upwind3(m);
  if (cfg->tadvect == 3) init_lw_lim(m);
  if (cfg->hmix_tracer == 3) init_gm(m);
  if (cfg->lsubmesoscale_mixing) init_submeso(m);
  if (cfg->tmix_opt == 3) init_rf(m);
  init_solver(m);
  if (cfg->preconditioner_choice == 1) { init_center_weight(m); init_evp(m); }   /* POP_SolversPrep :252-290 */
  if (cfg->solver_choice == 3) init_pcsi(m);   /* POP_SolversPrep: needs the operator weights */
  /* vmix_const.F90:121-122: constant for all time */
  for (size_t p = 0; p < (size_t)(km + 2) * a2; p++) { m->VDC[0][p] = 0.0; m->VDC[1][p] = 0.0; }
  if (cfg->vmix_choice == 1) {
    for (size_t p = 0; p < (size_t)(km + 2) * a2; p++) m->VDC[0][p] = cfg->const_vdc;
    for (size_t p = 0; p < a3; p++) m->VVC[p] = cfg->const_vvc;
  }
  if (cfg->vmix_choice == 3) init_vmix_kpp(m);
  if (cfg->lsw_absorb != 0) init_sw(m);   /* lsw_absorb: add_sw_absorb in tracer_update */
  init_ts(m);
  init_forcing(m);
  m->gin = NULL;
  return m;
}

void orc_destroy(orc_model *m) {
  if (!m) return;
  /* test infrastructure: process-lifetime allocations are released wholesale */
  double **dp[] = {&m->dz, &m->dzw, &m->zt, &m->zw, &m->c2dz, &m->dzr, &m->dz2r, &m->dzwr, &m->pressz, &m->bouss, &m->dt,
    &m->c2dtt, &m->afac_t, &m->afac_u, &m->hfac, &m->ULAT, &m->ULON, &m->TLAT, &m->TLON, &m->ANGLE, &m->HTN, &m->HTE, &m->HUS, &m->HUW, &m->DXU,
    &m->DYU, &m->DXT, &m->DYT, &m->DXUR, &m->DYUR, &m->DXTR, &m->DYTR, &m->UAREA, &m->TAREA, &m->UAREA_R, &m->TAREA_R,
    &m->AU0, &m->AUN, &m->AUE, &m->AUNE, &m->FCOR, &m->FCORT, &m->HU, &m->HUR, &m->HT, &m->RCALCT, &m->RCALCU, &m->AMF,
    &m->AHF, &m->DTN, &m->DTS, &m->DTE, &m->DTW, &m->DUC, &m->DUN, &m->DUS, &m->DUE, &m->DUW, &m->DMC, &m->DMN, &m->DMS,
    &m->DME, &m->DMW, &m->DUM, &m->KXU, &m->KYU, &m->D4_AMF, &m->D4_AHF, &m->btropWgtNE, &m->btropWgtEast,
    &m->btropWgtNorth, &m->centerWgtIndep, &m->centerWgt, &m->mMask, &m->CHECKER, &m->CONSTNT, &m->PGUESS, &m->FW,
    &m->FW_OLD, &m->SHF_QSW, &m->CHL, &m->DH, &m->DHU, &m->ZX, &m->ZY, &m->UH, &m->VH, &m->RHS, &m->HBLT, &m->HMXL, &m->HMXL_DR, &m->VVC,
    &m->VDC[0], &m->VDC[1], &m->DZBC, &m->DZT, &m->DZU};
  for (size_t i = 0; i < sizeof(dp) / sizeof(dp[0]); i++) free(*dp[i]);
  int *ip[] = {m->KMT, m->KMU, m->KMTN, m->KMTS, m->KMTE, m->KMTW, m->KMTEE, m->KMTNN, m->KBL, m->i_glob, m->j_glob,
    m->blk_ib, m->blk_ie, m->blk_jb, m->blk_je};
  for (size_t i = 0; i < sizeof(ip) / sizeof(ip[0]); i++) free(ip[i]);
  for (int t = 0; t < 3; t++) {
    for (int n = 0; n < m->nt; n++) free(m->TRACER[n][t]);
    free(m->UVEL[t]); free(m->VVEL[t]); free(m->RHO[t]); free(m->PSURF[t]); free(m->GRADPX[t]); free(m->GRADPY[t]);
    free(m->UBTROP[t]); free(m->VBTROP[t]);
  }
  for (int n = 0; n < 2; n++) { free(m->SMF[n]); free(m->SMFT[n]); }
  for (int n = 0; n < m->nt; n++) { free(m->STF[n]); free(m->TFW[n]); free(m->KPP_SRC[n]); }
  free_vmix_kpp(m);
  free_tidal(m);
  free_aniso(m);
  free_submeso(m);
  if (m->sw) { orc_sw *SW = (orc_sw *)m->sw; free(SW->swabs); free(SW->ztr); free(SW->Tr); free(SW); m->sw = NULL; }
  free_lw_lim(m);
  free_gm(m);
  free(m);
}

static int tlidx(orc_model *m, int tl) { return tl == 0 ? m->oldtime : tl == 1 ? m->curtime : m->newtime; }

double *orc_field(orc_model *m, const char *name, int tl, int n) {
#define F2(nm) if (!strcmp(name, #nm)) return m->nm;
  F2(ULAT) F2(ULON) F2(TLAT) F2(TLON) F2(ANGLE) F2(HTN) F2(HTE) F2(HUS) F2(HUW) F2(DXU) F2(DYU) F2(DXT) F2(DYT) F2(DXUR) F2(DYUR)
  F2(UAREA) F2(TAREA) F2(UAREA_R) F2(TAREA_R) F2(AU0) F2(AUN) F2(AUE) F2(AUNE) F2(FCOR) F2(FCORT) F2(HU) F2(HUR) F2(HT)
  F2(RCALCT) F2(RCALCU) F2(AMF) F2(AHF) F2(DTN) F2(DTS) F2(DTE) F2(DTW) F2(DUC) F2(DUN) F2(DUS) F2(DUE) F2(DUW)
  F2(DMC) F2(DMN) F2(DMS) F2(DME) F2(DMW) F2(DUM) F2(KXU) F2(KYU) F2(D4_AMF) F2(D4_AHF)
  F2(btropWgtNE) F2(btropWgtEast) F2(btropWgtNorth) F2(centerWgtIndep) F2(centerWgt) F2(mMask) F2(CHECKER) F2(CONSTNT)
  F2(DZBC) F2(DZT) F2(DZU)   /* DZT, DZU: (nx,ny,0:km+1,blocks); NULL without partial bottom cells */
  F2(PGUESS) F2(FW) F2(FW_OLD) F2(SHF_QSW) F2(CHL) F2(DH) F2(DHU) F2(ZX) F2(ZY) F2(UH) F2(VH) F2(RHS) F2(HBLT) F2(HMXL) F2(HMXL_DR) F2(VVC)
#undef F2
  if (!strcmp(name, "TRACER")) return (n >= 0 && n < m->nt) ? m->TRACER[n][tlidx(m, tl)] : NULL;
  if (!strcmp(name, "UVEL")) return m->UVEL[tlidx(m, tl)];
  if (!strcmp(name, "VVEL")) return m->VVEL[tlidx(m, tl)];
  if (!strcmp(name, "RHO")) return m->RHO[tlidx(m, tl)];
  if (!strcmp(name, "PSURF")) return m->PSURF[tlidx(m, tl)];
  if (!strcmp(name, "GRADPX")) return m->GRADPX[tlidx(m, tl)];
  if (!strcmp(name, "GRADPY")) return m->GRADPY[tlidx(m, tl)];
  if (!strcmp(name, "UBTROP")) return m->UBTROP[tlidx(m, tl)];
  if (!strcmp(name, "VBTROP")) return m->VBTROP[tlidx(m, tl)];
  if (!strcmp(name, "SMF")) return (n == 0 || n == 1) ? m->SMF[n] : NULL;
  if (!strcmp(name, "SMFT")) return (n == 0 || n == 1) ? m->SMFT[n] : NULL;
  if (!strcmp(name, "STF")) return (n >= 0 && n < m->nt) ? m->STF[n] : NULL;
  if (!strcmp(name, "TFW")) return (n >= 0 && n < m->nt) ? m->TFW[n] : NULL;
  if (!strcmp(name, "KPP_SRC")) return (n >= 0 && n < m->nt) ? m->KPP_SRC[n] : NULL;
  if (m->gm && (!strcmp(name, "UISOP") || !strcmp(name, "VISOP") || !strcmp(name, "WISOP") || !strncmp(name, "GM_SF_", 6) || !strncmp(name, "TLT_", 4))) return orc_gm_field(m, name, n);
  if (m->del4) {
    const orc_del4 *D = (const orc_del4 *)m->del4;
#define FD(nm) if (!strcmp(name, "d4" #nm)) return D->nm;
    FD(DUC) FD(DUN) FD(DUS) FD(DUE) FD(DUW) FD(DMC) FD(DMN) FD(DMS) FD(DME) FD(DMW) FD(DUM) FD(DTN) FD(DTS) FD(DTE) FD(DTW)
#undef FD
  }
  if (m->upw3) {
    const orc_upw3 *U = (const orc_upw3 *)m->upw3;
#define FU(nm) if (!strcmp(name, #nm)) return U->nm;
    FU(TALFXP) FU(TBETXP) FU(TGAMXP) FU(TALFYP) FU(TBETYP) FU(TGAMYP) FU(TALFXM) FU(TBETXM) FU(TDELXM) FU(TALFYM) FU(TBETYM) FU(TDELYM)
#undef FU
  }
  if (!strcmp(name, "VDC")) return (n == 0 || n == 1) ? m->VDC[n] : NULL; /* (nx,ny,0:km+1,blocks) */
  if (m->submeso) { double *f = orc_submeso_field(m, name, n); if (f) return f; }
  if (m->aniso) {
    const orc_aniso *A = (const orc_aniso *)m->aniso;
#define FA(nm) if (!strcmp(name, #nm)) return A->nm;
    FA(HDU) FA(HDV) FA(F_PARA) FA(F_PERP) FA(AMAX_CFL) FA(H1E) FA(H1W) FA(H2N) FA(H2S) FA(K1E) FA(K1W) FA(K2N) FA(K2S)
#undef FA
  }
  if (m->tidal || m->bck) { double *f = orc_tidal_field(m, name); if (f) return f; }
  return NULL;
}
int *orc_ifield(orc_model *m, const char *name) {
#define FI(nm) if (!strcmp(name, #nm)) return m->nm;
  FI(KMT) FI(KMU) FI(KMTN) FI(KMTS) FI(KMTE) FI(KMTW) FI(KMTEE) FI(KMTNN) FI(KBL) FI(i_glob) FI(j_glob)
  FI(blk_ib) FI(blk_ie) FI(blk_jb) FI(blk_je)
#undef FI
  return NULL;
}
double *orc_vfield(orc_model *m, const char *name) {
#define FV(nm) if (!strcmp(name, #nm)) return m->nm;
  FV(dz) FV(dzw) FV(zt) FV(zw) FV(c2dz) FV(dzr) FV(dz2r) FV(dzwr) FV(pressz) FV(bouss) FV(dt) FV(c2dtt) FV(afac_t) FV(afac_u)
#undef FV
  if (m->upw3) {
    const orc_upw3 *U = (const orc_upw3 *)m->upw3;
#define FU(nm) if (!strcmp(name, #nm)) return U->nm;
    FU(talfzp) FU(tbetzp) FU(tgamzp) FU(talfzm) FU(tbetzm) FU(tdelzm)
#undef FU
  }
  return NULL;
}
int orc_dim(orc_model *m, const char *name) {
  if (!strcmp(name, "nx_block")) return m->nxb;
  if (!strcmp(name, "ny_block")) return m->nyb;
  if (!strcmp(name, "km")) return m->km;
  if (!strcmp(name, "nt")) return m->nt;
  if (!strcmp(name, "nblocks")) return m->nblocks;
  if (!strcmp(name, "nblocks_x")) return m->nbx;
  if (!strcmp(name, "nblocks_y")) return m->nby;
  if (!strcmp(name, "oldtime")) return m->oldtime;
  if (!strcmp(name, "curtime")) return m->curtime;
  if (!strcmp(name, "newtime")) return m->newtime;
  if (!strcmp(name, "leapfrogts")) return m->leapfrogts;
  if (!strcmp(name, "avg_ts")) return m->avg_ts;
  if (!strcmp(name, "nsteps_total")) return m->nsteps_total;
  if (!strcmp(name, "nsteps_per_interval")) return m->nsteps_per_interval;
  return -1;
}
double orc_scalar(orc_model *m, const char *name) {
  if (!strcmp(name, "dtt")) return m->dtt;
  if (!strcmp(name, "dtu")) return m->dtu;
  if (!strcmp(name, "dtp")) return m->dtp;
  if (!strcmp(name, "residualNorm")) return m->residualNorm;
  if (!strcmp(name, "convergenceCriterion")) return m->convergenceCriterion;
  if (!strcmp(name, "rcheck")) return m->rcheck;
  if (!strcmp(name, "rconst")) return m->rconst;
  if (!strcmp(name, "uarea_equator")) return m->uarea_equator;
  if (!strcmp(name, "rmsResidual")) return m->rmsResidual;
  if (m->pcsi) {
    const orc_pcsi *Pc = (const orc_pcsi *)m->pcsi;
    if (!strcmp(name, "PcsiMaxEigs")) return Pc->maxeig;
    if (!strcmp(name, "PcsiMinEigs")) return Pc->mineig;
    if (!strcmp(name, "lanczos_steps")) return (double)Pc->lanczos_steps;
  }
  if (m->rf) {
    const orc_rf *R = (const orc_rf *)m->rf;
    if (!strcmp(name, "robert_curtime")) return R->robert_curtime;
    if (!strcmp(name, "robert_newtime")) return R->robert_newtime;
    if (!strcmp(name, "rf_volume_2_km")) return R->rf_volume_2_km;
    if (!strcmp(name, "open_ocean_volume_2_km")) return R->open_ocean_volume_2_km;
    if (!strcmp(name, "bgtarea_t_1")) return R->bgtarea_t_k[1];
    if (!strcmp(name, "rf_S1")) return R->rf_S[0];
    if (!strcmp(name, "rf_S2")) return R->rf_S[1];
  }
  return NAN;
}
/* preconditioner (:2268-2369) on every block: EVP sub-block solves when enabled, else r/diag with the current centre weight */
void orc_preconditioner(orc_model *m, const double *X, double *PX) {
  const size_t nall = m->n2 * m->nblocks;
  if (m->evp) { for (int b = 0; b < m->nblocks; b++) evp_apply(m, b, PX, X); return; }
  for (size_t p = 0; p < nall; p++) PX[p] = X[p] * ((m->centerWgt[p] != 0.0) ? 1.0 / m->centerWgt[p] : 0.0);   /* A0R form :1961-1972 */
}
/* btropOperator (:2414-2426) on every block; the caller updates the halo of X first */
void orc_btrop_operator(orc_model *m, const double *X, double *AX) {
  for (int b = 0; b < m->nblocks; b++) btrop_operator(m, b, AX, X);
}
/* POP_SolversRun (:327-417) with the configured solver and the current centre weight: X = first guess in, solution out */
int orc_solver_run(orc_model *m, double *X, const double *B) {
  return (m->c.solver_choice == 2) ? solver_chrongear(m, X, B) : (m->c.solver_choice == 3) ? solver_pcsi(m, X, B) : solver_pcg(m, X, B);
}
/* operators.F90 on whole 2-D fields (all blocks) at level k: op 0 grad (F -> O1,O2 at U points), 1 div, 2 zcurl (A,B -> O1 at T points) */
void orc_operator(orc_model *m, int op, int k, const double *A, const double *B, double *O1, double *O2) {
  const size_t n2 = m->n2;
  for (int b = 0; b < m->nblocks; b++) {
    const size_t o = (size_t)b * n2;
    if (op == 0) op_grad(m, b, k, O1 + o, O2 + o, A + o);
    else if (op == 1) op_div(m, b, k, O1 + o, A + o, B + o);
    else op_zcurl(m, b, k, O1 + o, A + o, B + o);
  }
}
int orc_evp_info(orc_model *m, int what, int idx) {   /* 0: xnb, 1: ynb, 2: xidx[idx], 3: yidx[idx], 4: land flag of sub-block idx */
  const orc_evp *E = (const orc_evp *)m->evp;
  if (!E) return -1;
  return what == 0 ? E->xnb : what == 1 ? E->ynb : what == 2 ? E->xidx[idx] : what == 3 ? E->yidx[idx] : what == 4 ? E->land[idx] : -1;
}
int orc_solver_iterations(orc_model *m) { return m->numIterations; }
double orc_solver_rms(orc_model *m) { return m->rmsResidual; }
