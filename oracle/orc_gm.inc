/* orc_gm.inc -- Gent-McWilliams eddy transport and isopycnal (Redi) diffusion of tracers (hmix_tracer = 3) of the reference,
 * restated for the CPU oracle.  TEST INFRASTRUCTURE ONLY.
 *   init_meso_mixing                  hmix_gm_submeso_share.F90:65-143   HYX, HXY
 *   tracer_diffs_and_isopyc_slopes    hmix_gm_submeso_share.F90:149-432  TX, TY, TZ, RX, RY, SLX, SLY
 *   init_gm                           hmix_gm.F90:283-1095               HYXW, HXYS, RBR, cancellation_occurs, diff_tapering
 *   hdifft_gm                         hmix_gm.F90:1102-2226
 *   hdifft (gm branch)                horizontal_mix.F90:549-554
 * in the set-up the code's own defaults of hmix_gm_nml give (hmix_gm.F90:364-428): kappa_isop_choice = kappa_thic_choice =
 * 'constant' (KAPPA_VERTICAL = 1), kappa_freq_choice = 'never', use_const_ah_bkg_srfbl = .true., ah_bkg_bottom = 0,
 * transition_layer_on = .false., slope_control_choice = 'notanh' or 'tanh'; or with kappa_isop_choice = kappa_thic_choice = 'bfre'
 * (buoyancy_frequency_dependent_profile :3011-3180; kappa_isop_deep = kappa_thic_deep = 0.1, kappa_freq_choice 'never' -- the profile
 * of the first step of the run is kept -- or 'every_time_step').  ah_bolus /= ah or slm_b /= slm_r take the branch without
 * cancellation of the skew-flux terms.  Also: the transition layer (:3183-3848), kappa_freq 'once_a_day', and the bolus velocity of
 * diag_gm_bolus (:2079-2151) as an optional output.  tavg fields are not formed.
 * The reference's module arrays keep their values from step to step; every element that is read is either assigned every step under
 * a mask that does not change (KMT) or never assigned (0 from init), so zeroing the work space each step changes nothing. */
typedef struct {
  double *HYX, *HXY, *HYXW, *HXYS, *RBR;        /* (nx,ny,block) */
  double ah, ah_bolus, ah_bkg_srfbl, slm_r, slm_b;
  int diff_tapering, cancellation_occurs, slope_tanh, bfreq, every_step, tlt_on;
  double *DIABATIC_DEPTH, *THICKNESS, *INTERIOR_DEPTH, *SLA_SAVE;   /* TLT of the block being stepped; SLA_SAVE [2 halves][0..km] */
  int *K_LEVEL, *ZTW;
  double *UIT, *VIT, *WTOP, *WBOT;               /* diag_gm_bolus: carried from level to level */
  double *UISOP, *VISOP, *WISOP;                 /* (nx,ny,km,block): U_ISOP, V_ISOP, WTOP_ISOP of every level */
  double *KAPPA_VERTICAL;                        /* (nx,ny,0..km,block): module state (1 until computed) */
  /* work space of the block being stepped */
  double *SLX, *SLY, *SF_SLX, *SF_SLY;          /* [2 faces][2 halves][0..km] levels of n2 */
  double *TX, *TY, *TZ;                         /* [nt][0..km] */
  double *RX, *RY;                              /* [2 faces][0..km] */
  double *RZ_SAVE;                              /* [0..km]: min(RZ, 0) (hmix_gm_submeso_share.F90:398), read by the submesoscale scheme; levels 0, 1 stay 0 */
  double *KAPPA_ISOP, *KAPPA_THIC, *HOR_DIFF;   /* [2 halves][0..km] */
  double *FZTOP;                                /* [nt] */
  double *BL_DEPTH, *W;                         /* 2-D work */
} orc_gm;
#define GM4(A, n, s, kk) ((A) + (size_t)((((n) * 2 + (s)) * (km + 1)) + (kk)) * n2)   /* n = ieast/jnorth 0, iwest/jsouth 1; s = ktp 0, kbt 1 */
#define GM3(A, s, kk) ((A) + (size_t)(((s) * (km + 1)) + (kk)) * n2)
enum { GM_KTP = 0, GM_KBT = 1, GM_E = 0, GM_W = 1, GM_N = 0, GM_S = 1 };

static void init_gm(orc_model *m) {
  const int nxb = m->nxb, nyb = m->nyb, km = m->km, nt = m->nt;
  const size_t n2 = m->n2, a2 = n2 * m->nblocks;
  const orc_config *c = &m->c;
  orc_gm *G = (orc_gm *)calloc(1, sizeof(orc_gm));
  m->gm = G;
  G->ah = c->ah;
  G->ah_bolus = (c->ah_bolus != 0.0) ? c->ah_bolus : c->ah;
  G->ah_bkg_srfbl = (c->ah_bkg_srfbl != 0.0) ? c->ah_bkg_srfbl : c->ah;
  G->slm_r = (c->slm_r != 0.0) ? c->slm_r : 0.3;
  G->slm_b = (c->slm_b != 0.0) ? c->slm_b : 0.3;
  G->slope_tanh = c->gm_slope_control == 1;
  G->bfreq = c->gm_kappa_type == 1; G->every_step = c->gm_kappa_freq == 1;
  G->tlt_on = c->gm_transition_layer == 1;
  G->diff_tapering = G->slm_r != G->slm_b;                                   /* :964-968 */
  G->cancellation_occurs = !(G->diff_tapering || G->ah != G->ah_bolus);       /* :970-983, both kappa types equal */
  if (c->gm_transition_layer == 1) G->cancellation_occurs = 0;                /* :987 */
  G->HYX = dalloc(a2); G->HXY = dalloc(a2); G->HYXW = dalloc(a2); G->HXYS = dalloc(a2); G->RBR = dalloc(a2);
  for (size_t p = 0; p < a2; p++) {
    G->HYX[p] = m->HTE[p] / m->HUS[p];                                        /* share :131-137 */
    G->HXY[p] = m->HTN[p] / m->HUW[p];
    double r = fabs(m->FCORT[p]) / 200.0;                                     /* :889-894 */
    r = (r < 1.0 / 1.5e+6) ? r : 1.0 / 1.5e+6;
    r = (r > 1.e-7) ? r : 1.e-7;
    G->RBR[p] = r;
  }
  for (int b = 0; b < m->nblocks; b++) {                                      /* eoshift :876-877 */
    const size_t o = (size_t)b * n2;
    for (int j = 1; j <= nyb; j++) for (int i = 1; i <= nxb; i++) {
      const size_t p = o + (size_t)(j - 1) * nxb + (i - 1);
      G->HYXW[p] = (i > 1) ? G->HYX[p - 1] : 0.0;
      G->HXYS[p] = (j > 1) ? G->HXY[p - nxb] : 0.0;
    }
  }
  const size_t lv = (size_t)(km + 1) * n2;
  G->KAPPA_VERTICAL = dalloc(lv * m->nblocks);
  for (size_t p = 0; p < lv * m->nblocks; p++) G->KAPPA_VERTICAL[p] = 1.0;   /* :860 */
  if (c->gm_kappa_type == 2) {   /* kappa_type_depth (:850-874) */
    const double sc = (c->kappa_depth_scale != 0.0) ? c->kappa_depth_scale : 150000.0;
    for (int b = 0; b < m->nblocks; b++) for (int k = 1; k <= km; k++) {
      const double kd = c->kappa_depth_1 + c->kappa_depth_2 * exp(-m->zt[k] / sc);
      for (size_t p = 0; p < n2; p++) G->KAPPA_VERTICAL[(size_t)b * lv + (size_t)k * n2 + p] = kd;
    }
  }
  G->SLX = dalloc(4 * lv); G->SLY = dalloc(4 * lv); G->SF_SLX = dalloc(4 * lv); G->SF_SLY = dalloc(4 * lv);
  G->TX = dalloc(nt * lv); G->TY = dalloc(nt * lv); G->TZ = dalloc(nt * lv);
  G->RX = dalloc(2 * lv); G->RY = dalloc(2 * lv); G->RZ_SAVE = dalloc(lv);
  G->KAPPA_ISOP = dalloc(2 * lv); G->KAPPA_THIC = dalloc(2 * lv); G->HOR_DIFF = dalloc(2 * lv);
  G->DIABATIC_DEPTH = dalloc(n2); G->THICKNESS = dalloc(n2); G->INTERIOR_DEPTH = dalloc(n2); G->SLA_SAVE = dalloc(2 * lv);
  G->K_LEVEL = (int *)calloc(n2, sizeof(int)); G->ZTW = (int *)calloc(n2, sizeof(int));
  if (c->gm_diag_bolus) {
    G->UIT = dalloc(n2); G->VIT = dalloc(n2); G->WTOP = dalloc(n2); G->WBOT = dalloc(n2);
    G->UISOP = dalloc(m->n3 * m->nblocks); G->VISOP = dalloc(m->n3 * m->nblocks); G->WISOP = dalloc(m->n3 * m->nblocks);
  }
  G->FZTOP = dalloc(nt * n2); G->BL_DEPTH = dalloc(n2); G->W = dalloc((size_t)(16 + 2 * nt) * n2);
}
static void free_gm(orc_model *m) {
  orc_gm *G = (orc_gm *)m->gm;
  if (!G) return;
  double *p[] = {G->HYX, G->HXY, G->HYXW, G->HXYS, G->RBR, G->SLX, G->SLY, G->SF_SLX, G->SF_SLY, G->TX, G->TY, G->TZ, G->RX, G->RY, G->RZ_SAVE,
                 G->KAPPA_ISOP, G->KAPPA_THIC, G->HOR_DIFF, G->FZTOP, G->BL_DEPTH, G->W, G->KAPPA_VERTICAL};
  for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); i++) free(p[i]);
  free(G->UIT); free(G->VIT); free(G->WTOP); free(G->WBOT); free(G->UISOP); free(G->VISOP); free(G->WISOP);
  free(G->DIABATIC_DEPTH); free(G->THICKNESS); free(G->INTERIOR_DEPTH); free(G->SLA_SAVE); free(G->K_LEVEL); free(G->ZTW);
  free(G); m->gm = NULL;
}

/* hmix_gm_submeso_share.F90:149-432 */
static void gm_tracer_diffs_and_isopyc_slopes(orc_model *m, int b) {
  DECL_DIMS DECL_BLK
  orc_gm *G = (orc_gm *)m->gm;
  const int nt = m->nt;
  const size_t lv = (size_t)(km + 1) * n2;
  const int *KMT = m->KMT + o2, *KMTE = m->KMTE + o2, *KMTN = m->KMTN + o2;
  const double *T[8];
  for (int n = 0; n < nt; n++) T[n] = m->TRACER[n][m->mixtime] + o3;
#define TM(n, i, j, kk) T[n][P3(i, j, kk)]
  memset(G->SLX, 0, 4 * lv * sizeof(double)); memset(G->SLY, 0, 4 * lv * sizeof(double));
  memset(G->TX, 0, nt * lv * sizeof(double)); memset(G->TY, 0, nt * lv * sizeof(double)); memset(G->TZ, 0, nt * lv * sizeof(double));
  memset(G->RX, 0, 2 * lv * sizeof(double)); memset(G->RY, 0, 2 * lv * sizeof(double));
  double *DRDT = G->W, *DRDS = DRDT + n2, *RZ = DRDS + n2, *KMASK = RZ + n2, *KMASKE = KMASK + n2, *KMASKN = KMASKE + n2, *RHO = KMASKN + n2;
  double *TXP[2] = {RHO + n2, RHO + 2 * n2}, *TYP[2] = {RHO + 3 * n2, RHO + 4 * n2}, *TZP[2] = {RHO + 5 * n2, RHO + 6 * n2}, *TEMP[2] = {RHO + 7 * n2, RHO + 8 * n2};
  for (size_t p = 0; p < n2; p++) { DRDT[p] = DRDS[p] = 0.0; for (int s = 0; s < 2; s++) TXP[s][p] = TYP[s][p] = TZP[s][p] = TEMP[s][p] = 0.0; }
#define TXn(n, kk) (G->TX + (size_t)((n) * (km + 1) + (kk)) * n2)
#define TYn(n, kk) (G->TY + (size_t)((n) * (km + 1) + (kk)) * n2)
#define TZn(n, kk) (G->TZ + (size_t)((n) * (km + 1) + (kk)) * n2)
  int kn = 0, ks = 1;
  /* one level's horizontal differences, expansion coefficients and density differences (:195-262 for kk = 1, :302-353 for kk + 1) */
#define LEVEL_RXRY(kk, sl)                                                                                                                  \
  do {                                                                                                                                        \
    for (int j = 1; j <= nyb; j++) for (int i = 1; i <= nxb - 1; i++)                                                                          \
      TXP[sl][P2(i, j)] = KMASKE[P2(i, j)] * (TEMP[sl][P2(i + 1, j)] - TEMP[sl][P2(i, j)]);                                                    \
    for (int j = 1; j <= nyb - 1; j++) for (int i = 1; i <= nxb; i++)                                                                          \
      TYP[sl][P2(i, j)] = KMASKN[P2(i, j)] * (TEMP[sl][P2(i, j + 1)] - TEMP[sl][P2(i, j)]);                                                    \
    for (int n = 0; n < nt; n++) {                                                                                                            \
      for (int j = 1; j <= nyb; j++) for (int i = 1; i <= nxb - 1; i++)                                                                        \
        TXn(n, kk)[P2(i, j)] = KMASKE[P2(i, j)] * (TM(n, i + 1, j, kk) - TM(n, i, j, kk));                                                     \
      for (int j = 1; j <= nyb - 1; j++) for (int i = 1; i <= nxb; i++)                                                                        \
        TYn(n, kk)[P2(i, j)] = KMASKN[P2(i, j)] * (TM(n, i, j + 1, kk) - TM(n, i, j, kk));                                                     \
    }                                                                                                                                         \
    orc_state(m, kk, kk, T[0] + (size_t)((kk)-1) * n2, T[1] + (size_t)((kk)-1) * n2, RHO, DRDT, DRDS, (int)n2);                                \
    for (size_t p = 0; p < n2; p++) {                                                                                                         \
      GM3(G->RX, GM_E, kk)[p] = DRDT[p] * TXP[sl][p] + DRDS[p] * TXn(1, kk)[p];                                                               \
      GM3(G->RY, GM_N, kk)[p] = DRDT[p] * TYP[sl][p] + DRDS[p] * TYn(1, kk)[p];                                                               \
    }                                                                                                                                         \
    for (int j = 1; j <= nyb; j++) for (int i = 2; i <= nxb; i++)                                                                              \
      GM3(G->RX, GM_W, kk)[P2(i, j)] = DRDT[P2(i, j)] * TXP[sl][P2(i - 1, j)] + DRDS[P2(i, j)] * TXn(1, kk)[P2(i - 1, j)];                     \
    for (int j = 2; j <= nyb; j++) for (int i = 1; i <= nxb; i++)                                                                              \
      GM3(G->RY, GM_S, kk)[P2(i, j)] = DRDT[P2(i, j)] * TYP[sl][P2(i, j - 1)] + DRDS[P2(i, j)] * TYn(1, kk)[P2(i, j - 1)];                     \
  } while (0)
  for (int kk = 1; kk <= km; kk++) {
    for (size_t p = 0; p < n2; p++) KMASK[p] = (kk < KMT[p]) ? 1.0 : 0.0;
    if (kk == 1) {
      for (size_t p = 0; p < n2; p++) {
        KMASKE[p] = (kk <= KMT[p] && kk <= KMTE[p]) ? 1.0 : 0.0;
        KMASKN[p] = (kk <= KMT[p] && kk <= KMTN[p]) ? 1.0 : 0.0;
        TEMP[kn][p] = (T[0][p] > -2.0) ? T[0][p] : -2.0;
      }
      LEVEL_RXRY(1, kn);
    }
    if (kk < km) {
      const double *T1k = T[0] + (size_t)(kk - 1) * n2, *T1kp = T[0] + (size_t)kk * n2;
      const double *T2k = T[1] + (size_t)(kk - 1) * n2, *T2kp = T[1] + (size_t)kk * n2;
      for (size_t p = 0; p < n2; p++) {
        TEMP[ks][p] = (T1kp[p] > -2.0) ? T1kp[p] : -2.0;
        TZn(0, kk + 1)[p] = T1k[p] - T1kp[p];
        TZn(1, kk + 1)[p] = T2k[p] - T2kp[p];
        TZP[ks][p] = TEMP[kn][p] - TEMP[ks][p];
        double rz = DRDT[p] * TZP[ks][p] + DRDS[p] * TZn(1, kk + 1)[p];            /* :283-284 */
        rz = (rz < -1.0e-20) ? rz : -1.0e-20;
        GM4(G->SLX, GM_E, GM_KBT, kk)[p] = KMASK[p] * GM3(G->RX, GM_E, kk)[p] / rz;   /* :286-291 */
        GM4(G->SLX, GM_W, GM_KBT, kk)[p] = KMASK[p] * GM3(G->RX, GM_W, kk)[p] / rz;
        GM4(G->SLY, GM_N, GM_KBT, kk)[p] = KMASK[p] * GM3(G->RY, GM_N, kk)[p] / rz;
        GM4(G->SLY, GM_S, GM_KBT, kk)[p] = KMASK[p] * GM3(G->RY, GM_S, kk)[p] / rz;
        KMASKE[p] = (kk + 1 <= KMT[p] && kk + 1 <= KMTE[p]) ? 1.0 : 0.0;
        KMASKN[p] = (kk + 1 <= KMT[p] && kk + 1 <= KMTN[p]) ? 1.0 : 0.0;
      }
      LEVEL_RXRY(kk + 1, ks);
      for (size_t p = 0; p < n2; p++) {
        double rz = DRDT[p] * TZP[ks][p] + DRDS[p] * TZn(1, kk + 1)[p];            /* :383-385 */
        G->RZ_SAVE[(size_t)(kk + 1) * n2 + p] = (rz < 0.0) ? rz : 0.0;            /* :398 */
        rz = (rz < -1.0e-20) ? rz : -1.0e-20;
        if (kk + 1 <= KMT[p]) {                                                    /* :395-400 */
          GM4(G->SLX, GM_E, GM_KTP, kk + 1)[p] = GM3(G->RX, GM_E, kk + 1)[p] / rz;
          GM4(G->SLX, GM_W, GM_KTP, kk + 1)[p] = GM3(G->RX, GM_W, kk + 1)[p] / rz;
          GM4(G->SLY, GM_N, GM_KTP, kk + 1)[p] = GM3(G->RY, GM_N, kk + 1)[p] / rz;
          GM4(G->SLY, GM_S, GM_KTP, kk + 1)[p] = GM3(G->RY, GM_S, kk + 1)[p] / rz;
        }
      }
    }
    const int kt = kn; kn = ks; ks = kt;
  }
#undef LEVEL_RXRY
#undef TM
}

/* buoyancy_frequency_dependent_profile (:3011-3180), no N^2 data file, no transition layer: KAPPA_VERTICAL of block b */
static void gm_buoyancy_frequency_profile(orc_model *m, int b) {
  DECL_DIMS DECL_BLK
  orc_gm *G = (orc_gm *)m->gm;
  const int *KMT = m->KMT + o2;
  const double *T = m->TRACER[0][m->mixtime] + o3, *S = m->TRACER[1][m->mixtime] + o3;
  double *KV = G->KAPPA_VERTICAL + (size_t)b * (km + 1) * n2;
  double *BFSQ = dalloc((size_t)(km + 1) * n2), *NORM = dalloc((size_t)(km + 1) * n2);   /* zero: the module arrays' initial values where never assigned */
  double *RHOT = G->W, *RHOS = RHOT + n2, *RHO = RHOS + n2, *REF = RHO + n2, *SDL = REF + n2, *TEMP_K = SDL + n2, *TEMP_KP1 = TEMP_K + n2;
  int *K_MIN = (int *)malloc(n2 * sizeof(int));
  for (int k = 0; k <= km; k++) for (size_t p = 0; p < n2; p++) KV[(size_t)k * n2 + p] = 1.0;
  for (size_t p = 0; p < n2; p++) {
    REF[p] = 0.0;
    K_MIN[p] = (KMT[p] != 0) ? km + 1 : 0;
    SDL[p] = (m->c.vmix_choice == 3) ? m->HBLT[o2 + p] : m->zw[1];
    if (G->tlt_on) SDL[p] = G->INTERIOR_DEPTH[p];                          /* :3083 */
  }
  for (int k = 1; k <= km - 1; k++) {
    const double *Tk = T + (size_t)(k - 1) * n2, *Tkp = T + (size_t)k * n2, *Sk = S + (size_t)(k - 1) * n2, *Skp = S + (size_t)k * n2;
    if (k == 1) for (size_t p = 0; p < n2; p++) TEMP_K[p] = (Tk[p] > -2.0) ? Tk[p] : -2.0;
    for (size_t p = 0; p < n2; p++) TEMP_KP1[p] = (Tkp[p] > -2.0) ? Tkp[p] : -2.0;
    orc_state(m, k, k + 1, Tk, Sk, RHO, RHOT, RHOS, (int)n2);
    for (size_t p = 0; p < n2; p++) {
      if (k < KMT[p]) {
        const double v = -(orc_grav * m->dzwr[k] * (RHOT[p] * (TEMP_K[p] - TEMP_KP1[p]) + RHOS[p] * (Sk[p] - Skp[p])));
        BFSQ[(size_t)k * n2 + p] = (v > 0.0) ? v : 0.0;
      }
      TEMP_K[p] = TEMP_KP1[p];
    }
  }
  for (int k = 1; k <= km - 1; k++) for (size_t p = 0; p < n2; p++)
    if (K_MIN[p] == km + 1 && m->zw[k] > SDL[p] && k <= KMT[p] && BFSQ[(size_t)k * n2 + p] > 0.0) { REF[p] = BFSQ[(size_t)k * n2 + p]; K_MIN[p] = k; }
  for (int k = 1; k <= km - 1; k++) for (size_t p = 0; p < n2; p++) {
    double *nr = &NORM[(size_t)k * n2 + p];
    if (k >= K_MIN[p] && k < KMT[p] && REF[p] != 0.0) {
      const double r = BFSQ[(size_t)k * n2 + p] / REF[p];
      *nr = (r > 0.1) ? r : 0.1;
      *nr = (*nr < 1.0) ? *nr : 1.0;
    } else *nr = 1.0;
  }
  for (int k = 1; k <= km - 1; k++) for (size_t p = 0; p < n2; p++)
    if (k == KMT[p] - 1) NORM[(size_t)(k + 1) * n2 + p] = NORM[(size_t)k * n2 + p];
  for (int k = 2; k <= km; k++) for (size_t p = 0; p < n2; p++)
    if (k > K_MIN[p] && k <= KMT[p]) KV[(size_t)k * n2 + p] = NORM[(size_t)(k - 1) * n2 + p];
  free(BFSQ); free(NORM); free(K_MIN);
}

/* smooth_hblt(.false., .true., ...) (vmix_kpp.F90:3699-3881): one pass of the 1-1-4-1-1 filter over HMXL, capped at the depth of the
 * bottom T point; no partial bottom cells */
static void gm_smooth_hmxl(orc_model *m, int b, double *OUT) {
  DECL_DIMS DECL_BLK
  const int *KMT = m->KMT + o2;
  const double *W1 = m->HMXL + o2;
  for (size_t p = 0; p < n2; p++) OUT[p] = W1[p];
  for (int j = 2; j <= nyb - 1; j++) for (int i = 2; i <= nxb - 1; i++) {
    if (KMT[P2(i, j)] == 0) continue;
    double cw = 0.125, ce = 0.125, cn = 0.125, cs = 0.125, cc = 0.5;
    if (KMT[P2(i - 1, j)] == 0) { cc = cc + cw; cw = 0.0; }
    if (KMT[P2(i + 1, j)] == 0) { cc = cc + ce; ce = 0.0; }
    if (KMT[P2(i, j - 1)] == 0) { cc = cc + cs; cs = 0.0; }
    if (KMT[P2(i, j + 1)] == 0) { cc = cc + cn; cn = 0.0; }
    OUT[P2(i, j)] = cw * W1[P2(i - 1, j)] + ce * W1[P2(i + 1, j)] + cs * W1[P2(i, j - 1)] + cn * W1[P2(i, j + 1)] + cc * W1[P2(i, j)];
  }
  for (int k = 1; k <= km; k++) for (int j = 2; j <= nyb - 1; j++) for (int i = 2; i <= nxb - 1; i++)
    if (k == KMT[P2(i, j)] && OUT[P2(i, j)] > m->zt[k]) OUT[P2(i, j)] = m->zt[k];   /* -zgrid(k) = zt(k) */
}

/* transition_layer (hmix_gm.F90:3183-3440) */
static void gm_transition_layer(orc_model *m, int b) {
  DECL_DIMS DECL_BLK
  orc_gm *G = (orc_gm *)m->gm;
  const int *KMT = m->KMT + o2;
  const double *DD = G->DIABATIC_DEPTH, *RBR = G->RBR + o2, *zt = m->zt, *zw = m->zw;
#define SS(s, kk) GM3(G->SLA_SAVE, s, kk)
  for (size_t p = 0; p < n2; p++) {
    int K_START = 0, K_SUB = 0, K_LEVEL = 0, ZTW = 0, COMPUTE = (KMT[p] != 0);
    double THICK = 0.0, INTERIOR = 0.0;
    const double RB = 1.0 / RBR[p];                                       /* :897 */
    for (int k = 1; k <= km; k++) {                                        /* :3252-3281 */
      if (COMPUTE && DD[p] < zw[k]) { K_START = k + 1; K_SUB = 1; THICK = zw[k] - DD[p]; K_LEVEL = k; ZTW = 2; COMPUTE = 0; }
      if (k != 1 && K_START == k + 1 && DD[p] < zt[k]) { K_START = k; K_SUB = 2; THICK = zt[k] - DD[p]; K_LEVEL = k; ZTW = 1; }
    }
    COMPUTE = !(KMT[p] == 0 || K_START > KMT[p] || (K_START == KMT[p] && K_SUB == 2));   /* :3300-3306 */
    for (int k = 1; k <= km - 1; k++) {                                    /* :3308-3334 */
      double WORK = 0.0;
      if (COMPUTE && K_SUB == 2 && K_START < KMT[p] && K_START == k) {
        const double a = SS(GM_KBT, k)[p], c = SS(GM_KTP, k + 1)[p];
        WORK = ((a > c) ? a : c) * RB;
      }
      if (WORK != 0.0 && DD[p] < (zw[k] - WORK)) COMPUTE = 0;
      if (WORK != 0.0 && DD[p] >= (zw[k] - WORK)) { K_START = K_START + 1; K_SUB = 1; THICK = zw[k] - DD[p]; K_LEVEL = k; ZTW = 2; }
    }
    for (int k = 2; k <= km; k++) {                                        /* :3342-3393 */
      const double refd[2] = {zt[k], zw[k]};
      for (int kk = 1; kk <= 2; kk++) {
        double WORK = 0.0;
        if (kk == 1) {
          if (COMPUTE && K_START <= KMT[p] && K_START == k) {
            const double a = SS(GM_KTP, k)[p], c = SS(GM_KBT, k)[p];
            WORK = ((a > c) ? a : c) * RB;
          }
        } else {
          if (k < km && COMPUTE && K_START < KMT[p] && K_START == k) {
            const double a = SS(GM_KBT, k)[p], c = SS(GM_KTP, k + 1)[p];
            WORK = ((a > c) ? a : c) * RB;
          }
          if (COMPUTE && K_START == KMT[p] && K_START == k) WORK = SS(GM_KBT, k)[p] * RB;
        }
        if (WORK != 0.0 && DD[p] < (refd[kk - 1] - WORK)) COMPUTE = 0;
        if (WORK != 0.0 && DD[p] >= (refd[kk - 1] - WORK)) { THICK = refd[kk - 1] - DD[p]; K_LEVEL = k; ZTW = kk; }
      }
      if (COMPUTE && K_START == k) K_START = K_START + 1;
    }
    for (int k = 1; k <= km; k++) {                                        /* :3410-3419 */
      if (K_LEVEL == k && ZTW == 1) INTERIOR = zt[k];
      if (K_LEVEL == k && ZTW == 2) INTERIOR = zw[k];
    }
    G->THICKNESS[p] = THICK; G->INTERIOR_DEPTH[p] = INTERIOR; G->K_LEVEL[p] = K_LEVEL; G->ZTW[p] = ZTW;
  }
#undef SS
}

/* merged_streamfunction (:3441-3743): SF_SLX, SF_SLY of every half cell from the interior streamfunction and its first derivative
 * at the interior depth, linear in the diabatic region, quadratic in the transition layer */
static void gm_merged_streamfunction(orc_model *m, int b) {
  DECL_DIMS DECL_BLK
  orc_gm *G = (orc_gm *)m->gm;
  const int *KMT = m->KMT + o2;
  const double *dz = m->dz, *dzwr = m->dzwr, *zt = m->zt;
  const double eps = 1.0e-10;
  memset(G->SF_SLX, 0, 4 * (size_t)(km + 1) * n2 * sizeof(double)); memset(G->SF_SLY, 0, 4 * (size_t)(km + 1) * n2 * sizeof(double));
#define KT(s, kk) GM3(G->KAPPA_THIC, s, kk)[p]
#define SX(n, s, kk) GM4(G->SLX, n, s, kk)[p]
#define SY(n, s, kk) GM4(G->SLY, n, s, kk)[p]
  for (size_t p = 0; p < n2; p++) {
    double W1[2] = {0, 0}, W2[2] = {0, 0}, W3[2] = {0, 0}, W4[2] = {0, 0};
    double W2N = 0.0, W4N = 0.0;                                           /* WORK2_NEXT, WORK4_NEXT: 2-D arrays that keep their last value */
    const int KL = G->K_LEVEL[p], ZT = G->ZTW[p];
    for (int k = 1; k <= km - 1; k++) for (int n = 0; n < 2; n++) {
      int LM = (KL == k && KL < KMT[p] && ZT == 1);
      if (LM) {
        W1[n] = KT(GM_KBT, k) * SX(n, GM_KBT, k) * dz[k];
        W2[n] = 2.0 * dzwr[k] * (W1[n] - KT(GM_KTP, k + 1) * SX(n, GM_KTP, k + 1) * dz[k + 1]);
        W2N = 2.0 * (KT(GM_KTP, k + 1) * SX(n, GM_KTP, k + 1) - KT(GM_KBT, k + 1) * SX(n, GM_KBT, k + 1));
        W3[n] = KT(GM_KBT, k) * SY(n, GM_KBT, k) * dz[k];
        W4[n] = 2.0 * dzwr[k] * (W3[n] - KT(GM_KTP, k + 1) * SY(n, GM_KTP, k + 1) * dz[k + 1]);
        W4N = 2.0 * (KT(GM_KTP, k + 1) * SY(n, GM_KTP, k + 1) - KT(GM_KBT, k + 1) * SY(n, GM_KBT, k + 1));
      }
      if (LM && fabs(W2N) < fabs(W2[n])) W2[n] = W2N;
      if (LM && fabs(W4N) < fabs(W4[n])) W4[n] = W4N;
      LM = (KL == k && KL < KMT[p] && ZT == 2);
      if (LM) {
        W1[n] = KT(GM_KTP, k + 1) * SX(n, GM_KTP, k + 1);
        W2[n] = 2.0 * (W1[n] - (KT(GM_KBT, k + 1) * SX(n, GM_KBT, k + 1)));
        W1[n] = W1[n] * dz[k + 1];
        W3[n] = KT(GM_KTP, k + 1) * SY(n, GM_KTP, k + 1);
        W4[n] = 2.0 * (W3[n] - (KT(GM_KBT, k + 1) * SY(n, GM_KBT, k + 1)));
        W3[n] = W3[n] * dz[k + 1];
      }
      LM = LM && (KL + 1 < KMT[p]);
      if (k < km - 1 && LM) {
        W2N = 2.0 * dzwr[k + 1] * (KT(GM_KBT, k + 1) * SX(n, GM_KBT, k + 1) * dz[k + 1] - KT(GM_KTP, k + 2) * SX(n, GM_KTP, k + 2) * dz[k + 2]);
        W4N = 2.0 * dzwr[k + 1] * (KT(GM_KBT, k + 1) * SY(n, GM_KBT, k + 1) * dz[k + 1] - KT(GM_KTP, k + 2) * SY(n, GM_KTP, k + 2) * dz[k + 2]);
      }
      if (LM && fabs(W2N) < fabs(W2[n])) W2[n] = W2N;
      if (LM && fabs(W4N) < fabs(W4[n])) W4[n] = W4N;
    }
    const double DD = G->DIABATIC_DEPTH[p], TH = G->THICKNESS[p], ID = G->INTERIOR_DEPTH[p];
    const double W5 = (KMT[p] != 0) ? 1.0 / (2.0 * DD + TH) : 0.0;
    const double W6 = (KMT[p] != 0 && TH > eps) ? W5 / TH : 0.0;
    for (int k = 1; k <= km; k++) {
      const double refd[2] = {zt[k] - 0.25 * dz[k], zt[k] + 0.25 * dz[k]};
      for (int s = 0; s < 2; s++) {
        if (!(k <= KMT[p])) continue;
        const double rd = refd[s];
        if (rd <= DD) {
          for (int n = 0; n < 2; n++) {
            GM4(G->SF_SLX, n, s, k)[p] = rd * W5 * (2.0 * W1[n] + TH * W2[n]);
            GM4(G->SF_SLY, n, s, k)[p] = rd * W5 * (2.0 * W3[n] + TH * W4[n]);
          }
        }
        if (rd > DD && rd <= ID) {
          const double W7 = (DD - rd) * (DD - rd);
          for (int n = 0; n < 2; n++) {
            GM4(G->SF_SLX, n, s, k)[p] = -W7 * W6 * (W1[n] + ID * W2[n]) + rd * W5 * (2.0 * W1[n] + TH * W2[n]);
            GM4(G->SF_SLY, n, s, k)[p] = -W7 * W6 * (W3[n] + ID * W4[n]) + rd * W5 * (2.0 * W3[n] + TH * W4[n]);
          }
        }
        if (rd > ID) {
          for (int n = 0; n < 2; n++) {
            GM4(G->SF_SLX, n, s, k)[p] = KT(s, k) * SX(n, s, k) * dz[k];
            GM4(G->SF_SLY, n, s, k)[p] = KT(s, k) * SY(n, s, k) * dz[k];
          }
        }
      }
    }
  }
#undef KT
#undef SX
#undef SY
}

/* apply_vertical_profile_to_isop_hor_diff (:3745-3846) */
static void gm_apply_vertical_profile(orc_model *m, int b) {
  DECL_DIMS DECL_BLK
  orc_gm *G = (orc_gm *)m->gm;
  const int *KMT = m->KMT + o2;
  const double eps = 1.0e-10;
  for (int k = 1; k <= km; k++) {
    const double refd[2] = {m->zt[k] - 0.25 * m->dz[k], m->zt[k] + 0.25 * m->dz[k]};
    for (int s = 0; s < 2; s++) for (size_t p = 0; p < n2; p++) {
      if (!(k <= KMT[p])) continue;
      const double rd = refd[s], DD = G->DIABATIC_DEPTH[p], TH = G->THICKNESS[p], ID = G->INTERIOR_DEPTH[p];
      if (rd <= DD) GM3(G->KAPPA_ISOP, s, k)[p] = 0.0;
      if (rd > DD && rd <= ID && TH > eps) {
        GM3(G->HOR_DIFF, s, k)[p] = (ID - rd) * GM3(G->HOR_DIFF, s, k)[p] / TH;
        GM3(G->KAPPA_ISOP, s, k)[p] = (rd - DD) * GM3(G->KAPPA_ISOP, s, k)[p] / TH;
      }
      if (rd > ID) GM3(G->HOR_DIFF, s, k)[p] = 0.0;
    }
  }
}

/* the k == 1 part of hdifft_gm (:1192-1706): tapered diffusivities of every level and the thickness-diffusion stream function terms */
static void gm_coefficients(orc_model *m, int b) {
  DECL_DIMS DECL_BLK
  orc_gm *G = (orc_gm *)m->gm;
  const orc_config *c = &m->c;
  const int *KMT = m->KMT + o2;
  const double *DXT = m->DXT + o2, *DYT = m->DYT + o2, *RBR = G->RBR + o2;
  const double eps = 1.0e-10, pi = 3.14159265358979323846;
  double *BL = G->BL_DEPTH, *SLA = G->W, *TAPER1 = SLA + n2, *TAPER2 = TAPER1 + n2, *TAPER3 = TAPER2 + n2;
  for (size_t p = 0; p < n2; p++) BL[p] = (c->vmix_choice == 3) ? m->HBLT[o2 + p] : m->zw[1];   /* :1210-1212 */
  if (G->tlt_on) {   /* :1222-1250 */
    if (c->vmix_choice == 3) gm_smooth_hmxl(m, b, G->DIABATIC_DEPTH);
    else for (size_t p = 0; p < n2; p++) G->DIABATIC_DEPTH[p] = m->zw[1];
    for (int kk = 1; kk <= km; kk++) for (int s = 0; s < 2; s++) {
      const int kid = kk + (s + 1) - 2;
      for (size_t p = 0; p < n2; p++) {
        const double xe = GM4(G->SLX, GM_E, s, kk)[p], xw = GM4(G->SLX, GM_W, s, kk)[p], yn = GM4(G->SLY, GM_N, s, kk)[p], ys = GM4(G->SLY, GM_S, s, kk)[p];
        GM3(G->SLA_SAVE, s, kk)[p] = m->dzw[kid] * sqrt(0.5 * ((xe * xe + xw * xw) / (DXT[p] * DXT[p]) + (yn * yn + ys * ys) / (DYT[p] * DYT[p]))) + eps;
      }
    }
    gm_transition_layer(m, b);
  }
  /* compute_kappa (:1258-1332): the first step of the run, or every step */
  if (G->bfreq && (G->every_step || m->nsteps_total == 1 || (c->gm_kappa_freq == 2 && m->eod_last))) gm_buoyancy_frequency_profile(m, b);
  const double *KV = G->KAPPA_VERTICAL + (size_t)b * (km + 1) * n2;
  for (int s = 0; s < 2; s++) for (int kk = 0; kk <= km; kk++) for (size_t p = 0; p < n2; p++) {
    if (c->gm_kappa_type == 2 && kk >= 1) {   /* :1360-1366, 1375-1381: KAPPA_LATERAL (= ah) | ah_bolus times the depth profile */
      const double kv = KV[(size_t)kk * n2 + p];
      GM3(G->KAPPA_ISOP, s, kk)[p] = G->ah * kv; GM3(G->KAPPA_THIC, s, kk)[p] = G->ah_bolus * kv;
    } else if (G->bfreq && kk >= 1) {   /* :1353-1358, 1382-1387: KAPPA_LATERAL = ah, kappa_isop_deep = kappa_thic_deep = 0.1 */
      const double kv = KV[(size_t)kk * n2 + p], f = (kv > 0.1) ? kv : 0.1;
      GM3(G->KAPPA_ISOP, s, kk)[p] = G->ah * f; GM3(G->KAPPA_THIC, s, kk)[p] = G->ah_bolus * f;
    } else { GM3(G->KAPPA_ISOP, s, kk)[p] = G->ah; GM3(G->KAPPA_THIC, s, kk)[p] = G->ah_bolus; }   /* :1344-1345, 1373-1374 */
    GM3(G->HOR_DIFF, s, kk)[p] = 0.0;
  }
  for (size_t p = 0; p < n2; p++)   /* :1208, and :1369-1370 without use_const_ah_bkg_srfbl: the untapered KAPPA_ISOP */
    GM3(G->HOR_DIFF, GM_KTP, 1)[p] = c->gm_kappa_bkg_srfbl ? GM3(G->KAPPA_ISOP, GM_KTP, 1)[p] : G->ah_bkg_srfbl;
  for (int kk = 1; kk <= km; kk++) {
    const double dz_bottom = (kk == 1) ? 0.0 : m->zt[kk - 1];
    const int kp1 = (kk + 1 < km) ? kk + 1 : km;                                                  /* :1408-1411 */
    const double refdepth[2] = {(kk == km) ? m->zw[kp1] : m->zt[kp1], m->zw[kp1]};
    for (int s = GM_KTP; s <= GM_KBT; s++) {
      const int kid = kk + (s + 1) - 2;                                                           /* kk_sub = s + 1 */
      for (size_t p = 0; p < n2; p++) {
        const double xe = GM4(G->SLX, GM_E, s, kk)[p], xw = GM4(G->SLX, GM_W, s, kk)[p], yn = GM4(G->SLY, GM_N, s, kk)[p], ys = GM4(G->SLY, GM_S, s, kk)[p];
        SLA[p] = m->dzw[kid] * sqrt(0.5 * ((xe * xe + xw * xw) / (DXT[p] * DXT[p]) + (yn * yn + ys * ys) / (DYT[p] * DYT[p]))) + eps;   /* :1431-1436 */
        const double w1r = m->zt[kk] * RBR[p] / SLA[p], W1 = (w1r < 1.0) ? w1r : 1.0;
        double t1 = G->slope_tanh ? 0.5 * (1.0 + sin(pi * (W1 - 0.5))) : (0.5 + 2.0 * (W1 - 0.5) * (1.0 - fabs(W1 - 0.5)));              /* :1450-1465 */
        TAPER1[p] = (dz_bottom <= BL[p]) ? t1 : 1.0;
        if (G->tlt_on) { SLA[p] = GM3(G->SLA_SAVE, s, kk)[p]; TAPER1[p] = 1.0; }                  /* :1428-1429, 1438-1439 */
        double t2 = 1.0, t3 = 1.0;
        if (G->slope_tanh) {                                                                      /* :1490-1506 */
          t2 = (SLA[p] < G->slm_r) ? 0.5 * (1.0 - tanh(10.0 * SLA[p] / G->slm_r - 4.0)) : 0.0;
          t3 = G->diff_tapering ? ((SLA[p] < G->slm_b) ? 0.5 * (1.0 - tanh(10.0 * SLA[p] / G->slm_b - 4.0)) : 0.0) : t2;
        } else if (c->gm_slope_control == 2) {                                                    /* :1541-1573: clip the slopes themselves */
          const double dzwk = m->dzw[kid], dzwrk = m->dzwr[kid], hus = m->HUS[o2 + p], huw = m->HUW[o2 + p];
          for (int n = 0; n < 2; n++) {
            double *sx = &GM4(G->SLX, n, s, kk)[p], *sy = &GM4(G->SLY, n, s, kk)[p];
            if (fabs(*sx * dzwk / hus) > G->slm_r) *sx = copysign(G->slm_r * hus * dzwrk, *sx);
            if (fabs(*sy * dzwk / huw) > G->slm_r) *sy = copysign(G->slm_r * huw * dzwrk, *sy);
          }
        } else if (c->gm_slope_control == 3) {                                                    /* :1575-1594 Gerdes et al. */
          if (SLA[p] > G->slm_r) t2 = (G->slm_r / SLA[p]) * (G->slm_r / SLA[p]);
          if (G->diff_tapering) { if (SLA[p] > G->slm_b) t3 = (G->slm_b / SLA[p]) * (G->slm_b / SLA[p]); } else t3 = t2;
        } else {                                                                                  /* :1508-1539 */
          if (SLA[p] > 0.2 * G->slm_r && SLA[p] < 0.6 * G->slm_r)
            t2 = 0.5 * (1.0 - (2.5 * SLA[p] / G->slm_r - 1.0) * (4.0 - fabs(10.0 * SLA[p] / G->slm_r - 4.0)));
          else if (SLA[p] >= 0.6 * G->slm_r) t2 = 0.0;
          if (G->diff_tapering) {
            if (SLA[p] > 0.2 * G->slm_b && SLA[p] < 0.6 * G->slm_b)
              t3 = 0.5 * (1.0 - (2.5 * SLA[p] / G->slm_b - 1.0) * (4.0 - fabs(10.0 * SLA[p] / G->slm_b - 4.0)));
            else if (SLA[p] >= 0.6 * G->slm_b) t3 = 0.0;
          } else t3 = t2;
        }
        if (G->tlt_on && refdepth[s] <= G->DIABATIC_DEPTH[p]) { t2 = 1.0; t3 = 1.0; }             /* :1591-1596 */
        TAPER2[p] = t2; TAPER3[p] = t3;
        if (G->tlt_on) GM3(G->HOR_DIFF, s, kk)[p] = c->gm_kappa_bkg_srfbl ? GM3(G->KAPPA_ISOP, s, kk)[p] : G->ah_bkg_srfbl;   /* :1598-1608 */
        else if (!(kk == 1 && s == GM_KTP)) {                                                     /* :1615-1631 */
          if (c->gm_kappa_bkg_srfbl) GM3(G->HOR_DIFF, s, kk)[p] = (dz_bottom <= BL[p]) ? GM3(G->KAPPA_ISOP, s, kk)[p] * (1.0 - TAPER1[p] * TAPER2[p]) : 0.0;
          else GM3(G->HOR_DIFF, s, kk)[p] = (dz_bottom <= BL[p]) ? G->ah_bkg_srfbl * (1.0 - TAPER1[p] * TAPER2[p]) * KV[(size_t)kk * n2 + p] : 0.0;
        }
        GM3(G->KAPPA_ISOP, s, kk)[p] = TAPER1[p] * TAPER2[p] * GM3(G->KAPPA_ISOP, s, kk)[p];      /* :1636-1639 */
        GM3(G->KAPPA_THIC, s, kk)[p] = TAPER1[p] * TAPER3[p] * GM3(G->KAPPA_THIC, s, kk)[p];
      }
    }
    for (size_t p = 0; p < n2; p++)
      if (kk == KMT[p]) { GM3(G->KAPPA_ISOP, GM_KBT, kk)[p] = 0.0; GM3(G->KAPPA_THIC, GM_KBT, kk)[p] = 0.0; }   /* :1654-1657 */
  }
  for (size_t p = 0; p < n2; p++) { GM3(G->KAPPA_ISOP, GM_KTP, 1)[p] = 0.0; GM3(G->KAPPA_THIC, GM_KTP, 1)[p] = 0.0; }   /* :1663-1664 */
  for (size_t p = 0; p < n2 * m->nt; p++) G->FZTOP[p] = 0.0;
  if (G->tlt_on) { gm_merged_streamfunction(m, b); gm_apply_vertical_profile(m, b); return; }   /* :1668-1674 */
  memset(G->SF_SLX, 0, 4 * (size_t)(km + 1) * n2 * sizeof(double)); memset(G->SF_SLY, 0, 4 * (size_t)(km + 1) * n2 * sizeof(double));
  for (int kk = 1; kk <= km; kk++) for (int s = 0; s < 2; s++) for (size_t p = 0; p < n2; p++)
    if (kk <= KMT[p]) {                                                                           /* :1680-1700 */
      const double kt = GM3(G->KAPPA_THIC, s, kk)[p];
      GM4(G->SF_SLX, GM_E, s, kk)[p] = kt * GM4(G->SLX, GM_E, s, kk)[p] * m->dz[kk];
      GM4(G->SF_SLX, GM_W, s, kk)[p] = kt * GM4(G->SLX, GM_W, s, kk)[p] * m->dz[kk];
      GM4(G->SF_SLY, GM_N, s, kk)[p] = kt * GM4(G->SLY, GM_N, s, kk)[p] * m->dz[kk];
      GM4(G->SF_SLY, GM_S, s, kk)[p] = kt * GM4(G->SLY, GM_S, s, kk)[p] * m->dz[kk];
    }
}

/* hdifft (horizontal_mix.F90:549-554) + hdifft_gm (hmix_gm.F90:1102-2226) for level k of block b: GTK (n2 * nt), and the
 * isopycnal part of the vertical diffusivity added to VDC(k) */
static void hdifft_gm(orc_model *m, int b, int k, double *GTK) {
  DECL_DIMS DECL_BLK
  orc_gm *G = (orc_gm *)m->gm;
  const orc_config *c = &m->c;
  const int nt = m->nt;
  if (k == 1) { gm_tracer_diffs_and_isopyc_slopes(m, b); gm_coefficients(m, b); }
  const int *KMT = m->KMT + o2, *KMTE = m->KMTE + o2, *KMTN = m->KMTN + o2;
  const double *HYX = G->HYX + o2, *HXY = G->HXY + o2, *HYXW = G->HYXW + o2, *HXYS = G->HXYS + o2, *TAR = m->TAREA_R + o2;
  const double *dz = m->dz;
  double *CX = G->W, *CY = CX + n2, *KMASK = CY + n2, *WORK1 = KMASK + n2, *WORK2 = WORK1 + n2, *WORK3 = WORK2 + n2, *WORK4 = WORK3 + n2;
  double *FX = WORK4 + n2 /* nt */, *FY = FX + (size_t)nt * n2 /* nt */, *W3 = FY + (size_t)nt * n2;
  for (size_t p = 0; p < n2; p++) {
    CX[p] = (k <= KMT[p] && k <= KMTE[p]) ? HYX[p] * 0.25 : 0.0;                                  /* :1217-1220 */
    CY[p] = (k <= KMT[p] && k <= KMTN[p]) ? HXY[p] * 0.25 : 0.0;
    KMASK[p] = (k < KMT[p]) ? 1.0 : 0.0;
    WORK1[p] = WORK2[p] = WORK3[p] = WORK4[p] = 0.0;
  }
#define KI(s, kk) GM3(G->KAPPA_ISOP, s, kk)
#define HD(s, kk) GM3(G->HOR_DIFF, s, kk)
#define SQ(x) ((x) * (x))
  if (k < km) {                                                                                   /* :1725-1748 */
    const int nvdc = (c->vmix_choice == 3) ? 2 : 1;
    for (size_t p = 0; p < n2; p++) {
      const double w = m->dzw[k] * KMASK[p] * TAR[p] *
        (dz[k] * 0.25 * KI(GM_KBT, k)[p] *
           (HYX[p] * SQ(GM4(G->SLX, GM_E, GM_KBT, k)[p]) + HYXW[p] * SQ(GM4(G->SLX, GM_W, GM_KBT, k)[p]) +
            HXY[p] * SQ(GM4(G->SLY, GM_N, GM_KBT, k)[p]) + HXYS[p] * SQ(GM4(G->SLY, GM_S, GM_KBT, k)[p])) +
         dz[k + 1] * 0.25 * KI(GM_KTP, k + 1)[p] *
           (HYX[p] * SQ(GM4(G->SLX, GM_E, GM_KTP, k + 1)[p]) + HYXW[p] * SQ(GM4(G->SLX, GM_W, GM_KTP, k + 1)[p]) +
            HXY[p] * SQ(GM4(G->SLY, GM_N, GM_KTP, k + 1)[p]) + HXYS[p] * SQ(GM4(G->SLY, GM_S, GM_KTP, k + 1)[p])));
      for (int n = 0; n < nvdc; n++) VDCP(n, b)[(size_t)k * n2 + p] = VDCP(n, b)[(size_t)k * n2 + p] + w;
    }
  }
  if (c->ah_bkg_bottom != 0.0)   /* :1757-1761 */
    for (size_t p = 0; p < n2; p++) if (k == KMT[p]) HD(GM_KBT, k)[p] = c->ah_bkg_bottom;
  for (int j = 1; j <= nyb; j++) for (int i = 1; i <= nxb - 1; i++) {                             /* :1769-1780 */
    const size_t p = P2(i, j), q = P2(i + 1, j);
    WORK3[p] = KI(GM_KTP, k)[p] + HD(GM_KTP, k)[p] + KI(GM_KBT, k)[p] + HD(GM_KBT, k)[p] + KI(GM_KTP, k)[q] + HD(GM_KTP, k)[q] + KI(GM_KBT, k)[q] + HD(GM_KBT, k)[q];
  }
  for (int j = 1; j <= nyb - 1; j++) for (int i = 1; i <= nxb; i++) {                             /* :1782-1793 */
    const size_t p = P2(i, j), q = P2(i, j + 1);
    WORK4[p] = KI(GM_KTP, k)[p] + HD(GM_KTP, k)[p] + KI(GM_KBT, k)[p] + HD(GM_KBT, k)[p] + KI(GM_KTP, k)[q] + HD(GM_KTP, k)[q] + KI(GM_KBT, k)[q] + HD(GM_KBT, k)[q];
  }
  const int kp1 = (k == km) ? k : k + 1;
  const double dz_bottom = (k < km) ? dz[kp1] : 0.0, factor = (k < km) ? 1.0 : 0.0;
  for (int n = 0; n < nt; n++) for (size_t p = 0; p < n2; p++) {                                  /* :1827-1828 */
    FX[(size_t)n * n2 + p] = dz[k] * CX[p] * TXn(n, k)[p] * WORK3[p];
    FY[(size_t)n * n2 + p] = dz[k] * CY[p] * TYn(n, k)[p] * WORK4[p];
  }
  if (!G->cancellation_occurs) {                                                                  /* :1832-1898 */
    for (int j = 1; j <= nyb; j++) for (int i = 1; i <= nxb - 1; i++) {
      const size_t p = P2(i, j), q = P2(i + 1, j);
      WORK1[p] = KI(GM_KTP, k)[p] * GM4(G->SLX, GM_E, GM_KTP, k)[p] * dz[k] - GM4(G->SF_SLX, GM_E, GM_KTP, k)[p];
      WORK2[p] = KI(GM_KBT, k)[p] * GM4(G->SLX, GM_E, GM_KBT, k)[p] * dz[k] - GM4(G->SF_SLX, GM_E, GM_KBT, k)[p];
      WORK3[p] = KI(GM_KTP, k)[q] * GM4(G->SLX, GM_W, GM_KTP, k)[q] * dz[k] - GM4(G->SF_SLX, GM_W, GM_KTP, k)[q];
      WORK4[p] = KI(GM_KBT, k)[q] * GM4(G->SLX, GM_W, GM_KBT, k)[q] * dz[k] - GM4(G->SF_SLX, GM_W, GM_KBT, k)[q];
    }
    if (k < km) for (int n = 2; n < nt; n++) {                                                    /* :1851-1852: TZ of the passive tracers is formed here only */
      const double *Tk = m->TRACER[n][m->mixtime] + o3 + (size_t)(k - 1) * n2, *Tkp = Tk + n2;
      for (size_t p = 0; p < n2; p++) TZn(n, k + 1)[p] = Tk[p] - Tkp[p];
    }
    for (int n = 0; n < nt; n++) for (int j = 1; j <= nyb; j++) for (int i = 1; i <= nxb - 1; i++) {
      const size_t p = P2(i, j), q = P2(i + 1, j);
      FX[(size_t)n * n2 + p] = FX[(size_t)n * n2 + p] - CX[p] * (WORK1[p] * TZn(n, k)[p] + WORK2[p] * TZn(n, kp1)[p] + WORK3[p] * TZn(n, k)[q] + WORK4[p] * TZn(n, kp1)[q]);
    }
    for (int j = 1; j <= nyb - 1; j++) for (int i = 1; i <= nxb; i++) {
      const size_t p = P2(i, j), q = P2(i, j + 1);
      WORK1[p] = KI(GM_KTP, k)[p] * GM4(G->SLY, GM_N, GM_KTP, k)[p] * dz[k] - GM4(G->SF_SLY, GM_N, GM_KTP, k)[p];
      WORK2[p] = KI(GM_KBT, k)[p] * GM4(G->SLY, GM_N, GM_KBT, k)[p] * dz[k] - GM4(G->SF_SLY, GM_N, GM_KBT, k)[p];
      WORK3[p] = KI(GM_KTP, k)[q] * GM4(G->SLY, GM_S, GM_KTP, k)[q] * dz[k] - GM4(G->SF_SLY, GM_S, GM_KTP, k)[q];
      WORK4[p] = KI(GM_KBT, k)[q] * GM4(G->SLY, GM_S, GM_KBT, k)[q] * dz[k] - GM4(G->SF_SLY, GM_S, GM_KBT, k)[q];
    }
    for (int n = 0; n < nt; n++) for (int j = 1; j <= nyb - 1; j++) for (int i = 1; i <= nxb; i++) {
      const size_t p = P2(i, j), q = P2(i, j + 1);
      FY[(size_t)n * n2 + p] = FY[(size_t)n * n2 + p] - CY[p] * (WORK1[p] * TZn(n, k)[p] + WORK2[p] * TZn(n, kp1)[p] + WORK3[p] * TZn(n, k)[q] + WORK4[p] * TZn(n, kp1)[q]);
    }
  }
  for (int n = 0; n < nt; n++) {                                                                  /* :1900-2070 */
    double *GT = GTK + (size_t)n * n2, *FZT = G->FZTOP + (size_t)n * n2;
    const double *fx = FX + (size_t)n * n2, *fy = FY + (size_t)n * n2;
    for (size_t p = 0; p < n2; p++) GT[p] = 0.0;
    for (int j = jb; j <= je; j++) for (int i = ib; i <= ie; i++) {
      const size_t p = P2(i, j), pw = P2(i - 1, j), ps = P2(i, j - 1);
      double fz = 0.0;
      if (k < km) {
        /* the four face terms of one half cell: slope * metric * difference, east, north, west, south */
#define FACES(SX, SY, s, kk) (GM4(SX, GM_E, s, kk)[p] * HYX[p] * TXn(n, kk)[p] + GM4(SY, GM_N, s, kk)[p] * HXY[p] * TYn(n, kk)[p] + \
                              GM4(SX, GM_W, s, kk)[p] * HYX[pw] * TXn(n, kk)[pw] + GM4(SY, GM_S, s, kk)[p] * HXY[ps] * TYn(n, kk)[ps])
        double w3;
        if (!G->cancellation_occurs) {                                                            /* :1923-1992 */
          w3 = 0.0;
          w3 = w3 + (dz[k] * KI(GM_KBT, k)[p] * FACES(G->SLX, G->SLY, GM_KBT, k));
          w3 = w3 + FACES(G->SF_SLX, G->SF_SLY, GM_KBT, k);
          w3 = w3 + (dz_bottom * KI(GM_KTP, kp1)[p] * FACES(G->SLX, G->SLY, GM_KTP, kp1));
          w3 = w3 + (factor * FACES(G->SF_SLX, G->SF_SLY, GM_KTP, kp1));
          fz = -KMASK[p] * 0.25 * w3;
        } else {                                                                                  /* :2011-2050 */
          w3 = (dz[k] * KI(GM_KBT, k)[p] * FACES(G->SLX, G->SLY, GM_KBT, k));
          w3 = w3 + (dz_bottom * KI(GM_KTP, kp1)[p] * FACES(G->SLX, G->SLY, GM_KTP, kp1));
          fz = -KMASK[p] * 0.5 * w3;
        }
#undef FACES
        GT[p] = (fx[p] - fx[pw] + fy[p] - fy[ps] + FZT[p] - fz) * m->dzr[k] * TAR[p];
        FZT[p] = fz;
      } else {                                                                                    /* :2056-2066 */
        GT[p] = (fx[p] - fx[pw] + fy[p] - fy[ps] + FZT[p]) * m->dzr[k] * TAR[p];
        FZT[p] = 0.0;
      }
    }
  }
  if (c->gm_diag_bolus) {   /* :2079-2151: the eddy-induced velocity from the thickness-diffusion stream function */
    double *UIB = WORK3, *VIB = WORK4;
    if (k == 1) for (size_t p = 0; p < n2; p++) { G->UIT[p] = 0.0; G->VIT[p] = 0.0; G->WBOT[p] = 0.0; }
    for (size_t p = 0; p < n2; p++) { G->WTOP[p] = G->WBOT[p]; WORK1[p] = 0.0; WORK2[p] = 0.0; }   /* (the reference leaves stale work values in the last column / row) */
    for (int j = 1; j <= nyb - 1; j++) for (int i = 1; i <= nxb - 1; i++) {
      const size_t p = P2(i, j), pe = P2(i + 1, j), pn = P2(i, j + 1);
      WORK1[p] = (GM4(G->SF_SLX, GM_E, GM_KBT, k)[p] + factor * GM4(G->SF_SLX, GM_E, GM_KTP, kp1)[p] +
                  GM4(G->SF_SLX, GM_W, GM_KBT, k)[pe] + factor * GM4(G->SF_SLX, GM_W, GM_KTP, kp1)[pe]) * 0.25 * HYX[p];
      WORK2[p] = (GM4(G->SF_SLY, GM_N, GM_KBT, k)[p] + factor * GM4(G->SF_SLY, GM_N, GM_KTP, kp1)[p] +
                  GM4(G->SF_SLY, GM_S, GM_KBT, k)[pn] + factor * GM4(G->SF_SLY, GM_S, GM_KTP, kp1)[pn]) * 0.25 * HXY[p];
    }
    double *UO = G->UISOP + o3 + (size_t)(k - 1) * n2, *VO = G->VISOP + o3 + (size_t)(k - 1) * n2, *WO = G->WISOP + o3 + (size_t)(k - 1) * n2;
    for (size_t p = 0; p < n2; p++) {
      UIB[p] = (k < KMT[p] && k < KMTE[p]) ? WORK1[p] : 0.0;
      VIB[p] = (k < KMT[p] && k < KMTN[p]) ? WORK2[p] : 0.0;
      WORK1[p] = (k <= KMT[p] && k <= KMTE[p]) ? G->UIT[p] - UIB[p] : 0.0;
      WORK2[p] = (k <= KMT[p] && k <= KMTN[p]) ? G->VIT[p] - VIB[p] : 0.0;
      UO[p] = WORK1[p] * m->dzr[k] / m->HTE[o2 + p];
      VO[p] = WORK2[p] * m->dzr[k] / m->HTN[o2 + p];
      WO[p] = G->WTOP[p];
    }
    for (int j = jb; j <= je; j++) for (int i = ib; i <= ie; i++) {
      const size_t p = P2(i, j);
      G->WBOT[p] = (k < KMT[p]) ? G->WTOP[p] + TAR[p] * (WORK1[p] - WORK1[P2(i - 1, j)] + WORK2[p] - WORK2[P2(i, j - 1)]) : 0.0;
    }
    for (size_t p = 0; p < n2; p++) { G->UIT[p] = UIB[p]; G->VIT[p] = VIB[p]; }
  }
  (void)W3;
#undef KI
#undef HD
#undef SQ
}
#undef TXn
#undef TYn
#undef TZn
static double *orc_gm_field(orc_model *m, const char *name, int n) {
  orc_gm *G = (orc_gm *)m->gm;
  const int km = m->km; const size_t n2 = m->n2;
  /* work arrays of the block stepped last: meaningful for one-block configurations (the pins of tests/pins.py); levels 1 .. km */
  if (!strcmp(name, "GM_SF_SLX")) return (m->nblocks == 1 && n >= 0 && n < 4) ? GM4(G->SF_SLX, n / 2, n % 2, 1) : NULL;   /* n = 2 face + half */
  if (!strcmp(name, "GM_SF_SLY")) return (m->nblocks == 1 && n >= 0 && n < 4) ? GM4(G->SF_SLY, n / 2, n % 2, 1) : NULL;
  if (!strcmp(name, "TLT_DIABATIC_DEPTH")) return m->nblocks == 1 ? G->DIABATIC_DEPTH : NULL;
  if (!strcmp(name, "TLT_THICKNESS")) return m->nblocks == 1 ? G->THICKNESS : NULL;
  if (!strcmp(name, "TLT_INTERIOR_DEPTH")) return m->nblocks == 1 ? G->INTERIOR_DEPTH : NULL;
  return !strcmp(name, "UISOP") ? G->UISOP : !strcmp(name, "VISOP") ? G->VISOP : G->WISOP;
}
