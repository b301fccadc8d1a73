/* orc_submeso.inc -- the submesoscale mixed-layer eddy scheme of Fox-Kemper, Ferrari and Hallberg (source/mix_submeso.F90,
 * lsubmesoscale_mixing of hmix_nml) restated for the CPU oracle.  TEST INFRASTRUCTURE ONLY.
 *
 * With hmix_tracer = 3 only (del2 / del4 and partial bottom cells are refused by orc_create, as on the device): the tracer
 * differences TX, TY, TZ and the density differences RX, RY, RZ_SAVE are the ones tracer_diffs_and_isopyc_slopes has just formed
 * for Gent-McWilliams (orc_gm.inc).  The diagnostic velocities USUBM, VSUBM, WSUBM (mix_submeso.F90:599-661) and the tavg fluxes are
 * not formed: nothing on the path reads them.  Integer powers: x**2 = x*x.
 */
typedef struct {
  double efficiency_factor, time_scale_constant, hor_length_scale, max_hor_grid_scale;
  double *TIME_SCALE, *ML_DEPTH, *HLS;     /* (nx,ny,blocks) */
  double *SF_SUBM_X, *SF_SUBM_Y;           /* [2 faces][2 halves][0..km] levels of n2, of the block being stepped (GM4 indexing) */
  double *FZTOP_SUBM, *TDTK;               /* [nt] levels of n2 */
  double *TEND[2];                         /* SUBM_ADV_TEND of T and S, (nx,ny,km,blocks) */
} orc_submeso;

/* init_submeso (mix_submeso.F90:140-334) */
static void init_submeso(orc_model *m) {
  DECL_DIMS
  const orc_config *c = &m->c;
  const size_t a2 = n2 * m->nblocks, lv = (size_t)(km + 1) * n2;
  orc_submeso *S = (orc_submeso *)calloc(1, sizeof(orc_submeso));
  m->submeso = S;
  S->efficiency_factor = c->efficiency_factor != 0.0 ? c->efficiency_factor : 0.07;          /* :183-186 */
  S->time_scale_constant = c->time_scale_constant != 0.0 ? c->time_scale_constant : 3.456e5;
  S->hor_length_scale = c->hor_length_scale != 0.0 ? c->hor_length_scale : 5.0e5;
  S->max_hor_grid_scale = 111.0e5;
  S->TIME_SCALE = dalloc(a2); S->ML_DEPTH = dalloc(a2); S->HLS = dalloc(a2);
  S->SF_SUBM_X = dalloc(4 * lv); S->SF_SUBM_Y = dalloc(4 * lv);
  S->FZTOP_SUBM = dalloc((size_t)m->nt * n2); S->TDTK = dalloc((size_t)m->nt * n2);
  S->TEND[0] = dalloc(n3 * m->nblocks); S->TEND[1] = dalloc(n3 * m->nblocks);
  for (size_t p = 0; p < a2; p++)   /* :266-269 */
    S->TIME_SCALE[p] = 1.0 / sqrt(m->FCORT[p] * m->FCORT[p] + 1.0 / (S->time_scale_constant * S->time_scale_constant));
}
static void free_submeso(orc_model *m) {
  orc_submeso *S = (orc_submeso *)m->submeso;
  if (!S) return;
  double *p[] = {S->TIME_SCALE, S->ML_DEPTH, S->HLS, S->SF_SUBM_X, S->SF_SUBM_Y, S->FZTOP_SUBM, S->TDTK, S->TEND[0], S->TEND[1]};
  for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); i++) free(p[i]);
  free(S); m->submeso = NULL;
}

/* submeso_sf (mix_submeso.F90:341-597) for block b: the stream function from the mixtime density differences and this step's HMXL */
static void submeso_sf(orc_model *m, int b) {
  DECL_DIMS DECL_BLK
  orc_submeso *S = (orc_submeso *)m->submeso;
  const orc_gm *G = (const orc_gm *)m->gm;
  const int *KMT = m->KMT + o2;
  const double *DXT = m->DXT + o2, *DYT = m->DYT + o2, *TIME_SCALE = S->TIME_SCALE + o2;
  const double *zw = m->zw, *zt = m->zt, *dz = m->dz;
  const double sqrt_grav = sqrt(orc_grav);
  double *ML_DEPTH = S->ML_DEPTH + o2, *HLS = S->HLS + o2;
  double *W = dalloc(7 * n2), *WORK1 = W, *WORK2 = W + n2, *WORK3 = W + 2 * n2;
  double *BX1 = W + 3 * n2, *BX2 = W + 4 * n2, *BY1 = W + 5 * n2, *BY2 = W + 6 * n2;   /* BX_VERT_AVG(:,:,1:2), BY_VERT_AVG(:,:,1:2) */
  int *CONTINUE_INTEGRAL = ialloc(n2);
  memset(S->SF_SUBM_X, 0, 4 * (size_t)(km + 1) * n2 * sizeof(double));
  memset(S->SF_SUBM_Y, 0, 4 * (size_t)(km + 1) * n2 * sizeof(double));
  for (size_t p = 0; p < n2; p++) {
    HLS[p] = 0.0;
    ML_DEPTH[p] = zw[1];
    if (m->c.vmix_choice == 3) ML_DEPTH[p] = m->HMXL[o2 + p];   /* :424-426 */
    CONTINUE_INTEGRAL[p] = (KMT[p] == 0) ? 0 : 1;
  }
  /* vertical averages of the horizontal buoyancy differences within the mixed layer :441-484 */
  for (int k = 1; k <= km; k++) {
    double zw_top = 0.0;
    if (k > 1) zw_top = zw[k - 1];
    for (size_t p = 0; p < n2; p++) {
      WORK3[p] = 0.0;
      if (CONTINUE_INTEGRAL[p] && ML_DEPTH[p] > zw[k]) WORK3[p] = dz[k];
      if (CONTINUE_INTEGRAL[p] && ML_DEPTH[p] <= zw[k] && ML_DEPTH[p] > zw_top) WORK3[p] = ML_DEPTH[p] - zw_top;
      if (CONTINUE_INTEGRAL[p]) {
        BX1[p] = BX1[p] + GM3(G->RX, GM_E, k)[p] * WORK3[p];
        BX2[p] = BX2[p] + GM3(G->RX, GM_W, k)[p] * WORK3[p];
        BY1[p] = BY1[p] + GM3(G->RY, GM_N, k)[p] * WORK3[p];
        BY2[p] = BY2[p] + GM3(G->RY, GM_S, k)[p] * WORK3[p];
      }
      if (CONTINUE_INTEGRAL[p] && ML_DEPTH[p] <= zw[k] && ML_DEPTH[p] > zw_top) CONTINUE_INTEGRAL[p] = 0;
    }
  }
  for (size_t p = 0; p < n2; p++)
    if (KMT[p] > 0) {
      BX1[p] = -orc_grav * BX1[p] / ML_DEPTH[p]; BX2[p] = -orc_grav * BX2[p] / ML_DEPTH[p];
      BY1[p] = -orc_grav * BY1[p] / ML_DEPTH[p]; BY2[p] = -orc_grav * BY2[p] / ML_DEPTH[p];
    }
  /* horizontal length scale :492-554 */
  if (m->c.luse_const_horiz_len_scale) {
    for (size_t p = 0; p < n2; p++) if (KMT[p] > 0) HLS[p] = S->hor_length_scale;
  } else {
    for (size_t p = 0; p < n2; p++) {
      WORK1[p] = 0.0;
      if (KMT[p] > 0) {
        WORK1[p] = sqrt(0.5 * ((BX1[p] * BX1[p] + BX2[p] * BX2[p]) / (DXT[p] * DXT[p]) + (BY1[p] * BY1[p] + BY2[p] * BY2[p]) / (DYT[p] * DYT[p])));
        WORK1[p] = WORK1[p] * ML_DEPTH[p] * (TIME_SCALE[p] * TIME_SCALE[p]);
      }
      CONTINUE_INTEGRAL[p] = (KMT[p] == 0) ? 0 : 1;
      WORK2[p] = 0.0;
    }
    for (int k = 2; k <= km; k++) {
      const double *RZ_SAVE = G->RZ_SAVE + (size_t)k * n2;
      for (size_t p = 0; p < n2; p++) {
        WORK3[p] = 0.0;
        if (CONTINUE_INTEGRAL[p] && ML_DEPTH[p] > zt[k]) WORK3[p] = m->dzw[k - 1];
        if (CONTINUE_INTEGRAL[p] && ML_DEPTH[p] <= zt[k] && ML_DEPTH[p] >= zt[k - 1])
          WORK3[p] = ((ML_DEPTH[p] - zt[k - 1]) * (ML_DEPTH[p] - zt[k - 1])) * m->dzwr[k - 1];
        if (CONTINUE_INTEGRAL[p]) WORK2[p] = WORK2[p] + sqrt(-RZ_SAVE[p] * WORK3[p]);
        if (CONTINUE_INTEGRAL[p] && ML_DEPTH[p] <= zt[k] && ML_DEPTH[p] >= zt[k - 1]) CONTINUE_INTEGRAL[p] = 0;
      }
    }
    for (size_t p = 0; p < n2; p++)
      if (KMT[p] > 0) {
        WORK2[p] = sqrt_grav * WORK2[p] * TIME_SCALE[p];
        double h = WORK1[p] > WORK2[p] ? WORK1[p] : WORK2[p];
        HLS[p] = h > S->hor_length_scale ? h : S->hor_length_scale;
      }
  }
  /* the stream function :562-597 */
  for (int k = 1; k <= km; k++) {
    const double reference_depth[2] = {zt[k] - 0.25 * dz[k], zt[k] + 0.25 * dz[k]};
    for (int kk = GM_KTP; kk <= GM_KBT; kk++)
      for (size_t p = 0; p < n2; p++)
        if (reference_depth[kk] < ML_DEPTH[p] && KMT[p] >= k) {
          const double r = 1.0 - (2.0 * reference_depth[kk] / ML_DEPTH[p]);
          const double w3 = r * r;
          const double w2 = (1.0 - w3) * (1.0 + (5.0 / 21.0) * w3);
          const double w1 = S->efficiency_factor * (ML_DEPTH[p] * ML_DEPTH[p]) * w2 * TIME_SCALE[p] / HLS[p];
          const double dx = DXT[p] < S->max_hor_grid_scale ? DXT[p] : S->max_hor_grid_scale;
          const double dy = DYT[p] < S->max_hor_grid_scale ? DYT[p] : S->max_hor_grid_scale;
          GM4(S->SF_SUBM_X, GM_E, kk, k)[p] = w1 * BX1[p] * dx;
          GM4(S->SF_SUBM_X, GM_W, kk, k)[p] = w1 * BX2[p] * dx;
          GM4(S->SF_SUBM_Y, GM_N, kk, k)[p] = w1 * BY1[p] * dy;
          GM4(S->SF_SUBM_Y, GM_S, kk, k)[p] = w1 * BY2[p] * dy;
        }
  }
  free(W); free(CONTINUE_INTEGRAL);
}

/* submeso_flux (mix_submeso.F90:779-1008) at level k of block b: GTK (n2 * nt) */
static void submeso_flux(orc_model *m, int b, int k, double *GTK) {
  DECL_DIMS DECL_BLK
  orc_submeso *S = (orc_submeso *)m->submeso;
  const orc_gm *G = (const orc_gm *)m->gm;
  const int nt = m->nt;
  const int *KMT = m->KMT + o2, *KMTE = m->KMTE + o2, *KMTN = m->KMTN + o2;
  const double *HYX = G->HYX + o2, *HXY = G->HXY + o2, *TAREA_R = m->TAREA_R + o2;
  double *W = dalloc((size_t)(5 + 2 * nt) * n2), *CX = W, *CY = W + n2, *KMASK = W + 2 * n2, *WORK1 = W + 3 * n2, *WORK2 = W + 4 * n2;
  double *FX = W + 5 * n2, *FY = FX + (size_t)nt * n2;
#define SX(f, s, kk) GM4(S->SF_SUBM_X, f, s, kk)
#define SY(f, s, kk) GM4(S->SF_SUBM_Y, f, s, kk)
#define TXs(n, kk) (G->TX + (size_t)((n) * (km + 1) + (kk)) * n2)
#define TYs(n, kk) (G->TY + (size_t)((n) * (km + 1) + (kk)) * n2)
#define TZs(n, kk) (G->TZ + (size_t)((n) * (km + 1) + (kk)) * n2)
  if (k == 1) for (size_t p = 0; p < (size_t)nt * n2; p++) S->FZTOP_SUBM[p] = 0.0;
  for (size_t p = 0; p < n2; p++) {
    CX[p] = (k <= KMT[p] && k <= KMTE[p]) ? HYX[p] * 0.25 : 0.0;
    CY[p] = (k <= KMT[p] && k <= KMTN[p]) ? HXY[p] * 0.25 : 0.0;
    KMASK[p] = (k < KMT[p]) ? 1.0 : 0.0;
  }
  int kp1 = k + 1;
  if (k == km) kp1 = k;
  const double factor = (k < km) ? 1.0 : 0.0;
  for (int n = 0; n < nt; n++) {
    double *fx = FX + (size_t)n * n2, *fy = FY + (size_t)n * n2;
    const double *TZk = TZs(n, k), *TZkp = TZs(n, kp1);
    for (int j = 1; j <= nyb; j++) for (int i = 1; i <= nxb - 1; i++) {
      const size_t p = P2(i, j), pe = P2(i + 1, j);
      fx[p] = CX[p] * (SX(GM_E, GM_KTP, k)[p] * TZk[p] + SX(GM_E, GM_KBT, k)[p] * TZkp[p] + SX(GM_W, GM_KTP, k)[pe] * TZk[pe] + SX(GM_W, GM_KBT, k)[pe] * TZkp[pe]);
    }
    for (int j = 1; j <= nyb - 1; j++) for (int i = 1; i <= nxb; i++) {
      const size_t p = P2(i, j), pn = P2(i, j + 1);
      fy[p] = CY[p] * (SY(GM_N, GM_KTP, k)[p] * TZk[p] + SY(GM_N, GM_KBT, k)[p] * TZkp[p] + SY(GM_S, GM_KTP, k)[pn] * TZk[pn] + SY(GM_S, GM_KBT, k)[pn] * TZkp[pn]);
    }
  }
  for (size_t p = 0; p < n2; p++) { WORK1[p] = 0.0; WORK2[p] = 0.0; }
  for (int n = 0; n < nt; n++) {
    double *GT = GTK + (size_t)n * n2, *FZT = S->FZTOP_SUBM + (size_t)n * n2;
    const double *fx = FX + (size_t)n * n2, *fy = FY + (size_t)n * n2;
    for (size_t p = 0; p < n2; p++) GT[p] = 0.0;
    if (k < km) {
      for (int j = jb; j <= je; j++) for (int i = ib; i <= ie; i++) {
        const size_t p = P2(i, j), pw = P2(i - 1, j), ps = P2(i, j - 1);
        WORK1[p] = SX(GM_E, GM_KBT, k)[p] * HYX[p] * TXs(n, k)[p] + SY(GM_N, GM_KBT, k)[p] * HXY[p] * TYs(n, k)[p] +
                   SX(GM_W, GM_KBT, k)[p] * HYX[pw] * TXs(n, k)[pw] + SY(GM_S, GM_KBT, k)[p] * HXY[ps] * TYs(n, k)[ps];
        WORK2[p] = factor * (SX(GM_E, GM_KTP, kp1)[p] * HYX[p] * TXs(n, kp1)[p] + SY(GM_N, GM_KTP, kp1)[p] * HXY[p] * TYs(n, kp1)[p] +
                             SX(GM_W, GM_KTP, kp1)[p] * HYX[pw] * TXs(n, kp1)[pw] + SY(GM_S, GM_KTP, kp1)[p] * HXY[ps] * TYs(n, kp1)[ps]);
      }
      for (int j = jb; j <= je; j++) for (int i = ib; i <= ie; i++) {
        const size_t p = P2(i, j);
        const double fz = -KMASK[p] * 0.25 * (WORK1[p] + WORK2[p]);
        GT[p] = (fx[p] - fx[P2(i - 1, j)] + fy[p] - fy[P2(i, j - 1)] + FZT[p] - fz) * m->dzr[k] * TAREA_R[p];
        FZT[p] = fz;
      }
    } else {
      for (int j = jb; j <= je; j++) for (int i = ib; i <= ie; i++) {
        const size_t p = P2(i, j);
        GT[p] = (fx[p] - fx[P2(i - 1, j)] + fy[p] - fy[P2(i, j - 1)] + FZT[p]) * m->dzr[k] * TAREA_R[p];
        FZT[p] = 0.0;
      }
    }
    if (n < 2) memcpy(S->TEND[n] + o3 + (size_t)(k - 1) * n2, GT, n2 * sizeof(double));   /* tavg SUBM_ADV_TEND_<tracer> :994 */
  }
#undef SX
#undef SY
#undef TXs
#undef TYs
#undef TZs
  free(W);
}
static double *orc_submeso_field(orc_model *m, const char *name, int n) {
  const orc_submeso *S = (const orc_submeso *)m->submeso;
  if (!strcmp(name, "SUBM_ML_DEPTH")) return S->ML_DEPTH;
  if (!strcmp(name, "HLS_SUBM")) return S->HLS;
  if (!strcmp(name, "SUBM_TIME_SCALE")) return S->TIME_SCALE;
  if (!strcmp(name, "SUBM_ADV_TEND")) return (n == 0 || n == 1) ? S->TEND[n] : NULL;
  return NULL;
}
