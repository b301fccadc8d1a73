/* orc_aniso.inc -- anisotropic horizontal viscosity (hmix_momentum_choice 'anis', source/hmix_aniso.F90) restated for the CPU
 * oracle.  TEST INFRASTRUCTURE ONLY.
 *
 * Selections: hmix_alignment_choice 'grid' | 'east' ('flow' is refused, as on the device); constant viscosities or the
 * 'ccsm-internal' variable ones (compute_ccsm_var_viscosity) with the AMAX_CFL taper of init_aniso; partial bottom cells.
 * Not restated, refused by orc_create: lsmag_aniso (the Smagorinsky viscosities, hmix_aniso.F90:807-856, 510-533).
 * Integer powers: x**2 = x*x, x**3 = (x*x)*x.
 */
typedef struct {
  double *H1E, *H1W, *H2N, *H2S, *K1E, *K1W, *K2N, *K2S, *AMAX_CFL;   /* (nx,ny,blocks) */
  double *F_PARA, *F_PERP;                                             /* (nx,ny,km,blocks); NULL without lvariable_hmix_aniso */
  double *HDU, *HDV;                                                   /* the friction of the last clinic, (nx,ny,km,blocks) */
} orc_aniso;

/* compute_ccsm_var_viscosity (hmix_aniso.F90:1069-1296) */
static void compute_ccsm_var_viscosity(orc_model *m, orc_aniso *A) {
  DECL_DIMS
  const orc_config *c = &m->c;
  const int nxg = c->nx_global, nyg = c->ny_global;
  const double pi = 4.0 * atan(1.0), radian = 180.0 / pi, dist_max = 1.e10;
  const double vconst_1 = c->vconst_1 != 0.0 ? c->vconst_1 : 1.e7, vconst_2 = c->vconst_2 != 0.0 ? c->vconst_2 : 24.5;
  const double vconst_3 = c->vconst_3 != 0.0 ? c->vconst_3 : 0.2, vconst_4 = c->vconst_4 != 0.0 ? c->vconst_4 : 1.e-8;
  const int vconst_5 = c->vconst_5 != 0 ? c->vconst_5 : 3;
  const double vconst_6 = c->vconst_6 != 0.0 ? c->vconst_6 : 1.e7, vconst_7 = c->vconst_7 != 0.0 ? c->vconst_7 : 45.0;
  const size_t ng = (size_t)nxg * nyg;
  double *HTN_G = dalloc(ng), *DIST_G = dalloc(ng), *DIST = dalloc(n2 * m->nblocks), *BETA_F = dalloc(n2 * m->nblocks);
  int *KMU_G = ialloc(ng), *NWBP_G = ialloc(ng), *iwp = ialloc(nxg + 1);
#define G2(A, ig, jg) (A)[(size_t)((jg)-1) * nxg + (ig)-1]
  for (size_t p = 0; p < n2 * m->nblocks; p++) BETA_F[p] = 2.0 * orc_omega * cos(m->ULAT[p]) / orc_radius;
  /* gather_global: the physical cells of every block */
  for (int b = 0; b < m->nblocks; b++) {
    DECL_BLK
    const int *ig = m->i_glob + (size_t)b * nxb, *jg = m->j_glob + (size_t)b * nyb;
    for (int j = jb; j <= je; j++) for (int i = ib; i <= ie; i++)
      if (ig[i - 1] > 0 && jg[j - 1] > 0) {
        G2(HTN_G, ig[i - 1], jg[j - 1]) = m->HTN[o2 + P2(i, j)];
        G2(KMU_G, ig[i - 1], jg[j - 1]) = m->KMU[o2 + P2(i, j)];
      }
  }
  for (int k = 1; k <= km; k++) {
    for (size_t p = 0; p < ng; p++) NWBP_G[p] = 0;
    for (int jg = 1; jg <= nyg; jg++) {   /* nearest western boundary :1173-1200 */
      int ncount = 0;
      for (int ig = 1; ig <= nxg; ig++) {
        int igp1 = ig + 1;
        if (ig == nxg) igp1 = 1;
        if (G2(KMU_G, ig, jg) < k && G2(KMU_G, igp1, jg) >= k) { ncount = ncount + 1; iwp[ncount] = ig; }
      }
      if (ncount > 0) {
        for (int n = 1; n <= ncount - 1; n++) {
          const int is = iwp[n], ie_ = iwp[n + 1] - 1;
          for (int ig = is; ig <= ie_; ig++) G2(NWBP_G, ig, jg) = is;
        }
        for (int ig = 1; ig <= nxg; ig++) if (G2(NWBP_G, ig, jg) == 0) G2(NWBP_G, ig, jg) = iwp[ncount];
      }
    }
    for (int jg = 1; jg <= nyg; jg++)   /* distance to it :1207-1240 */
      for (int ig = 1; ig <= nxg; ig++) {
        const int index = G2(NWBP_G, ig, jg), indexo = index + vconst_5;
        if (index == 0) G2(DIST_G, ig, jg) = dist_max;
        else if (ig >= index && ig <= indexo) G2(DIST_G, ig, jg) = 0.0;
        else if (ig > indexo) G2(DIST_G, ig, jg) = G2(HTN_G, ig, jg) + G2(DIST_G, ig - 1, jg);
        else if (ig < index) {
          if (indexo <= nxg) {
            if (ig == 1) {
              G2(DIST_G, ig, jg) = 0.0;
              for (int ii = indexo + 1; ii <= nxg; ii++) G2(DIST_G, ig, jg) = G2(HTN_G, ii, jg) + G2(DIST_G, ig, jg);
              G2(DIST_G, ig, jg) = G2(HTN_G, ig, jg) + G2(DIST_G, ig, jg);
            } else G2(DIST_G, ig, jg) = G2(HTN_G, ig, jg) + G2(DIST_G, ig - 1, jg);
          } else {
            if (ig <= indexo - nxg) G2(DIST_G, ig, jg) = 0.0;
            else G2(DIST_G, ig, jg) = G2(HTN_G, ig, jg) + G2(DIST_G, ig - 1, jg);
          }
        }
      }
    scatter_global_r8(m, DIST, DIST_G, ORC_NECORNER);
    for (int b = 0; b < m->nblocks; b++) {
      DECL_BLK
      for (size_t p = 0; p < n2; p++) {   /* :1273-1283 */
        const double alat = fabs(m->ULAT[o2 + p] * radian);
        double bv = ((alat < vconst_7 ? alat : vconst_7) * 90.0 / vconst_7) / radian;
        const double bu = vconst_1 * (1.0 + vconst_2 * (1.0 - cos(2.0 * bv)));
        const double dxu = m->DXU[o2 + p], vd = vconst_4 * DIST[o2 + p];
        bv = vconst_3 * BETA_F[o2 + p] * ((dxu * dxu) * dxu);
        bv = bv * exp(-(vd * vd));
        A->F_PERP[o3 + (size_t)(k - 1) * n2 + p] = bu > bv ? bu : bv;
        A->F_PARA[o3 + (size_t)(k - 1) * n2 + p] = bv > vconst_6 ? bv : vconst_6;
      }
    }
  }
#undef G2
  free(HTN_G); free(DIST_G); free(DIST); free(BETA_F); free(KMU_G); free(NWBP_G); free(iwp);
}

/* init_aniso (hmix_aniso.F90:372-393, 408-464); after init_time (dtu) */
static void init_aniso(orc_model *m) {
  DECL_DIMS
  const size_t a2 = n2 * m->nblocks, a3 = n3 * m->nblocks;
  orc_aniso *A = (orc_aniso *)calloc(1, sizeof(orc_aniso));
  m->aniso = A;
  A->H1E = dalloc(a2); A->H1W = dalloc(a2); A->H2N = dalloc(a2); A->H2S = dalloc(a2);
  A->K1E = dalloc(a2); A->K1W = dalloc(a2); A->K2N = dalloc(a2); A->K2S = dalloc(a2); A->AMAX_CFL = dalloc(a2);
  A->HDU = dalloc(a3); A->HDV = dalloc(a3);
  double *WORKA = dalloc(n2), *WORKB = dalloc(n2);
#define E(X, i, j) esh(X, nxb, nyb, i, j)
  for (int b = 0; b < m->nblocks; b++) {
    DECL_BLK
    double *H2S = A->H2S + o2, *H1W = A->H1W + o2, *H2N = A->H2N + o2, *H1E = A->H1E + o2;
    double *K1W = A->K1W + o2, *K1E = A->K1E + o2, *K2S = A->K2S + o2, *K2N = A->K2N + o2;
    for (size_t p = 0; p < n2; p++) { H2S[p] = m->HTE[o2 + p]; H1W[p] = m->HTN[o2 + p]; }
    for (int j = 1; j <= nyb; j++) for (int i = 1; i <= nxb; i++) { H2N[P2(i, j)] = E(H2S, i, j + 1); H1E[P2(i, j)] = E(H1W, i + 1, j); }
    for (size_t p = 0; p < n2; p++) WORKA[p] = H2S[p] + H2N[p];
    for (int j = 1; j <= nyb; j++) for (int i = 1; i <= nxb; i++) WORKB[P2(i, j)] = E(WORKA, i - 1, j);
    for (size_t p = 0; p < n2; p++) K1W[p] = 2.0 * (WORKA[p] - WORKB[p]) / (WORKA[p] + WORKB[p]) / H1W[p];
    for (int j = 1; j <= nyb; j++) for (int i = 1; i <= nxb; i++) K1E[P2(i, j)] = E(K1W, i + 1, j);
    for (size_t p = 0; p < n2; p++) WORKA[p] = H1W[p] + H1E[p];
    for (int j = 1; j <= nyb; j++) for (int i = 1; i <= nxb; i++) WORKB[P2(i, j)] = E(WORKA, i, j - 1);
    for (size_t p = 0; p < n2; p++) K2S[p] = 2.0 * (WORKA[p] - WORKB[p]) / (WORKA[p] + WORKB[p]) / H2S[p];
    for (int j = 1; j <= nyb; j++) for (int i = 1; i <= nxb; i++) K2N[P2(i, j)] = E(K2S, i, j + 1);
    for (size_t p = 0; p < n2; p++)
      A->AMAX_CFL[o2 + p] = 0.125 / (m->dtu * (m->DXUR[o2 + p] * m->DXUR[o2 + p] + m->DYUR[o2 + p] * m->DYUR[o2 + p]));
  }
#undef E
  free(WORKA); free(WORKB);
  if (m->c.lvariable_hmix_aniso) {
    A->F_PARA = dalloc(a3); A->F_PERP = dalloc(a3);
    compute_ccsm_var_viscosity(m, A);
    for (int b = 0; b < m->nblocks; b++)   /* the taper :444-464 (lsmag_aniso is refused) */
      for (int k = 1; k <= km; k++) for (size_t p = 0; p < n2; p++) {
        const size_t q = (size_t)b * n3 + (size_t)(k - 1) * n2 + p;
        if (A->F_PARA[q] > A->AMAX_CFL[(size_t)b * n2 + p]) A->F_PARA[q] = A->AMAX_CFL[(size_t)b * n2 + p];
        if (A->F_PERP[q] > A->AMAX_CFL[(size_t)b * n2 + p]) A->F_PERP[q] = A->AMAX_CFL[(size_t)b * n2 + p];
      }
  }
}
static void free_aniso(orc_model *m) {
  orc_aniso *A = (orc_aniso *)m->aniso;
  if (!A) return;
  double *p[] = {A->H1E, A->H1W, A->H2N, A->H2S, A->K1E, A->K1W, A->K2N, A->K2S, A->AMAX_CFL, A->F_PARA, A->F_PERP, A->HDU, A->HDV};
  for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); i++) free(p[i]);
  free(A); m->aniso = NULL;
}

/* hdiffu_aniso (hmix_aniso.F90:557-1062) at level k of block b; HDUK, HDVK (nx,ny) */
static void hdiffu_aniso(orc_model *m, int b, int k, double *HDUK, double *HDVK, const double *UMIXK, const double *VMIXK) {
  DECL_DIMS DECL_BLK
  const orc_config *c = &m->c;
  const orc_aniso *A = (const orc_aniso *)m->aniso;
  const double *H1E = A->H1E + o2, *H1W = A->H1W + o2, *H2N = A->H2N + o2, *H2S = A->H2S + o2;
  const double *K1E = A->K1E + o2, *K1W = A->K1W + o2, *K2N = A->K2N + o2, *K2S = A->K2S + o2;
  const double *ANGLE = m->ANGLE + o2, *UAREA = m->UAREA + o2;
  const int *KMU = m->KMU + o2;
  const double *DZU = PBC ? DZUP(b) : NULL;
  double *W = dalloc(n2 * 30), *w = W;
#define TK4 ((w += 4 * n2) - 4 * n2)
  double *E11 = TK4, *E22 = TK4, *E12 = TK4, *S11 = TK4, *S22 = TK4, *S12 = TK4;
#undef TK4
  double *GW = w, *GE = w + n2, *GS = w + 2 * n2, *GN = w + 3 * n2, *NORM1 = w + 4 * n2, *NORM2 = w + 5 * n2;
#define Q(X, i, j, iq) (X)[(size_t)((iq)-1) * n2 + P2(i, j)]
  for (size_t p = 0; p < n2; p++) { HDUK[p] = 0.0; HDVK[p] = 0.0; }
  if (PBC) {   /* :689-704 */
    for (int j = jb - 1; j <= je + 1; j++) for (int i = ib - 1; i <= ie + 1; i++) {
      const double d0 = DZ3(DZU, i, j, k);
      GW[P2(i, j)] = dmin2(d0, DZ3(DZU, i - 1, j, k)) / d0;
      GE[P2(i, j)] = dmin2(d0, DZ3(DZU, i + 1, j, k)) / d0;
      GS[P2(i, j)] = dmin2(d0, DZ3(DZU, i, j - 1, k)) / d0;
      GN[P2(i, j)] = dmin2(d0, DZ3(DZU, i, j + 1, k)) / d0;
    }
  } else for (size_t p = 0; p < n2; p++) { GN[p] = 1.0; GS[p] = 1.0; GE[p] = 1.0; GW[p] = 1.0; }
  /* rate-of-strain tensor in each quarter cell :718-765 */
  for (int j = jb - 1; j <= je + 1; j++) for (int i = ib - 1; i <= ie + 1; i++) {
    const size_t p = P2(i, j);
    const double uw = GW[p] * UMIXK[P2(i - 1, j)], ue = GE[p] * UMIXK[P2(i + 1, j)], us = GS[p] * UMIXK[P2(i, j - 1)], un = GN[p] * UMIXK[P2(i, j + 1)];
    const double vw = GW[p] * VMIXK[P2(i - 1, j)], ve = GE[p] * VMIXK[P2(i + 1, j)], vs = GS[p] * VMIXK[P2(i, j - 1)], vn = GN[p] * VMIXK[P2(i, j + 1)];
    double work1 = (UMIXK[p] - uw) / H1W[p], work2 = (ue - UMIXK[p]) / H1E[p];
    double work3 = 0.5 * K2S[p] * (VMIXK[p] + vs), work4 = 0.5 * K2N[p] * (VMIXK[p] + vn);
    Q(E11, i, j, 1) = work1 + work3; Q(E11, i, j, 2) = work1 + work4; Q(E11, i, j, 3) = work2 + work4; Q(E11, i, j, 4) = work2 + work3;
    work1 = (VMIXK[p] - vs) / H2S[p]; work2 = (vn - VMIXK[p]) / H2N[p];
    work3 = 0.5 * K1W[p] * (UMIXK[p] + uw); work4 = 0.5 * K1E[p] * (UMIXK[p] + ue);
    Q(E22, i, j, 1) = work1 + work3; Q(E22, i, j, 2) = work2 + work3; Q(E22, i, j, 3) = work2 + work4; Q(E22, i, j, 4) = work1 + work4;
    work1 = (UMIXK[p] - us) / H2S[p]; work2 = (un - UMIXK[p]) / H2N[p];
    work3 = (VMIXK[p] - vw) / H1W[p]; work4 = (ve - VMIXK[p]) / H1E[p];
    const double work5 = K2S[p] * (UMIXK[p] + us), work6 = K2N[p] * (UMIXK[p] + un);
    const double work7 = K1W[p] * (VMIXK[p] + vw), work8 = K1E[p] * (VMIXK[p] + ve);
    Q(E12, i, j, 1) = work1 + work3 - 0.5 * (work5 + work7);
    Q(E12, i, j, 2) = work2 + work3 - 0.5 * (work6 + work7);
    Q(E12, i, j, 3) = work2 + work4 - 0.5 * (work6 + work8);
    Q(E12, i, j, 4) = work1 + work4 - 0.5 * (work5 + work8);
  }
  if (c->aniso_alignment == 1)   /* 'east' :777-780 */
    for (size_t p = 0; p < n2; p++) { NORM1[p] = cos(ANGLE[p]); NORM2[p] = -sin(ANGLE[p]); }
  /* viscosities :857-867, coefficients :881-911 and stress :913-926 */
  for (int iq = 1; iq <= 4; iq++)
    for (int j = jb - 1; j <= je + 1; j++) for (int i = ib - 1; i <= ie + 1; i++) {
      const size_t p = P2(i, j);
      double VTMP1 = c->visc_para, VTMP2 = c->visc_perp;
      if (c->lvariable_hmix_aniso) { VTMP1 = A->F_PARA[o3 + (size_t)(k - 1) * n2 + p]; VTMP2 = A->F_PERP[o3 + (size_t)(k - 1) * n2 + p]; }
      double Ac, Bc, Cc, Dc;
      if (c->aniso_alignment == 0) { Ac = 0.5 * (VTMP1 + VTMP2); Bc = 0.5 * (VTMP1 + VTMP2); Cc = 0.0; Dc = VTMP2; }
      else {
        const double nn = NORM1[p] * NORM2[p];
        Ac = 0.5 * (VTMP1 + VTMP2) - 2.0 * (VTMP1 - VTMP2) * (nn * nn);
        Bc = 0.5 * (VTMP1 + VTMP2) - 2.0 * (VTMP1 - VTMP2) * (nn * nn);
        Cc = (VTMP1 - VTMP2) * NORM1[p] * NORM2[p] * (NORM1[p] * NORM1[p] - NORM2[p] * NORM2[p]);
        Dc = VTMP2 + 2.0 * (VTMP1 - VTMP2) * (nn * nn);
      }
      const double e11 = Q(E11, i, j, iq), e22 = Q(E22, i, j, iq), e12 = Q(E12, i, j, iq);
      Q(S11, i, j, iq) = Ac * e11 - Bc * e22 + Cc * e12;
      Q(S22, i, j, iq) = -Bc * e11 + Ac * e22 - Cc * e12;
      Q(S12, i, j, iq) = Cc * (e11 - e22) + Dc * e12;
    }
  /* friction from the stresses :940-1035 */
  for (int j = jb; j <= je; j++) for (int i = ib; i <= ie; i++) {
    const size_t p = P2(i, j), pe = P2(i + 1, j), pw = P2(i - 1, j), pn = P2(i, j + 1), ps = P2(i, j - 1);
    double work1 = H2S[p] * Q(S11, i, j, 1) + H2N[p] * Q(S11, i, j, 2);
    double work2 = H2S[p] * Q(S11, i, j, 4) + H2N[p] * Q(S11, i, j, 3);
    double work3 = (H2S[pe] * Q(S11, i + 1, j, 1) + H2N[pe] * Q(S11, i + 1, j, 2)) * GE[p];
    double work4 = (H2S[pw] * Q(S11, i - 1, j, 4) + H2N[pw] * Q(S11, i - 1, j, 3)) * GW[p];
    double FX = 0.25 * (work2 + work3 - work1 - work4);
    work1 = H1W[p] * Q(S12, i, j, 1) + H1E[p] * Q(S12, i, j, 4);
    work2 = H1W[p] * Q(S12, i, j, 2) + H1E[p] * Q(S12, i, j, 3);
    work3 = (H1W[pn] * Q(S12, i, j + 1, 1) + H1E[pn] * Q(S12, i, j + 1, 4)) * GN[p];
    work4 = (H1W[ps] * Q(S12, i, j - 1, 2) + H1E[ps] * Q(S12, i, j - 1, 3)) * GS[p];
    FX = FX + 0.25 * ((work2 + work3) * (1.0 + 0.5 * H2N[p] * K2N[p]) - (work1 + work4) * (1.0 - 0.5 * H2S[p] * K2S[p]));
    work1 = H2S[p] * Q(S22, i, j, 1) + H2N[p] * Q(S22, i, j, 2);
    work2 = H2S[p] * Q(S22, i, j, 4) + H2N[p] * Q(S22, i, j, 3);
    work3 = (H2S[pe] * Q(S22, i + 1, j, 1) + H2N[pe] * Q(S22, i + 1, j, 2)) * GE[p];
    work4 = (H2S[pw] * Q(S22, i - 1, j, 4) + H2N[pw] * Q(S22, i - 1, j, 3)) * GW[p];
    FX = FX - 0.125 * ((work2 + work3) * H1E[p] * K1E[p] + (work1 + work4) * H1W[p] * K1W[p]);
    work1 = H1W[p] * Q(S22, i, j, 1) + H1E[p] * Q(S22, i, j, 4);
    work2 = H1W[p] * Q(S22, i, j, 2) + H1E[p] * Q(S22, i, j, 3);
    work3 = (H1W[pn] * Q(S22, i, j + 1, 1) + H1E[pn] * Q(S22, i, j + 1, 4)) * GN[p];
    work4 = (H1W[ps] * Q(S22, i, j - 1, 2) + H1E[ps] * Q(S22, i, j - 1, 3)) * GS[p];
    double FY = 0.25 * (work2 + work3 - work1 - work4);
    work1 = H2S[p] * Q(S12, i, j, 1) + H2N[p] * Q(S12, i, j, 2);
    work2 = H2S[p] * Q(S12, i, j, 4) + H2N[p] * Q(S12, i, j, 3);
    work3 = (H2S[pe] * Q(S12, i + 1, j, 1) + H2N[pe] * Q(S12, i + 1, j, 2)) * GE[p];
    work4 = (H2S[pw] * Q(S12, i - 1, j, 4) + H2N[pw] * Q(S12, i - 1, j, 3)) * GW[p];
    FY = FY + 0.25 * ((work2 + work3) * (1.0 + 0.5 * H1E[p] * K1E[p]) - (work1 + work4) * (1.0 - 0.5 * H1W[p] * K1W[p]));
    work1 = H1W[p] * Q(S11, i, j, 1) + H1E[p] * Q(S11, i, j, 4);
    work2 = H1W[p] * Q(S11, i, j, 2) + H1E[p] * Q(S11, i, j, 3);
    work3 = (H1W[pn] * Q(S11, i, j + 1, 1) + H1E[pn] * Q(S11, i, j + 1, 4)) * GN[p];
    work4 = (H1W[ps] * Q(S11, i, j - 1, 2) + H1E[ps] * Q(S11, i, j - 1, 3)) * GS[p];
    FY = FY - 0.125 * ((work2 + work3) * H2N[p] * K2N[p] + (work1 + work4) * H2S[p] * K2S[p]);
    if (KMU[p] >= k) { HDUK[p] = FX / UAREA[p]; HDVK[p] = FY / UAREA[p]; }
    else { HDUK[p] = 0.0; HDVK[p] = 0.0; }
  }
#undef Q
  free(W);
  memcpy(A->HDU + o3 + (size_t)(k - 1) * n2, HDUK, n2 * sizeof(double));
  memcpy(A->HDV + o3 + (size_t)(k - 1) * n2, HDVK, n2 * sizeof(double));
}
