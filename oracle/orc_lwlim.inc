/* orc_lwlim.inc -- tracer advection with one-dimensional flux limiters ('lw_lim': second-order forward-in-time
 * Lax-Wendroff fluxes, limited direction by direction) of the reference (source/advection.F90), restated for the CPU
 * oracle.  TEST INFRASTRUCTURE ONLY.
 *   grid coefficients      init_advection        :566-694
 * with the partial_bottom_cells branches (:582-590, :629-640, :667-678, :2040-2062, :2110, :2757-2766, :2792, :2912-2944,
 * :3065, :3140): face velocities and vertical fluxes weighted with the cell thicknesses DZU / DZT.
 *   comp_flux_vel_ghost    :1014-1120  flux velocities of the outermost ghost ring, level by level, with halo updates
 *   comp_flux_vel          :1970-2130  the luse_lw_lim branches (jend = je+2, ghost-ring patches)
 *   advt (lw_lim part)     :1667-1708  flux velocities of level k+1 kept for the next level (FLUX_VEL_prev)
 *   advt_lw_lim            :2684-2825
 *   lw_lim                 :2832-3280  (no overflows)
 *   zero_ghost_cells       :3290-3340
 * The reference's work arrays LW_z, MU_z, LW_x, MU_x, LW_y, MU_y are assigned in exactly the sign branches that read
 * them (see DESIGN.md 7); here they are zero-initialised per call, which changes nothing that is read. */
typedef struct {
  double *p5_dz_ph_r;                                                /* 1..km */
  double *p5_DXT_ph_R, *p5_DYT_ph_R;                                  /* (nx,ny,block) */
  double *UTE_to_UVEL_E, *VTN_to_VVEL_N;                              /* (nx,ny,block), with partial bottom cells (nx,ny,km,block) */
  double *UTE_jbm2, *WTKB_jbm2, *WTKB_jep2;                           /* (nx,km,block) */
  double *WTKB_ibm2, *WTKB_iep2;                                      /* (ny,km,block) */
  double *FLUX_VEL_prev;                                              /* (nx,ny,5,block) */
  double *AUX;                                                        /* (nx,ny,nt,block): flux through the top face */
} orc_lwlim;

static void init_lw_lim(orc_model *m) {
  const int nxb = m->nxb, nyb = m->nyb, km = m->km;
  const size_t n2 = m->n2, a2 = n2 * m->nblocks;
  orc_lwlim *L = (orc_lwlim *)calloc(1, sizeof(orc_lwlim));
  m->lwlim = L;
  L->p5_dz_ph_r = dalloc(km + 2);
  const size_t nlev = PBC ? (size_t)km : 1;
  L->p5_DXT_ph_R = dalloc(a2); L->p5_DYT_ph_R = dalloc(a2); L->UTE_to_UVEL_E = dalloc(a2 * nlev); L->VTN_to_VVEL_N = dalloc(a2 * nlev);
  L->UTE_jbm2 = dalloc((size_t)nxb * km * m->nblocks); L->WTKB_jbm2 = dalloc((size_t)nxb * km * m->nblocks);
  L->WTKB_jep2 = dalloc((size_t)nxb * km * m->nblocks);
  L->WTKB_ibm2 = dalloc((size_t)nyb * km * m->nblocks); L->WTKB_iep2 = dalloc((size_t)nyb * km * m->nblocks);
  L->FLUX_VEL_prev = dalloc(a2 * 5); L->AUX = dalloc(a2 * m->nt);
  for (int k = 1; k <= km - 1; k++) L->p5_dz_ph_r[k] = 1.0 / (m->dz[k] + m->dz[k + 1]);
  L->p5_dz_ph_r[km] = 0.5 / m->dz[km];
  for (int b = 0; b < m->nblocks; b++) {
    const int ib = m->blk_ib[b], ie = m->blk_ie[b], jb = m->blk_jb[b], je = m->blk_je[b];
    const size_t o = (size_t)b * n2;
#define Q2(i, j) ((size_t)((j)-1) * nxb + (i)-1)
    for (int j = jb - 2; j <= je + 2; j++) for (int i = ib - 2; i <= ie + 1; i++) {
      L->p5_DXT_ph_R[o + Q2(i, j)] = 1.0 / (m->DXT[o + Q2(i, j)] + m->DXT[o + Q2(i + 1, j)]);
      if (!PBC) L->UTE_to_UVEL_E[o + Q2(i, j)] = 1.0 / m->HTE[o + Q2(i, j)];
      else for (int k = 1; k <= km; k++)   /* :629-640 */
        L->UTE_to_UVEL_E[(size_t)b * n2 * km + (size_t)(k - 1) * n2 + Q2(i, j)] =
          1.0 / m->HTE[o + Q2(i, j)] / dmin2(DZL(DZTP(b), Q2(i, j), k), DZL(DZTP(b), Q2(i + 1, j), k));
    }
    for (int j = jb - 2; j <= je + 1; j++) for (int i = ib; i <= ie; i++) {
      L->p5_DYT_ph_R[o + Q2(i, j)] = 1.0 / (m->DYT[o + Q2(i, j)] + m->DYT[o + Q2(i, j + 1)]);
      if (!PBC) L->VTN_to_VVEL_N[o + Q2(i, j)] = 1.0 / m->HTN[o + Q2(i, j)];
      else for (int k = 1; k <= km; k++)   /* :667-678 */
        L->VTN_to_VVEL_N[(size_t)b * n2 * km + (size_t)(k - 1) * n2 + Q2(i, j)] =
          1.0 / m->HTN[o + Q2(i, j)] / dmin2(DZL(DZTP(b), Q2(i, j), k), DZL(DZTP(b), Q2(i, j + 1), k));
    }
#undef Q2
  }
}
static void free_lw_lim(orc_model *m) {
  orc_lwlim *L = (orc_lwlim *)m->lwlim;
  if (!L) return;
  double *p[] = {L->p5_dz_ph_r, L->p5_DXT_ph_R, L->p5_DYT_ph_R, L->UTE_to_UVEL_E, L->VTN_to_VVEL_N, L->UTE_jbm2, L->WTKB_jbm2,
                 L->WTKB_jep2, L->WTKB_ibm2, L->WTKB_iep2, L->FLUX_VEL_prev, L->AUX};
  for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); i++) free(p[i]);
  free(L); m->lwlim = NULL;
}

/* :3290-3340 */
static void zero_ghost_cells(orc_model *m, int b, double *F) {
  DECL_DIMS DECL_BLK
  for (int j = 1; j <= jb - 1; j++) for (int i = 1; i <= nxb; i++) F[P2(i, j)] = 0.0;
  for (int j = jb; j <= je; j++) {
    for (int i = 1; i <= ib - 1; i++) F[P2(i, j)] = 0.0;
    for (int i = ie + 1; i <= nxb; i++) F[P2(i, j)] = 0.0;
  }
  for (int j = je + 1; j <= nyb; j++) for (int i = 1; i <= nxb; i++) F[P2(i, j)] = 0.0;
}

/* comp_flux_vel with luse_lw_lim (:2017-2125); patch = 0 inside comp_flux_vel_ghost's own pass over the levels: there the
 * patched ring is overwritten by the halo updates that follow, so the stale edge values it would copy are never seen */
static void comp_flux_vel_lw(orc_model *m, int b, int k, const double *WTK, double *UTE, double *UTW, double *VTN, double *VTS,
                             double *WTKB, int patch) {
  DECL_DIMS DECL_BLK
  orc_lwlim *L = (orc_lwlim *)m->lwlim;
  zero_ghost_cells(m, b, UTE); zero_ghost_cells(m, b, UTW); zero_ghost_cells(m, b, VTN); zero_ghost_cells(m, b, VTS);
  if (k > km) { for (size_t p = 0; p < n2; p++) WTKB[p] = 0.0; return; }
  const double *UUU = m->UVEL[m->curtime] + o3, *VVV = m->VVEL[m->curtime] + o3;
  const double *DYU = m->DYU + o2, *DXU = m->DXU + o2;
  if (PBC) {   /* :2040-2062 */
    const double *DZU = DZUP(b);
#define ZU(i, j) DZL(DZU, P2(i, j), k)
    for (int j = jb - 1; j <= je + 2; j++) for (int i = ib - 1; i <= ie + 1; i++) {
      UTE[P2(i, j)] = 0.5 * (UUU[P3(i, j, k)] * DYU[P2(i, j)] * ZU(i, j) + UUU[P3(i, j - 1, k)] * DYU[P2(i, j - 1)] * ZU(i, j - 1));
      UTW[P2(i, j)] = 0.5 * (UUU[P3(i - 1, j, k)] * DYU[P2(i - 1, j)] * ZU(i - 1, j) + UUU[P3(i - 1, j - 1, k)] * DYU[P2(i - 1, j - 1)] * ZU(i - 1, j - 1));
      VTN[P2(i, j)] = 0.5 * (VVV[P3(i, j, k)] * DXU[P2(i, j)] * ZU(i, j) + VVV[P3(i - 1, j, k)] * DXU[P2(i - 1, j)] * ZU(i - 1, j));
      VTS[P2(i, j)] = 0.5 * (VVV[P3(i, j - 1, k)] * DXU[P2(i, j - 1)] * ZU(i, j - 1) + VVV[P3(i - 1, j - 1, k)] * DXU[P2(i - 1, j - 1)] * ZU(i - 1, j - 1));
    }
#undef ZU
  } else
  for (int j = jb - 1; j <= je + 2; j++) for (int i = ib - 1; i <= ie + 1; i++) {
    UTE[P2(i, j)] = 0.5 * (UUU[P3(i, j, k)] * DYU[P2(i, j)] + UUU[P3(i, j - 1, k)] * DYU[P2(i, j - 1)]);
    UTW[P2(i, j)] = 0.5 * (UUU[P3(i - 1, j, k)] * DYU[P2(i - 1, j)] + UUU[P3(i - 1, j - 1, k)] * DYU[P2(i - 1, j - 1)]);
    VTN[P2(i, j)] = 0.5 * (VVV[P3(i, j, k)] * DXU[P2(i, j)] + VVV[P3(i - 1, j, k)] * DXU[P2(i - 1, j)]);
    VTS[P2(i, j)] = 0.5 * (VVV[P3(i, j - 1, k)] * DXU[P2(i, j - 1)] + VVV[P3(i - 1, j - 1, k)] * DXU[P2(i - 1, j - 1)]);
  }
  if (patch) {
    const double *ujb = L->UTE_jbm2 + ((size_t)b * km + (k - 1)) * nxb;
    for (int i = 1; i <= nxb; i++) UTE[P2(i, jb - 2)] = ujb[i - 1];
    for (int i = 2; i <= nxb; i++) UTW[P2(i, jb - 2)] = UTE[P2(i - 1, jb - 2)];
    for (int j = 1; j <= nyb; j++) UTE[P2(ib - 2, j)] = UTW[P2(ib - 1, j)];
    for (int i = 1; i <= nxb; i++) VTN[P2(i, jb - 2)] = VTS[P2(i, jb - 1)];
  }
  if (k < km) {
    for (size_t p = 0; p < n2; p++) {
      const double FC = (VTN[p] - VTS[p] + UTE[p] - UTW[p]) * m->TAREA_R[o2 + p];
      WTKB[p] = (k < m->KMT[o2 + p]) ? (PBC ? WTK[p] + FC : WTK[p] + m->dz[k] * FC) : 0.0;   /* :2110 */
    }
    if (patch) {
      const double *wjb = L->WTKB_jbm2 + ((size_t)b * km + (k - 1)) * nxb, *wje = L->WTKB_jep2 + ((size_t)b * km + (k - 1)) * nxb;
      const double *wib = L->WTKB_ibm2 + ((size_t)b * km + (k - 1)) * nyb, *wie = L->WTKB_iep2 + ((size_t)b * km + (k - 1)) * nyb;
      for (int i = 1; i <= nxb; i++) { WTKB[P2(i, jb - 2)] = wjb[i - 1]; WTKB[P2(i, je + 2)] = wje[i - 1]; }
      for (int j = 1; j <= nyb; j++) { WTKB[P2(ib - 2, j)] = wib[j - 1]; WTKB[P2(ie + 2, j)] = wie[j - 1]; }
    }
  } else for (size_t p = 0; p < n2; p++) WTKB[p] = 0.0;
}

/* :1014-1120 */
static void comp_flux_vel_ghost(orc_model *m) {
  const int nxb = m->nxb, nyb = m->nyb, km = m->km;
  const size_t n2 = m->n2, a2 = n2 * m->nblocks;
  orc_lwlim *L = (orc_lwlim *)m->lwlim;
  double *UTE = dalloc(a2 * 6), *UTW = UTE + a2, *VTN = UTW + a2, *VTS = VTN + a2, *WTK = VTS + a2, *WTKB = WTK + a2;
  for (int k = 1; k <= km; k++) {
    for (int b = 0; b < m->nblocks; b++) {
      const size_t o = (size_t)b * n2;
      memcpy(WTK + o, (k == 1) ? m->DH + o : WTKB + o, n2 * sizeof(double));
      comp_flux_vel_lw(m, b, k, WTK + o, UTE + o, UTW + o, VTN + o, VTS + o, WTKB + o, 0);
    }
    orc_halo(m, UTE, 1, ORC_EFACE, ORC_VECTOR);
    orc_halo(m, WTKB, 1, ORC_CENTER, ORC_SCALAR);
    for (int b = 0; b < m->nblocks; b++) {
      const int ib = m->blk_ib[b], ie = m->blk_ie[b], jb = m->blk_jb[b], je = m->blk_je[b];
      const size_t o = (size_t)b * n2;
#define Q2(i, j) ((size_t)((j)-1) * nxb + (i)-1)
      for (int i = 1; i <= nxb; i++) {
        L->UTE_jbm2[((size_t)b * km + (k - 1)) * nxb + i - 1] = UTE[o + Q2(i, jb - 2)];
        L->WTKB_jbm2[((size_t)b * km + (k - 1)) * nxb + i - 1] = WTKB[o + Q2(i, jb - 2)];
        L->WTKB_jep2[((size_t)b * km + (k - 1)) * nxb + i - 1] = WTKB[o + Q2(i, je + 2)];
      }
      for (int j = 1; j <= nyb; j++) {
        L->WTKB_ibm2[((size_t)b * km + (k - 1)) * nyb + j - 1] = WTKB[o + Q2(ib - 2, j)];
        L->WTKB_iep2[((size_t)b * km + (k - 1)) * nyb + j - 1] = WTKB[o + Q2(ie + 2, j)];
      }
#undef Q2
    }
  }
  free(UTE);
}

/* lw_lim :2832-3280 for one tracer array X = TMIX(:,:,:,n) of this block */
static void lw_lim_tracer(orc_model *m, int b, int k, double adv_dt, const double *UVEL_E_dt, const double *VVEL_N_dt, double *XOUT,
                          const double *X, const double *AUX, const double *WTK, const double *WTKB, const double *WTKBp1, double *AUXB,
                          const double *CN, const double *CS, const double *CE, const double *CW, const double *KMASKE, const double *KMASKN,
                          double *TRACER_E, double *TRACER_N, const double *LW_z, const double *MU_z, const double *LW_x, const double *MU_x,
                          const double *LW_y, const double *MU_y, const double *DIV, double *XSTAR) {
  DECL_DIMS DECL_BLK
  (void)UVEL_E_dt; (void)VVEL_N_dt; (void)WTKBp1;   /* kept in the argument list; not read here */
  zero_ghost_cells(m, b, TRACER_E); zero_ghost_cells(m, b, TRACER_N); zero_ghost_cells(m, b, AUXB);
  for (int j = jb - 2; j <= je + 2; j++) {
    for (int i = ib - 2; i <= ie + 2; i++) {
      const size_t p = P2(i, j);
      const int kmt = m->KMT[o2 + p];
      if (k + 1 <= kmt) {
        const double dTR = X[P3(i, j, k + 1)] - X[P3(i, j, k)];
        if (WTKB[p] > 0.0) {
          AUXB[p] = WTKB[p] * X[P3(i, j, k + 1)];
          if (k + 2 <= kmt) {
            const double dTRp1 = X[P3(i, j, k + 2)] - X[P3(i, j, k + 1)];
            if (dTR > 0.0 && dTRp1 > 0.0) {
              const double psi_dTR = fmin(LW_z[p] * dTR, MU_z[p] * dTRp1);
              AUXB[p] = WTKB[p] * (X[P3(i, j, k + 1)] - psi_dTR);
            } else if (dTR < 0.0 && dTRp1 < 0.0) {
              const double psi_dTR = fmax(LW_z[p] * dTR, MU_z[p] * dTRp1);
              AUXB[p] = WTKB[p] * (X[P3(i, j, k + 1)] - psi_dTR);
            }
          }
        } else if (WTKB[p] < 0.0) {
          AUXB[p] = WTKB[p] * X[P3(i, j, k)];
          if (k > 1) {
            const double dTRm1 = X[P3(i, j, k)] - X[P3(i, j, k - 1)];
            if (dTR > 0.0 && dTRm1 > 0.0) {
              const double psi_dTR = fmin(LW_z[p] * dTR, MU_z[p] * dTRm1);
              AUXB[p] = WTKB[p] * (X[P3(i, j, k)] + psi_dTR);
            } else if (dTR < 0.0 && dTRm1 < 0.0) {
              const double psi_dTR = fmax(LW_z[p] * dTR, MU_z[p] * dTRm1);
              AUXB[p] = WTKB[p] * (X[P3(i, j, k)] + psi_dTR);
            }
          }
        } else AUXB[p] = 0.0;
      } else AUXB[p] = 0.0;
      if (PBC) XOUT[p] = (AUX[p] - AUXB[p] - (WTK[p] - WTKB[p]) * X[P3(i, j, k)]) / DZL(DZTP(b), p, k);   /* :3140 */
      else XOUT[p] = (AUX[p] - AUXB[p] - (WTK[p] - WTKB[p]) * X[P3(i, j, k)]) * m->dzr[k];
      XSTAR[p] = X[P3(i, j, k)] - adv_dt * XOUT[p];
    }
    for (int i = ib - 1; i <= ie; i++) {
      const size_t p = P2(i, j);
      const double dTR = (XSTAR[P2(i + 1, j)] - XSTAR[p]) * KMASKE[p];
      if (CE[p] > 0.0) {
        const double dTRm1 = (XSTAR[p] - XSTAR[P2(i - 1, j)]) * KMASKE[P2(i - 1, j)];
        if (dTR > 0.0 && dTRm1 > 0.0) TRACER_E[p] = XSTAR[p] + fmin(LW_x[p] * dTR, MU_x[p] * dTRm1);
        else if (dTR < 0.0 && dTRm1 < 0.0) TRACER_E[p] = XSTAR[p] + fmax(LW_x[p] * dTR, MU_x[p] * dTRm1);
        else TRACER_E[p] = XSTAR[p];
      } else if (CE[p] < 0.0) {
        const double dTRp1 = (XSTAR[P2(i + 2, j)] - XSTAR[P2(i + 1, j)]) * KMASKE[P2(i + 1, j)];
        if (dTR > 0.0 && dTRp1 > 0.0) TRACER_E[p] = XSTAR[P2(i + 1, j)] - fmin(LW_x[p] * dTR, MU_x[p] * dTRp1);
        else if (dTR < 0.0 && dTRp1 < 0.0) TRACER_E[p] = XSTAR[P2(i + 1, j)] - fmax(LW_x[p] * dTR, MU_x[p] * dTRp1);
        else TRACER_E[p] = XSTAR[P2(i + 1, j)];
      } else TRACER_E[p] = XSTAR[p] + LW_x[p] * dTR;
    }
  }
  for (int j = jb - 2; j <= je + 2; j++) for (int i = ib; i <= ie; i++) {
    const size_t p = P2(i, j);
    const double work1 = CE[p] * TRACER_E[p] + CW[p] * TRACER_E[P2(i - 1, j)] - (CE[p] + CW[p]) * X[P3(i, j, k)];
    XOUT[p] = XOUT[p] + work1;
    XSTAR[p] = XSTAR[p] - adv_dt * work1;
  }
  for (int j = jb - 1; j <= je; j++) for (int i = ib; i <= ie; i++) {
    const size_t p = P2(i, j);
    const double dTR = (XSTAR[P2(i, j + 1)] - XSTAR[p]) * KMASKN[p];
    if (CN[p] > 0.0) {
      const double dTRm1 = (XSTAR[p] - XSTAR[P2(i, j - 1)]) * KMASKN[P2(i, j - 1)];
      if (dTR > 0.0 && dTRm1 > 0.0) TRACER_N[p] = XSTAR[p] + fmin(LW_y[p] * dTR, MU_y[p] * dTRm1);
      else if (dTR < 0.0 && dTRm1 < 0.0) TRACER_N[p] = XSTAR[p] + fmax(LW_y[p] * dTR, MU_y[p] * dTRm1);
      else TRACER_N[p] = XSTAR[p];
    } else if (CN[p] < 0.0) {
      const double dTRp1 = (XSTAR[P2(i, j + 2)] - XSTAR[P2(i, j + 1)]) * KMASKN[P2(i, j + 1)];
      if (dTR > 0.0 && dTRp1 > 0.0) TRACER_N[p] = XSTAR[P2(i, j + 1)] - fmin(LW_y[p] * dTR, MU_y[p] * dTRp1);
      else if (dTR < 0.0 && dTRp1 < 0.0) TRACER_N[p] = XSTAR[P2(i, j + 1)] - fmax(LW_y[p] * dTR, MU_y[p] * dTRp1);
      else TRACER_N[p] = XSTAR[P2(i, j + 1)];
    } else TRACER_N[p] = XSTAR[p] + LW_y[p] * dTR;
  }
  for (int j = jb - 1; j <= je; j++) for (int i = ib; i <= ie; i++) {
    const size_t p = P2(i, j);
    XOUT[p] = XOUT[p] + CN[p] * TRACER_N[p] + CS[p] * TRACER_N[P2(i, j - 1)] - (CN[p] + CS[p] - DIV[p]) * X[P3(i, j, k)];
  }
}

/* advt (lw_lim part) + advt_lw_lim + the tracer-independent part of lw_lim for level k of block b.  UTE..WTKB: flux
 * velocities of this level (in: from the caller for k = 1, otherwise overwritten with those kept from the previous
 * level); on return WTKB is the vertical velocity at the bottom of level k and FLUX_VEL_prev holds level k+1. */
static void advt_lw_lim(orc_model *m, int b, int k, double *LTK /* n2*nt */, const double *WTK, double *UTE, double *UTW,
                        double *VTN, double *VTS, double *WTKB) {
  DECL_DIMS DECL_BLK
  orc_lwlim *L = (orc_lwlim *)m->lwlim;
  double *FP = L->FLUX_VEL_prev + (size_t)b * 5 * n2;
  if (k == 1) comp_flux_vel_lw(m, b, k, WTK, UTE, UTW, VTN, VTS, WTKB, 1);
  else {
    memcpy(UTE, FP, n2 * sizeof(double)); memcpy(UTW, FP + n2, n2 * sizeof(double)); memcpy(VTN, FP + 2 * n2, n2 * sizeof(double));
    memcpy(VTS, FP + 3 * n2, n2 * sizeof(double)); memcpy(WTKB, FP + 4 * n2, n2 * sizeof(double));
  }
  comp_flux_vel_lw(m, b, k + 1, WTKB, FP, FP + n2, FP + 2 * n2, FP + 3 * n2, FP + 4 * n2, 1);
  const double *WTKBp1 = FP + 4 * n2;
  /* advt_lw_lim :2749-2790 */
  const double adv_dt = m->c2dtt[k], adv_dt_r = 1.0 / adv_dt;
  double *W = dalloc(n2 * 20), *w = W;
#define TK2 ((w += n2) - n2)
  double *UVEL_E_dt = TK2, *VVEL_N_dt = TK2, *FVN = TK2, *FVS = TK2, *FUE = TK2, *FUW = TK2, *KMASKE = TK2, *KMASKN = TK2, *WTK_EFF = TK2;
  double *LW_z = TK2, *MU_z = TK2, *LW_x = TK2, *MU_x = TK2, *LW_y = TK2, *MU_y = TK2, *DIV = TK2, *XSTAR = TK2, *AUXB = TK2, *TRACER_E = TK2, *TRACER_N = TK2;
#undef TK2
  const double *TAR = m->TAREA_R + o2, *DXT = m->DXT + o2, *DYT = m->DYT + o2;
  const double *PX = L->p5_DXT_ph_R + o2, *PY = L->p5_DYT_ph_R + o2;
  const double *DZT = PBC ? DZTP(b) : NULL;
  for (size_t p = 0; p < n2; p++) {
    if (PBC) {   /* :2757-2766 */
      UVEL_E_dt[p] = adv_dt * UTE[p] * L->UTE_to_UVEL_E[(size_t)b * n2 * km + (size_t)(k - 1) * n2 + p];
      VVEL_N_dt[p] = adv_dt * VTN[p] * L->VTN_to_VVEL_N[(size_t)b * n2 * km + (size_t)(k - 1) * n2 + p];
      const double WORK1 = TAR[p] / DZL(DZT, p, k);
      FVN[p] = VTN[p] * WORK1; FVS[p] = -VTS[p] * WORK1; FUE[p] = UTE[p] * WORK1; FUW[p] = -UTW[p] * WORK1;
    } else {
    UVEL_E_dt[p] = adv_dt * UTE[p] * L->UTE_to_UVEL_E[o2 + p];
    VVEL_N_dt[p] = adv_dt * VTN[p] * L->VTN_to_VVEL_N[o2 + p];
    FVN[p] = VTN[p] * TAR[p]; FVS[p] = -VTS[p] * TAR[p]; FUE[p] = UTE[p] * TAR[p]; FUW[p] = -UTW[p] * TAR[p];
    }
    KMASKE[p] = (k <= m->KMT[o2 + p] && k <= m->KMTE[o2 + p]) ? 1.0 : 0.0;
    KMASKN[p] = (k <= m->KMT[o2 + p] && k <= m->KMTN[o2 + p]) ? 1.0 : 0.0;
    WTK_EFF[p] = (k == 1) ? 0.0 : WTK[p];                       /* sfc_layer_varthick */
  }
  /* lw_lim :2903-3062: tracer-independent coefficients */
  const double *dz = m->dz, *PZ = L->p5_dz_ph_r;
  const double dzk_div_dt = dz[k] * adv_dt_r, dzkp1_div_dt = (k < km) ? dz[k + 1] * adv_dt_r : 0.0;
  const double work1 = dz[k] * PZ[k], work2 = (k < km) ? dz[k + 1] * PZ[k] : 0.0, work3 = adv_dt * PZ[k];
  if (PBC) {   /* :2912-2944 */
    for (int j = jb - 2; j <= je + 2; j++) for (int i = ib - 2; i <= ie + 2; i++) {
      const size_t p = P2(i, j);
      const double zm = DZL(DZT, p, k - 1), z0 = DZL(DZT, p, k), z1 = DZL(DZT, p, k + 1);
      if (WTKB[p] > 0.0) {
        LW_z[p] = (z1 - adv_dt * WTKB[p]) / (z0 + z1);
        if (WTKBp1[p] > 0.0) MU_z[p] = (z1 * adv_dt_r - WTKBp1[p]) / WTKB[p];
        else if (WTKBp1[p] < 0.0) MU_z[p] = -WTKBp1[p] / WTKB[p] * (z1 + adv_dt * WTKBp1[p]) / (z1 + DZL(DZT, p, k + 2));   /* WTKB > 0: k < km */
        else MU_z[p] = 0.0;
      } else if (WTKB[p] < 0.0) {
        LW_z[p] = (z0 + adv_dt * WTKB[p]) / (z0 + z1);
        if (WTK_EFF[p] < 0.0) MU_z[p] = -(z0 * adv_dt_r + WTK_EFF[p]) / WTKB[p];
        else if (WTK_EFF[p] > 0.0) MU_z[p] = -WTK_EFF[p] / WTKB[p] * (z0 - adv_dt * WTK_EFF[p]) / (zm + z0);
        else MU_z[p] = 0.0;
      }
    }
  } else
  for (int j = jb - 2; j <= je + 2; j++) for (int i = ib - 2; i <= ie + 2; i++) {
    const size_t p = P2(i, j);
    if (WTKB[p] > 0.0) {
      LW_z[p] = work2 - work3 * WTKB[p];
      if (WTKBp1[p] > 0.0) MU_z[p] = (dzkp1_div_dt - WTKBp1[p]) / WTKB[p];
      else if (WTKBp1[p] < 0.0) MU_z[p] = -WTKBp1[p] / WTKB[p] * (dz[k + 1] + adv_dt * WTKBp1[p]) * PZ[k + 1];
      else MU_z[p] = 0.0;
    } else if (WTKB[p] < 0.0) {
      LW_z[p] = work1 + work3 * WTKB[p];
      if (WTK_EFF[p] < 0.0) MU_z[p] = -(dzk_div_dt + WTK_EFF[p]) / WTKB[p];
      else if (WTK_EFF[p] > 0.0) MU_z[p] = -WTK_EFF[p] / WTKB[p] * (dz[k] - adv_dt * WTK_EFF[p]) * PZ[k - 1];
      else MU_z[p] = 0.0;
    }
  }
  for (int j = jb - 2; j <= je + 2; j++) {
    int i = ib - 2;
    if (UVEL_E_dt[P2(i, j)] < 0.0) LW_x[P2(i, j)] = (DXT[P2(i + 1, j)] + UVEL_E_dt[P2(i, j)]) * PX[P2(i, j)];
    for (i = ib - 1; i <= ie; i++) {
      const size_t p = P2(i, j);
      if (UVEL_E_dt[p] > 0.0) {
        LW_x[p] = (DXT[p] - UVEL_E_dt[p]) * PX[p];
        if (UVEL_E_dt[P2(i - 1, j)] > 0.0) MU_x[p] = (DXT[p] - UVEL_E_dt[P2(i - 1, j)]) / UVEL_E_dt[p];
        else MU_x[p] = 0.0;
      } else if (UVEL_E_dt[p] < 0.0) {
        LW_x[p] = (DXT[P2(i + 1, j)] + UVEL_E_dt[p]) * PX[p];
        if (UVEL_E_dt[P2(i + 1, j)] < 0.0) MU_x[p] = -(DXT[P2(i + 1, j)] + UVEL_E_dt[P2(i + 1, j)]) / UVEL_E_dt[p];
        else MU_x[p] = 0.0;
      } else LW_x[p] = DXT[p] * PX[p];
    }
    i = ie + 1;
    if (UVEL_E_dt[P2(i, j)] > 0.0) LW_x[P2(i, j)] = (DXT[P2(i, j)] - UVEL_E_dt[P2(i, j)]) * PX[P2(i, j)];
    for (i = ib - 1; i <= ie; i++) {
      const size_t p = P2(i, j);
      if (UVEL_E_dt[p] > 0.0 && UVEL_E_dt[P2(i - 1, j)] < 0.0) MU_x[p] = -UVEL_E_dt[P2(i - 1, j)] / UVEL_E_dt[p] * LW_x[P2(i - 1, j)];
      if (UVEL_E_dt[p] < 0.0 && UVEL_E_dt[P2(i + 1, j)] > 0.0) MU_x[p] = -UVEL_E_dt[P2(i + 1, j)] / UVEL_E_dt[p] * LW_x[P2(i + 1, j)];
    }
  }
  {
    int j = jb - 2;
    for (int i = ib; i <= ie; i++)
      if (VVEL_N_dt[P2(i, j)] < 0.0) LW_y[P2(i, j)] = (DYT[P2(i, j + 1)] + VVEL_N_dt[P2(i, j)]) * PY[P2(i, j)];
    for (j = jb - 1; j <= je; j++) for (int i = ib; i <= ie; i++) {
      const size_t p = P2(i, j);
      if (VVEL_N_dt[p] > 0.0) {
        LW_y[p] = (DYT[p] - VVEL_N_dt[p]) * PY[p];
        if (VVEL_N_dt[P2(i, j - 1)] > 0.0) MU_y[p] = (DYT[p] - VVEL_N_dt[P2(i, j - 1)]) / VVEL_N_dt[p];
        else MU_y[p] = 0.0;
      } else if (VVEL_N_dt[p] < 0.0) {
        LW_y[p] = (DYT[P2(i, j + 1)] + VVEL_N_dt[p]) * PY[p];
        if (VVEL_N_dt[P2(i, j + 1)] < 0.0) MU_y[p] = -(DYT[P2(i, j + 1)] + VVEL_N_dt[P2(i, j + 1)]) / VVEL_N_dt[p];
        else MU_y[p] = 0.0;
      } else LW_y[p] = DYT[p] * PY[p];
    }
    j = je + 1;
    for (int i = ib; i <= ie; i++)
      if (VVEL_N_dt[P2(i, j)] > 0.0) LW_y[P2(i, j)] = (DYT[P2(i, j)] - VVEL_N_dt[P2(i, j)]) * PY[P2(i, j)];
    for (j = jb - 1; j <= je; j++) for (int i = ib; i <= ie; i++) {
      const size_t p = P2(i, j);
      if (VVEL_N_dt[p] > 0.0 && VVEL_N_dt[P2(i, j - 1)] < 0.0) MU_y[p] = -VVEL_N_dt[P2(i, j - 1)] / VVEL_N_dt[p] * LW_y[P2(i, j - 1)];
      if (VVEL_N_dt[p] < 0.0 && VVEL_N_dt[P2(i, j + 1)] > 0.0) MU_y[p] = -VVEL_N_dt[P2(i, j + 1)] / VVEL_N_dt[p] * LW_y[P2(i, j + 1)];
    }
  }
  for (size_t p = 0; p < n2; p++)   /* :3065-3069 */
    DIV[p] = (PBC ? (WTK_EFF[p] - WTKB[p]) / DZL(DZT, p, k) : (WTK_EFF[p] - WTKB[p]) * m->dzr[k]) + FUE[p] + FUW[p] + FVN[p] + FVS[p];
  for (int n = 0; n < m->nt; n++) {
    const double *X = m->TRACER[n][m->mixtime] + o3;
    double *AUX = L->AUX + ((size_t)b * m->nt + n) * n2;
    if (k == 1) for (size_t p = 0; p < n2; p++) AUX[p] = WTK_EFF[p] * X[p];
    lw_lim_tracer(m, b, k, adv_dt, UVEL_E_dt, VVEL_N_dt, LTK + (size_t)n * n2, X, AUX, WTK_EFF, WTKB, WTKBp1, AUXB, FVN, FVS, FUE, FUW,
                  KMASKE, KMASKN, TRACER_E, TRACER_N, LW_z, MU_z, LW_x, MU_x, LW_y, MU_y, DIV, XSTAR);
    memcpy(AUX, AUXB, n2 * sizeof(double));
  }
  free(W);
}
