/* orc_dyn.inc -- dynamics of the CPU restatement (included by pop_oracle.c).
 * TEST INFRASTRUCTURE ONLY.  Every routine cites the reference lines it
 * restates; loops run in the reference's order over the reference's ranges
 * where a result that is later read depends on it.  Local work arrays that
 * the reference leaves uninitialised outside the computed range are zero
 * here; those cells are never read before the next halo update. */

#define P2(i, j) ((size_t)((j)-1) * nxb + (i)-1)
#define P3(i, j, k) ((size_t)((k)-1) * n2 + P2(i, j))
#define DECL_DIMS \
  const int nxb = m->nxb, nyb = m->nyb, km = m->km; \
  const size_t n2 = m->n2, n3 = m->n3; (void)nxb; (void)nyb; (void)km; (void)n3; (void)n2;
#define DECL_BLK \
  const int ib = m->blk_ib[b], ie = m->blk_ie[b], jb = m->blk_jb[b], je = m->blk_je[b]; \
  const size_t o2 = (size_t)b * n2, o3 = (size_t)b * n3; (void)ib; (void)ie; (void)jb; (void)je; (void)o2; (void)o3;

/* VDC is stored (nx,ny,0:km+1,ntype,block) for every vmix choice; const and
 * rich only use levels 1..km of type 1 (vmix_const.F90, vmix_rich.F90). */
#define VDCP(mt, b) (m->VDC[mt] + (size_t)(b) * (km + 2) * n2)
#define VDC_AT(V, i, j, k) (V)[(size_t)(k) * n2 + P2(i, j)]
/* partial bottom cells: DZT, DZU (nx,ny,0:km+1,block), grid.F90:926-1016 */
#define PBC (m->c.partial_bottom_cells != 0)
#define DZTP(b) (m->DZT + (size_t)(b) * (km + 2) * n2)
#define DZUP(b) (m->DZU + (size_t)(b) * (km + 2) * n2)
#define DZ3(D, i, j, k) (D)[(size_t)(k) * n2 + P2(i, j)]
#define DZL(D, p, k) (D)[(size_t)(k) * n2 + (p)]
static inline double dmin2(double a, double b) { return a < b ? a : b; }

/* ---- grid.F90:3297-3420 tgrid_to_ugrid / ugrid_to_tgrid ---------------- */
static void tgrid_to_ugrid(orc_model *m, int b, double *AU, const double *AT) {
  DECL_DIMS DECL_BLK
  for (int j = 1; j <= nyb - 1; j++) for (int i = 1; i <= nxb - 1; i++)
    AU[P2(i, j)] = m->AU0[o2 + P2(i, j)] * AT[P2(i, j)] + m->AUN[o2 + P2(i, j)] * AT[P2(i, j + 1)] +
                   m->AUE[o2 + P2(i, j)] * AT[P2(i + 1, j)] + m->AUNE[o2 + P2(i, j)] * AT[P2(i + 1, j + 1)];
  for (int i = 1; i <= nxb; i++) AU[P2(i, nyb)] = 0.0;
  for (int j = 1; j <= nyb; j++) AU[P2(nxb, j)] = 0.0;
}
static void ugrid_to_tgrid(orc_model *m, int b, double *AT, const double *AU) {
  DECL_DIMS (void)b;
  for (int j = 2; j <= nyb; j++) for (int i = 2; i <= nxb; i++)
    AT[P2(i, j)] = 0.25 * AU[P2(i, j)] + 0.25 * AU[P2(i, j - 1)] + 0.25 * AU[P2(i - 1, j)] + 0.25 * AU[P2(i - 1, j - 1)];
  for (int i = 1; i <= nxb; i++) AT[P2(i, 1)] = 0.0;
  for (int j = 1; j <= nyb; j++) AT[P2(1, j)] = 0.0;
}

/* ---- operators.F90:126-192 grad, :49-119 div --------------------------- */
static void op_grad(orc_model *m, int b, int k, double *GX, double *GY, const double *F) {
  DECL_DIMS DECL_BLK
  for (size_t p = 0; p < n2; p++) { GX[p] = 0.0; GY[p] = 0.0; }
  for (int j = 1; j <= nyb - 1; j++) for (int i = 1; i <= nxb - 1; i++)
    if (k <= m->KMU[o2 + P2(i, j)]) {
      GX[P2(i, j)] = m->DXUR[o2 + P2(i, j)] * 0.5 * (F[P2(i + 1, j + 1)] - F[P2(i, j)] - F[P2(i, j + 1)] + F[P2(i + 1, j)]);
      GY[P2(i, j)] = m->DYUR[o2 + P2(i, j)] * 0.5 * (F[P2(i + 1, j + 1)] - F[P2(i, j)] + F[P2(i, j + 1)] - F[P2(i + 1, j)]);
    }
}
static void op_div(orc_model *m, int b, int k, double *D, const double *UX, const double *UY) {
  DECL_DIMS DECL_BLK
  const double *DYU = m->DYU + o2, *DXU = m->DXU + o2;
  for (size_t p = 0; p < n2; p++) D[p] = 0.0;
  for (int j = 2; j <= nyb; j++) for (int i = 2; i <= nxb; i++)
    if (k <= m->KMT[o2 + P2(i, j)])
      D[P2(i, j)] = 0.5 * (UX[P2(i, j)] * DYU[P2(i, j)] + UX[P2(i, j - 1)] * DYU[P2(i, j - 1)] -
                           UX[P2(i - 1, j)] * DYU[P2(i - 1, j)] - UX[P2(i - 1, j - 1)] * DYU[P2(i - 1, j - 1)] +
                           UY[P2(i, j)] * DXU[P2(i, j)] + UY[P2(i - 1, j)] * DXU[P2(i - 1, j)] -
                           UY[P2(i, j - 1)] * DXU[P2(i, j - 1)] - UY[P2(i - 1, j - 1)] * DXU[P2(i - 1, j - 1)]);
}

/* operators.F90:199-272 zcurl: z-component of the curl of a U-point vector field, times the cell area, at T points */
static void op_zcurl(orc_model *m, int b, int k, double *CURL, const double *UX, const double *UY) {
  DECL_DIMS DECL_BLK
  const double *DYU = m->DYU + o2, *DXU = m->DXU + o2;
  for (size_t p = 0; p < n2; p++) CURL[p] = 0.0;
  for (int j = 2; j <= nyb; j++) for (int i = 2; i <= nxb; i++)
    if (k <= m->KMT[o2 + P2(i, j)])
      CURL[P2(i, j)] = 0.5 * (UY[P2(i, j)] * DYU[P2(i, j)] + UY[P2(i, j - 1)] * DYU[P2(i, j - 1)] -
                              UY[P2(i - 1, j)] * DYU[P2(i - 1, j)] - UY[P2(i - 1, j - 1)] * DYU[P2(i - 1, j - 1)] -
                              UX[P2(i, j)] * DXU[P2(i, j)] - UX[P2(i - 1, j)] * DXU[P2(i - 1, j)] +
                              UX[P2(i, j - 1)] * DXU[P2(i, j - 1)] + UX[P2(i - 1, j - 1)] * DXU[P2(i - 1, j - 1)]);
}

/* ---- surface_hgt.F90:208-286 dhdt -------------------------------------- */
void orc_dhdt(orc_model *m) {
  DECL_DIMS
  for (int b = 0; b < m->nblocks; b++) {
    DECL_BLK
    double *DH = m->DH + o2, *DHU = m->DHU + o2;
    const double *PC = m->PSURF[m->curtime] + o2, *PO = m->PSURF[m->oldtime] + o2;
    for (size_t p = 0; p < n2; p++) DH[p] = (PC[p] - PO[p]) / (orc_grav * m->dtp) - m->FW_OLD[o2 + p];
    tgrid_to_ugrid(m, b, DHU, DH);
    for (size_t p = 0; p < n2; p++) if (!(m->KMU[o2 + p] >= 1)) DHU[p] = 0.0;
  }
}

/* ---- state over a full 2-D level of a block ---------------------------- */
static void state_level(orc_model *m, int kk, const double *T, const double *S, double *RHOOUT, size_t n) {
  orc_state(m, kk, kk, T, S, RHOOUT, NULL, NULL, (int)n);
}

/* ---- vertical mixing coefficients --------------------------------------- */
/* vmix_const.F90:205-228 (convection_type='diffusion') */
static void vmix_coeffs_const(orc_model *m, int b, int k, double *RHOK, double *RHOKP) {
  DECL_DIMS DECL_BLK
  const orc_config *c = &m->c;
  double *VDC = VDCP(0, b), *VVC = m->VVC + o3;
  const double *T = m->TRACER[0][m->mixtime] + o3, *S = m->TRACER[1][m->mixtime] + o3;
  int kp1 = (k + 1 < km) ? k + 1 : km;
  for (size_t p = 0; p < n2; p++) { VVC[(size_t)(k - 1) * n2 + p] = c->const_vvc; VDC[(size_t)k * n2 + p] = c->const_vdc; }
  orc_state(m, k, kp1, T + (size_t)(k - 1) * n2, S + (size_t)(k - 1) * n2, RHOK, NULL, NULL, (int)n2);
  orc_state(m, kp1, kp1, T + (size_t)(kp1 - 1) * n2, S + (size_t)(kp1 - 1) * n2, RHOKP, NULL, NULL, (int)n2);
  double vvconv = (c->convect_visc != 0.0) ? c->convect_visc : c->const_vvc;
  for (size_t p = 0; p < n2; p++)
    if (RHOK[p] > RHOKP[p] && k < m->KMT[o2 + p]) { VDC[(size_t)k * n2 + p] = c->convect_diff; VVC[(size_t)(k - 1) * n2 + p] = vvconv; }
}

/* vmix_rich.F90:224-400 (convect_diff present) */
static void vmix_coeffs_rich(orc_model *m, int b, int k, double *UTK, double *VTK,
                             double *UTKP, double *VTKP, double *RHOK, double *RICH, double *RICHU) {
  DECL_DIMS DECL_BLK
  const orc_config *c = &m->c;
  const double eps = 1.0e-10;
  double *VDC = VDCP(0, b), *VVC = m->VVC + o3;
  const double *T = m->TRACER[0][m->mixtime] + o3, *S = m->TRACER[1][m->mixtime] + o3;
  const double *UM = m->UVEL[m->mixtime] + o3, *VM = m->VVEL[m->mixtime] + o3, *RHOMIX = m->RHO[m->mixtime] + o3;
  int kp1 = (k + 1 < km) ? k + 1 : km;
  if (PBC) {   /* :266-275: the vertical shear at U points, averaged to T points */
    const double *DZU = DZUP(b);
    for (size_t p = 0; p < n2; p++) {
      const double h = 0.5 * (DZL(DZU, p, k) + DZL(DZU, p, kp1));
      UTK[p] = (UM[(size_t)(k - 1) * n2 + p] - UM[(size_t)(kp1 - 1) * n2 + p]) / h;
      VTK[p] = (VM[(size_t)(k - 1) * n2 + p] - VM[(size_t)(kp1 - 1) * n2 + p]) / h;
    }
    ugrid_to_tgrid(m, b, UTKP, UTK);
    ugrid_to_tgrid(m, b, VTKP, VTK);
  } else {
    if (k == 1) { ugrid_to_tgrid(m, b, UTK, UM); ugrid_to_tgrid(m, b, VTK, VM); }
    ugrid_to_tgrid(m, b, UTKP, UM + (size_t)(kp1 - 1) * n2);
    ugrid_to_tgrid(m, b, VTKP, VM + (size_t)(kp1 - 1) * n2);
  }
  orc_state(m, k, kp1, T + (size_t)(k - 1) * n2, S + (size_t)(k - 1) * n2, RHOK, NULL, NULL, (int)n2);
  double critnu = c->convect_diff;
  for (int j = 1; j <= nyb; j++) for (int i = 1; i <= nxb; i++) {
    size_t p = P2(i, j);
    double *vdc = &VDC[(size_t)k * n2 + p];
    if (k < m->KMT[o2 + p]) {
      if (PBC) {   /* :308-312 */
        const double *DZT = DZTP(b);
        const double h = 0.5 * (DZL(DZT, p, k) + DZL(DZT, p, kp1));
        RICH[p] = -orc_grav * (RHOK[p] - RHOMIX[(size_t)(kp1 - 1) * n2 + p]) / h / (UTKP[p] * UTKP[p] + VTKP[p] * VTKP[p] + eps / (h * h));
      } else {
      double du = UTK[p] - UTKP[p], dv = VTK[p] - VTKP[p];
      RICH[p] = -orc_grav * m->dzw[k] * (RHOK[p] - RHOMIX[(size_t)(kp1 - 1) * n2 + p]) / (du * du + dv * dv + eps);
      }
      double f = 1.0 + 5.0 * RICH[p];
      double v = c->rich_bckgrnd_vdc + (c->rich_bckgrnd_vvc + c->rich_mix / (f * f)) / f;
      *vdc = critnu < v ? critnu : v;
    } else { RICH[p] = 0.0; *vdc = 0.0; }
    if (RICH[p] < 0.0) *vdc = critnu;
  }
  tgrid_to_ugrid(m, b, RICHU, RICH);
  critnu = c->convect_visc;
  for (int j = 1; j <= nyb; j++) for (int i = 1; i <= nxb; i++) {
    size_t p = P2(i, j);
    double *vvc = &VVC[(size_t)(k - 1) * n2 + p];
    if (k < m->KMU[o2 + p]) {
      double f = 1.0 + 5.0 * RICHU[p];
      double v = c->rich_bckgrnd_vvc + c->rich_mix / (f * f);
      *vvc = critnu < v ? critnu : v;
    } else { RICHU[p] = 0.0; *vvc = 0.0; }
    if (RICHU[p] < 0.0) *vvc = critnu;
  }
  if (!PBC) {
    memcpy(UTK, UTKP, n2 * sizeof(double));
    memcpy(VTK, VTKP, n2 * sizeof(double));
  }
}

#include "orc_tidal.inc"
#include "orc_kpp.inc"

/* ---- hmix_del2.F90:1030-1095 hdifft_del2 ------------------------------- */
static void hdifft_del2(orc_model *m, int b, int k, double *HDTK /* n2*nt */) {
  DECL_DIMS DECL_BLK
  const double ah = m->c.ah;
  for (size_t p = 0; p < n2 * m->nt; p++) HDTK[p] = 0.0;
  for (int n = 0; n < m->nt; n++) {
    const double *TM = m->TRACER[n][m->mixtime] + o3;
    for (int j = jb; j <= je; j++) for (int i = ib; i <= ie; i++) {
      size_t p = P2(i, j), q = o2 + p;
      int kmt = m->KMT[q];
      double CN = m->DTN[q], CS = m->DTS[q], CE = m->DTE[q], CW = m->DTW[q];
      if (PBC) {   /* hmix_del2.F90:1034-1051 */
        const double *DZT = DZTP(b);
        CN = m->DTN[q] * dmin2(DZ3(DZT, i, j, k), DZ3(DZT, i, j + 1, k)) / DZ3(DZT, i, j, k);
        CS = m->DTS[q] * dmin2(DZ3(DZT, i, j, k), DZ3(DZT, i, j - 1, k)) / DZ3(DZT, i, j, k);
        CE = m->DTE[q] * dmin2(DZ3(DZT, i, j, k), DZ3(DZT, i + 1, j, k)) / DZ3(DZT, i, j, k);
        CW = m->DTW[q] * dmin2(DZ3(DZT, i, j, k), DZ3(DZT, i - 1, j, k)) / DZ3(DZT, i, j, k);
      }
      if (!(k <= m->KMTN[q] && k <= kmt)) CN = 0.0;
      if (!(k <= m->KMTS[q] && k <= kmt)) CS = 0.0;
      if (!(k <= m->KMTE[q] && k <= kmt)) CE = 0.0;
      if (!(k <= m->KMTW[q] && k <= kmt)) CW = 0.0;
      double CC = -(CN + CS + CE + CW);
      HDTK[(size_t)n * n2 + p] = ah * (CC * TM[P3(i, j, k)] + CN * TM[P3(i, j + 1, k)] + CS * TM[P3(i, j - 1, k)] +
                                       CE * TM[P3(i + 1, j, k)] + CW * TM[P3(i - 1, j, k)]);
    }
  }
}

/* ---- hmix_del2.F90:892-927 hdiffu_del2 (no topostress, no pbc) ---------- */
static void hdiffu_del2(orc_model *m, int b, int k, double *HDUK, double *HDVK, const double *UMIXK, const double *VMIXK) {
  DECL_DIMS DECL_BLK
  const double am = m->c.am;
  for (size_t p = 0; p < n2; p++) { HDUK[p] = 0.0; HDVK[p] = 0.0; }
  for (int j = jb; j <= je; j++) for (int i = ib; i <= ie; i++) {
    size_t q = o2 + P2(i, j);
    double cc = m->DUC[q] + m->DUM[q];
    if (PBC) {   /* hmix_del2.F90:852-886: the four neighbour weights scaled by min(DZU) / DZU, the central one unchanged */
      const double *DZU = DZUP(b);
      const double cn = m->DUN[q] * dmin2(DZ3(DZU, i, j + 1, k), DZ3(DZU, i, j, k)) / DZ3(DZU, i, j, k);
      const double cs = m->DUS[q] * dmin2(DZ3(DZU, i, j - 1, k), DZ3(DZU, i, j, k)) / DZ3(DZU, i, j, k);
      const double ce = m->DUE[q] * dmin2(DZ3(DZU, i + 1, j, k), DZ3(DZU, i, j, k)) / DZ3(DZU, i, j, k);
      const double cw = m->DUW[q] * dmin2(DZ3(DZU, i - 1, j, k), DZ3(DZU, i, j, k)) / DZ3(DZU, i, j, k);
      HDUK[P2(i, j)] = am * ((cc * UMIXK[P2(i, j)] + cn * UMIXK[P2(i, j + 1)] + cs * UMIXK[P2(i, j - 1)] +
                              ce * UMIXK[P2(i + 1, j)] + cw * UMIXK[P2(i - 1, j)]) +
                             (m->DMC[q] * VMIXK[P2(i, j)] + m->DMN[q] * VMIXK[P2(i, j + 1)] + m->DMS[q] * VMIXK[P2(i, j - 1)] +
                              m->DME[q] * VMIXK[P2(i + 1, j)] + m->DMW[q] * VMIXK[P2(i - 1, j)]));
      HDVK[P2(i, j)] = am * ((cc * VMIXK[P2(i, j)] + cn * VMIXK[P2(i, j + 1)] + cs * VMIXK[P2(i, j - 1)] +
                              ce * VMIXK[P2(i + 1, j)] + cw * VMIXK[P2(i - 1, j)]) -
                             (m->DMC[q] * UMIXK[P2(i, j)] + m->DMN[q] * UMIXK[P2(i, j + 1)] + m->DMS[q] * UMIXK[P2(i, j - 1)] +
                              m->DME[q] * UMIXK[P2(i + 1, j)] + m->DMW[q] * UMIXK[P2(i - 1, j)]));
      continue;
    }
    HDUK[P2(i, j)] = am * ((cc * UMIXK[P2(i, j)] + m->DUN[q] * UMIXK[P2(i, j + 1)] + m->DUS[q] * UMIXK[P2(i, j - 1)] +
                            m->DUE[q] * UMIXK[P2(i + 1, j)] + m->DUW[q] * UMIXK[P2(i - 1, j)]) +
                           (m->DMC[q] * VMIXK[P2(i, j)] + m->DMN[q] * VMIXK[P2(i, j + 1)] + m->DMS[q] * VMIXK[P2(i, j - 1)] +
                            m->DME[q] * VMIXK[P2(i + 1, j)] + m->DMW[q] * VMIXK[P2(i - 1, j)]));
    HDVK[P2(i, j)] = am * ((cc * VMIXK[P2(i, j)] + m->DUN[q] * VMIXK[P2(i, j + 1)] + m->DUS[q] * VMIXK[P2(i, j - 1)] +
                            m->DUE[q] * VMIXK[P2(i + 1, j)] + m->DUW[q] * VMIXK[P2(i - 1, j)]) -
                           (m->DMC[q] * UMIXK[P2(i, j)] + m->DMN[q] * UMIXK[P2(i, j + 1)] + m->DMS[q] * UMIXK[P2(i, j - 1)] +
                            m->DME[q] * UMIXK[P2(i + 1, j)] + m->DMW[q] * UMIXK[P2(i - 1, j)]));
  }
  for (size_t p = 0; p < n2; p++) if (k > m->KMU[o2 + p]) { HDUK[p] = 0.0; HDVK[p] = 0.0; }
}

#undef P2
#undef P3
#include "orc_del4.inc"
#define P2(i, j) ((size_t)((j)-1) * nxb + (i)-1)
#define P3(i, j, k) ((size_t)((k)-1) * n2 + P2(i, j))
#include "orc_aniso.inc"

/* ---- advection.F90:2068-2127 comp_flux_vel (no lw_lim, no pbc) ---------- */
static void comp_flux_vel(orc_model *m, int b, int k, const double *WTK, double *UTE, double *UTW,
                          double *VTN, double *VTS, double *WTKB) {
  DECL_DIMS DECL_BLK
  const double *UUU = m->UVEL[m->curtime] + o3, *VVV = m->VVEL[m->curtime] + o3;
  const double *DYU = m->DYU + o2, *DXU = m->DXU + o2;
  if (PBC) {   /* advection.F90:2040-2062: face fluxes carry the thickness of the U cells */
    const double *DZU = DZUP(b);
    for (int j = jb - 1; j <= je + 1; j++) for (int i = ib - 1; i <= ie + 1; i++) {
      UTE[P2(i, j)] = 0.5 * (UUU[P3(i, j, k)] * DYU[P2(i, j)] * DZ3(DZU, i, j, k) + UUU[P3(i, j - 1, k)] * DYU[P2(i, j - 1)] * DZ3(DZU, i, j - 1, k));
      UTW[P2(i, j)] = 0.5 * (UUU[P3(i - 1, j, k)] * DYU[P2(i - 1, j)] * DZ3(DZU, i - 1, j, k) + UUU[P3(i - 1, j - 1, k)] * DYU[P2(i - 1, j - 1)] * DZ3(DZU, i - 1, j - 1, k));
      VTN[P2(i, j)] = 0.5 * (VVV[P3(i, j, k)] * DXU[P2(i, j)] * DZ3(DZU, i, j, k) + VVV[P3(i - 1, j, k)] * DXU[P2(i - 1, j)] * DZ3(DZU, i - 1, j, k));
      VTS[P2(i, j)] = 0.5 * (VVV[P3(i, j - 1, k)] * DXU[P2(i, j - 1)] * DZ3(DZU, i, j - 1, k) + VVV[P3(i - 1, j - 1, k)] * DXU[P2(i - 1, j - 1)] * DZ3(DZU, i - 1, j - 1, k));
    }
  } else
  for (int j = jb - 1; j <= je + 1; j++) for (int i = ib - 1; i <= ie + 1; i++) {
    UTE[P2(i, j)] = 0.5 * (UUU[P3(i, j, k)] * DYU[P2(i, j)] + UUU[P3(i, j - 1, k)] * DYU[P2(i, j - 1)]);
    UTW[P2(i, j)] = 0.5 * (UUU[P3(i - 1, j, k)] * DYU[P2(i - 1, j)] + UUU[P3(i - 1, j - 1, k)] * DYU[P2(i - 1, j - 1)]);
    VTN[P2(i, j)] = 0.5 * (VVV[P3(i, j, k)] * DXU[P2(i, j)] + VVV[P3(i - 1, j, k)] * DXU[P2(i - 1, j)]);
    VTS[P2(i, j)] = 0.5 * (VVV[P3(i, j - 1, k)] * DXU[P2(i, j - 1)] + VVV[P3(i - 1, j - 1, k)] * DXU[P2(i - 1, j - 1)]);
  }
  if (k < km) {
    for (size_t p = 0; p < n2; p++) {
      double FC = (VTN[p] - VTS[p] + UTE[p] - UTW[p]) * m->TAREA_R[o2 + p];
      if (PBC) WTKB[p] = (k < m->KMT[o2 + p]) ? WTK[p] + FC : 0.0;   /* :2110-2111 */
      else WTKB[p] = (k < m->KMT[o2 + p]) ? WTK[p] + m->dz[k] * FC : 0.0;
    }
  } else for (size_t p = 0; p < n2; p++) WTKB[p] = 0.0;
}

/* ---- advection.F90:2243-2301 advt_centered (varthick surface) ----------- */
static void advt_centered(orc_model *m, int b, int k, double *LTK, const double *WTK, const double *WTKB,
                          const double *UTE, const double *VTN) {
  DECL_DIMS DECL_BLK
  for (int n = 0; n < m->nt; n++) {
    const double *TR = m->TRACER[n][m->curtime] + o3;
    double *L = LTK + (size_t)n * n2;
    for (int j = jb; j <= je; j++) for (int i = ib; i <= ie; i++) {
      L[P2(i, j)] = 0.5 * ((VTN[P2(i, j)] - VTN[P2(i, j - 1)] + UTE[P2(i, j)] - UTE[P2(i - 1, j)]) * TR[P3(i, j, k)] +
                           VTN[P2(i, j)] * TR[P3(i, j + 1, k)] - VTN[P2(i, j - 1)] * TR[P3(i, j - 1, k)] +
                           UTE[P2(i, j)] * TR[P3(i + 1, j, k)] - UTE[P2(i - 1, j)] * TR[P3(i - 1, j, k)]) * m->TAREA_R[o2 + P2(i, j)];
      if (PBC) L[P2(i, j)] = L[P2(i, j)] / DZ3(DZTP(b), i, j, k);   /* advection.F90:2223-2238 */
    }
    if (k != 1)
      for (int j = jb; j <= je; j++) for (int i = ib; i <= ie; i++) {
        if (PBC) L[P2(i, j)] = L[P2(i, j)] + 0.5 / DZ3(DZTP(b), i, j, k) * WTK[P2(i, j)] * (TR[P3(i, j, k - 1)] + TR[P3(i, j, k)]);   /* :2278-2280 */
        else L[P2(i, j)] = L[P2(i, j)] + m->dz2r[k] * WTK[P2(i, j)] * (TR[P3(i, j, k - 1)] + TR[P3(i, j, k)]);
      }
    if (k < km)
      for (int j = jb; j <= je; j++) for (int i = ib; i <= ie; i++) {
        if (PBC) L[P2(i, j)] = L[P2(i, j)] - 0.5 / DZ3(DZTP(b), i, j, k) * WTKB[P2(i, j)] * (TR[P3(i, j, k)] + TR[P3(i, j, k + 1)]);   /* :2292-2294 */
        else L[P2(i, j)] = L[P2(i, j)] - m->dz2r[k] * WTKB[P2(i, j)] * (TR[P3(i, j, k)] + TR[P3(i, j, k + 1)]);
      }
  }
}

#include "orc_upwind3.inc"
#include "orc_lwlim.inc"
#include "orc_gm.inc"
#include "orc_submeso.inc"

/* ---- vertical_mix.F90:770-840 vdifft ------------------------------------ */
static void vdifft(orc_model *m, int b, int k, double *VDTK, double *VTF /* n2*nt carried */) {
  DECL_DIMS DECL_BLK
  int kp1 = (k < km) ? k + 1 : km;
  int nvdc = (m->c.vmix_choice == 3) ? 2 : 1;
  for (int n = 0; n < m->nt; n++) {
    int mt2 = (n + 1 < nvdc ? n + 1 : nvdc) - 1;
    const double *VDC = VDCP(mt2, b);
    const double *TOLD = m->TRACER[n][m->oldtime] + o3;
    double *vtf = VTF + (size_t)n * n2, *out = VDTK + (size_t)n * n2;
    if (k == 1) for (size_t p = 0; p < n2; p++) vtf[p] = (m->KMT[o2 + p] >= 1) ? m->STF[n][o2 + p] : 0.0;
    for (size_t p = 0; p < n2; p++) {
      double VTFB;
      if (PBC) {   /* vertical_mix.F90:790-807 */
        const double *DZT = DZTP(b);
        VTFB = (m->KMT[o2 + p] > k) ? VDC[(size_t)k * n2 + p] * (TOLD[(size_t)(k - 1) * n2 + p] - TOLD[(size_t)(kp1 - 1) * n2 + p]) /
                                      (0.5 * (DZL(DZT, p, k) + DZL(DZT, p, kp1))) : 0.0;
        out[p] = (k <= m->KMT[o2 + p]) ? (vtf[p] - VTFB) / DZL(DZT, p, k) : 0.0;
      } else {
        VTFB = (m->KMT[o2 + p] > k) ? VDC[(size_t)k * n2 + p] * (TOLD[(size_t)(k - 1) * n2 + p] - TOLD[(size_t)(kp1 - 1) * n2 + p]) * m->dzwr[k] : 0.0;
        out[p] = (k <= m->KMT[o2 + p]) ? (vtf[p] - VTFB) * m->dzr[k] : 0.0;
      }
      vtf[p] = VTFB;
    }
  }
}

/* ---- vertical_mix.F90:935-1010 vdiffu ----------------------------------- */
static void vdiffu(orc_model *m, int b, int k, double *VDUK, double *VDVK, double *VUF, double *VVF) {
  DECL_DIMS DECL_BLK
  int kp1 = (k < km) ? k + 1 : km;
  const double *VVC = m->VVC + o3, *UOLD = m->UVEL[m->oldtime] + o3, *VOLD = m->VVEL[m->oldtime] + o3;
  if (k == 1) for (size_t p = 0; p < n2; p++) {
    VUF[p] = (m->KMU[o2 + p] >= 1) ? m->SMF[0][o2 + p] : 0.0;
    VVF[p] = (m->KMU[o2 + p] >= 1) ? m->SMF[1][o2 + p] : 0.0;
  }
  for (int j = 1; j <= nyb; j++) for (int i = 1; i <= nxb; i++) {
    size_t p = P2(i, j);
    double VUFB = VVC[P3(i, j, k)] * (UOLD[P3(i, j, k)] - UOLD[P3(i, j, kp1)]) * m->dzwr[k];
    double VVFB = VVC[P3(i, j, k)] * (VOLD[P3(i, j, k)] - VOLD[P3(i, j, kp1)]) * m->dzwr[k];
    if (PBC) {   /* vertical_mix.F90:946-959 */
      const double *DZU = DZUP(b);
      const double WORK = (k < km) ? 0.5 * (DZ3(DZU, i, j, k) + DZ3(DZU, i, j, kp1)) : 0.5 * DZ3(DZU, i, j, kp1);
      VUFB = VVC[P3(i, j, k)] * (UOLD[P3(i, j, k)] - UOLD[P3(i, j, kp1)]) / WORK;
      VVFB = VVC[P3(i, j, k)] * (VOLD[P3(i, j, k)] - VOLD[P3(i, j, kp1)]) / WORK;
    }
    if (i >= ib && i <= ie && j >= jb && j <= je && k == m->KMU[o2 + p]) {
      double vmag = m->c.bottom_drag * sqrt(UOLD[P3(i, j, k)] * UOLD[P3(i, j, k)] + VOLD[P3(i, j, k)] * VOLD[P3(i, j, k)]);
      VUFB = vmag * UOLD[P3(i, j, k)];
      VVFB = vmag * VOLD[P3(i, j, k)];
    }
    if (PBC) {   /* :991-995 */
      VDUK[p] = (k <= m->KMU[o2 + p]) ? (VUF[p] - VUFB) / DZ3(DZUP(b), i, j, k) : 0.0;
      VDVK[p] = (k <= m->KMU[o2 + p]) ? (VVF[p] - VVFB) / DZ3(DZUP(b), i, j, k) : 0.0;
    } else {
    VDUK[p] = (k <= m->KMU[o2 + p]) ? (VUF[p] - VUFB) * m->dzr[k] : 0.0;
    VDVK[p] = (k <= m->KMU[o2 + p]) ? (VVF[p] - VVFB) * m->dzr[k] : 0.0;
    }
    VUF[p] = VUFB; VVF[p] = VVFB;
  }
}

/* ---- vertical_mix.F90:1263-1368 impvmixt; :1563-1658 impvmixt_correct --- */
static void impvmixt(orc_model *m, int b, double *const TNEW[], double *const TOLD[], const double *PSFC,
                     const double *RHS1 /* NULL => impvmixt; else corrector, n2*nt */, int nfirst, int nlast,
                     double *E, double *F) {
  DECL_DIMS DECL_BLK
  int nvdc = (m->c.vmix_choice == 3) ? 2 : 1;
  double *hfac_t = m->hfac;
  for (int k = 1; k <= km; k++) hfac_t[k] = m->dz[k] / m->c2dtt[k];
  for (int n = nfirst; n <= nlast; n++) {
    int mt2 = (n < nvdc ? n : nvdc) - 1;
    const double *VDC = VDCP(mt2, b);
    double *TN = TNEW[n - 1] + o3;
    for (int j = jb; j <= je; j++) for (int i = ib; i <= ie; i++) {
      size_t p = P2(i, j);
      int kmt = m->KMT[o2 + p];
      double H1 = hfac_t[1] + PSFC[p] / (orc_grav * m->c2dtt[1]);
      double A = m->afac_t[1] * VDC_AT(VDC, i, j, 1);
      double D = H1 + A;
      E[P3(i, j, 1)] = A / D;
      double B = H1 * E[P3(i, j, 1)];
      if (RHS1) F[P3(i, j, 1)] = hfac_t[1] * RHS1[(size_t)(n - 1) * n2 + p] / D;
      else F[P3(i, j, 1)] = hfac_t[1] * TN[P3(i, j, 1)] / D;
      for (int k = 2; k <= km; k++) {
        double C = A;
        A = m->afac_t[k] * VDC_AT(VDC, i, j, k);
        if (PBC) {   /* vertical_mix.F90:1279-1287, 1577-1585: the level thickness of this column (k = 1 keeps dz(1) and afac_t(1)) */
          const double *DZT = DZTP(b);
          A = m->c.aidif * VDC_AT(VDC, i, j, k) / (0.5 * (DZ3(DZT, i, j, k) + DZ3(DZT, i, j, k + 1)));
          hfac_t[k] = DZ3(DZT, i, j, k) / m->c2dtt[k];
        }
        if (k > kmt) F[P3(i, j, k)] = 0.0;
        else {
          if (k == kmt) D = hfac_t[k] + B; else D = hfac_t[k] + A + B;
          E[P3(i, j, k)] = A / D;
          B = (hfac_t[k] + B) * E[P3(i, j, k)];
          if (RHS1) F[P3(i, j, k)] = C * F[P3(i, j, k - 1)] / D;
          else F[P3(i, j, k)] = (hfac_t[k] * TN[P3(i, j, k)] + C * F[P3(i, j, k - 1)]) / D;
        }
      }
      for (int k = km - 1; k >= 1; k--)
        if (k < kmt) F[P3(i, j, k)] = F[P3(i, j, k)] + E[P3(i, j, k)] * F[P3(i, j, k + 1)];
      if (RHS1) for (int k = 1; k <= km; k++) TN[P3(i, j, k)] = TN[P3(i, j, k)] + F[P3(i, j, k)];
      else { const double *TO = TOLD[n - 1] + o3; for (int k = 1; k <= km; k++) TN[P3(i, j, k)] = TO[P3(i, j, k)] + F[P3(i, j, k)]; }
    }
  }
}

/* ---- vertical_mix.F90:1762-1868 impvmixu -------------------------------- */
static void impvmixu(orc_model *m, int b, double *UNEW, double *VNEW, double *E, double *F1, double *F2) {
  DECL_DIMS DECL_BLK
  const double *VVC = m->VVC + o3;
  double *hfac_u = m->hfac;
  for (int k = 1; k <= km; k++) hfac_u[k] = m->dz[k] / m->c2dtu;
  for (int j = jb; j <= je; j++) for (int i = ib; i <= ie; i++) {
    int kmu = m->KMU[o2 + P2(i, j)];
    for (int k = 1; k <= km; k++) { E[P3(i, j, k)] = 0.0; F1[P3(i, j, k)] = 0.0; F2[P3(i, j, k)] = 0.0; }
    double A = m->afac_u[1] * VVC[P3(i, j, 1)];
    double D = hfac_u[1] + A;
    E[P3(i, j, 1)] = A / D;
    double B = hfac_u[1] * E[P3(i, j, 1)];
    F1[P3(i, j, 1)] = hfac_u[1] * UNEW[P3(i, j, 1)] / D;
    F2[P3(i, j, 1)] = hfac_u[1] * VNEW[P3(i, j, 1)] / D;
    for (int k = 2; k <= km; k++) {
      double C = A;
      A = m->afac_u[k] * VVC[P3(i, j, k)];
      if (PBC) {   /* vertical_mix.F90:1777-1785 */
        const double *DZU = DZUP(b);
        hfac_u[k] = DZ3(DZU, i, j, k) / m->c2dtu;
        A = m->c.aidif * VVC[P3(i, j, k)] / (0.5 * (DZ3(DZU, i, j, k) + DZ3(DZU, i, j, k + 1)));
      }
      if (k < kmu) {
        D = hfac_u[k] + A + B;
        E[P3(i, j, k)] = A / D;
        B = (hfac_u[k] + B) * E[P3(i, j, k)];
        F1[P3(i, j, k)] = (hfac_u[k] * UNEW[P3(i, j, k)] + C * F1[P3(i, j, k - 1)]) / D;
        F2[P3(i, j, k)] = (hfac_u[k] * VNEW[P3(i, j, k)] + C * F2[P3(i, j, k - 1)]) / D;
      } else if (k == kmu) {
        D = hfac_u[k] + B;
        E[P3(i, j, k)] = A / D;
        B = (hfac_u[k] + B) * E[P3(i, j, k)];
        F1[P3(i, j, k)] = (hfac_u[k] * UNEW[P3(i, j, k)] + C * F1[P3(i, j, k - 1)]) / D;
        F2[P3(i, j, k)] = (hfac_u[k] * VNEW[P3(i, j, k)] + C * F2[P3(i, j, k - 1)]) / D;
      } else { F1[P3(i, j, k)] = 0.0; F2[P3(i, j, k)] = 0.0; }
    }
    for (int k = km - 1; k >= 1; k--)
      if (k < kmu) {
        F1[P3(i, j, k)] = F1[P3(i, j, k)] + E[P3(i, j, k)] * F1[P3(i, j, k + 1)];
        F2[P3(i, j, k)] = F2[P3(i, j, k)] + E[P3(i, j, k)] * F2[P3(i, j, k + 1)];
      }
    for (int k = 1; k <= km; k++) { UNEW[P3(i, j, k)] = F1[P3(i, j, k)]; VNEW[P3(i, j, k)] = F2[P3(i, j, k)]; }
  }
}

/* ---- advection.F90:1307-1491 advu (no partial bottom cells) ------------- */
static void advu(orc_model *m, int b, int k, double *LUK, double *LVK, double *WUK,
                 double *UUE, double *UUW, double *VUN, double *VUS, double *WUKB) {
  DECL_DIMS DECL_BLK
  const double *UUU = m->UVEL[m->curtime] + o3, *VVV = m->VVEL[m->curtime] + o3;
  const double *DYU = m->DYU + o2, *DXU = m->DXU + o2, *UAR = m->UAREA_R + o2;
  for (size_t p = 0; p < n2; p++) { UUW[p] = 0.0; UUE[p] = 0.0; VUN[p] = 0.0; VUS[p] = 0.0; }
  if (PBC) {   /* advection.F90:1245-1300: mass fluxes through the U-cell faces carry the cell thicknesses */
    const double *DZU = DZUP(b);
#define UD(i, j) (UUU[P3(i, j, k)] * DYU[P2(i, j)] * DZ3(DZU, i, j, k))
#define VD(i, j) (VVV[P3(i, j, k)] * DXU[P2(i, j)] * DZ3(DZU, i, j, k))
    for (int j = jb - 1; j <= je + 1; j++) for (int i = ib - 1; i <= ie + 1; i++) {
      UUW[P2(i, j)] = 0.25 * (UD(i, j) + UD(i - 1, j)) + 0.125 * (UD(i, j - 1) + UD(i - 1, j - 1) + UD(i, j + 1) + UD(i - 1, j + 1));
      UUE[P2(i, j)] = 0.25 * (UD(i + 1, j) + UD(i, j)) + 0.125 * (UD(i + 1, j - 1) + UD(i, j - 1) + UD(i + 1, j + 1) + UD(i, j + 1));
      VUS[P2(i, j)] = 0.25 * (VD(i, j) + VD(i, j - 1)) + 0.125 * (VD(i - 1, j) + VD(i - 1, j - 1) + VD(i + 1, j) + VD(i + 1, j - 1));
      VUN[P2(i, j)] = 0.25 * (VD(i, j + 1) + VD(i, j)) + 0.125 * (VD(i - 1, j + 1) + VD(i - 1, j) + VD(i + 1, j + 1) + VD(i + 1, j));
    }
#undef UD
#undef VD
  } else
  for (int j = jb - 1; j <= je + 1; j++) for (int i = ib - 1; i <= ie + 1; i++) {
    UUW[P2(i, j)] = 0.25 * (UUU[P3(i, j, k)] * DYU[P2(i, j)] + UUU[P3(i - 1, j, k)] * DYU[P2(i - 1, j)]) +
                    0.125 * (UUU[P3(i, j - 1, k)] * DYU[P2(i, j - 1)] + UUU[P3(i - 1, j - 1, k)] * DYU[P2(i - 1, j - 1)] +
                             UUU[P3(i, j + 1, k)] * DYU[P2(i, j + 1)] + UUU[P3(i - 1, j + 1, k)] * DYU[P2(i - 1, j + 1)]);
    UUE[P2(i, j)] = 0.25 * (UUU[P3(i + 1, j, k)] * DYU[P2(i + 1, j)] + UUU[P3(i, j, k)] * DYU[P2(i, j)]) +
                    0.125 * (UUU[P3(i + 1, j - 1, k)] * DYU[P2(i + 1, j - 1)] + UUU[P3(i, j - 1, k)] * DYU[P2(i, j - 1)] +
                             UUU[P3(i + 1, j + 1, k)] * DYU[P2(i + 1, j + 1)] + UUU[P3(i, j + 1, k)] * DYU[P2(i, j + 1)]);
    VUS[P2(i, j)] = 0.25 * (VVV[P3(i, j, k)] * DXU[P2(i, j)] + VVV[P3(i, j - 1, k)] * DXU[P2(i, j - 1)]) +
                    0.125 * (VVV[P3(i - 1, j, k)] * DXU[P2(i - 1, j)] + VVV[P3(i - 1, j - 1, k)] * DXU[P2(i - 1, j - 1)] +
                             VVV[P3(i + 1, j, k)] * DXU[P2(i + 1, j)] + VVV[P3(i + 1, j - 1, k)] * DXU[P2(i + 1, j - 1)]);
    VUN[P2(i, j)] = 0.25 * (VVV[P3(i, j + 1, k)] * DXU[P2(i, j + 1)] + VVV[P3(i, j, k)] * DXU[P2(i, j)]) +
                    0.125 * (VVV[P3(i - 1, j + 1, k)] * DXU[P2(i - 1, j + 1)] + VVV[P3(i - 1, j, k)] * DXU[P2(i - 1, j)] +
                             VVV[P3(i + 1, j + 1, k)] * DXU[P2(i + 1, j + 1)] + VVV[P3(i + 1, j, k)] * DXU[P2(i + 1, j)]);
  }
  for (size_t p = 0; p < n2; p++) {
    if (PBC) WUKB[p] = WUK[p] + (VUN[p] - VUS[p] + UUE[p] - UUW[p]) * UAR[p];   /* :1352-1353 */
    else WUKB[p] = WUK[p] + m->c2dz[k] * 0.5 * (VUN[p] - VUS[p] + UUE[p] - UUW[p]) * UAR[p];
  }
  for (size_t p = 0; p < n2; p++) { LUK[p] = 0.0; LVK[p] = 0.0; }
  for (int j = jb; j <= je; j++) for (int i = ib; i <= ie; i++) {
    double cc = VUS[P2(i, j + 1)] - VUS[P2(i, j)] + UUW[P2(i + 1, j)] - UUW[P2(i, j)];
    LUK[P2(i, j)] = 0.5 * (cc * UUU[P3(i, j, k)] + VUS[P2(i, j + 1)] * UUU[P3(i, j + 1, k)] - VUS[P2(i, j)] * UUU[P3(i, j - 1, k)] +
                           UUW[P2(i + 1, j)] * UUU[P3(i + 1, j, k)] - UUW[P2(i, j)] * UUU[P3(i - 1, j, k)]) * UAR[P2(i, j)];
    LVK[P2(i, j)] = 0.5 * (cc * VVV[P3(i, j, k)] + VUS[P2(i, j + 1)] * VVV[P3(i, j + 1, k)] - VUS[P2(i, j)] * VVV[P3(i, j - 1, k)] +
                           UUW[P2(i + 1, j)] * VVV[P3(i + 1, j, k)] - UUW[P2(i, j)] * VVV[P3(i - 1, j, k)]) * UAR[P2(i, j)];
    if (PBC) { LUK[P2(i, j)] = LUK[P2(i, j)] / DZ3(DZUP(b), i, j, k); LVK[P2(i, j)] = LVK[P2(i, j)] / DZ3(DZUP(b), i, j, k); }   /* :1381-1405 */
  }
  for (int j = jb; j <= je; j++) for (int i = ib; i <= ie; i++) {
    size_t p = P2(i, j);
    if (k == 1) {
      LUK[p] = LUK[p] + m->dzr[k] * WUK[p] * UUU[P3(i, j, k)];
      LVK[p] = LVK[p] + m->dzr[k] * WUK[p] * VVV[P3(i, j, k)];
    } else if (PBC) {   /* :1443-1448 */
      LUK[p] = LUK[p] + 0.5 / DZ3(DZUP(b), i, j, k) * WUK[p] * (UUU[P3(i, j, k - 1)] + UUU[P3(i, j, k)]);
      LVK[p] = LVK[p] + 0.5 / DZ3(DZUP(b), i, j, k) * WUK[p] * (VVV[P3(i, j, k - 1)] + VVV[P3(i, j, k)]);
    } else {
      LUK[p] = LUK[p] + m->dz2r[k] * WUK[p] * (UUU[P3(i, j, k - 1)] + UUU[P3(i, j, k)]);
      LVK[p] = LVK[p] + m->dz2r[k] * WUK[p] * (VVV[P3(i, j, k - 1)] + VVV[P3(i, j, k)]);
    }
    if (k < km && PBC) {   /* :1462-1467 */
      LUK[p] = LUK[p] - 0.5 / DZ3(DZUP(b), i, j, k) * WUKB[p] * (UUU[P3(i, j, k)] + UUU[P3(i, j, k + 1)]);
      LVK[p] = LVK[p] - 0.5 / DZ3(DZUP(b), i, j, k) * WUKB[p] * (VVV[P3(i, j, k)] + VVV[P3(i, j, k + 1)]);
    } else if (k < km) {
      LUK[p] = LUK[p] - m->dz2r[k] * WUKB[p] * (UUU[P3(i, j, k)] + UUU[P3(i, j, k + 1)]);
      LVK[p] = LVK[p] - m->dz2r[k] * WUKB[p] * (VVV[P3(i, j, k)] + VVV[P3(i, j, k + 1)]);
    }
    if (k <= m->KMU[o2 + p]) {
      double u = UUU[P3(i, j, k)], v = VVV[P3(i, j, k)];
      LUK[p] = LUK[p] + u * v * m->KYU[o2 + p] - v * v * m->KXU[o2 + p];
      LVK[p] = LVK[p] + u * v * m->KXU[o2 + p] - u * u * m->KYU[o2 + p];
    } else { LUK[p] = 0.0; LVK[p] = 0.0; }
  }
  memcpy(WUK, WUKB, n2 * sizeof(double));
}

/* ---- baroclinic.F90:578-1210 baroclinic_driver -------------------------- */
/* stages of baroclinic_driver for the phase-by-phase tests (the reference calls these routines one after the other):
 * 1 vmix_coeffs + tracer_update, 2 impvmixt + halo of T,S(new), 4 state of the new tracers, 8 clinic, 16 impvmixu +
 * add old + vertical-mean removal.  orc_baroclinic_driver = all of them. */
int orc_baroclinic_stages(orc_model *m, int stages);
int orc_baroclinic_driver(orc_model *m) { return orc_baroclinic_stages(m, 31); }
int orc_baroclinic_stages(orc_model *m, int stages) {
  DECL_DIMS
  m->ran = 1;
  const orc_config *c = &m->c;
  const int nt = m->nt;
  /* step_mod.F90:302-320 */
  if (m->leapfrogts) {
    m->mixtime = m->oldtime; m->beta = 1.0 / 3.0;
    for (int k = 1; k <= km; k++) m->c2dtt[k] = 2.0 * m->dt[k];
    m->c2dtu = 2.0 * m->dtu; m->c2dtp = 2.0 * m->dtp;
  } else {
    m->mixtime = m->curtime; m->beta = 0.5;
    for (int k = 1; k <= km; k++) m->c2dtt[k] = m->dt[k];
    m->c2dtu = m->dtu; m->c2dtp = m->dtp;
  }
  const double gamma = 1.0 - 2.0 * (1.0 / 3.0);
  const int pavg = c->lpressure_avg && m->leapfrogts;
  /* work space */
  double *W = dalloc(n2 * 40 + n2 * nt * 8), *w = W;
#define TAKE(n) (w += (n), w - (n))
  double *WTK = TAKE(n2), *WTKB = TAKE(n2), *UTE = TAKE(n2), *UTW = TAKE(n2), *VTN = TAKE(n2), *VTS = TAKE(n2);
  double *RHOK = TAKE(n2), *RHOKP = TAKE(n2), *UTK = TAKE(n2), *VTK = TAKE(n2), *UTKP = TAKE(n2), *VTKP = TAKE(n2);
  double *RICH = TAKE(n2), *RICHU = TAKE(n2);
  double *FX = TAKE(n2), *FY = TAKE(n2), *WX = TAKE(n2), *WY = TAKE(n2), *WUK = TAKE(n2), *WUKB = TAKE(n2);
  double *UUE = TAKE(n2), *UUW = TAKE(n2), *VUN = TAKE(n2), *VUS = TAKE(n2), *VUF = TAKE(n2), *VVF = TAKE(n2);
  double *RHOKX = TAKE(n2), *RHOKY = TAKE(n2), *RHOKMX = TAKE(n2), *RHOKMY = TAKE(n2), *SUMX = TAKE(n2), *SUMY = TAKE(n2);
  double *RHOAVG = TAKE(n2), *WORK1 = TAKE(n2), *WORK2 = TAKE(n2), *TRANSKM1 = TAKE(n2);
  double *FT = TAKE(n2 * nt), *WORKN = TAKE(n2 * nt), *VTF = TAKE(n2 * nt), *LTK = TAKE(n2 * nt);
  double *E3 = dalloc(n3), *F3 = dalloc(n3), *G3 = dalloc(n3);

  if (c->tadvect == 3 && (stages & 1)) comp_flux_vel_ghost(m);   /* baroclinic.F90:660-672 */
  /* ---------------- block loop 1: tracers (baroclinic.F90:696-904) -------- */
  for (int b = 0; b < m->nblocks; b++) {
    DECL_BLK
    for (int k = 1; k <= km && (stages & 1); k++) {
      /* vmix_coeffs (vertical_mix.F90:590-665) */
      if (c->vmix_choice == 1) vmix_coeffs_const(m, b, k, RHOK, RHOKP);
      else if (c->vmix_choice == 2) vmix_coeffs_rich(m, b, k, UTK, VTK, UTKP, VTKP, RHOK, RICH, RICHU);
      else if (k == 1) vmix_coeffs_kpp(m, b);
      /* tracer_update (baroclinic.F90:1981-2300) */
      for (size_t p = 0; p < n2 * nt; p++) FT[p] = 0.0;
      if (c->hmix_tracer == 2) hdifft_del2(m, b, k, WORKN);
      else if (c->hmix_tracer == 3) hdifft_gm(m, b, k, WORKN);   /* also adds the isopycnal part to VDC(k) before vdifft reads it */
      else hdifft_del4(m, b, k, WORKN);
      if (c->lsubmesoscale_mixing) {   /* horizontal_mix.F90:566-581: after GM, from the differences GM has just formed */
        double *TDTK = ((orc_submeso *)m->submeso)->TDTK;
        if (k == 1) submeso_sf(m, b);
        submeso_flux(m, b, k, TDTK);
        for (size_t p = 0; p < n2 * nt; p++) WORKN[p] = WORKN[p] + TDTK[p];
      }
      for (size_t p = 0; p < n2 * nt; p++) FT[p] = FT[p] + WORKN[p];
      if (k == 1) memcpy(WTK, m->DH + o2, n2 * sizeof(double));
      for (size_t p = 0; p < n2 * nt; p++) LTK[p] = 0.0;
      if (c->tadvect == 3) advt_lw_lim(m, b, k, LTK, WTK, UTE, UTW, VTN, VTS, WTKB);   /* forms the flux velocities itself */
      else {
        comp_flux_vel(m, b, k, WTK, UTE, UTW, VTN, VTS, WTKB);
        if (c->tadvect == 1) advt_centered(m, b, k, LTK, WTK, WTKB, UTE, VTN);
        else advt_upwind3(m, b, k, LTK, WTK, WTKB, UTE, UTW, VTN, VTS);
      }
      memcpy(WTK, WTKB, n2 * sizeof(double));
      for (size_t p = 0; p < n2 * nt; p++) FT[p] = FT[p] - LTK[p];
      vdifft(m, b, k, WORKN, VTF);
      for (size_t p = 0; p < n2 * nt; p++) FT[p] = FT[p] + WORKN[p];
      if (k == 1)
        for (int n = 0; n < nt; n++) for (size_t p = 0; p < n2; p++)
          FT[(size_t)n * n2 + p] = FT[(size_t)n * n2 + p] + m->dzr[1] * m->TFW[n][o2 + p];
      /* source terms: WORKN = 0 + kpp sources (vmix_kpp.F90:3633-3690) + penetrating short wave */
      for (size_t p = 0; p < n2 * nt; p++) WORKN[p] = 0.0;
      if (c->vmix_choice == 3)
        for (int n = 0; n < nt; n++) for (size_t p = 0; p < n2; p++)
          WORKN[(size_t)n * n2 + p] = WORKN[(size_t)n * n2 + p] + m->KPP_SRC[n][o3 + (size_t)(k - 1) * n2 + p];
      if (c->lsw_absorb != 0) {   /* add_sw_absorb (sw_absorption.F90:818-947): penetrating short wave, potential temperature only */
        const orc_sw *SW = (const orc_sw *)m->sw;
        for (size_t p = 0; p < n2; p++) {
          const double q = m->SHF_QSW[o2 + p] > 0.0 ? m->SHF_QSW[o2 + p] : 0.0;
          double top, bot;
          if (c->sw_absorption_type == 2) {
            if (k == 1) TRANSKM1[p] = 1.0;
            top = TRANSKM1[p];
            bot = sw_trans_chl(m, SW, 2 * k, 0.0, chl_index(SW, m->CHL[o2 + p]));
            TRANSKM1[p] = bot;
          } else { top = SW->swabs[k - 1]; bot = SW->swabs[k]; }
          if (PBC) WORKN[p] = WORKN[p] + ((k < m->KMT[o2 + p]) ? q * (top - bot) * m->dzr[k] : q * top / DZL(DZTP(b), p, k));   /* sw_absorption.F90:880-889, 913-921 */
          else WORKN[p] = WORKN[p] + ((k < m->KMT[o2 + p]) ? q * (top - bot) * m->dzr[k] : q * top * m->dzr[k]);
        }
      }
      for (size_t p = 0; p < n2 * nt; p++) FT[p] = FT[p] + WORKN[p];
      /* store RHS (implicit vmix, varthick) baroclinic.F90:2212-2237 */
      for (int n = 0; n < nt; n++) {
        double *TNEW = m->TRACER[n][m->newtime] + o3;
        const double *TCUR = m->TRACER[n][m->curtime] + o3;
        const double *PCUR = m->PSURF[m->curtime] + o2, *POLD = m->PSURF[m->oldtime] + o2;
        if (k == 1 && pavg && n < 2) {
          for (size_t p = 0; p < n2; p++)
            if (m->KMT[o2 + p] > 0)
              TNEW[p] = m->c2dtt[1] * FT[(size_t)n * n2 + p] - 2.0 * TCUR[p] * (PCUR[p] - POLD[p]) / (orc_grav * m->dz[1]);
        } else {
          for (size_t p = 0; p < n2; p++)
            TNEW[(size_t)(k - 1) * n2 + p] = (k <= m->KMT[o2 + p]) ? m->c2dtt[k] * FT[(size_t)n * n2 + p] : 0.0;
        }
      }
    }
    if (pavg && (stages & 2)) { double *tn[8], *to[8]; for (int n = 0; n < nt; n++) { tn[n] = m->TRACER[n][m->newtime]; to[n] = m->TRACER[n][m->oldtime]; }
      impvmixt(m, b, tn, to, m->PSURF[m->curtime] + o2, NULL, 1, 2, E3, F3); }
  }
  if (pavg && (stages & 2)) {
    orc_halo(m, m->TRACER[0][m->newtime], km, ORC_CENTER, ORC_SCALAR);
    orc_halo(m, m->TRACER[1][m->newtime], km, ORC_CENTER, ORC_SCALAR);
  }
  /* ---------------- block loop 2: momentum (baroclinic.F90:954-1165) ------ */
  for (int b = 0; b < m->nblocks; b++) {
    DECL_BLK
    double *ZX = m->ZX + o2, *ZY = m->ZY + o2;
    double *UNEW = m->UVEL[m->newtime] + o3, *VNEW = m->VVEL[m->newtime] + o3;
    const double *UCUR = m->UVEL[m->curtime] + o3, *VCUR = m->VVEL[m->curtime] + o3;
    const double *UOLD = m->UVEL[m->oldtime] + o3, *VOLD = m->VVEL[m->oldtime] + o3;
    const double *UMIX = m->UVEL[m->mixtime] + o3, *VMIX = m->VVEL[m->mixtime] + o3;
    if (stages & 8) for (size_t p = 0; p < n2; p++) { ZX[p] = 0.0; ZY[p] = 0.0; }
    for (int k = 1; k <= km; k++) {
      size_t ok = (size_t)(k - 1) * n2;
      if (pavg && (stages & 4)) state_level(m, k, m->TRACER[0][m->newtime] + o3 + ok, m->TRACER[1][m->newtime] + o3 + ok, m->RHO[m->newtime] + o3 + ok, n2);
      if (!(stages & 8)) continue;
      /* clinic (baroclinic.F90:1724-1890) */
      if (k == 1) memcpy(WUK, m->DHU + o2, n2 * sizeof(double));
      advu(m, b, k, WX, WY, WUK, UUE, UUW, VUN, VUS, WUKB);
      for (size_t p = 0; p < n2; p++) { FX[p] = -WX[p]; FY[p] = -WY[p]; }
      const double *FC = m->FCOR + o2;
      if (c->impcor && m->leapfrogts) {
        for (size_t p = 0; p < n2; p++) {
          FX[p] = FX[p] + FC[p] * (gamma * VCUR[ok + p] + (1.0 - gamma) * VOLD[ok + p]);
          FY[p] = FY[p] - FC[p] * (gamma * UCUR[ok + p] + (1.0 - gamma) * UOLD[ok + p]);
        }
      } else if (!c->impcor && m->leapfrogts) {
        for (size_t p = 0; p < n2; p++) { FX[p] = FX[p] + FC[p] * VCUR[ok + p]; FY[p] = FY[p] - FC[p] * UCUR[ok + p]; }
      } else {
        for (size_t p = 0; p < n2; p++) { FX[p] = FX[p] + FC[p] * VOLD[ok + p]; FY[p] = FY[p] - FC[p] * UOLD[ok + p]; }
      }
      /* gradp (pressure_grad.F90:258-301) */
      {
        const double *RN = m->RHO[m->newtime] + o3 + ok, *RC = m->RHO[m->curtime] + o3 + ok, *RO = m->RHO[m->oldtime] + o3 + ok;
        if (pavg) for (size_t p = 0; p < n2; p++) RHOAVG[p] = 0.25 * (RN[p] + 2.0 * RC[p] + RO[p]) * m->bouss[k];
        else for (size_t p = 0; p < n2; p++) RHOAVG[p] = RC[p] * m->bouss[k];
        op_grad(m, b, k, RHOKX, RHOKY, RHOAVG);
        if (k == 1) for (size_t p = 0; p < n2; p++) { RHOKMX[p] = RHOKX[p]; RHOKMY[p] = RHOKY[p]; SUMX[p] = 0.0; SUMY[p] = 0.0; }
        double factor = m->dzw[k - 1] * orc_grav * 0.5;
        for (size_t p = 0; p < n2; p++) {
          SUMX[p] = SUMX[p] + factor * (RHOKX[p] + RHOKMX[p]);
          SUMY[p] = SUMY[p] + factor * (RHOKY[p] + RHOKMY[p]);
          RHOKMX[p] = RHOKX[p]; RHOKMY[p] = RHOKY[p];
          FX[p] = FX[p] - SUMX[p]; FY[p] = FY[p] - SUMY[p];
        }
      }
      if (c->hmix_momentum == 2) hdiffu_del2(m, b, k, WX, WY, UMIX + ok, VMIX + ok);
      else if (c->hmix_momentum == 3) hdiffu_aniso(m, b, k, WX, WY, UMIX + ok, VMIX + ok);   /* horizontal_mix.F90:464-472 */
      else hdiffu_del4(m, b, k, WX, WY, UMIX + ok, VMIX + ok);
      for (size_t p = 0; p < n2; p++) { FX[p] = FX[p] + WX[p]; FY[p] = FY[p] + WY[p]; }
      vdiffu(m, b, k, WX, WY, VUF, VVF);
      for (size_t p = 0; p < n2; p++) { FX[p] = FX[p] + WX[p]; FY[p] = FY[p] + WY[p]; }
      for (size_t p = 0; p < n2; p++) if (k > m->KMU[o2 + p]) { FX[p] = 0.0; FY[p] = 0.0; }
      /* baroclinic.F90:1013-1045 */
      if (c->impcor) {
        for (size_t p = 0; p < n2; p++) {
          WORK1[p] = m->c2dtu * m->beta * FC[p];
          WORK2[p] = m->c2dtu / (1.0 + WORK1[p] * WORK1[p]);
          UNEW[ok + p] = (FX[p] + WORK1[p] * FY[p]) * WORK2[p];
          VNEW[ok + p] = (FY[p] - WORK1[p] * FX[p]) * WORK2[p];
        }
      } else for (size_t p = 0; p < n2; p++) { UNEW[ok + p] = m->c2dtu * FX[p]; VNEW[ok + p] = m->c2dtu * FY[p]; }
      if (PBC) for (size_t p = 0; p < n2; p++) { ZX[p] = ZX[p] + FX[p] * DZL(DZUP(b), p, k); ZY[p] = ZY[p] + FY[p] * DZL(DZUP(b), p, k); }   /* baroclinic.F90:1037-1039 */
      else for (size_t p = 0; p < n2; p++) { ZX[p] = ZX[p] + FX[p] * m->dz[k]; ZY[p] = ZY[p] + FY[p] * m->dz[k]; }
    }
    if (stages & 8) for (size_t p = 0; p < n2; p++) { ZX[p] = ZX[p] * m->HUR[o2 + p]; ZY[p] = ZY[p] * m->HUR[o2 + p]; }
    if (!(stages & 16)) continue;
    impvmixu(m, b, UNEW, VNEW, E3, F3, G3);
    for (size_t p = 0; p < n3; p++) { UNEW[p] = UOLD[p] + UNEW[p]; VNEW[p] = VOLD[p] + VNEW[p]; }
    for (size_t p = 0; p < n2; p++) { WORK1[p] = 0.0; WORK2[p] = 0.0; }
    for (int k = 1; k <= km; k++) for (size_t p = 0; p < n2; p++) {
      const double dzk = PBC ? DZL(DZUP(b), p, k) : m->dz[k];   /* baroclinic.F90:1097-1106 */
      WORK1[p] = WORK1[p] + UNEW[(size_t)(k - 1) * n2 + p] * dzk;
      WORK2[p] = WORK2[p] + VNEW[(size_t)(k - 1) * n2 + p] * dzk;
    }
    for (size_t p = 0; p < n2; p++) { WORK1[p] = WORK1[p] * m->HUR[o2 + p]; WORK2[p] = WORK2[p] * m->HUR[o2 + p]; }
    for (int k = 1; k <= km; k++) for (size_t p = 0; p < n2; p++) {
      size_t q = (size_t)(k - 1) * n2 + p;
      if (k <= m->KMU[o2 + p]) { UNEW[q] = UNEW[q] - WORK1[p]; VNEW[q] = VNEW[q] - WORK2[p]; }
      else { UNEW[q] = 0.0; VNEW[q] = 0.0; }
    }
  }
  free(W); free(E3); free(F3); free(G3);
#undef TAKE
  return 0;
}

/* ---- POP_SolversMod.F90:2414-2426 btropOperator ------------------------- */
static void btrop_operator(orc_model *m, int b, double *AX, const double *X) {
  DECL_DIMS DECL_BLK
  const double *C = m->centerWgt + o2, *N = m->btropWgtNorth + o2, *Ea = m->btropWgtEast + o2, *NE = m->btropWgtNE + o2;
  double *ax = AX + o2; const double *x = X + o2;
  for (size_t p = 0; p < n2; p++) ax[p] = 0.0;
  for (int j = 2; j <= nyb - 1; j++) for (int i = 2; i <= nxb - 1; i++)
    ax[P2(i, j)] = C[P2(i, j)] * x[P2(i, j)] + N[P2(i, j)] * x[P2(i, j + 1)] + N[P2(i, j - 1)] * x[P2(i, j - 1)] +
                   Ea[P2(i, j)] * x[P2(i + 1, j)] + Ea[P2(i - 1, j)] * x[P2(i - 1, j)] +
                   NE[P2(i, j)] * x[P2(i + 1, j + 1)] + NE[P2(i, j - 1)] * x[P2(i + 1, j - 1)] +
                   NE[P2(i - 1, j)] * x[P2(i - 1, j + 1)] + NE[P2(i - 1, j - 1)] * x[P2(i - 1, j - 1)];
}

#include "orc_evp.inc"
/* z = M^-1 r: EVP sub-block solves + halo, or r/diag (preconditioner call sites :1322, :1646, :2010, :2118, :2789) */
static int use_evp(const orc_model *m) { return m->c.preconditioner_choice == 1; }
#include "orc_pcsi.inc"

/* ---- POP_SolversMod.F90:1255-1503 pcg (diagonal or EVP preconditioner) --------- */
static int solver_pcg(orc_model *m, double *X, const double *B) {
  DECL_DIMS
  size_t nall = n2 * m->nblocks;
  double *R = dalloc(nall), *S = dalloc(nall), *Q = dalloc(nall), *work0 = dalloc(nall), *work1 = dalloc(nall);
  double eta0, eta1, rr = 0.0;
  for (int b = 0; b < m->nblocks; b++) btrop_operator(m, b, S, X);
  for (size_t p = 0; p < nall; p++) { R[p] = B[p] - S[p]; S[p] = 0.0; }
  orc_halo(m, R, 1, ORC_CENTER, ORC_SCALAR);
  eta0 = 1.0;
  m->numIterations = m->c.max_iterations;
  for (int it = 1; it <= m->c.max_iterations; it++) {
    if (use_evp(m)) {
      for (int b = 0; b < m->nblocks; b++) evp_apply(m, b, work1, R);
      for (size_t p = 0; p < nall; p++) work0[p] = R[p] * work1[p];
      orc_halo(m, work1, 1, ORC_CENTER, ORC_SCALAR);   /* :1352-1362 */
    } else for (size_t p = 0; p < nall; p++) {
      if (m->centerWgt[p] != 0.0) work1[p] = R[p] / m->centerWgt[p]; else work1[p] = 0.0;
      work0[p] = R[p] * work1[p];
    }
    eta1 = orc_global_sum(m, work0, m->mMask);
    for (size_t p = 0; p < nall; p++) S[p] = work1[p] + S[p] * (eta1 / eta0);
    for (int b = 0; b < m->nblocks; b++) btrop_operator(m, b, Q, S);
    for (size_t p = 0; p < nall; p++) work0[p] = Q[p] * S[p];
    orc_halo(m, Q, 1, ORC_CENTER, ORC_SCALAR);
    eta0 = eta1;
    eta1 = eta0 / orc_global_sum(m, work0, m->mMask);
    for (size_t p = 0; p < nall; p++) { X[p] = X[p] + eta1 * S[p]; R[p] = R[p] - eta1 * Q[p]; }
    if (it % m->c.convergence_check_freq == 0) {
      for (int b = 0; b < m->nblocks; b++) btrop_operator(m, b, R, X);
      for (size_t p = 0; p < nall; p++) { R[p] = B[p] - R[p]; work0[p] = R[p] * R[p]; }
      orc_halo(m, R, 1, ORC_CENTER, ORC_SCALAR);
      rr = orc_global_sum(m, work0, m->mMask);
      if (rr < m->convergenceCriterion) { m->numIterations = it; break; }
    }
  }
  m->rmsResidual = sqrt(rr * m->residualNorm);
  free(R); free(S); free(Q); free(work0); free(work1);
  if (m->numIterations == m->c.max_iterations && m->convergenceCriterion != 0.0) return 1;
  return 0;
}

/* ---- POP_SolversMod.F90:1960-2266 ChronGear (diagonal or EVP preconditioner) --- */
static int solver_chrongear(orc_model *m, double *X, const double *B) {
  DECL_DIMS
  size_t nall = n2 * m->nblocks;
  double *R = dalloc(nall), *S = dalloc(nall), *Q = dalloc(nall), *Z = dalloc(nall), *AZ = dalloc(nall);
  double *A0R = dalloc(nall), *W1 = dalloc(nall), *W2 = dalloc(nall);
  double rr = 0.0, cgRhoOld, cgSigma, cgAlpha, cgRho, cgDelta, cgBeta;
  for (size_t p = 0; p < nall; p++) A0R[p] = (m->centerWgt[p] != 0.0) ? 1.0 / m->centerWgt[p] : 0.0;
  for (int b = 0; b < m->nblocks; b++) btrop_operator(m, b, S, X);
  for (size_t p = 0; p < nall; p++) R[p] = B[p] - S[p];
  orc_halo(m, R, 1, ORC_CENTER, ORC_SCALAR);
  if (use_evp(m)) {
    for (int b = 0; b < m->nblocks; b++) evp_apply(m, b, Z, R);
    orc_halo(m, Z, 1, ORC_CENTER, ORC_SCALAR);   /* :2023-2032 */
    for (size_t p = 0; p < nall; p++) { W1[p] = R[p] * Z[p]; S[p] = Z[p]; }
  } else
  for (size_t p = 0; p < nall; p++) { Z[p] = R[p] * A0R[p]; W1[p] = R[p] * Z[p]; S[p] = Z[p]; }
  for (int b = 0; b < m->nblocks; b++) btrop_operator(m, b, Q, S);
  for (size_t p = 0; p < nall; p++) W2[p] = S[p] * Q[p];
  orc_halo(m, Q, 1, ORC_CENTER, ORC_SCALAR);
  cgRhoOld = orc_global_sum(m, W1, m->mMask);
  cgSigma = orc_global_sum(m, W2, m->mMask);
  cgAlpha = cgRhoOld / cgSigma;
  for (size_t p = 0; p < nall; p++) { X[p] = X[p] + cgAlpha * S[p]; R[p] = R[p] - cgAlpha * Q[p]; }
  m->numIterations = m->c.max_iterations;
  for (int it = 1; it <= m->c.max_iterations; it++) {
    if (use_evp(m)) for (int b = 0; b < m->nblocks; b++) evp_apply(m, b, Z, R);
    else for (size_t p = 0; p < nall; p++) Z[p] = R[p] * A0R[p];
    orc_halo(m, Z, 1, ORC_CENTER, ORC_SCALAR);
    for (int b = 0; b < m->nblocks; b++) btrop_operator(m, b, AZ, Z);
    for (size_t p = 0; p < nall; p++) { W1[p] = R[p] * Z[p]; W2[p] = AZ[p] * Z[p]; }
    cgRho = orc_global_sum(m, W1, m->mMask);
    cgDelta = orc_global_sum(m, W2, m->mMask);
    cgBeta = cgRho / cgRhoOld;
    cgSigma = cgDelta - (cgBeta * cgBeta) * cgSigma;
    cgAlpha = cgRho / cgSigma;
    cgRhoOld = cgRho;
    for (size_t p = 0; p < nall; p++) {
      S[p] = Z[p] + cgBeta * S[p];
      Q[p] = AZ[p] + cgBeta * Q[p];
      X[p] = X[p] + cgAlpha * S[p];
      R[p] = R[p] - cgAlpha * Q[p];
    }
    if (it % m->c.convergence_check_freq == 0) {
      for (int b = 0; b < m->nblocks; b++) btrop_operator(m, b, Z, X);
      for (size_t p = 0; p < nall; p++) { R[p] = B[p] - Z[p]; W1[p] = R[p] * R[p]; }
      orc_halo(m, R, 1, ORC_CENTER, ORC_SCALAR);
      rr = orc_global_sum(m, W1, m->mMask);
      if (rr < m->convergenceCriterion) { m->numIterations = it; break; }
    }
  }
  m->rmsResidual = sqrt(rr * m->residualNorm);
  free(R); free(S); free(Q); free(Z); free(AZ); free(A0R); free(W1); free(W2);
  if (m->numIterations == m->c.max_iterations && m->convergenceCriterion != 0.0) return 1;
  return 0;
}

/* ---- barotropic.F90:417-731 barotropic_driver --------------------------- */
int orc_barotropic_driver(orc_model *m) {
  DECL_DIMS
  const orc_config *c = &m->c;
  const double gamma = 1.0 - 2.0 * (1.0 / 3.0);
  double *W1 = dalloc(n2), *W2 = dalloc(n2), *W3 = dalloc(n2), *W4 = dalloc(n2);
  /* halo ZX, ZY: step_mod.F90:405-423 */
  orc_halo(m, m->ZX, 1, ORC_NECORNER, ORC_VECTOR);
  orc_halo(m, m->ZY, 1, ORC_NECORNER, ORC_VECTOR);
  for (int b = 0; b < m->nblocks; b++) {
    DECL_BLK
    const double *ZX = m->ZX + o2, *ZY = m->ZY + o2, *FC = m->FCOR + o2, *HU = m->HU + o2;
    const double *GXC = m->GRADPX[m->curtime] + o2, *GXO = m->GRADPX[m->oldtime] + o2;
    const double *GYC = m->GRADPY[m->curtime] + o2, *GYO = m->GRADPY[m->oldtime] + o2;
    double *UH = m->UH + o2, *VH = m->VH + o2, *RHS = m->RHS + o2;
    if (m->leapfrogts) for (size_t p = 0; p < n2; p++) {
      W3[p] = m->c2dtp * (ZX[p] - gamma * GXC[p] - (1.0 - gamma) * GXO[p]);
      W4[p] = m->c2dtp * (ZY[p] - gamma * GYC[p] - (1.0 - gamma) * GYO[p]);
    } else for (size_t p = 0; p < n2; p++) {
      W3[p] = m->c2dtp * (ZX[p] - GXC[p]);
      W4[p] = m->c2dtp * (ZY[p] - GYC[p]);
    }
    if (c->impcor) for (size_t p = 0; p < n2; p++) {
      W1[p] = m->c2dtp * m->beta * FC[p];
      W2[p] = 1.0 / (1.0 + W1[p] * W1[p]);
      UH[p] = W2[p] * (W3[p] + W1[p] * W4[p]) + m->UBTROP[m->oldtime][o2 + p];
      VH[p] = W2[p] * (W4[p] - W1[p] * W3[p]) + m->VBTROP[m->oldtime][o2 + p];
    } else for (size_t p = 0; p < n2; p++) {
      UH[p] = W3[p] + m->UBTROP[m->oldtime][o2 + p];
      VH[p] = W4[p] + m->VBTROP[m->oldtime][o2 + p];
    }
    if (m->leapfrogts) for (size_t p = 0; p < n2; p++) {
      W3[p] = HU[p] * (UH[p] + m->beta * m->c2dtp * GXO[p]);
      W4[p] = HU[p] * (VH[p] + m->beta * m->c2dtp * GYO[p]);
    } else for (size_t p = 0; p < n2; p++) {
      W3[p] = HU[p] * (UH[p] + m->beta * m->c2dtp * GXC[p]);
      W4[p] = HU[p] * (VH[p] + m->beta * m->c2dtp * GYC[p]);
    }
    op_div(m, b, 1, RHS, W3, W4);
    for (size_t p = 0; p < n2; p++) RHS[p] = RHS[p] / (m->beta * m->c2dtp);
    for (size_t p = 0; p < n2; p++) {
      double dc = (m->KMT[o2 + p] >= 1) ? m->TAREA[o2 + p] / (m->beta * m->c2dtp * m->dtp * orc_grav) : 0.0;
      RHS[p] = RHS[p] - dc * m->PSURF[m->curtime][o2 + p] - m->FW[o2 + p] * m->TAREA[o2 + p] / (m->beta * m->c2dtp);
      m->centerWgt[o2 + p] = m->centerWgtIndep[o2 + p] - dc;
      m->PSURF[m->newtime][o2 + p] = m->PGUESS[o2 + p];
    }
  }
  orc_halo(m, m->RHS, 1, ORC_CENTER, ORC_SCALAR);
  int err = (c->solver_choice == 2) ? solver_chrongear(m, m->PSURF[m->newtime], m->RHS)
          : (c->solver_choice == 3) ? solver_pcsi(m, m->PSURF[m->newtime], m->RHS)
                                    : solver_pcg(m, m->PSURF[m->newtime], m->RHS);
  /* checkerboard null space barotropic.F90:606-630 */
  double *PCHECK = dalloc(n2 * m->nblocks);
  for (size_t p = 0; p < n2 * m->nblocks; p++) PCHECK[p] = m->PSURF[m->newtime][p] * m->CHECKER[p];
  double xcheck = orc_global_sum(m, PCHECK, NULL);
  free(PCHECK);
  for (int b = 0; b < m->nblocks; b++) {
    DECL_BLK
    double *PN = m->PSURF[m->newtime] + o2, *GXN = m->GRADPX[m->newtime] + o2, *GYN = m->GRADPY[m->newtime] + o2;
    for (size_t p = 0; p < n2; p++)
      PN[p] = PN[p] + m->CONSTNT[o2 + p] * m->rcheck * xcheck - m->CHECKER[o2 + p] * m->rconst * xcheck;
    op_grad(m, b, 1, GXN, GYN, PN);
    const double *GXR = m->leapfrogts ? m->GRADPX[m->oldtime] + o2 : m->GRADPX[m->curtime] + o2;
    const double *GYR = m->leapfrogts ? m->GRADPY[m->oldtime] + o2 : m->GRADPY[m->curtime] + o2;
    for (size_t p = 0; p < n2; p++) {
      m->UBTROP[m->newtime][o2 + p] = m->UH[o2 + p] - m->beta * m->c2dtp * (GXN[p] - GXR[p]);
      m->VBTROP[m->newtime][o2 + p] = m->VH[o2 + p] - m->beta * m->c2dtp * (GYN[p] - GYR[p]);
    }
  }
  orc_halo(m, m->PSURF[m->newtime], 1, ORC_CENTER, ORC_SCALAR);
  orc_halo(m, m->GRADPX[m->newtime], 1, ORC_NECORNER, ORC_VECTOR);
  orc_halo(m, m->GRADPY[m->newtime], 1, ORC_NECORNER, ORC_VECTOR);
  free(W1); free(W2); free(W3); free(W4);
  return err;
}

/* ---- baroclinic.F90:1283-1480 baroclinic_correct_adjust ----------------- */
void orc_baroclinic_correct_adjust(orc_model *m) {
  DECL_DIMS
  const orc_config *c = &m->c;
  const int nt = m->nt;
  const int pavg = c->lpressure_avg && m->leapfrogts;
  double *RHS1 = dalloc(n2 * nt), *E3 = dalloc(n3), *F3 = dalloc(n3);
  for (int b = 0; b < m->nblocks; b++) {
    DECL_BLK
    const double *PO = m->PSURF[m->oldtime] + o2, *PC = m->PSURF[m->curtime] + o2, *PN = m->PSURF[m->newtime] + o2;
    const double *PM = m->PSURF[m->mixtime] + o2;
    double *tn[8], *to[8];
    for (int n = 0; n < nt; n++) { tn[n] = m->TRACER[n][m->newtime]; to[n] = m->TRACER[n][m->oldtime]; }
    if (pavg) {
      for (int n = 0; n < 2; n++) {
        const double *TC = m->TRACER[n][m->curtime] + o3, *TO = m->TRACER[n][m->oldtime] + o3, *TN = m->TRACER[n][m->newtime] + o3;
        for (size_t p = 0; p < n2; p++)
          RHS1[(size_t)n * n2 + p] = (m->KMT[o2 + p] > 0)
            ? ((2.0 * TC[p] - TO[p]) * (PC[p] - PO[p]) - TN[p] * (PN[p] - PC[p])) / (orc_grav * m->dz[1]) : 0.0;
      }
      impvmixt(m, b, tn, to, PN, RHS1, 1, 2, E3, F3);
    } else {
      for (int n = 0; n < nt; n++) {
        double *TN = m->TRACER[n][m->newtime] + o3; const double *TO = m->TRACER[n][m->oldtime] + o3;
        for (size_t p = 0; p < n2; p++)
          if (m->KMT[o2 + p] > 0) TN[p] = TN[p] - TO[p] * (PN[p] - PM[p]) / (orc_grav * m->dz[1]);
      }
      impvmixt(m, b, tn, to, PN, NULL, 1, nt, E3, F3);
    }
    if (c->reset_to_freezing) {
      double *TN = m->TRACER[0][m->newtime] + o3;
      for (size_t p = 0; p < n2; p++) TN[p] = TN[p] > -2.0 ? TN[p] : -2.0;
    }
    for (int k = 1; k <= km; k++) {
      size_t ok = (size_t)(k - 1) * n2;
      state_level(m, k, m->TRACER[0][m->newtime] + o3 + ok, m->TRACER[1][m->newtime] + o3 + ok, m->RHO[m->newtime] + o3 + ok, n2);
    }
  }
  free(RHS1); free(E3); free(F3);
}

#include "orc_rf.inc"

/* ---- step_mod.F90:467-832 halo updates, add barotropic, PGUESS, time-level
 *      update (averaging step or rotation) -------------------------------- */
void orc_step_tail(orc_model *m) {
  DECL_DIMS
  const int nt = m->nt;
  orc_halo(m, m->UBTROP[m->newtime], 1, ORC_NECORNER, ORC_VECTOR);
  orc_halo(m, m->VBTROP[m->newtime], 1, ORC_NECORNER, ORC_VECTOR);
  orc_halo(m, m->UVEL[m->newtime], km, ORC_NECORNER, ORC_VECTOR);
  orc_halo(m, m->VVEL[m->newtime], km, ORC_NECORNER, ORC_VECTOR);
  orc_halo(m, m->RHO[m->newtime], km, ORC_CENTER, ORC_SCALAR);
  for (int n = 0; n < nt; n++) orc_halo(m, m->TRACER[n][m->newtime], km, ORC_CENTER, ORC_SCALAR);
  for (int b = 0; b < m->nblocks; b++) {
    DECL_BLK
    double *UN = m->UVEL[m->newtime] + o3, *VN = m->VVEL[m->newtime] + o3;
    for (int k = 1; k <= km; k++) for (size_t p = 0; p < n2; p++)
      if (k <= m->KMU[o2 + p]) {
        UN[(size_t)(k - 1) * n2 + p] = UN[(size_t)(k - 1) * n2 + p] + m->UBTROP[m->newtime][o2 + p];
        VN[(size_t)(k - 1) * n2 + p] = VN[(size_t)(k - 1) * n2 + p] + m->VBTROP[m->newtime][o2 + p];
      }
  }
  size_t a2 = n2 * m->nblocks, a3 = n3 * m->nblocks;
  for (size_t p = 0; p < a2; p++)
    m->PGUESS[p] = 3.0 * (m->PSURF[m->newtime][p] - m->PSURF[m->curtime][p]) + m->PSURF[m->oldtime][p];
  if (m->avg_ts) {
    int o = m->oldtime, c = m->curtime, nw = m->newtime;
#define AVG2(F) for (size_t p = 0; p < a2; p++) { F[o][p] = 0.5 * (F[o][p] + F[c][p]); } \
                for (size_t p = 0; p < a2; p++) { F[c][p] = 0.5 * (F[c][p] + F[nw][p]); }
    for (size_t p = 0; p < a2; p++) m->UBTROP[o][p] = 0.5 * (m->UBTROP[o][p] + m->UBTROP[c][p]);
    for (size_t p = 0; p < a2; p++) m->VBTROP[o][p] = 0.5 * (m->VBTROP[o][p] + m->VBTROP[c][p]);
    for (size_t p = 0; p < a2; p++) m->UBTROP[c][p] = 0.5 * (m->UBTROP[c][p] + m->UBTROP[nw][p]);
    for (size_t p = 0; p < a2; p++) m->VBTROP[c][p] = 0.5 * (m->VBTROP[c][p] + m->VBTROP[nw][p]);
    AVG2(m->GRADPX) AVG2(m->GRADPY)
    for (size_t p = 0; p < a2; p++) m->FW_OLD[p] = 0.5 * (m->FW[p] + m->FW_OLD[p]);
    for (size_t p = 0; p < a3; p++) m->UVEL[o][p] = 0.5 * (m->UVEL[o][p] + m->UVEL[c][p]);
    for (size_t p = 0; p < a3; p++) m->VVEL[o][p] = 0.5 * (m->VVEL[o][p] + m->VVEL[c][p]);
    for (size_t p = 0; p < a3; p++) m->UVEL[c][p] = 0.5 * (m->UVEL[c][p] + m->UVEL[nw][p]);
    for (size_t p = 0; p < a3; p++) m->VVEL[c][p] = 0.5 * (m->VVEL[c][p] + m->VVEL[nw][p]);
    for (int b = 0; b < m->nblocks; b++) {
      DECL_BLK
      const double *PO = m->PSURF[o] + o2, *PC = m->PSURF[c] + o2, *PN = m->PSURF[nw] + o2;
      for (int n = 0; n < nt; n++) {
        double *TO = m->TRACER[n][o] + o3, *TC = m->TRACER[n][c] + o3; const double *TN = m->TRACER[n][nw] + o3;
        for (int k = 2; k <= km; k++) for (size_t p = 0; p < n2; p++) {
          size_t q = (size_t)(k - 1) * n2 + p;
          TO[q] = 0.5 * (TO[q] + TC[q]);
          TC[q] = 0.5 * (TC[q] + TN[q]);
        }
        for (size_t p = 0; p < n2; p++) {
          double PFO = 0.5 * (PO[p] + PC[p]), PFC = 0.5 * (PC[p] + PN[p]);
          double wmin = TO[p] < TC[p] ? TO[p] : TC[p], wmax = TO[p] > TC[p] ? TO[p] : TC[p];
          double t = 0.5 * ((m->dz[1] + PO[p] / orc_grav) * TO[p] + (m->dz[1] + PC[p] / orc_grav) * TC[p]);
          t = t / (m->dz[1] + PFO / orc_grav);
          if (t < wmin) t = wmin;
          if (t > wmax) t = wmax;
          TO[p] = t;
          wmin = TC[p] < TN[p] ? TC[p] : TN[p]; wmax = TC[p] > TN[p] ? TC[p] : TN[p];
          t = 0.5 * ((m->dz[1] + PC[p] / orc_grav) * TC[p] + (m->dz[1] + PN[p] / orc_grav) * TN[p]);
          t = t / (m->dz[1] + PFC / orc_grav);
          if (t < wmin) t = wmin;
          if (t > wmax) t = wmax;
          TC[p] = t;
        }
      }
      for (size_t p = 0; p < n2; p++) {
        double PFO = 0.5 * (PO[p] + PC[p]), PFC = 0.5 * (PC[p] + PN[p]);
        m->PSURF[o][o2 + p] = PFO; m->PSURF[c][o2 + p] = PFC;
      }
      for (int k = 1; k <= km; k++) {
        size_t ok = (size_t)(k - 1) * n2;
        state_level(m, k, m->TRACER[0][o] + o3 + ok, m->TRACER[1][o] + o3 + ok, m->RHO[o] + o3 + ok, n2);
        state_level(m, k, m->TRACER[0][c] + o3 + ok, m->TRACER[1][c] + o3 + ok, m->RHO[c] + o3 + ok, n2);
      }
      for (size_t p = 0; p < n2; p++) m->PGUESS[o2 + p] = 0.5 * (m->PGUESS[o2 + p] + m->PSURF[nw][o2 + p]);
    }
#undef AVG2
  } else if (m->c.tmix_opt == 3) {   /* step_mod.F90:798-802 */
    step_RF(m);
  } else {
    memcpy(m->FW_OLD, m->FW, a2 * sizeof(double));
    int tmp = m->oldtime; m->oldtime = m->curtime; m->curtime = m->newtime; m->newtime = tmp;
  }
}

int orc_step(orc_model *m) {
  orc_time_manager(m);
  orc_dhdt(m);
  int e = orc_baroclinic_driver(m);
  if (e) return e;
  e = orc_barotropic_driver(m);
  if (e) return e;
  orc_baroclinic_correct_adjust(m);
  orc_step_tail(m);
  return 0;
}
