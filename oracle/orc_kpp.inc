/* orc_kpp.inc -- native KPP vertical mixing of the reference (the `.not. lcvmix` branches of
 * source/vmix_kpp.F90), restated for the CPU oracle.  TEST INFRASTRUCTURE ONLY.
 *
 * Selections (SURVEY.md 8c): lcvmix=.false., lniw_mixing=.false., linertial=.false., langmuir off, SMFT available
 * (forcing_ws.F90:307).  ltidal_mixing (Jayne) and lhoriz_varying_bckgrnd after their init calls: orc_tidal.inc.
 * The CVMix path (the CESM default) lives in an un-vendored third party (CVMix v0.98-beta,
 * Externals_POP.cfg:1-6): parity for it is unpinned; this is the path testmod pop/no_cvmix runs.
 * Diagnostic outputs HMXL, HMXL_DR: with kpp_ml_diagnostics = 1; tavg fields are not computed.
 *
 * Integer powers follow the usual compiler expansion: x**2 = x*x, x**3 = (x*x)*x,
 * x**4 = (x*x)*(x*x).
 */
typedef struct {
  double *bckgrnd_vdc, *bckgrnd_vvc, *zgrid, *hwide, *Ricr;   /* vertical, zgrid/hwide 0..km+1 */
  double Vtc, cg;
} orc_kpp;
/* short-wave absorption tables (sw_absorption.F90): sw_absorb(0:km) of 'top-layer' / 'jerlov' (:355-370); for 'chlorophyll'
 * (:120-230, 525-728) the transmission table Tr(0:2km, 0:400) over the levels ztr (mid-points and interfaces) and 401
 * chlorophyll amounts between 0.001 and 10 mg/m^3.  Used by KPP (lshort_wave) and by add_sw_absorb (tracer_update). */
typedef struct { double *swabs, *ztr, *Tr, chlmin, chlmax, dlogchl; } orc_sw;

static const double kpp_epssfc = 0.1, kpp_Riinfty = 0.8, kpp_Rrho0 = 2.55, kpp_dsfmax = 1.0, kpp_cstar = 10.0,
  kpp_zeta_m = -0.2, kpp_zeta_s = -1.0, kpp_c_m = 8.38, kpp_c_s = 98.96, kpp_a_m = 1.26, kpp_a_s = -28.86,
  kpp_concv = 1.7, kpp_vonkar = 0.4, kpp_eps = 1.0e-10, kpp_eps2 = 1.0e-20, kpp_cekman = 0.7, kpp_cmonob = 1.0;

static void init_sw(orc_model *m);
/* vmix_kpp.F90:458-459, 530-539, 621-626, 641 */
static void init_vmix_kpp(orc_model *m) {
  const orc_config *c = &m->c;
  int km = m->km;
  orc_kpp *K = (orc_kpp *)calloc(1, sizeof(orc_kpp));
  m->kpp = K;
  K->bckgrnd_vdc = dalloc(km + 3); K->bckgrnd_vvc = dalloc(km + 3); K->zgrid = dalloc(km + 3);
  K->hwide = dalloc(km + 3); K->Ricr = dalloc(km + 3);
  K->Vtc = sqrt(0.2 / kpp_c_s / kpp_epssfc) / (kpp_vonkar * kpp_vonkar);
  K->cg = kpp_cstar * kpp_vonkar * pow(kpp_c_s * kpp_vonkar * kpp_epssfc, 1.0 / 3.0);
  K->zgrid[0] = kpp_eps; K->hwide[0] = kpp_eps;
  for (int k = 1; k <= km; k++) { K->zgrid[k] = -m->zt[k]; K->hwide[k] = m->dz[k]; }
  K->zgrid[km + 1] = -m->zw[km]; K->hwide[km + 1] = kpp_eps;
  for (int k = 1; k <= km; k++) {
    K->bckgrnd_vdc[k] = c->bckgrnd_vdc1 + c->bckgrnd_vdc2 * atan(c->bckgrnd_vdc_linv * (m->zw[k] - c->bckgrnd_vdc_dpth));
    K->bckgrnd_vvc[k] = c->Prandtl * K->bckgrnd_vdc[k];
    K->Ricr[k] = 0.3;
  }
  if (c->lshort_wave) init_sw(m);
}
static void free_vmix_kpp(orc_model *m) {
  orc_kpp *K = (orc_kpp *)m->kpp;
  if (!K) return;
  free(K->bckgrnd_vdc); free(K->bckgrnd_vvc); free(K->zgrid); free(K->hwide); free(K->Ricr); free(K);
  m->kpp = NULL;
}

/* sw_absorb_frac (sw_absorption.F90:736-811): fraction of the surface short-wave flux that penetrates to `depth` (cm, > 0)
 * in Jerlov water type jt = 1..5 (I, IA, IB, II, III); two-band model of Simpson and Paulson (1977), zero below 200 m */
static double sw_absorb_frac(double depth, int jt) {
  static const double rfac[5] = {0.58, 0.62, 0.67, 0.77, 0.78}, depth1[5] = {0.35, 0.60, 1.00, 1.50, 1.40},
                      depth2[5] = {23.0, 20.0, 17.0, 14.0, 7.90};
  const double depth_neg_meters = -depth * 0.01;
  if (depth_neg_meters < -200.0) return 0.0;
  return rfac[jt - 1] * exp(depth_neg_meters / depth1[jt - 1]) + (1.0 - rfac[jt - 1]) * exp(depth_neg_meters / depth2[jt - 1]);
}
/* Ohlmann (2003) two-band fit of the solar transmission for 31 chlorophyll amounts: published table as the reference holds
 * it (sw_absorption.F90:135-216): transmission to depth z (m) = A_1 exp(-B_1 z) + A_2 exp(-B_2 z) */
#define ORC_NCHL 31
#define ORC_NSUB 400
static const double chl_cnc[ORC_NCHL] = {.001, .005, .01, .02, .03, .05, .10, .15, .20, .25, .30, .35, .40, .45, .50, .60, .70, .80, .90,
  1.00, 1.50, 2.00, 2.50, 3.00, 4.00, 5.00, 6.00, 7.00, 8.00, 9.00, 10.00};
static const double chl_A1[ORC_NCHL] = {0.4421, 0.4451, 0.4488, 0.4563, 0.4622, 0.4715, 0.4877, 0.4993, 0.5084, 0.5159, 0.5223, 0.5278,
  0.5326, 0.5369, 0.5408, 0.5474, 0.5529, 0.5576, 0.5615, 0.5649, 0.5757, 0.5802, 0.5808, 0.5788, 0.56965, 0.55638, 0.54091, 0.52442,
  0.50766, 0.49110, 0.47505};
static const double chl_A2[ORC_NCHL] = {0.2981, 0.2963, 0.2940, 0.2894, 0.2858, 0.2800, 0.2703, 0.2628, 0.2571, 0.2523, 0.2481, 0.2444,
  0.2411, 0.2382, 0.2356, 0.2309, 0.2269, 0.2235, 0.2206, 0.2181, 0.2106, 0.2089, 0.2113, 0.2167, 0.23357, 0.25504, 0.27829, 0.30274,
  0.32698, 0.35056, 0.37303};
static const double chl_B1[ORC_NCHL] = {0.0287, 0.0301, 0.0319, 0.0355, 0.0384, 0.0434, 0.0532, 0.0612, 0.0681, 0.0743, 0.0800, 0.0853,
  0.0902, 0.0949, 0.0993, 0.1077, 0.1154, 0.1227, 0.1294, 0.1359, 0.1640, 0.1876, 0.2082, 0.2264, 0.25808, 0.28498, 0.30844, 0.32932,
  0.34817, 0.36540, 0.38132};
static const double chl_B2[ORC_NCHL] = {0.3192, 0.3243, 0.3306, 0.3433, 0.3537, 0.3705, 0.4031, 0.4262, 0.4456, 0.4621, 0.4763, 0.4889,
  0.4999, 0.5100, 0.5191, 0.5347, 0.5477, 0.5588, 0.5682, 0.5764, 0.6042, 0.6206, 0.6324, 0.6425, 0.66172, 0.68144, 0.70086, 0.72144,
  0.74178, 0.76190, 0.78155};
static double sw_absorb_frac(double depth, int jt);
/* init_sw_absorption (:355-370) and set_chl_trn (sw_absorption.F90:650-716) */
static void init_sw(orc_model *m) {
  if (m->sw) return;
  orc_sw *K = (orc_sw *)calloc(1, sizeof(orc_sw));
  m->sw = K;
  const int km = m->km, ksol = 2 * km;
  K->swabs = dalloc(km + 1);
  K->swabs[0] = 1.0;
  if (m->c.sw_absorption_type == 1)
    for (int k = 1; k <= km - 1; k++) K->swabs[k] = sw_absorb_frac(m->zw[k], m->c.jerlov_water_type ? m->c.jerlov_water_type : 3);
  if (m->c.sw_absorption_type != 2) return;
  /* no chlorophyll forcing file here: a uniform 0.25 mg/m^3 until the caller sets the field "CHL" */
  for (size_t p = 0; p < m->n2 * m->nblocks; p++) m->CHL[p] = 0.25;
  K->ztr = dalloc(ksol + 1); K->Tr = dalloc((size_t)(ksol + 1) * (ORC_NSUB + 1));
  K->ztr[0] = 0.0;
  for (int k = 1; k <= km; k++) { K->ztr[2 * k - 1] = m->zt[k]; K->ztr[2 * k] = m->zw[k]; }
  K->chlmin = chl_cnc[0]; K->chlmax = chl_cnc[ORC_NCHL - 1];
  K->dlogchl = (log10(K->chlmax) - log10(K->chlmin)) / (double)ORC_NSUB;
  double logchl = log10(K->chlmin) - K->dlogchl;
  for (int n = 0; n <= ORC_NSUB; n++) {
    logchl = logchl + K->dlogchl;
    const double chlamnt = pow(10.0, logchl);
    int mc = -1;
    for (int q = 0; q < ORC_NCHL - 1; q++) if (chl_cnc[q] <= chlamnt && chlamnt <= chl_cnc[q + 1]) { mc = q; break; }
    if (mc < 0) mc = (chlamnt < chl_cnc[0]) ? 0 : ORC_NCHL - 2;   /* the reference aborts here; rounding at the ends of the range only */
    const double w2 = (chlamnt - chl_cnc[mc]) / (chl_cnc[mc + 1] - chl_cnc[mc]), w1 = 1.0 - w2;
    const double A1 = chl_A1[mc] * w1 + chl_A1[mc + 1] * w2, A2 = chl_A2[mc] * w1 + chl_A2[mc + 1] * w2;
    const double B1 = chl_B1[mc] * w1 + chl_B1[mc + 1] * w2, B2 = chl_B2[mc] * w1 + chl_B2[mc + 1] * w2;
    double *Trn = K->Tr + (size_t)n * (ksol + 1);
    Trn[0] = 1.0;
    for (int k = 1; k <= ksol; k++) {
      double arg = B1 * K->ztr[k] * 0.01; arg = arg < 35.0 ? arg : 35.0;
      Trn[k] = A1 * exp(-arg);
      arg = B2 * K->ztr[k] * 0.01; arg = arg < 35.0 ? arg : 35.0;
      Trn[k] = Trn[k] + A2 * exp(-arg);
    }
  }
}
/* set_chl (:500-512): table column of a chlorophyll amount (the assignment to an integer array truncates) */
static int chl_index(const orc_sw *K, double chl) {
  chl = chl > K->chlmin ? chl : K->chlmin;
  chl = chl < K->chlmax ? chl : K->chlmax;
  int idx = (int)(log10(chl / K->chlmin) / K->dlogchl);
  if (idx < 0) idx = 0;
  if (idx > ORC_NSUB) idx = ORC_NSUB;
  return idx;
}
/* sw_trans_chl (:951-1047): kin > 0: transmission to level kin of ztr; kin = 0: interpolated to depth ztrans */
static double sw_trans_chl(const orc_model *m, const orc_sw *K, int kin, double ztrans, int idx) {
  const int ksol = 2 * m->km;
  const double *Trn = K->Tr + (size_t)idx * (ksol + 1);
  if (kin > 0) return Trn[kin];
  int kindx = ksol - 1;
  double w1 = 0.0, w2 = 0.0;   /* the reference leaves the weights of the previous call where no interval matches (depth >= ztr(ksol)) */
  for (int k = 1; k <= ksol; k++)
    if (K->ztr[k - 1] <= ztrans && ztrans < K->ztr[k]) {
      w2 = (ztrans - K->ztr[k - 1]) / (K->ztr[k] - K->ztr[k - 1]);
      w1 = 1.0 - w2;
      kindx = k - 1;
    }
  return w1 * Trn[kindx] + w2 * Trn[kindx + 1];
}
/* surface buoyancy forcing with the radiative contribution down to `depth` (vmix_kpp.F90:2236-2256, 2387-2412, 2707-2742):
 * sw_absorption_type = sw_absorption_type 0 'top-layer', 1 'jerlov' (water type jerlov_water_type, 0 = 3) */
static double kpp_bfsfc(const orc_model *m, double bo, double bosol, double depth, int kin, int chlidx) {
  const orc_config *c = &m->c;
  if (!c->lshort_wave) return bo;
  if (c->sw_absorption_type == 0) return bo + bosol;
  if (c->sw_absorption_type == 2) return bo + bosol * (1.0 - sw_trans_chl(m, (const orc_sw *)m->sw, kin, depth, chlidx));   /* 'chlorophyll' */
  return bo + bosol * (1.0 - sw_absorb_frac(depth, c->jerlov_water_type ? c->jerlov_water_type : 3));
}
/* state over a level with optional derivatives (RHOFULL, DRHODT, DRHODS) */
static void kstate(orc_model *m, int kk, const double *T, const double *S, double *R, double *DT, double *DS, size_t n) {
  orc_state(m, kk, kk, T, S, R, DT, DS, (int)n);
}

/* vmix_kpp.F90:3234-3337 wscale; m_or_s: 1 wm, 2 ws, 3 both */
static void kpp_wscale(size_t n2, const double *SIGMA, const double *HBL, const double *USTAR, const double *BFSFC,
                       int m_or_s, double *WM, double *WS) {
  for (size_t p = 0; p < n2; p++) {
    double ZETAH = SIGMA[p] * HBL[p] * kpp_vonkar * BFSFC[p];
    double u3 = (USTAR[p] * USTAR[p]) * USTAR[p];
    double ZETA = ZETAH / (u3 + kpp_eps);
    if (m_or_s == 1 || m_or_s == 3) {
      if (ZETA >= 0.0) WM[p] = kpp_vonkar * USTAR[p] / (1.0 + 5.0 * ZETA);
      else if (ZETA >= kpp_zeta_m) WM[p] = kpp_vonkar * USTAR[p] * pow(1.0 - 16.0 * ZETA, 0.25);
      else WM[p] = kpp_vonkar * pow(kpp_a_m * u3 - kpp_c_m * ZETAH, 1.0 / 3.0);
    }
    if (m_or_s == 2 || m_or_s == 3) {
      if (ZETA >= 0.0) WS[p] = kpp_vonkar * USTAR[p] / (1.0 + 5.0 * ZETA);
      else if (ZETA >= kpp_zeta_s) WS[p] = kpp_vonkar * USTAR[p] * sqrt(1.0 - 16.0 * ZETA);
      else WS[p] = kpp_vonkar * pow(kpp_a_s * u3 - kpp_c_s * ZETAH, 1.0 / 3.0);
    }
  }
}

/* vmix_coeffs_kpp (vmix_kpp.F90:918-1310) for block b: fills VDC[0..1] (0:km+1), VVC, KPP_SRC,
 * HBLT, KBL */
static void vmix_coeffs_kpp(orc_model *m, int b) {
  DECL_DIMS DECL_BLK
  const orc_config *c = &m->c;
  orc_kpp *K = (orc_kpp *)m->kpp;
  const double *zgrid = K->zgrid, *hwide = K->hwide;
  const double *T = m->TRACER[0][m->mixtime] + o3, *S = m->TRACER[1][m->mixtime] + o3;
  const double *UUU = m->UVEL[m->mixtime] + o3, *VVV = m->VVEL[m->mixtime] + o3;
  double *VDC1 = VDCP(0, b), *VDC2 = VDCP(1, b), *VVC = m->VVC + o3;
  const int *KMT = m->KMT + o2, *KMU = m->KMU + o2;
  const size_t nk = (size_t)(km + 2) * n2;
  /* partial bottom cells: level thicknesses of this block (0:km+1), else NULL */
  const double *DZT = PBC ? DZTP(b) : NULL, *DZU = PBC ? DZUP(b) : NULL;
#define L3(A, k) ((A) + (size_t)((k)-1) * n2)      /* level k of a 1..km array   */
#define L0(A, k) ((A) + (size_t)(k) * n2)          /* level k of a 0..km+1 array */
  double *TEMPMASK = dalloc(n3), *DBLOC = dalloc(n3), *DBSFC = dalloc(n3), *RHOSUM = dalloc(n3), *GHAT = dalloc(n3);
  double *VISC = dalloc(nk), *WORK0 = dalloc(nk), *RI_LOC = dalloc(n3), *FRI = dalloc(n3), *VSH3 = dalloc(n3);
  double *BLMC = dalloc(3 * n3);
  double *W = dalloc(n2 * 48), *w = W;
#define TK ((w += n2) - n2)
  double *RHOKM = TK, *RHOK = TK, *RHOAVG = TK, *WORK1 = TK, *WORK2 = TK, *USTAR = TK, *BFSFC = TK, *STABLE = TK;
  double *RHO1 = TK, *TALPHA = TK, *SBETA = TK, *BO = TK, *BOSOL = TK, *ZKL = TK, *HBLT = TK, *UREF = TK, *VREF = TK;
  double *WORK = TK, *VSHEAR = TK, *SIGMA = TK, *WM = TK, *WS = TK, *B_FRQNCY = TK, *CASEA = TK, *F1 = TK, *DELHAT = TK;
  double *RIB = TK; (void)TK; (void)TK;   /* RI_BULK(:,:,3) */
  double *GAT1 = TK; (void)TK; (void)TK;
  double *DAT1 = TK; (void)TK; (void)TK;
  double *DKM1 = TK; (void)TK; (void)TK;
  double *TA2 = TK, *SB2 = TK, *TA3 = TK, *SB3 = TK, *FCON = TK;
  int *KBL = m->KBL + o2, *KN = ialloc(n2);

  /* ---------------- buoydiff (vmix_kpp.F90:3575-3621) ---------------- */
  for (size_t p = 0; p < n3; p++) TEMPMASK[p] = (T[p] < -2.0) ? -2.0 : T[p];
  for (size_t p = 0; p < n2; p++) L3(DBSFC, 1)[p] = 0.0;
  for (int k = 2; k <= km; k++) {
    kstate(m, k, L3(TEMPMASK, k - 1), L3(S, k - 1), RHOKM, NULL, NULL, n2);
    kstate(m, k, L3(TEMPMASK, k), L3(S, k), RHOK, NULL, NULL, n2);
    double SURFTHICK = kpp_epssfc * m->zt[k];
    int kref = k;
    for (int ktmp = 1; ktmp <= k; ktmp++) {
      kstate(m, k, L3(TEMPMASK, ktmp), L3(S, ktmp), L3(RHOSUM, ktmp), NULL, NULL, n2);
      if (m->zw[ktmp] >= SURFTHICK) { kref = ktmp; break; }
    }
    if (kref == 1) memcpy(RHOAVG, L3(RHOSUM, 1), n2 * sizeof(double));
    else {
      for (size_t p = 0; p < n2; p++) RHOAVG[p] = L3(RHOSUM, kref)[p] * (SURFTHICK - m->zw[kref - 1]);
      for (int ktmp = 1; ktmp <= kref - 1; ktmp++)
        for (size_t p = 0; p < n2; p++) RHOAVG[p] = RHOAVG[p] + m->dz[ktmp] * L3(RHOSUM, ktmp)[p];
      for (size_t p = 0; p < n2; p++) RHOAVG[p] = RHOAVG[p] / SURFTHICK;
    }
    for (size_t p = 0; p < n2; p++) {
      if (RHOK[p] != 0.0) {
        L3(DBSFC, k)[p] = orc_grav * (1.0 - RHOAVG[p] / RHOK[p]);
        L3(DBLOC, k - 1)[p] = orc_grav * (1.0 - RHOKM[p] / RHOK[p]);
      } else { L3(DBSFC, k)[p] = 0.0; L3(DBLOC, k - 1)[p] = 0.0; }
      if (k - 1 >= KMT[p]) L3(DBLOC, k - 1)[p] = 0.0;
    }
  }
  for (size_t p = 0; p < n2; p++) L3(DBLOC, km)[p] = 0.0;

  /* ---------------- ri_iwmix (vmix_kpp.F90:1505-1603, 1774-1929, 1978-1986) -------------- */
  for (size_t p = 0; p < n2; p++) L0(WORK0, 0)[p] = 0.0;
  for (int k = 1; k <= km; k++) {
    if (k < km) {
      for (size_t p = 0; p < n2; p++) {
        double du = L3(UUU, k)[p] - L3(UUU, k + 1)[p], dv = L3(VVV, k)[p] - L3(VVV, k + 1)[p];
        WORK1[p] = du * du + dv * dv;
        if (PBC) { const double h = 0.5 * (DZL(DZU, p, k) + DZL(DZU, p, k + 1)); WORK1[p] = WORK1[p] / (h * h); }   /* :1531-1533 */
      }
      ugrid_to_tgrid(m, b, L3(VSH3, k), WORK1);
    } else for (size_t p = 0; p < n2; p++) L3(VSH3, k)[p] = 0.0;
    for (size_t p = 0; p < n2; p++) {
      if (PBC) {   /* :1553-1563 */
        if (k < km) {
          const double h = 0.5 * (DZL(DZT, p, k) + DZL(DZT, p, k + 1));
          L3(RI_LOC, k)[p] = L3(DBLOC, k)[p] / (L3(VSH3, k)[p] + kpp_eps / (h * h)) / h;
        } else {
          const double h = 0.5 * DZL(DZT, p, k);
          L3(RI_LOC, k)[p] = L3(DBLOC, k)[p] / (L3(VSH3, k)[p] + kpp_eps / (h * h)) / h;
        }
      } else
      L3(RI_LOC, k)[p] = L3(DBLOC, k)[p] * (zgrid[k] - zgrid[k + 1]) / (L3(VSH3, k)[p] + kpp_eps);
      L0(WORK0, k)[p] = (k <= KMT[p]) ? L3(RI_LOC, k)[p] : L0(WORK0, k - 1)[p];
    }
  }
  for (int n = 1; n <= c->num_v_smooth_Ri; n++) {
    for (size_t p = 0; p < n2; p++) { WORK1[p] = 0.25 * L0(WORK0, 1)[p]; L0(WORK0, km + 1)[p] = L0(WORK0, km)[p]; }
    for (int k = 1; k <= km; k++)
      for (size_t p = 0; p < n2; p++) {
        L3(RI_LOC, k)[p] = L0(WORK0, k)[p];
        if (KMT[p] >= 3) L0(WORK0, k)[p] = WORK1[p] + 0.5 * L3(RI_LOC, k)[p] + 0.25 * L0(WORK0, k + 1)[p];
        WORK1[p] = 0.25 * L3(RI_LOC, k)[p];
      }
    for (int k = 1; k <= km; k++)
      for (size_t p = 0; p < n2; p++) {
        double v = L0(WORK0, k)[p]; v = v > 0.0 ? v : 0.0;
        v = v / kpp_Riinfty;
        L3(FRI, k)[p] = v < 1.0 ? v : 1.0;
      }
  }
  /* the background at level k of cell p: the vertical profile, or after orc_init_kpp_bckgrnd the 2-D field the reference copies to every level */
  const orc_bck *BCK = (const orc_bck *)m->bck;
  const double *BV2 = (BCK && BCK->VDC) ? BCK->VDC + o2 : NULL, *BM2 = (BCK && BCK->VVC) ? BCK->VVC + o2 : NULL;
#define BVDC(k, p) (BV2 ? BV2[p] : K->bckgrnd_vdc[k])
#define BVVC(k, p) (BM2 ? BM2[p] : K->bckgrnd_vvc[k])
  const orc_tidal *TID = tidal_on(m);
  double *TD = NULL, *TN2 = NULL, *KVMIX = NULL, *KVMIX_M = NULL;
  if (TID) {   /* :1758-1759 */
    TD = TID->DIFF + o3; TN2 = TID->N2 + o3; KVMIX = TID->KVMIX + o3; KVMIX_M = TID->KVMIX_M + o3;
    for (size_t p = 0; p < n3; p++) { TD[p] = 0.0; TN2[p] = 0.0; KVMIX[p] = 0.0; KVMIX_M[p] = 0.0; }
  }
  for (int k = 1; k <= km; k++) {
    if (TID) {   /* :1791-1857 */
      for (size_t p = 0; p < n2; p++) {
        if (PBC) WORK1[p] = L3(DBLOC, k)[p] / (0.5 * (DZL(DZT, p, k) + DZL(DZT, p, k + 1)));
        else WORK1[p] = L3(DBLOC, k)[p] / (zgrid[k] - zgrid[k + 1]);
      }
      tidal_compute_diff(m, TID, b, k, WORK1, TD);
      const double tidal_mix_max = TID->nml.tidal_mix_max;
      for (size_t p = 0; p < n2; p++) {
        const double WORKN = BVVC(k, p);
        const double sm = WORKN / c->Prandtl + L3(TD, k)[p];
        const double W1 = c->Prandtl * (sm < tidal_mix_max ? sm : tidal_mix_max);
        if (k < km) {
          const double sd = BVDC(k, p) + L3(TD, k)[p];
          L0(VDC2, k)[p] = sd < tidal_mix_max ? sd : tidal_mix_max;
          /* the diagnostics KVMIX, KVMIX_M, TIDAL_N2 (:1830, 1841, 1961) hold 0 at and below the bottom level here, as the device's do;
           * the reference leaves the background sum there, which nothing reads */
          if (k < KMT[p]) { L3(KVMIX_M, k)[p] = W1; L3(KVMIX, k)[p] = L0(VDC2, k)[p]; L3(TN2, k)[p] = WORK1[p]; }
        }
        if (c->lrich) {
          double f = 1.0 - L3(FRI, k)[p] * L3(FRI, k)[p];
          double f3 = (f * f) * f;
          L0(VISC, k)[p] = W1 + c->kpp_rich_mix * f3;
          if (k < km) { L0(VDC2, k)[p] = L0(VDC2, k)[p] + c->kpp_rich_mix * f3; L0(VDC1, k)[p] = L0(VDC2, k)[p]; }
        } else {
          L0(VISC, k)[p] = W1;
          if (k < km) L0(VDC1, k)[p] = L0(VDC2, k)[p];
        }
      }
    } else
    for (size_t p = 0; p < n2; p++) {
      if (c->lrich) {
        double f = 1.0 - L3(FRI, k)[p] * L3(FRI, k)[p];
        double f3 = (f * f) * f;
        L0(VISC, k)[p] = BVVC(k, p) + c->kpp_rich_mix * f3;
        if (k < km) { L0(VDC2, k)[p] = BVDC(k, p) + c->kpp_rich_mix * f3; L0(VDC1, k)[p] = L0(VDC2, k)[p]; }
      } else {
        L0(VISC, k)[p] = BVVC(k, p);
        if (k < km) { L0(VDC2, k)[p] = BVDC(k, p); L0(VDC1, k)[p] = L0(VDC2, k)[p]; }
      }
    }
    for (size_t p = 0; p < n2; p++)
      if (k >= KMT[p]) { L0(VISC, k)[p] = 0.0; L0(VDC1, k)[p] = 0.0; L0(VDC2, k)[p] = 0.0; }
  }
#undef BVDC
#undef BVVC
  for (size_t p = 0; p < n2; p++) {
    L0(VISC, 0)[p] = 0.0; L0(VDC1, 0)[p] = 0.0; L0(VDC2, 0)[p] = 0.0;
    L0(VISC, km + 1)[p] = 0.0; L0(VDC1, km + 1)[p] = 0.0; L0(VDC2, km + 1)[p] = 0.0;
  }

  /* ---------------- ddmix (vmix_kpp.F90:3404-3497) ---------------- */
  if (c->ldbl_diff) {
    double *TAu = TA2, *SBu = SB2, *TAn = TA3, *SBn = SB3;
    for (size_t p = 0; p < n2; p++) WORK1[p] = (L3(T, 1)[p] < -2.0) ? -2.0 : L3(T, 1)[p];
    kstate(m, 1, WORK1, L3(S, 1), RHOK, TAu, SBu, n2);
    for (int k = 1; k <= km; k++) {
      if (k < km) {
        for (size_t p = 0; p < n2; p++) WORK1[p] = (L3(T, k + 1)[p] < -2.0) ? -2.0 : L3(T, k + 1)[p];
        kstate(m, k + 1, WORK1, L3(S, k + 1), RHOK, TAn, SBn, n2);
      }
      for (size_t p = 0; p < n2; p++) {
        double ALPHADT = 0.0, BETADS = 0.0;
        if (k < km) {
          ALPHADT = -0.5 * (TAu[p] + TAn[p]) * (L3(T, k)[p] - L3(T, k + 1)[p]);
          BETADS = 0.5 * (SBu[p] + SBn[p]) * (L3(S, k)[p] - L3(S, k + 1)[p]);
        }
        double RRHO, DIFFDD, PRANDTL;
        if (ALPHADT > BETADS && BETADS > 0.0) {   /* salt fingering */
          RRHO = ALPHADT / BETADS; RRHO = RRHO < kpp_Rrho0 ? RRHO : kpp_Rrho0;
          double f = 1.0 - (RRHO - 1.0) / (kpp_Rrho0 - 1.0);
          DIFFDD = kpp_dsfmax * ((f * f) * f);
          L0(VDC1, k)[p] = L0(VDC1, k)[p] + 0.7 * DIFFDD;
          L0(VDC2, k)[p] = L0(VDC2, k)[p] + DIFFDD;
        }
        if (ALPHADT < 0.0 && BETADS < 0.0 && ALPHADT > BETADS) {   /* diffusive convection */
          RRHO = ALPHADT / BETADS;
          DIFFDD = 1.5e-2 * 0.909 * exp(4.6 * exp(-0.54 * (1.0 / RRHO - 1.0)));
          PRANDTL = 0.15 * RRHO;
        } else { RRHO = 0.0; DIFFDD = 0.0; PRANDTL = 0.0; }
        if (RRHO > 0.5) PRANDTL = (1.85 - 0.85 / RRHO) * RRHO;
        L0(VDC1, k)[p] = L0(VDC1, k)[p] + DIFFDD;
        L0(VDC2, k)[p] = L0(VDC2, k)[p] + PRANDTL * DIFFDD;
      }
      if (k < km) { double *t = TAu; TAu = TAn; TAn = t; t = SBu; SBu = SBn; SBn = t; }
    }
  }

  /* chlorophyll index of the transmission table (set_chl, sw_absorption.F90:500-512) */
  int *CHLI = NULL;
  if (c->lshort_wave && c->sw_absorption_type == 2) {
    CHLI = ialloc(n2);
    for (size_t p = 0; p < n2; p++) CHLI[p] = chl_index((const orc_sw *)m->sw, m->CHL[o2 + p]);
  }
  /* ---------------- bldepth (vmix_kpp.F90:2140-2755) ---------------- */
  for (size_t p = 0; p < n2; p++) {
    double s1 = m->SMFT[0][o2 + p], s2 = m->SMFT[1][o2 + p];
    USTAR[p] = sqrt(sqrt(s1 * s1 + s2 * s2));
    USTAR[p] = USTAR[p] > kpp_eps ? USTAR[p] : kpp_eps;
    WORK[p] = (L3(T, 1)[p] < -2.0) ? -2.0 : L3(T, 1)[p];
  }
  kstate(m, 1, WORK, L3(S, 1), RHO1, TALPHA, SBETA, n2);
  for (size_t p = 0; p < n2; p++) {
    if (RHO1[p] != 0.0) {
      BO[p] = orc_grav * (-TALPHA[p] * m->STF[0][o2 + p] - SBETA[p] * m->STF[1][o2 + p]) / RHO1[p];
      BOSOL[p] = -orc_grav * TALPHA[p] * m->SHF_QSW[o2 + p] / RHO1[p];
    } else { BO[p] = 0.0; BOSOL[p] = 0.0; }
  }
  int kupper = 0, kup = 1, kdn = 2;
  double z_upper = 0.0, z_up = zgrid[1];
  for (size_t p = 0; p < n2; p++) { (RIB + kupper * n2)[p] = 0.0; (RIB + kup * n2)[p] = 0.0; KBL[p] = (KMT[p] > 1) ? KMT[p] : 1; }
  for (int kl = 1; kl <= km; kl++)
    for (size_t p = 0; p < n2; p++) {
      double zkl = -zgrid[kl];
      if (PBC) zkl = (kl > 1) ? -zgrid[kl - 1] + 0.5 * (DZL(DZT, p, kl) + DZL(DZT, p, kl - 1)) : -zgrid[1];   /* :2212-2220 */
      if (kl == KBL[p]) HBLT[p] = zkl;
    }
  /* lcheckekmo: Ekman and Monin-Obukhov depth limits under stable forcing (:2231-2265) */
  double *EKMO = c->lcheckekmo ? dalloc(5 * n2) : NULL;
  double *HEKMAN = EKMO, *HLIMIT = EKMO ? EKMO + n2 : NULL, *HMONOB = EKMO ? EKMO + 2 * n2 : NULL;   /* HMONOB(:,:,3) rotates with RI_BULK */
  if (c->lcheckekmo) {
    for (size_t p = 0; p < n2; p++) {
      HEKMAN[p] = -zgrid[km] + kpp_eps; HLIMIT[p] = -zgrid[km] + kpp_eps;
      double bf = kpp_bfsfc(m, BO[p], BOSOL[p], -z_up, 1, CHLI ? CHLI[p] : 0);
      const double st = (bf >= 0.0) ? 1.0 : 0.0;
      bf = bf + st * kpp_eps;
      const double w = st * kpp_cmonob * USTAR[p] * USTAR[p] * USTAR[p] / kpp_vonkar / bf + (st - 1.0) * zgrid[km];
      (HMONOB + kup * n2)[p] = (w <= -z_up) ? -z_up + kpp_eps : w;
    }
  }
  for (int kl = 2; kl <= km; kl++) {
    double SURFTHICK = kpp_epssfc * m->zt[kl];
    int kref = kl;
    for (int ktmp = 1; ktmp <= kl; ktmp++) if (m->zw[ktmp] >= SURFTHICK) { kref = ktmp; break; }
    if (kref > 1) {
      for (size_t p = 0; p < n2; p++) {
        UREF[p] = L3(UUU, kref)[p] * (SURFTHICK - m->zw[kref - 1]);
        VREF[p] = L3(VVV, kref)[p] * (SURFTHICK - m->zw[kref - 1]);
      }
      for (int ktmp = 1; ktmp <= kref - 1; ktmp++)
        for (size_t p = 0; p < n2; p++) {
          UREF[p] = UREF[p] + m->dz[ktmp] * L3(UUU, ktmp)[p];
          VREF[p] = VREF[p] + m->dz[ktmp] * L3(VVV, ktmp)[p];
        }
      for (size_t p = 0; p < n2; p++) { UREF[p] = UREF[p] / SURFTHICK; VREF[p] = VREF[p] / SURFTHICK; }
    } else { memcpy(UREF, L3(UUU, 1), n2 * sizeof(double)); memcpy(VREF, L3(VVV, 1), n2 * sizeof(double)); }
    for (size_t p = 0; p < n2; p++) {
      double du = UREF[p] - L3(UUU, kl)[p], dv = VREF[p] - L3(VVV, kl)[p];
      WORK[p] = du * du + dv * dv;
      ZKL[p] = -zgrid[kl];
      if (PBC) {   /* :2359-2366 */
        const double h = -zgrid[kl - 1] + 0.5 * (DZL(DZU, p, kl) + DZL(DZU, p, kl - 1) - DZL(DZU, p, 1));
        WORK[p] = WORK[p] / (h * h);
        ZKL[p] = -zgrid[kl - 1] + 0.5 * (DZL(DZT, p, kl) + DZL(DZT, p, kl - 1));
      }
    }
    for (int i = 1; i <= nxb; i++) VSHEAR[P2(i, 1)] = 0.0;
    for (int j = 2; j <= nyb; j++) {
      VSHEAR[P2(1, j)] = 0.0;
      for (int i = 2; i <= nxb; i++) {
        double v = WORK[P2(i, j)];
        if (WORK[P2(i - 1, j)] > v) v = WORK[P2(i - 1, j)];
        if (WORK[P2(i, j - 1)] > v) v = WORK[P2(i, j - 1)];
        if (WORK[P2(i - 1, j - 1)] > v) v = WORK[P2(i - 1, j - 1)];
        VSHEAR[P2(i, j)] = v;
      }
    }
    for (size_t p = 0; p < n2; p++) {
      BFSFC[p] = kpp_bfsfc(m, BO[p], BOSOL[p], ZKL[p], 2 * kl - 1, CHLI ? CHLI[p] : 0);
      STABLE[p] = (BFSFC[p] >= 0.0) ? 1.0 : 0.0;
      BFSFC[p] = BFSFC[p] + STABLE[p] * kpp_eps;
      SIGMA[p] = kpp_epssfc;
    }
    if (c->lcheckekmo)   /* :2426-2455 */
      for (size_t p = 0; p < n2; p++) {
        if (STABLE[p] > 0.5 && HEKMAN[p] >= -zgrid[km]) {
          const double e = kpp_cekman * USTAR[p] / (fabs(m->FCORT[o2 + p]) + kpp_eps);
          HEKMAN[p] = (ZKL[p] > e) ? ZKL[p] : e;
        }
        (HMONOB + kdn * n2)[p] = STABLE[p] * kpp_cmonob * USTAR[p] * USTAR[p] * USTAR[p] / kpp_vonkar / BFSFC[p] + (STABLE[p] - 1.0) * zgrid[km];
        if ((HMONOB + kdn * n2)[p] <= ZKL[p] && (HMONOB + kup * n2)[p] > -z_up) {
          const double w = ((HMONOB + kdn * n2)[p] - (HMONOB + kup * n2)[p]) / (z_up + ZKL[p]);
          HLIMIT[p] = ((HMONOB + kdn * n2)[p] - w * ZKL[p]) / (1.0 - w);
        }
      }
    kpp_wscale(n2, SIGMA, ZKL, USTAR, BFSFC, 2, WM, WS);
    for (size_t p = 0; p < n2; p++) {
      double db = L3(DBLOC, kl)[p];
      if (PBC) {   /* :2486-2496 */
        if (kl < km) B_FRQNCY[p] = sqrt(0.5 * (db + fabs(db) + kpp_eps2) / (0.5 * (DZL(DZT, p, kl) + DZL(DZT, p, kl + 1))));
        else B_FRQNCY[p] = sqrt(0.5 * (db + fabs(db) + kpp_eps2) / DZL(DZT, p, kl));
      } else
      B_FRQNCY[p] = sqrt(0.5 * (db + fabs(db) + kpp_eps2) / (zgrid[kl] - zgrid[kl + 1]));
      double ZREF = -SURFTHICK / 2.0;
      double t = 2.1 - 200.0 * B_FRQNCY[p]; t = t > kpp_concv ? t : kpp_concv;
      WM[p] = ZKL[p] * WS[p] * B_FRQNCY[p] * ((K->Vtc / K->Ricr[kl]) * t);
      if (PBC) {   /* :2561-2575 */
        const double ht = -zgrid[kl - 1] + 0.5 * (DZL(DZT, p, kl - 1) + DZL(DZT, p, kl) - DZL(DZT, p, 1));
        const double hu = -zgrid[kl - 1] + 0.5 * (DZL(DZU, p, kl) + DZL(DZU, p, kl - 1) - DZL(DZU, p, 1));
        const double wk = (KMT[p] >= kl) ? L3(DBSFC, kl)[p] / ht : 0.0;
        WM[p] = WM[p] / (ht * ht);
        (RIB + kdn * n2)[p] = wk / (VSHEAR[p] + WM[p] + kpp_eps / (hu * hu));
      } else {
      double wk = (KMT[p] >= kl) ? (ZREF - zgrid[kl]) * L3(DBSFC, kl)[p] : 0.0;
      (RIB + kdn * n2)[p] = wk / (VSHEAR[p] + WM[p] + kpp_eps);
      }
    }
    for (size_t p = 0; p < n2; p++) {
      double rdn = (RIB + kdn * n2)[p], rup = (RIB + kup * n2)[p], rupper = (RIB + kupper * n2)[p];
      if (KBL[p] == KMT[p] && rdn > K->Ricr[kl]) {
        double slope_up = (rupper - rup) / (z_up - z_upper);
        double d = z_up + ZKL[p];
        double a_co = (rdn - rup - slope_up * (ZKL[p] + z_up)) / (d * d);
        double b_co = slope_up + 2.0 * a_co * z_up;
        double c_co = rup + z_up * (a_co * z_up + slope_up) - K->Ricr[kl];
        double sqrt_arg = b_co * b_co - 4.0 * a_co * c_co;
        if ((fabs(b_co) > kpp_eps && fabs(a_co) / fabs(b_co) <= kpp_eps) || sqrt_arg <= 0.0)
          HBLT[p] = -z_up + (z_up + ZKL[p]) * (K->Ricr[kl] - rup) / (rdn - rup);
        else HBLT[p] = (-b_co + sqrt(sqrt_arg)) / (2.0 * a_co);
        KBL[p] = kl;
      }
    }
    int kt = kupper; kupper = kup; kup = kdn; kdn = kt;
    z_upper = z_up; z_up = zgrid[kl];
  }
  if (c->lcheckekmo) {   /* :2676-2690; ZKL still holds the last pass of the march, -zgrid(km), as in the reference */
    for (size_t p = 0; p < n2; p++) if (HEKMAN[p] < HLIMIT[p]) HLIMIT[p] = HEKMAN[p];
    for (int kl = 2; kl <= km; kl++)
      for (size_t p = 0; p < n2; p++)
        if (HLIMIT[p] < HBLT[p] && HLIMIT[p] > -zgrid[kl - 1] && HLIMIT[p] <= ZKL[p]) { HBLT[p] = HLIMIT[p]; KBL[p] = kl; }
    free(EKMO);
  }
  /* smooth_hblt(.true.,.false.) vmix_kpp.F90:3797-3870 */
  memcpy(WORK1, HBLT, n2 * sizeof(double));
  memcpy(WORK2, HBLT, n2 * sizeof(double));
  for (int j = 2; j <= nyb - 1; j++) for (int i = 2; i <= nxb - 1; i++)
    if (KMT[P2(i, j)] != 0) {
      double cw = 0.125, ce = 0.125, cn = 0.125, cs = 0.125, cc = 0.5;
      if (KMT[P2(i - 1, j)] == 0) { cc = cc + cw; cw = 0.0; }
      if (KMT[P2(i + 1, j)] == 0) { cc = cc + ce; ce = 0.0; }
      if (KMT[P2(i, j - 1)] == 0) { cc = cc + cs; cs = 0.0; }
      if (KMT[P2(i, j + 1)] == 0) { cc = cc + cn; cn = 0.0; }
      WORK2[P2(i, j)] = cw * WORK1[P2(i - 1, j)] + ce * WORK1[P2(i + 1, j)] + cs * WORK1[P2(i, j - 1)] +
                        cn * WORK1[P2(i, j + 1)] + cc * WORK1[P2(i, j)];
    }
  /* ztmp: -zgrid(k), or with partial bottom cells (:3835-3841, :3858-3864) -zgrid(k-1) + p5*(DZT(k-1) + DZT(k)) (DZT(0) = 0) */
#define ZTMP(i, j, k) (PBC ? -zgrid[(k) - 1] + 0.5 * (DZ3(DZT, i, j, (k) - 1) + DZ3(DZT, i, j, k)) : -zgrid[k])
  for (int k = 1; k <= km; k++)
    for (int j = 2; j <= nyb - 1; j++) for (int i = 2; i <= nxb - 1; i++)
      if (k == KMT[P2(i, j)] && WORK2[P2(i, j)] > ZTMP(i, j, k)) WORK2[P2(i, j)] = ZTMP(i, j, k);
  for (size_t p = 0; p < n2; p++) HBLT[p] = WORK2[p] > -zgrid[1] ? WORK2[p] : -zgrid[1];
  for (int k = 1; k <= km; k++)
    for (int j = 2; j <= nyb - 1; j++) for (int i = 2; i <= nxb - 1; i++)
      if (KMT[P2(i, j)] != 0 && HBLT[P2(i, j)] > -zgrid[k - 1] && HBLT[P2(i, j)] <= ZTMP(i, j, k)) KBL[P2(i, j)] = k > 2 ? k : 2;
#undef ZTMP
  /* BFSFC keeps the value of the last kl pass without short wave; with it: forcing down to the boundary layer depth
   * (vmix_kpp.F90:2707-2750) */
  for (size_t p = 0; p < n2; p++) {
    if (c->lshort_wave) BFSFC[p] = kpp_bfsfc(m, BO[p], BOSOL[p], HBLT[p], 0, CHLI ? CHLI[p] : 0);
    STABLE[p] = (BFSFC[p] >= 0.0) ? 1.0 : 0.0;
    BFSFC[p] = BFSFC[p] + STABLE[p] * kpp_eps;
  }
  memcpy(m->HBLT + o2, HBLT, n2 * sizeof(double));

  /* ---------------- blmix (vmix_kpp.F90:2900-3222) ---------------- */
  for (size_t p = 0; p < n2; p++) SIGMA[p] = kpp_epssfc;
  kpp_wscale(n2, SIGMA, HBLT, USTAR, BFSFC, 3, WM, WS);
  for (size_t p = 0; p < n2; p++) {
    int k = KBL[p];
    double x = -zgrid[k] - 0.5 * hwide[k] - HBLT[p];
    if (PBC) x = (k == 1) ? -zgrid[0] - HBLT[p] : -zgrid[k - 1] + 0.5 * DZL(DZT, p, k - 1) - HBLT[p];   /* :2911-2923 */
    CASEA[p] = 0.5 + (x >= 0.0 ? 0.5 : -0.5);
    int nc = (int)lround(CASEA[p]);
    KN[p] = nc * (KBL[p] - 1) + (1 - nc) * KBL[p];
    double u2 = USTAR[p] * USTAR[p];
    F1[p] = STABLE[p] * 5.0 * BFSFC[p] / (u2 * u2 + kpp_eps);
    for (int q = 0; q < 3; q++) { (GAT1 + q * n2)[p] = 0.0; (DAT1 + q * n2)[p] = 0.0; }
  }
  for (int k = 1; k <= km; k++)
    for (size_t p = 0; p < n2; p++)
      if (k == KN[p]) {
        double dh = 0.5 * hwide[k] - zgrid[k] - HBLT[p];
        double R = 1.0 - dh / hwide[k];
        double hup = hwide[k], hdn = hwide[k + 1];
        if (PBC) {   /* :2948-2973 */
          const double w1 = (k == 1) ? 0.0 : DZL(DZT, p, k - 1);
          hdn = (k == km) ? kpp_eps : DZL(DZT, p, k + 1);
          hup = DZL(DZT, p, k);
          dh = -zgrid[k - 1] + DZL(DZT, p, k) + 0.5 * w1 - HBLT[p];
          R = 1.0 - dh / DZL(DZT, p, k);
        }
        const double *F[3] = {VISC, VDC2, VDC1};
        double P_[3], H_[3];
        for (int q = 0; q < 3; q++) {
          double up = (L0(F[q], k - 1)[p] - L0(F[q], k)[p]) / hup;
          double dn = (L0(F[q], k)[p] - L0(F[q], k + 1)[p]) / hdn;
          P_[q] = 0.5 * ((1.0 - R) * (up + fabs(up)) + R * (dn + fabs(dn)));
          H_[q] = L0(F[q], k)[p] + P_[q] * dh;
        }
        (GAT1 + 0 * n2)[p] = H_[0] / HBLT[p] / (WM[p] + kpp_eps);
        (DAT1 + 0 * n2)[p] = -P_[0] / (WM[p] + kpp_eps) + F1[p] * H_[0];
        (GAT1 + 1 * n2)[p] = H_[1] / HBLT[p] / (WS[p] + kpp_eps);
        (DAT1 + 1 * n2)[p] = -P_[1] / (WS[p] + kpp_eps) + F1[p] * H_[1];
        (GAT1 + 2 * n2)[p] = H_[2] / HBLT[p] / (WS[p] + kpp_eps);
        (DAT1 + 2 * n2)[p] = -P_[2] / (WS[p] + kpp_eps) + F1[p] * H_[2];
      }
  for (size_t p = 0; p < 3 * n2; p++) DAT1[p] = DAT1[p] < 0.0 ? DAT1[p] : 0.0;
  for (int k = 1; k <= km; k++) {
    for (size_t p = 0; p < n2; p++) {
      SIGMA[p] = (-zgrid[k] + 0.5 * hwide[k]) / HBLT[p];
      if (PBC && k > 1) SIGMA[p] = (-zgrid[k - 1] + 0.5 * DZL(DZT, p, k - 1) + DZL(DZT, p, k)) / HBLT[p];   /* :3075-3083 */
      F1[p] = SIGMA[p] < kpp_epssfc ? SIGMA[p] : kpp_epssfc;
    }
    kpp_wscale(n2, F1, HBLT, USTAR, BFSFC, 3, WM, WS);
    for (size_t p = 0; p < n2; p++) {
      double s = SIGMA[p];
      for (int q = 0; q < 3; q++) {
        double wv = (q == 0) ? WM[p] : WS[p];
        (BLMC + q * n3 + (size_t)(k - 1) * n2)[p] = HBLT[p] * wv * s *
          (1.0 + s * ((s - 2.0) + (3.0 - 2.0 * s) * (GAT1 + q * n2)[p] + (s - 1.0) * (DAT1 + q * n2)[p]));
      }
      L3(GHAT, k)[p] = (1.0 - STABLE[p]) * K->cg / (WS[p] * HBLT[p] + kpp_eps);
    }
  }
  for (size_t p = 0; p < n2; p++) {
    int k = KBL[p] - 1;
    SIGMA[p] = -zgrid[k] / HBLT[p];
    F1[p] = SIGMA[p] < kpp_epssfc ? SIGMA[p] : kpp_epssfc;
  }
  kpp_wscale(n2, F1, HBLT, USTAR, BFSFC, 3, WM, WS);
  for (size_t p = 0; p < n2; p++) {
    double s = SIGMA[p];
    for (int q = 0; q < 3; q++) {
      double wv = (q == 0) ? WM[p] : WS[p];
      (DKM1 + q * n2)[p] = HBLT[p] * wv * s * (1.0 + s * ((s - 2.0) + (3.0 - 2.0 * s) * (GAT1 + q * n2)[p] + (s - 1.0) * (DAT1 + q * n2)[p]));
    }
  }
  for (int k = 1; k <= km - 1; k++)
    for (size_t p = 0; p < n2; p++)
      if (k == KBL[p] - 1) {
        double dh = (HBLT[p] + zgrid[k]) / (zgrid[k] - zgrid[k + 1]);
        if (PBC) {   /* :3155-3165 */
          const double w1 = (k == 1) ? -0.5 * DZL(DZT, p, k) : zgrid[k - 1] - 0.5 * (DZL(DZT, p, k - 1) + DZL(DZT, p, k));
          dh = (HBLT[p] + w1) / (0.5 * (DZL(DZT, p, k) + DZL(DZT, p, k + 1)));
        }
        DELHAT[p] = dh;
        const double *F[3] = {VISC, VDC2, VDC1};
        for (int q = 0; q < 3; q++) {
          double *bl = BLMC + q * n3 + (size_t)(k - 1) * n2;
          double omd = 1.0 - dh;
          bl[p] = omd * L0(F[q], k)[p] + dh * ((omd * omd) * (DKM1 + q * n2)[p] +
                  (dh * dh) * (CASEA[p] * L0(F[q], k)[p] + (1.0 - CASEA[p]) * bl[p]));
        }
        L3(GHAT, k)[p] = (1.0 - CASEA[p]) * L3(GHAT, k)[p];
      }
  for (int k = 1; k <= km; k++)
    for (size_t p = 0; p < n2; p++) {
      if (k < KBL[p]) {
        L0(VISC, k)[p] = (BLMC + 0 * n3 + (size_t)(k - 1) * n2)[p];
        L0(VDC2, k)[p] = (BLMC + 1 * n3 + (size_t)(k - 1) * n2)[p];
        L0(VDC1, k)[p] = (BLMC + 2 * n3 + (size_t)(k - 1) * n2)[p];
      } else L3(GHAT, k)[p] = 0.0;
    }

  /* ---------------- interior convection, U-grid viscosity (vmix_kpp.F90:1218-1262) -------- */
  for (int k = 1; k <= km - 1; k++) {
    for (size_t p = 0; p < n2; p++) {
      double N2 = L3(DBLOC, k)[p] / (zgrid[k] - zgrid[k + 1]);
      if (PBC) N2 = L3(DBLOC, k)[p] / (0.5 * (DZL(DZT, p, k) + DZL(DZT, p, k + 1)));   /* :1220-1222 */
      FCON[p] = (N2 > 0.0) ? 0.0 : 1.0;
      double cvv = 0.0, cvd = 0.0;
      if (k >= KBL[p]) { cvv = c->convect_visc * FCON[p]; cvd = c->convect_diff * FCON[p]; }
      if (k < KMT[p]) {
        L0(VISC, k)[p] = L0(VISC, k)[p] + cvv;
        L0(VDC1, k)[p] = L0(VDC1, k)[p] + cvd;
        L0(VDC2, k)[p] = L0(VDC2, k)[p] + cvd;
      } else { L0(VISC, k)[p] = 0.0; L0(VDC1, k)[p] = 0.0; L0(VDC2, k)[p] = 0.0; }
    }
    tgrid_to_ugrid(m, b, WORK2, L0(VISC, k));
    for (size_t p = 0; p < n2; p++) L3(VVC, k)[p] = (k < KMU[p]) ? WORK2[p] : 0.0;
  }
  for (size_t p = 0; p < n2; p++) { L0(VDC1, km)[p] = 0.0; L0(VDC2, km)[p] = 0.0; L3(VVC, km)[p] = 0.0; }

  /* ---------------- non-local source (vmix_kpp.F90:1283-1306) ---------------- */
  for (int n = 0; n < m->nt; n++) {
    const double *VD = (n == 0) ? VDC1 : VDC2;
    double *SRC = m->KPP_SRC[n] + o3;
    const double *STF = m->STF[n] + o2;
    for (size_t p = 0; p < n2; p++) L3(SRC, 1)[p] = STF[p] / m->dz[1] * (-L0(VD, 1)[p] * L3(GHAT, 1)[p]);
    for (int k = 2; k <= km; k++)
      for (size_t p = 0; p < n2; p++)
        L3(SRC, k)[p] = STF[p] / (PBC ? DZL(DZT, p, k) : m->dz[k]) * (L0(VD, k - 1)[p] * L3(GHAT, k - 1)[p] - L0(VD, k)[p] * L3(GHAT, k)[p]);   /* :1296-1302 */
  }
  /* ---------------- diagnostic mixed-layer depths (vmix_kpp.F90:1310-1418), kpp_ml_diagnostics = 1 ----------------
   * HMXL: depth of the maximum buoyancy gradient (USTAR, BFSFC and VISC are reused as work space there, here WORK0);
   * HMXL_DR: depth where the potential density exceeds the surface value by 3e-5 g/cm^3 */
  if (c->kpp_ml_diagnostics == 1) {
    double *HMXL = m->HMXL + o2, *HMXL_DR = m->HMXL_DR + o2, *GRD = WORK0;
    for (size_t p = 0; p < n2; p++) { USTAR[p] = 0.0; HMXL[p] = (KMT[p] == 1) ? m->zt[1] : 0.0; }
    for (int k = 2; k <= km; k++)
      for (size_t p = 0; p < n2; p++)
        if (k <= KMT[p]) {
          /* partial bottom cells (:1326-1332): the depth of the T point is built from the cell thicknesses */
          const double zk = PBC ? m->zt[k - 1] + 0.5 * (DZL(DZT, p, k - 1) + DZL(DZT, p, k)) : m->zt[k];
          const double q = L3(DBSFC, k)[p] / zk;
          USTAR[p] = (q > USTAR[p]) ? q : USTAR[p];
          HMXL[p] = zk;
        }
    for (size_t p = 0; p < n2; p++) L3(GRD, 1)[p] = 0.0;
    for (int k = 2; k <= km; k++)
      for (size_t p = 0; p < n2; p++) {
        const double dzk = PBC ? 0.5 * (DZL(DZT, p, k) + DZL(DZT, p, k - 1)) : (m->zt[k] - m->zt[k - 1]);   /* :1337-1338 | :1369-1370 */
        const double v = (USTAR[p] > 0.0) ? (L3(DBSFC, k)[p] - L3(DBSFC, k - 1)[p]) / dzk : 0.0;
        L3(GRD, k)[p] = v;
        if (v >= USTAR[p] && (v - L3(GRD, k - 1)[p]) != 0.0 && USTAR[p] > 0.0) {
          const double bf = (v - USTAR[p]) / (v - L3(GRD, k - 1)[p]);
          if (PBC)   /* :1350-1351 (DZT(0) = 0) */
            HMXL[p] = (m->zt[k - 1] + 0.25 * (DZL(DZT, p, k - 1) + DZL(DZT, p, k))) * (1.0 - bf) +
                      (m->zt[k - 1] - 0.25 * (DZL(DZT, p, k - 2) + DZL(DZT, p, k - 1))) * bf;
          else
            HMXL[p] = -0.5 * (zgrid[k] + zgrid[k - 1]) * (1.0 - bf) - 0.5 * (zgrid[k - 1] + zgrid[k - 2]) * bf;
          USTAR[p] = 0.0;
        }
      }
    for (size_t p = 0; p < n2; p++) { HMXL_DR[p] = (KMT[p] == 1) ? m->zt[1] : 0.0; WORK[p] = (KMT[p] == 1) ? 1.0 : 0.0; /* FLGMOD */ }
    orc_state(m, 1, 1, L3(TEMPMASK, 1), L3(S, 1), RHO1, NULL, NULL, (int)n2);
    for (size_t p = 0; p < n2; p++) { WORK2[p] = RHO1[p] + 3.0e-05; RHOK[p] = RHO1[p]; }
    for (int k = 1; k <= km - 1; k++) {
      orc_state(m, k + 1, 1, L3(TEMPMASK, k + 1), L3(S, k + 1), RHOKM, NULL, NULL, (int)n2);   /* RHOKP1 */
      for (size_t p = 0; p < n2; p++) {
        if (WORK2[p] > RHOK[p] && WORK2[p] <= RHOKM[p] && WORK[p] == 0.0) {
          HMXL_DR[p] = m->zt[k] + (WORK2[p] - RHOK[p]) * (m->zt[k + 1] - m->zt[k]) / (RHOKM[p] - RHOK[p] + kpp_eps);
          WORK[p] = 1.0;
        }
        RHOK[p] = RHOKM[p];
      }
    }
  }
#undef TK
#undef L3
#undef L0
  free(CHLI);
  free(TEMPMASK); free(DBLOC); free(DBSFC); free(RHOSUM); free(GHAT); free(VISC); free(WORK0); free(RI_LOC); free(FRI);
  free(VSH3); free(BLMC); free(W); free(KN);
}
