// kernels_tidal.hpp -- Jayne and St. Laurent (2001) tidal mixing inside KPP's interior coefficients: the ltidal_mixing branch of
// ri_iwmix (vmix_kpp.F90:1791-1857, without lniw_mixing) with tidal_compute_diff (tidal_mixing.F90:3046-3140) and the region
// minimum of tidal_min_regions_set (:3374-3429).  TIDAL_COEF_3D and the region boxes come from host_tidal.cpp.
//
// Arrangement: with tidal mixing on the interior kernels of kernels_kpp.hpp run with a background of zeros and write
//   VISC = rich_mix f3,  VDC = rich_mix f3 (+ double diffusion),  0 at k >= KMT,
// and k_kpp_tidal, launched behind them on the same stream and before k_kpp_blmix, adds
//   KVMIX_M = Prandtl min(bckgrnd_vvc / Prandtl + TIDAL_DIFF, tidal_mix_max)   to VISC,
//   KVMIX   = min(bckgrnd_vdc + TIDAL_DIFF, tidal_mix_max)                      to VDC.
// The reference forms WORK1 + rich_mix f3; a sum of two terms does not depend on their order, so without double diffusion the
// result is bitwise the reference's, with it within a rounding of the three-term sum.
#pragma once

namespace pop {

struct TidalDev {
  const double *COEF = nullptr;     // TIDAL_COEF_3D (nxb, nyb, km, nblocks)
  const int *BOX = nullptr;         // REGION_BOX2D; nullptr without ltidal_min_regions
  CArr zgrid, bvdc, bvvc_pr;        // KPP's zgrid; bckgrnd_vdc(k), bckgrnd_vvc(k) / Prandtl (1..km): wave-uniform index, scalar loads
  const double *B2 = nullptr, *BPR2 = nullptr;   // lhoriz_varying_bckgrnd (HV): bckgrnd_vdc(i,j), bckgrnd_vvc(i,j) / Prandtl; set at the launch
  CArr minval;                      // tidal_min_values by region, 1-based
  CArrI klev;                       // tidal_min_regions_klevels by region, 1-based
  double mix_max = 0.0, prandtl = 0.0;
  int lmax = 0, stabc = 0;          // ltidal_max; ltidal_stabc .and. .not. lccsm_control_compatible
  double *DIFF = nullptr, *N2 = nullptr, *KV = nullptr, *KVM = nullptr;   // tidal_diag: TIDAL_DIFF, TIDAL_N2, KVMIX, KVMIX_M (all or none)
};

// One thread per column, i fastest, marching k over the levels above the bottom (k < KMT: the interior kernels wrote 0 at and below
// it and nothing is added there; the diagnostics keep the 0 they were allocated with).  Per level 2 loads (DBLOC, TIDAL_COEF_3D), a
// read-modify-write of VISC and of VDC (of both VDC arrays with double diffusion) and, with tidal_diag, 4 stores; the operands of
// level k + 1 are requested before level k is evaluated.  The previous level's final TIDAL_DIFF stays in a register for the
// stability control.
struct TidalRaw { double db, co, visc, vd1, vd2; };
// HV (after pop_init_kpp_bckgrnd): the background is the column's value of the two 2-D fields, loaded once, not the per-level one.
template <bool PBC = false, bool HV = false>
__global__ void __launch_bounds__(POP_COL_THREADS)
k_kpp_tidal(DevGrid g, TidalDev td, int vdc_same, const double *__restrict__ DBLOC, double *__restrict__ VISC,
            double *__restrict__ VDC1, double *__restrict__ VDC2) {
  Col c;
  if (!col_setup(g, c, false)) return;
  const int km = g.km;
  const long long n2 = g.n2;
  const int kmt = g.KMT[c.q2];
  if (kmt < 2) return;
  const long long vb = ((long long)c.b * (km + 2)) * n2 + c.p2;
  const double dzbc = PBC ? g.DZBC[c.q2] : 0.0;
  double hb = 0.0, hbpr = 0.0;
  if constexpr (HV) { hb = td.B2[c.q2]; hbpr = td.BPR2[c.q2]; }
  // region minimum: the levels klo .. KMT - 1 of a column inside a box (REGION_BOX3D, tidal_mixing.F90:986-997)
  double rmin = 0.0; int klo = km + 1;
  if (td.BOX) {
    const int r = td.BOX[c.q2];
    if (r > 0) {
      rmin = td.minval[r];
      const int kl = td.klev[r];
      if (kl == 2) klo = max(3, kmt - 2);
      else if (kl == 6) klo = max(7, kmt - 6);
    }
  }
  auto load = [&](int k) {
    TidalRaw r;
    const long long o = c.base3 + (long long)(k - 1) * n2;
    r.db = DBLOC[o]; r.co = td.COEF[o]; r.visc = VISC[o]; r.vd1 = VDC1[vb + (long long)k * n2];
    r.vd2 = vdc_same ? 0.0 : VDC2[vb + (long long)k * n2];
    return r;
  };
  TidalRaw cu = load(1);
  double prev = 0.0;                                   // TIDAL_DIFF(k - 1), final value
#pragma unroll 1
  for (int k = 1; k < kmt; ++k) {                      // k <= km - 1
    const TidalRaw nx = load(k + 1 < kmt ? k + 1 : k);
    const long long o = c.base3 + (long long)(k - 1) * n2;
    const double h = PBC ? 0.5 * (pbc_dz(g, k, kmt, dzbc) + pbc_dz(g, k + 1, kmt, dzbc)) : td.zgrid[k] - td.zgrid[k + 1];
    const double N2 = cu.db / h;
    double t = (N2 > 0.0) ? cu.co / N2 : 0.0;
    if (td.lmax) t = fmin(t, td.mix_max);
    if (td.stabc && k > 2 && k >= kmt - 2) t = fmax(t, prev);   // k == KMT - 1 or KMT - 2
    if (k >= klo) t = fmax(t, rmin);
    prev = t;
    const double kv = fmin((HV ? hb : td.bvdc[k]) + t, td.mix_max);
    const double kvm = td.prandtl * fmin((HV ? hbpr : td.bvvc_pr[k]) + t, td.mix_max);
    VISC[o] = cu.visc + kvm;
    VDC1[vb + (long long)k * n2] = cu.vd1 + kv;
    if (!vdc_same) VDC2[vb + (long long)k * n2] = cu.vd2 + kv;
    if (td.DIFF) { td.DIFF[o] = t; td.N2[o] = N2; td.KV[o] = kv; td.KVM[o] = kvm; }
    cu = nx;
  }
}

}  // namespace pop
