// kernels_submeso.hpp -- the submesoscale mixed-layer eddy scheme of Fox-Kemper, Ferrari and Hallberg (2008), lsubmesoscale_mixing
// (source/mix_submeso.F90:341-772 submeso_sf, :779-1005 submeso_flux; the work arrays RX, RY, RZ_SAVE, TX, TY, TZ of
// hmix_gm_submeso_share.F90:149-432 tracer_diffs_and_isopyc_slopes).  Its tendency is added to the Gent-McWilliams one
// (horizontal_mix.F90:566-581), so it runs after k_gm_flux / k_gm_flux_tile on the launch stream.
//
// The reference stores the stream function SF_SUBM_X / SF_SUBM_Y of the 2 x 2 quarter-cell faces of both halves of every cell
// (8 km values per column).  Every one of them is
//     ((eff * ML_DEPTH**2) * shape(reference_depth / ML_DEPTH)) * TIME_SCALE / HLS  *  B  *  min(DXT | DYT, max_hor_grid_scale)
// with B one of four vertically averaged buoyancy differences of the column: six 2-D fields (ML_DEPTH, HLS, BX e / w, BY n / s) carry all
// of it and the flux kernel forms each value it needs again, in the reference's operation order:
//   k_submeso_column  one thread per column of the block (ghost cells included; a difference towards a neighbour outside the block is 0,
//                     as in the reference's block-local arrays): marches down to the level that holds ML_DEPTH, forms RX, RY, RZ_SAVE
//                     of each level on the way and accumulates the two integrals; writes the six 2-D fields;
//   k_submeso_flux    64 x 4 tiles of the block, one thread per physical cell, both tracers: a k-march with FZTOP in a register, from
//                     level 1 down to the last level of the tile that can hold a non-zero tendency; GTK = GTK + TDTK;
//   k_submeso_vel     submeso_diag: U_SUBM, V_SUBM, WTOP_SUBM (:599-661), one thread per column.
#pragma once
#include "kernels_common.hpp"

namespace pop {

struct SubmDev {
  double *ML, *HLS, *B[4];          // ML_DEPTH, HLS, BX_VERT_AVG east / west, BY_VERT_AVG north / south (2-D)
  double *GTK[2];                   // the Gent-McWilliams tendency the result is added to
  double *TD[2];                    // submeso_diag: TDTK alone (SUBM_ADV_TEND), nullptr otherwise
  double *US, *VS, *WS;             // submeso_diag: U_SUBM, V_SUBM (east / north face), WTOP_SUBM (top of the cell)
  const double *TS;                 // TIME_SCALE
  const double *HMXL;               // nullptr without KPP: ML_DEPTH = zw(1)
  const double *HYX, *HXY, *DXT, *DYT, *HTE, *HTN;
  double eff, hls0, max_hgs, grav, sqrt_grav;
  int const_hls, all_levels;
};

// one thread per column: the vertical averages of the horizontal buoyancy differences over the mixed layer (:441-484) and the
// horizontal length scale (:492-554)
__global__ void __launch_bounds__(256)
k_submeso_column(DevGrid g, SubmDev w, const double *__restrict__ T, const double *__restrict__ S) {
  const int p2 = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (p2 >= g.n2) return;
  const int nxb = g.nxb, nyb = g.nyb, km = g.km, i = p2 % nxb, j = p2 / nxb;
  const long long n2 = g.n2, q = (long long)b * n2 + p2, base = (long long)b * g.n3 + p2;
  const int kmt = g.KMT[q];
  const double ml = w.HMXL ? w.HMXL[q] : g.zw[1];
  const bool he = i <= nxb - 2, hw = i >= 1, hn = j <= nyb - 2, hs = j >= 1;
  const long long de = he ? 1 : 0, dw = hw ? 1 : 0, dn = hn ? nxb : 0, ds = hs ? nxb : 0;
  const int ke = g.KMT[q + de], kw = g.KMT[q - dw], kn = g.KMT[q + dn], ks = g.KMT[q - ds];
  auto temp = [&](long long oo) { return fmax(-2.0, T[oo]); };
  double bx[4] = {0.0, 0.0, 0.0, 0.0}, work2 = 0.0;
  bool cont1 = kmt != 0, cont2 = kmt != 0 && !w.const_hls;
  double tup = 0.0, sup = 0.0;                                 // clamped temperature and salinity of the level above
  for (int k = 1; k <= km && (cont1 || cont2); ++k) {
    const long long o = base + (long long)(k - 1) * n2;
    const double tc = temp(o), sc = S[o];
    double drdt, drds;
    const MwjfP P = mwjf_level(g.pressz[k]);
    mwjf_rho<true>(P, T[o], S[o], &drdt, &drds);
    if (cont1) {
      const double zw_top = (k > 1) ? g.zw[k - 1] : 0.0;
      // below the level that would hold ML_DEPTH every weight is 0 (a column whose ML_DEPTH <= 0 never ends its integral in the reference)
      if (!(ml > zw_top)) cont1 = false;
      else {
        const bool last = ml <= g.zw[k];
        const double w3 = last ? ml - zw_top : g.dz[k];
        const double mke = ((k <= kmt) & (k <= ke)) ? 1.0 : 0.0, mkw = ((k <= kw) & (k <= kmt)) ? 1.0 : 0.0;
        const double mkn = ((k <= kmt) & (k <= kn)) ? 1.0 : 0.0, mks = ((k <= ks) & (k <= kmt)) ? 1.0 : 0.0;
        const double rxe = he ? drdt * (mke * (temp(o + de) - tc)) + drds * (mke * (S[o + de] - sc)) : 0.0;
        const double rxw = hw ? drdt * (mkw * (tc - temp(o - dw))) + drds * (mkw * (sc - S[o - dw])) : 0.0;
        const double ryn = hn ? drdt * (mkn * (temp(o + dn) - tc)) + drds * (mkn * (S[o + dn] - sc)) : 0.0;
        const double rys = hs ? drdt * (mks * (tc - temp(o - ds))) + drds * (mks * (sc - S[o - ds])) : 0.0;
        bx[0] = bx[0] + rxe * w3; bx[1] = bx[1] + rxw * w3; bx[2] = bx[2] + ryn * w3; bx[3] = bx[3] + rys * w3;
        if (last) cont1 = false;
      }
    }
    if (cont2 && k >= 2) {
      if (!(ml >= g.zt[k - 1])) cont2 = false;                 // ML_DEPTH above zt(1): every weight is 0
      else {
        const bool last = ml <= g.zt[k];
        const double d = ml - g.zt[k - 1];
        const double w3 = last ? (d * d) * g.dzwr[k - 1] : g.dzw[k - 1];
        const double rz = fmin(drdt * (tup - tc) + drds * (sup - sc), 0.0);   // RZ_SAVE(k) (share :397-398)
        work2 = work2 + sqrt(-rz * w3);
        if (last) cont2 = false;
      }
    }
    tup = tc; sup = sc;
  }
  double hls = 0.0;
  if (kmt > 0) {
#pragma unroll
    for (int n = 0; n < 4; ++n) bx[n] = -w.grav * bx[n] / ml;
    if (w.const_hls) hls = w.hls0;
    else {
      const double dxt = w.DXT[q], dyt = w.DYT[q], ts = w.TS[q];
      double work1 = sqrt(0.5 * ((bx[0] * bx[0] + bx[1] * bx[1]) / (dxt * dxt) + (bx[2] * bx[2] + bx[3] * bx[3]) / (dyt * dyt)));
      work1 = work1 * ml * (ts * ts);
      work2 = w.sqrt_grav * work2 * ts;
      hls = fmax(fmax(work1, work2), w.hls0);
    }
  }
  w.ML[q] = ml; w.HLS[q] = hls;
#pragma unroll
  for (int n = 0; n < 4; ++n) w.B[n][q] = bx[n];
}

// what the stream function of a column is made of besides B and the grid scale
struct SubmCell { double a0, ml, ts, hls; int kmt; };
__device__ __forceinline__ SubmCell subm_cell(const DevGrid &g, const SubmDev &w, long long q) {
  SubmCell c;
  c.ml = w.ML[q]; c.a0 = w.eff * (c.ml * c.ml); c.ts = w.TS[q]; c.hls = w.HLS[q]; c.kmt = g.KMT[q];
  return c;
}
// WORK1 of :572-578 for the top (half 0) or bottom (half 1) half of level k, 0 where the reference leaves SF_SUBM at 0
__device__ __forceinline__ double subm_w1(const DevGrid &g, const SubmCell &c, int k, int half) {
  const double rd = half ? g.zt[k] + 0.25 * g.dz[k] : g.zt[k] - 0.25 * g.dz[k];
  const double r = 1.0 - (2.0 * rd / c.ml);
  const double w3 = r * r;
  const double w2 = (1.0 - w3) * (1.0 + (5.0 / 21.0) * w3);
  const double v = c.a0 * w2 * c.ts / c.hls;
  return (rd < c.ml && c.kmt >= k) ? v : 0.0;
}
__device__ __forceinline__ double subm_mask(int kk, int ka, int kb) { return ((kk <= ka) & (kk <= kb)) ? 1.0 : 0.0; }
__device__ __forceinline__ double subm_tz(const double *__restrict__ X, int kk, long long o, long long n2) {
  const double d = X[o - (kk >= 2 ? n2 : 0)] - X[o];
  return (kk >= 2) ? d : 0.0;                                  // TZ(1) is never assigned in the reference
}

// last level of a column march that can hold a non-zero tendency when no mixed layer it reads is deeper than mlmax: level k >= 2 reads the
// bottom half of level k - 1 (through FZTOP) as the shallowest half cell, reference depth zt(k-1) + dz(k-1) / 4
__device__ __forceinline__ int subm_last_level(const DevGrid &g, double mlmax) {
  int kl = 1;
  while (kl < g.km && g.zt[kl] + 0.25 * g.dz[kl] < mlmax) ++kl;
  return kl;
}

#define POP_SUBM_TX 64
#define POP_SUBM_TY 4
// the tendency of both tracers on the physical cells of a 64 x 4 tile, added to GTK (submeso_flux)
// TZ0 (passive tracers n >= 3 while Gent-McWilliams runs its cancellation branch): the vertical differences TZ are 0.  The reference forms
// TZ(:,:,:,n) of T and S in tracer_diffs_and_isopyc_slopes (hmix_gm_submeso_share.F90:315-316) and of the tracers n > 2 inside hdifft_gm,
// in the branch `.not. cancellation_occurs` only (hmix_gm.F90:1832, 1851-1852); with cancellation the array keeps the zeros it was
// allocated with, and submeso_flux (mix_submeso.F90:851-884) reads those: its FX, FY vanish for n > 2, the vertical flux (from TX, TY) does not.
template <bool TZ0 = false>
__global__ void __launch_bounds__(POP_SUBM_TX * POP_SUBM_TY)
k_submeso_flux(DevGrid g, SubmDev w, const double *__restrict__ X0, const double *__restrict__ X1) {
  __shared__ unsigned long long mlmax_bits;
  const int nxb = g.nxb, nyb = g.nyb, km = g.km;
  const int tiles_i = (nxb + POP_SUBM_TX - 1) / POP_SUBM_TX;
  const int i = (blockIdx.x % tiles_i) * POP_SUBM_TX + threadIdx.x, j = (blockIdx.x / tiles_i) * POP_SUBM_TY + threadIdx.y, b = blockIdx.y;
  const bool phys = i < nxb && j < nyb && i + 1 >= g.ib && i + 1 <= blk_ie(g, b) && j + 1 >= g.jb && j + 1 <= blk_je(g, b);
  const long long n2 = g.n2;
  // threads outside the physical domain take part in the tile's maximum with a physical cell's values, then leave
  const int p2 = phys ? j * nxb + i : (g.jb - 1) * nxb + (g.ib - 1);
  const long long q = (long long)b * n2 + p2, base = (long long)b * g.n3 + p2;
  const SubmCell cc = subm_cell(g, w, q), ce = subm_cell(g, w, q + 1), cw = subm_cell(g, w, q - 1), cn = subm_cell(g, w, q + nxb), cs = subm_cell(g, w, q - nxb);
  if (threadIdx.x == 0 && threadIdx.y == 0) mlmax_bits = 0ull;
  __syncthreads();
  int klast = km;
  if (!w.all_levels) {
    const double m = fmax(fmax(fmax(cc.ml, ce.ml), fmax(cw.ml, cn.ml)), fmax(cs.ml, 0.0));
    atomicMax(&mlmax_bits, (unsigned long long)__double_as_longlong(m));   // m >= 0: the bit patterns order as the values do
    __syncthreads();
    klast = subm_last_level(g, __longlong_as_double((long long)mlmax_bits));
  }
  if (!phys) return;
  const double hyx = w.HYX[q], hxy = w.HXY[q], hyxw = w.HYX[q - 1], hxys = w.HXY[q - nxb];
  const double tar = g.TAREA_R[q];
  const double gx = fmin(w.DXT[q], w.max_hgs), gy = fmin(w.DYT[q], w.max_hgs);
  const double gxe = fmin(w.DXT[q + 1], w.max_hgs), gxw = fmin(w.DXT[q - 1], w.max_hgs);
  const double gyn = fmin(w.DYT[q + nxb], w.max_hgs), gys = fmin(w.DYT[q - nxb], w.max_hgs);
  const double bxe = w.B[0][q], bxw = w.B[1][q], byn = w.B[2][q], bys = w.B[3][q];
  const double bxw_e = w.B[1][q + 1], bxe_w = w.B[0][q - 1], bys_n = w.B[3][q + nxb], byn_s = w.B[2][q - nxb];
  double fzt0 = 0.0, fzt1 = 0.0;                               // FZTOP_SUBM of the two tracers
  double w1t = subm_w1(g, cc, 1, 0);                           // WORK1 of the top half of the level at hand
  for (int k = 1; k <= klast; ++k) {
    const long long o = base + (long long)(k - 1) * n2;
    const int kp1 = (k == km) ? k : k + 1;
    const long long okp = o + (long long)(kp1 - k) * n2;
    const double w1b = subm_w1(g, cc, k, 1), w1n = subm_w1(g, cc, kp1, 0);
    const double e_t = subm_w1(g, ce, k, 0), e_b = subm_w1(g, ce, k, 1), w_t = subm_w1(g, cw, k, 0), w_b = subm_w1(g, cw, k, 1);
    const double n_t = subm_w1(g, cn, k, 0), n_b = subm_w1(g, cn, k, 1), s_t = subm_w1(g, cs, k, 0), s_b = subm_w1(g, cs, k, 1);
    const double cx = ((k <= cc.kmt) & (k <= ce.kmt)) ? hyx * 0.25 : 0.0, cxw = ((k <= cw.kmt) & (k <= cc.kmt)) ? hyxw * 0.25 : 0.0;
    const double cy = ((k <= cc.kmt) & (k <= cn.kmt)) ? hxy * 0.25 : 0.0, cys = ((k <= cs.kmt) & (k <= cc.kmt)) ? hxys * 0.25 : 0.0;
    const double me = subm_mask(k, cc.kmt, ce.kmt), mn = subm_mask(k, cc.kmt, cn.kmt), mw = subm_mask(k, cw.kmt, cc.kmt), ms = subm_mask(k, cs.kmt, cc.kmt);
    const double pe = subm_mask(k + 1, cc.kmt, ce.kmt), pn = subm_mask(k + 1, cc.kmt, cn.kmt), pw = subm_mask(k + 1, cw.kmt, cc.kmt), ps = subm_mask(k + 1, cs.kmt, cc.kmt);
    const double kmask = (k < cc.kmt) ? 1.0 : 0.0;
    auto tz = [&](const double *__restrict__ X, int kk, long long oo, long long nn) { return TZ0 ? 0.0 : subm_tz(X, kk, oo, nn); };
    auto one = [&](const double *__restrict__ X, double &fztop) {
      const double tzc = tz(X, k, o, n2), tzc1 = tz(X, kp1, okp, n2);
      const double fxe = cx * (w1t * bxe * gx * tzc + w1b * bxe * gx * tzc1 + e_t * bxw_e * gxe * tz(X, k, o + 1, n2) + e_b * bxw_e * gxe * tz(X, kp1, okp + 1, n2));
      const double fxw = cxw * (w_t * bxe_w * gxw * tz(X, k, o - 1, n2) + w_b * bxe_w * gxw * tz(X, kp1, okp - 1, n2) + w1t * bxw * gx * tzc + w1b * bxw * gx * tzc1);
      const double fyn = cy * (w1t * byn * gy * tzc + w1b * byn * gy * tzc1 + n_t * bys_n * gyn * tz(X, k, o + nxb, n2) + n_b * bys_n * gyn * tz(X, kp1, okp + nxb, n2));
      const double fys = cys * (s_t * byn_s * gys * tz(X, k, o - nxb, n2) + s_b * byn_s * gys * tz(X, kp1, okp - nxb, n2) + w1t * bys * gy * tzc + w1b * bys * gy * tzc1);
      double td;
      if (k < km) {
        const double xc = X[o], xp = X[okp];
        const double work1 = w1b * bxe * gx * hyx * (me * (X[o + 1] - xc)) + w1b * byn * gy * hxy * (mn * (X[o + nxb] - xc)) +
                             w1b * bxw * gx * hyxw * (mw * (xc - X[o - 1])) + w1b * bys * gy * hxys * (ms * (xc - X[o - nxb]));
        const double work2 = 1.0 * (w1n * bxe * gx * hyx * (pe * (X[okp + 1] - xp)) + w1n * byn * gy * hxy * (pn * (X[okp + nxb] - xp)) +
                                    w1n * bxw * gx * hyxw * (pw * (xp - X[okp - 1])) + w1n * bys * gy * hxys * (ps * (xp - X[okp - nxb])));
        const double fz = -kmask * 0.25 * (work1 + work2);
        td = (fxe - fxw + fyn - fys + fztop - fz) * g.dzr[k] * tar;
        fztop = fz;
      } else {
        td = (fxe - fxw + fyn - fys + fztop) * g.dzr[k] * tar;
        fztop = 0.0;
      }
      return td;
    };
    const double td0 = one(X0, fzt0), td1 = one(X1, fzt1);
    w.GTK[0][o] = w.GTK[0][o] + td0; w.GTK[1][o] = w.GTK[1][o] + td1;
    if (w.TD[0]) { w.TD[0][o] = td0; w.TD[1][o] = td1; }
    w1t = w1n;
  }
}

// diagnostic submeso velocities (:599-661): one thread per column carries the stream function at the top of the level on its east
// and north face (U_SUBM, V_SUBM of the cell) and, at physical cells, on the east face of its west and the north face of its south
// neighbour (the divergence that integrates to WTOP_SUBM)
__global__ void __launch_bounds__(256)
k_submeso_vel(DevGrid g, SubmDev w) {
  const int p2 = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (p2 >= g.n2) return;
  const int nxb = g.nxb, nyb = g.nyb, km = g.km, i = p2 % nxb, j = p2 / nxb;
  const long long n2 = g.n2, q = (long long)b * n2 + p2, base = (long long)b * g.n3 + p2;
  const bool phys = i + 1 >= g.ib && i + 1 <= blk_ie(g, b) && j + 1 >= g.jb && j + 1 <= blk_je(g, b);
  const bool has_e = i <= nxb - 2, has_n = j <= nyb - 2;
  // stream function at the bottom of level k on the east face of the cell with 2-D index qq (:620-624, 635), and on its north face
  auto psi_e = [&](long long qq, int k) {
    const SubmCell a = subm_cell(g, w, qq), e = subm_cell(g, w, qq + 1);
    const double factor = (k < km) ? 1.0 : 0.0;
    const int kp1 = (k < km) ? k + 1 : k;
    const double ga = fmin(w.DXT[qq], w.max_hgs), ge = fmin(w.DXT[qq + 1], w.max_hgs);
    const double v = (subm_w1(g, a, k, 1) * w.B[0][qq] * ga + factor * (subm_w1(g, a, kp1, 0) * w.B[0][qq] * ga) +
                      subm_w1(g, e, k, 1) * w.B[1][qq + 1] * ge + factor * (subm_w1(g, e, kp1, 0) * w.B[1][qq + 1] * ge)) * 0.25 * w.HYX[qq];
    return (k < a.kmt && k < e.kmt) ? v : 0.0;
  };
  auto psi_n = [&](long long qq, int k) {
    const SubmCell a = subm_cell(g, w, qq), n = subm_cell(g, w, qq + nxb);
    const double factor = (k < km) ? 1.0 : 0.0;
    const int kp1 = (k < km) ? k + 1 : k;
    const double ga = fmin(w.DYT[qq], w.max_hgs), gn = fmin(w.DYT[qq + nxb], w.max_hgs);
    const double v = (subm_w1(g, a, k, 1) * w.B[2][qq] * ga + factor * (subm_w1(g, a, kp1, 0) * w.B[2][qq] * ga) +
                      subm_w1(g, n, k, 1) * w.B[3][qq + nxb] * gn + factor * (subm_w1(g, n, kp1, 0) * w.B[3][qq + nxb] * gn)) * 0.25 * w.HXY[qq];
    return (k < a.kmt && k < n.kmt) ? v : 0.0;
  };
  const int kmt = g.KMT[q];
  double mlmax = 0.0;
  if (phys) mlmax = fmax(fmax(fmax(w.ML[q], w.ML[q + 1]), fmax(w.ML[q - 1], w.ML[q + nxb])), w.ML[q - nxb]);
  double ut_e = 0.0, ut_w = 0.0, vt_n = 0.0, vt_s = 0.0, wtop = 0.0;
  const double hte = w.HTE[q], htn = w.HTN[q], tar = g.TAREA_R[q];
  for (int k = 1; k <= km; ++k) {
    const long long o = base + (long long)(k - 1) * n2;
    const double ub_e = has_e ? psi_e(q, k) : 0.0, vb_n = has_n ? psi_n(q, k) : 0.0;
    const double w1 = (has_e && k <= kmt && k <= g.KMT[q + (has_e ? 1 : 0)]) ? ut_e - ub_e : 0.0;
    const double w2 = (has_n && k <= kmt && k <= g.KMT[q + (has_n ? nxb : 0)]) ? vt_n - vb_n : 0.0;
    w.US[o] = w1 * g.dzr[k] / hte;
    w.VS[o] = w2 * g.dzr[k] / htn;
    w.WS[o] = wtop;
    if (phys) {
      const double ub_w = psi_e(q - 1, k), vb_s = psi_n(q - nxb, k);
      const double w1w = (k <= g.KMT[q - 1] && k <= kmt) ? ut_w - ub_w : 0.0;
      const double w2s = (k <= g.KMT[q - nxb] && k <= kmt) ? vt_s - vb_s : 0.0;
      wtop = (k < kmt && g.zw[k] < mlmax) ? wtop + tar * (w1 - w1w + w2 - w2s) : 0.0;   // WBOT_SUBM of this level = WTOP_SUBM of the next
      ut_w = ub_w; vt_s = vb_s;
    }
    ut_e = ub_e; vt_n = vb_n;
  }
}

}  // namespace pop
