// kernels_diag.hpp -- global and CFL diagnostics (diagnostics.F90) on the device.
//
// Global sums (diag_global_preupdate :1174-1431, diag_global_afterupdate :1548-1770).  One launch per site forms every term of
// the site in the reference's order of operations and reduces it per workgroup: grid (chunks of 256 consecutive cells, levels
// 0 .. km, blocks).  Level slot 0 holds the 2-D quantities of the site, slot k the terms of level k, so every source is read once.
// A workgroup reduces its NF values by the fixed tree of wg_reduce_store and stores one partial per (block, slot, quantity, chunk);
// k_diag_block_sums adds the chunks of a (block, slot, quantity) by block_sum_ordered into the vector of block sums, indexed by the
// global block id.  The host adds levels in the order k = 1 .. and blocks in block-id order (launch_diag.hpp).  No atomics, no 3-D
// work field.  Land cells enter with the reference's merge(..., c0, ...): these kernels do NOT apply DevGrid::skip.
//
// CFL numbers (cfl_advect :2262-2425, cfl_hdiff :2695-2767; the flux velocities of comp_flux_vel, advection.F90:1970-2132): one
// thread per column marches k and carries WTK; per level the workgroup reduces the (value, cell index) pairs of the four
// advective numbers and of the two horizontal-mixing numbers with the first-index rule (the first physical cell in (j, i) order
// that attains the maximum), shuffles inside a wave, LDS across the four waves; one pair per (block, level, quantity, chunk)
// goes to memory and k_cfl_block_max combines the chunks of a block in chunk order.
//
// The library is built with -ffp-contract=off; the pragma below says so again for this file.
#pragma once
#include "kernels_barotropic.hpp"

namespace pop {

constexpr int DIAG_NQ_CFL = 6;   // advu, advv, advw, advt, hdifft, hdiffu
enum DiagCflQ { CQ_ADVU = 0, CQ_ADVV, CQ_ADVW, CQ_ADVT, CQ_HDIFFT, CQ_HDIFFU };

// the tree of wg_reduce_store; value f goes to out[f * stride]
template <int NF>
__device__ __forceinline__ void diag_wg_reduce(double (&v)[NF], double *out, long long stride) {
  __shared__ double sh[NF][POP_RED_THREADS];
  const int t = threadIdx.x;
#pragma unroll
  for (int f = 0; f < NF; ++f) sh[f][t] = v[f];
  __syncthreads();
  if (t < 64) {
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const double x = tree_tail64((sh[f][t] + sh[f][t + 128]) + (sh[f][t + 64] + sh[f][t + 192]));
      if (t == 0) out[f * stride] = x;
    }
  }
}

// partial of (block b, slot lev, quantity f, chunk): partial[((b * nlev + lev) * NF + f) * nchunk + chunk]
struct DiagSumOut { double *partial; int nchunk, nlev; };
__device__ __forceinline__ double *diag_slot(const DiagSumOut &o, int b, int lev, int nf) {
  return o.partial + ((long long)b * o.nlev + lev) * nf * o.nchunk + blockIdx.x;
}
// UFACT = UAREA * RCALCU, 0 at the redundant half of the top row of a tripole grid (diagnostics.F90:1249-1254)
__device__ __forceinline__ double diag_ufact(const double *UAREA, const double *RCALCU, const double *DUP, long long q2) {
#pragma clang fp contract(off)
  return (DUP && DUP[q2] != 0.0) ? 0.0 : UAREA[q2] * RCALCU[q2];
}

// ---- diag_global_afterupdate: quantity 0 = sea level (slot 0) / kinetic energy (slot k); 1 + n = surface flux / tracer n
struct DiagAfterArgs {
  const double *U, *V, *PS, *TR[MAXNT], *TFW[MAXNT];
  const double *UAREA, *RCALCU, *DUP;
  double grav;
  DiagSumOut out;
};
template <int NT, bool PBC>
__global__ void __launch_bounds__(POP_RED_THREADS) k_diag_after(DevGrid g, DiagAfterArgs a) {
#pragma clang fp contract(off)
  constexpr int NF = NT + 1;
  const int p2 = blockIdx.x * POP_RED_THREADS + threadIdx.x, lev = blockIdx.y, b = blockIdx.z;
  double v[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) v[f] = 0.0;
  if (p2 < g.n2 && interior(g, b, p2 % g.nxb, p2 / g.nxb)) {
    const long long q2 = (long long)b * g.n2 + p2;
    if (lev == 0) {
      const double tfact = g.TAREA[q2] * g.RCALCT[q2];
      v[0] = a.PS[q2] / a.grav * tfact;
#pragma unroll
      for (int n = 0; n < NT; ++n) v[1 + n] = a.TFW[n][q2] * tfact;
    } else {
      const int k = lev;
      const long long o = (long long)b * g.n3 + (long long)(k - 1) * g.n2 + p2;
      const int kmu = g.KMU[q2], kmt = g.KMT[q2];
      if (kmu >= k) {
        const double u = a.U[o], w = a.V[o];
        const double dzu = PBC ? pbc_dz(g, k, kmu, g.DZUB[q2]) : g.dz.u(k);
        v[0] = 0.5 * (u * u + w * w) * diag_ufact(a.UAREA, a.RCALCU, a.DUP, q2) * dzu;
      }
      if (kmt >= k) {
        const double tarea = g.TAREA[q2];
        if (k == 1) {   // the variable-thickness surface layer
          const double dz1 = g.dz.u(1), fac = 1.0 + a.PS[q2] / (dz1 * a.grav);
#pragma unroll
          for (int n = 0; n < NT; ++n) v[1 + n] = a.TR[n][o] * tarea * fac * dz1;
        } else {
          const double dzt = PBC ? pbc_dz(g, k, kmt, g.DZBC[q2]) : g.dz.u(k);
#pragma unroll
          for (int n = 0; n < NT; ++n) v[1 + n] = a.TR[n][o] * tarea * dzt;
        }
      }
    }
  }
  diag_wg_reduce<NF>(v, diag_slot(a.out, b, lev, NF), a.out.nchunk);
}

// ---- diag_global_preupdate: slot 0 = diag_ws, diag_press_free, diag_ke_free, diag_ke_psfc; slot k: 2 n = the change of tracer n
// at level k, 2 n + 1 = its absolute value
struct DiagPreArgs {
  const double *U, *V, *UB, *VB, *GX, *GY, *DH, *DHU, *PSC, *PSN, *PSM, *TN[MAXNT], *TO[MAXNT];
  const double *UAREA, *RCALCU, *DUP;
  double grav;
  DiagSumOut out;
};
template <int NT, bool PBC>
__global__ void __launch_bounds__(POP_RED_THREADS) k_diag_pre(DevGrid g, DiagPreArgs a) {
#pragma clang fp contract(off)
  constexpr int NF = 2 * NT;
  const int p2 = blockIdx.x * POP_RED_THREADS + threadIdx.x, lev = blockIdx.y, b = blockIdx.z;
  double v[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) v[f] = 0.0;
  if (p2 < g.n2 && interior(g, b, p2 % g.nxb, p2 / g.nxb)) {
    const long long q2 = (long long)b * g.n2 + p2;
    if (lev == 0) {
      const double tfact = g.TAREA[q2] * g.RCALCT[q2], ufact = diag_ufact(a.UAREA, a.RCALCU, a.DUP, q2);
      const long long o = (long long)b * g.n3 + p2;
      const double u = a.U[o], w = a.V[o];
      v[0] = (u * g.SMF1[q2] + w * g.SMF2[q2]) * ufact;
      v[1] = -(a.UB[q2] * a.GX[q2] + a.VB[q2] * a.GY[q2]) * g.HU[q2] * ufact;
      v[2] = 0.5 * (u * u + w * w) * a.DHU[q2] * ufact;
      v[3] = a.PSC[q2] * a.DH[q2] * tfact;
    } else {
      const int k = lev, kmt = g.KMT[q2];
      if (k <= kmt) {
        const long long o = (long long)b * g.n3 + (long long)(k - 1) * g.n2 + p2;
        const double tarea = g.TAREA[q2];
        if (k == 1) {
          const double dz1 = g.dz.u(1), hn = dz1 + a.PSN[q2] / a.grav, hm = dz1 + a.PSM[q2] / a.grav;
#pragma unroll
          for (int n = 0; n < NT; ++n) { const double d = tarea * (hn * a.TN[n][o] - hm * a.TO[n][o]); v[2 * n] = d; v[2 * n + 1] = fabs(d); }
        } else {
          const double dzt = PBC ? pbc_dz(g, k, kmt, g.DZBC[q2]) : g.dz.u(k);
#pragma unroll
          for (int n = 0; n < NT; ++n) { const double d = dzt * tarea * (a.TN[n][o] - a.TO[n][o]); v[2 * n] = d; v[2 * n + 1] = fabs(d); }
        }
      }
    }
  }
  diag_wg_reduce<NF>(v, diag_slot(a.out, b, lev, NF), a.out.nchunk);
}

// the chunks of one (block, slot, quantity) added by block_sum_ordered: grid (nlev * nf, blocks).
// vec[(gid[b] * nlev + lev) * nf + f], the vector of block sums of the whole decomposition (other ranks' entries stay 0)
__global__ void __launch_bounds__(POP_RED_THREADS) k_diag_block_sums(const double *__restrict__ partial, int nchunk, int nslots,
                                                                   const int *__restrict__ gid, double *__restrict__ vec) {
  const int s = blockIdx.x, b = blockIdx.y;
  double r[1];
  block_sum_ordered<1>(partial + ((long long)b * nslots + s) * nchunk, nchunk, r);
  if (threadIdx.x == 0) vec[(long long)gid[b] * nslots + s] = r[0];
}

// ---- CFL numbers -----------------------------------------------------------------------------------------------------------
// first-index maximum of (value, index) pairs; index < 0: no candidate
__device__ __forceinline__ void cfl_take(double &v, int &ix, double v2, int i2) {
  if (i2 >= 0 && (ix < 0 || v2 > v || (v2 == v && i2 < ix))) { v = v2; ix = i2; }
}
struct DiagCflArgs {
  const double *U, *V, *DH;
  const double *DXTR, *DYTR, *HT_COEF, *HU_COEF;   // horizontal mixing: 2-D factors AHF / AMF (null: none)
  const double *KI0, *KI1, *FPARA;                 // 3-D coefficients: the halves of KAPPA_ISOP (gm), F_PARA (anis, variable); null: none
  double ct, cu;                                   // c4 ah | c16 ah, c4 am | c16 am | c4 visc_para
  int pow_t, pow_u;                                // 1: del2 / gm / anis, 2: del4 (the square of the metric sum)
  int with_u;                                      // 0: the momentum number is not formed (Smagorinsky)
  double dt;                                       // dt(k), the same at every level here
  double *val; int *idx;                           // [((b * km + k - 1) * DIAG_NQ_CFL + q) * nchunk + chunk]
  int nchunk;
};
template <bool PBC>
__global__ void __launch_bounds__(POP_RED_THREADS) k_cfl_partial(DevGrid g, DiagCflArgs a) {
#pragma clang fp contract(off)
  __shared__ double sv[DIAG_NQ_CFL][4];
  __shared__ int si[DIAG_NQ_CFL][4];
  const int p2 = blockIdx.x * POP_RED_THREADS + threadIdx.x, b = blockIdx.y, t = threadIdx.x, nxb = g.nxb, km = g.km;
  const int ci = p2 % nxb, cj = p2 / nxb;
  // the flux velocities read the U points west and south of the cell: the physical cells have them inside the block
  const bool in = p2 < g.n2 && interior(g, b, ci, cj);
  const long long q2 = (long long)b * g.n2 + (in ? p2 : 0), base3 = (long long)b * g.n3 + (in ? p2 : 0);
  double dyu00 = 0, dyu0m = 0, dyum0 = 0, dyumm = 0, dxu00 = 0, dxu0m = 0, dxum0 = 0, dxumm = 0, tarear = 0, wtk = 0, mt = 0, mu = 0;
  int kmt = 0, kmu00 = 0, kmu0m = 0, kmum0 = 0, kmumm = 0;
  double dzub00 = 0, dzub0m = 0, dzubm0 = 0, dzubmm = 0, dzbc = 0;
  if (in) {
    dyu00 = g.DYU[q2]; dyu0m = g.DYU[q2 - nxb]; dyum0 = g.DYU[q2 - 1]; dyumm = g.DYU[q2 - 1 - nxb];
    dxu00 = g.DXU[q2]; dxu0m = g.DXU[q2 - nxb]; dxum0 = g.DXU[q2 - 1]; dxumm = g.DXU[q2 - 1 - nxb];
    tarear = g.TAREA_R[q2]; wtk = a.DH[q2]; kmt = g.KMT[q2]; kmu00 = g.KMU[q2];
    const double dxt = a.DXTR[q2], dyt = a.DYTR[q2], dxu = g.DXUR[q2], dyu = g.DYUR[q2];
    mt = dxt * dxt + dyt * dyt; mu = dxu * dxu + dyu * dyu;
    if (a.pow_t == 2) mt = mt * mt;
    if (a.pow_u == 2) mu = mu * mu;
    if (PBC) {
      kmu0m = g.KMU[q2 - nxb]; kmum0 = g.KMU[q2 - 1]; kmumm = g.KMU[q2 - 1 - nxb];
      dzub00 = g.DZUB[q2]; dzub0m = g.DZUB[q2 - nxb]; dzubm0 = g.DZUB[q2 - 1]; dzubmm = g.DZUB[q2 - 1 - nxb];
      dzbc = g.DZBC[q2];
    }
  }
  const double ht = (in && a.HT_COEF) ? a.HT_COEF[q2] : 1.0, hu = (in && a.HU_COEF) ? a.HU_COEF[q2] : 1.0;
  for (int k = 1; k <= km; ++k) {
    double val[DIAG_NQ_CFL];
    int idx[DIAG_NQ_CFL];
#pragma unroll
    for (int q = 0; q < DIAG_NQ_CFL; ++q) { val[q] = 0.0; idx[q] = -1; }
    if (in) {
      const long long o = base3 + (long long)(k - 1) * g.n2;
      const double u00 = a.U[o], u0m = a.U[o - nxb], um0 = a.U[o - 1], umm = a.U[o - 1 - nxb];
      const double v00 = a.V[o], v0m = a.V[o - nxb], vm0 = a.V[o - 1], vmm = a.V[o - 1 - nxb];
      double UTE, UTW, VTN, VTS;
      if (PBC) {
        const double z00 = pbc_dz(g, k, kmu00, dzub00), z0m = pbc_dz(g, k, kmu0m, dzub0m), zm0 = pbc_dz(g, k, kmum0, dzubm0), zmm = pbc_dz(g, k, kmumm, dzubmm);
        UTE = 0.5 * (u00 * dyu00 * z00 + u0m * dyu0m * z0m);
        UTW = 0.5 * (um0 * dyum0 * zm0 + umm * dyumm * zmm);
        VTN = 0.5 * (v00 * dxu00 * z00 + vm0 * dxum0 * zm0);
        VTS = 0.5 * (v0m * dxu0m * z0m + vmm * dxumm * zmm);
      } else {
        UTE = 0.5 * (u00 * dyu00 + u0m * dyu0m);
        UTW = 0.5 * (um0 * dyum0 + umm * dyumm);
        VTN = 0.5 * (v00 * dxu00 + vm0 * dxum0);
        VTS = 0.5 * (v0m * dxu0m + vmm * dxumm);
      }
      double wtkb = 0.0;
      if (k < km) { const double FC = (VTN - VTS + UTE - UTW) * tarear; wtkb = (k < kmt) ? (PBC ? wtk + FC : wtk + g.dz.u(k) * FC) : 0.0; }
      double cE, cW, cN, cS, cT, cB;
      if (PBC) {   // the horizontal numbers divide by DZU at the T-cell index, as the reference does
        const double dzu = pbc_dz(g, k, kmu00, dzub00), dzt = pbc_dz(g, k, kmt, dzbc);
        cE = fabs(UTE * tarear / dzu) * a.dt; cW = fabs(UTW * tarear / dzu) * a.dt;
        cN = fabs(VTN * tarear / dzu) * a.dt; cS = fabs(VTS * tarear / dzu) * a.dt;
        cT = fabs(wtk / dzt) * a.dt; cB = fabs(wtkb / dzt) * a.dt;
      } else {
        const double dzk = g.dz.u(k);
        cE = fabs(UTE * tarear) * a.dt; cW = fabs(UTW * tarear) * a.dt;
        cN = fabs(VTN * tarear) * a.dt; cS = fabs(VTS * tarear) * a.dt;
        cT = fabs(wtk / dzk) * a.dt; cB = fabs(wtkb / dzk) * a.dt;
      }
      // a cell's two candidates are taken one after the other with a strict >, so the cell enters with the larger of them
      val[CQ_ADVU] = (cW > cE) ? cW : cE; val[CQ_ADVV] = (cS > cN) ? cS : cN; val[CQ_ADVW] = (cB > cT) ? cB : cT;
      val[CQ_ADVT] = 0.5 * (cE + cW + cN + cS + cT + cB);
      idx[CQ_ADVU] = idx[CQ_ADVV] = idx[CQ_ADVW] = idx[CQ_ADVT] = p2;
      wtk = wtkb;
      // horizontal mixing: the block maximum starts at 0 with a strict >, so only positive numbers are candidates
      double xt = 0.0, xu = 0.0;
      if (kmt > k) { const double cf = a.KI0 ? 4.0 * (0.5 * (a.KI0[o] + a.KI1[o])) : a.ct * ht; xt = fabs(cf * mt); }
      if (a.with_u && kmu00 > k) { const double cf = a.FPARA ? 4.0 * a.FPARA[o] : a.cu * hu; xu = fabs(cf * mu); }
      if (xt > 0.0) { val[CQ_HDIFFT] = xt; idx[CQ_HDIFFT] = p2; }
      if (xu > 0.0) { val[CQ_HDIFFU] = xu; idx[CQ_HDIFFU] = p2; }
    }
#pragma unroll
    for (int q = 0; q < DIAG_NQ_CFL; ++q) {
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {
        const double v2 = __shfl_down(val[q], s, 64);
        const int i2 = __shfl_down(idx[q], s, 64);
        cfl_take(val[q], idx[q], v2, i2);
      }
      if ((t & 63) == 0) { sv[q][t >> 6] = val[q]; si[q][t >> 6] = idx[q]; }
    }
    __syncthreads();
    if (t < DIAG_NQ_CFL) {
      double bv = sv[t][0];
      int bi = si[t][0];
      for (int w = 1; w < 4; ++w) cfl_take(bv, bi, sv[t][w], si[t][w]);
      const long long slot = (((long long)b * km + (k - 1)) * DIAG_NQ_CFL + t) * a.nchunk + blockIdx.x;
      a.val[slot] = bv; a.idx[slot] = bi;
    }
    __syncthreads();
  }
}
// the chunks of one (block, level, quantity) in chunk order: grid (km * DIAG_NQ_CFL, blocks), one wave.
// vec[2 * (gid[b] * km * NQ + s)] = value, + 1 = cell index within the block (-1: no candidate), as doubles
__global__ void __launch_bounds__(64) k_cfl_block_max(const double *__restrict__ val, const int *__restrict__ idx, int nchunk, int nslots,
                                                      const int *__restrict__ gid, double *__restrict__ vec) {
  const int s = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const long long base = ((long long)b * nslots + s) * nchunk;
  double bv = 0.0;
  int bi = -1;
  for (int c = t; c < nchunk; c += 64) cfl_take(bv, bi, val[base + c], idx[base + c]);
#pragma unroll
  for (int sft = 32; sft > 0; sft >>= 1) {
    const double v2 = __shfl_down(bv, sft, 64);
    const int i2 = __shfl_down(bi, sft, 64);
    cfl_take(bv, bi, v2, i2);
  }
  if (t == 0) { const long long o = 2 * ((long long)gid[b] * nslots + s); vec[o] = bv; vec[o + 1] = (double)bi; }
}

}  // namespace pop
