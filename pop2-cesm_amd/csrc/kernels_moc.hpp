// kernels_moc.hpp -- meridional overturning circulation (compute_moc, diags_on_lat_aux_grid.F90:942-1288) accumulated on the device.
//
// compute_moc is linear in its inputs, so the sums it forms from time means are formed here every step and weighted like a tavg entry.
//   k_moc_w     one thread per column marches k and carries WTK as comp_flux_vel does (advection.F90:1970-2132; the march of
//               k_cfl_partial): WE(k) = merge(WTK(k) * TAREA, 0, k <= KMT), WTK at the top of cell k -- the WVEL advt accumulates (:1750).
//   k_moc_bin   one workgroup per (cell list, level): the cells of one block that lie in one latitude bin (host_lat_aux.cpp).  Thread t
//               adds the cells t, t + 256, ... in that order, the workgroup reduces by the fixed tree of wg_reduce_store, and thread 0
//               does ACC = ACC + dtavg * sum for every component and region (the product rounded first).  Terms: WE, and
//               merge(WISOP * TAREA, 0, k <= KMT), merge(WSUBM * TAREA, 0, k <= KMT) (:1027, 1036, 1045).
//   k_moc_bnd   the same for the row south of region 2 (:1094-1152): p5 V(i,j) DXU(i,j) + p5 V(i-1,j) DXU(i-1,j), VISOP HTN, VSUBM HTN.
// One writer per accumulator, no atomics, nothing leaves the device.
//
// The library is built with -ffp-contract=off; the pragma below says so again for this file.
#pragma once
#include "kernels_diag.hpp"

namespace pop {

struct MocArgs {
  const double *U, *V, *DH;
  const double *W2, *W3, *V2, *V3;   // WISOP, WSUBM, VISOP, VSUBM; W2 / V2 null: the component stays 0
  const double *HTN;
  double *WE;                        // (nxb, nyb, km, nblocks) scratch
  const MocList *lists, *blists;     // block = LOCAL block index here
  const int *cells, *bcells;
  double *ACC, *BACC;                // [list][k][comp][region], [blist][k][comp]
  double dtavg;
  int nreg;
};

__global__ void __launch_bounds__(POP_RED_THREADS) k_moc_w(DevGrid g, MocArgs a) {
#pragma clang fp contract(off)
  const int p2 = blockIdx.x * POP_RED_THREADS + threadIdx.x, b = blockIdx.y, nxb = g.nxb, km = g.km;
  if (p2 >= g.n2 || !interior(g, b, p2 % nxb, p2 / nxb)) return;   // physical cells have their west and south U points inside the block
  const long long q2 = (long long)b * g.n2 + p2, base3 = (long long)b * g.n3 + p2;
  const double dyu00 = g.DYU[q2], dyu0m = g.DYU[q2 - nxb], dyum0 = g.DYU[q2 - 1], dyumm = g.DYU[q2 - 1 - nxb];
  const double dxu00 = g.DXU[q2], dxu0m = g.DXU[q2 - nxb], dxum0 = g.DXU[q2 - 1], dxumm = g.DXU[q2 - 1 - nxb];
  const double tarear = g.TAREA_R[q2], tarea = g.TAREA[q2];
  const int kmt = g.KMT[q2];
  double wtk = a.DH[q2];
  for (int k = 1; k <= km; ++k) {
    const long long o = base3 + (long long)(k - 1) * g.n2;
    a.WE[o] = (k <= kmt) ? wtk * tarea : 0.0;
    double wtkb = 0.0;
    if (k < km && k < kmt) {
      const double u00 = a.U[o], u0m = a.U[o - nxb], um0 = a.U[o - 1], umm = a.U[o - 1 - nxb];
      const double v00 = a.V[o], v0m = a.V[o - nxb], vm0 = a.V[o - 1], vmm = a.V[o - 1 - nxb];
      const double UTE = 0.5 * (u00 * dyu00 + u0m * dyu0m), UTW = 0.5 * (um0 * dyum0 + umm * dyumm);
      const double VTN = 0.5 * (v00 * dxu00 + vm0 * dxum0), VTS = 0.5 * (v0m * dxu0m + vmm * dxumm);
      const double FC = (VTN - VTS + UTE - UTW) * tarear;
      wtkb = wtk + g.dz.u(k) * FC;
    }
    wtk = wtkb;
  }
}

// the tree of wg_reduce_store; every thread of the first wave returns, lane 0 holds the sums
template <int NF>
__device__ __forceinline__ void moc_wg_reduce(double (&v)[NF]) {
  __shared__ double sh[NF][POP_RED_THREADS];
  const int t = threadIdx.x;
#pragma unroll
  for (int f = 0; f < NF; ++f) sh[f][t] = v[f];
  __syncthreads();
  if (t < 64) {
#pragma unroll
    for (int f = 0; f < NF; ++f) v[f] = tree_tail64((sh[f][t] + sh[f][t + 128]) + (sh[f][t + 64] + sh[f][t + 192]));
  }
}

template <int NC>
__global__ void __launch_bounds__(POP_RED_THREADS) k_moc_bin(DevGrid g, MocArgs a) {
#pragma clang fp contract(off)
  const int l = blockIdx.x, k = blockIdx.y + 1, t = threadIdx.x;
  const MocList L = a.lists[l];
  const long long b2 = (long long)L.block * g.n2, b3 = (long long)L.block * g.n3 + (long long)(k - 1) * g.n2;
  double v[2 * NC];
#pragma unroll
  for (int f = 0; f < 2 * NC; ++f) v[f] = 0.0;
  for (int c = t; c < L.cnt; c += POP_RED_THREADS) {
    const int w = a.cells[L.off + c], p2 = w & ((1 << MOC_FLAG_SHIFT) - 1), fl = w >> MOC_FLAG_SHIFT;
    double x[NC];
    x[0] = a.WE[b3 + p2];
    if constexpr (NC > 1) {
      const bool wet = k <= g.KMT[b2 + p2];
      const double tarea = g.TAREA[b2 + p2];
      x[1] = (a.W2 && wet) ? a.W2[b3 + p2] * tarea : 0.0;
      if constexpr (NC > 2) x[2] = wet ? a.W3[b3 + p2] * tarea : 0.0;
    }
#pragma unroll
    for (int f = 0; f < NC; ++f) {
      if (fl & 1) v[2 * f] = v[2 * f] + x[f];
      if (fl & 2) v[2 * f + 1] = v[2 * f + 1] + x[f];
    }
  }
  moc_wg_reduce<2 * NC>(v);
  if (t == 0) {
    double *acc = a.ACC + ((long long)l * g.km + (k - 1)) * NC * a.nreg;
#pragma unroll
    for (int f = 0; f < NC; ++f) {
      acc[f * a.nreg] = acc[f * a.nreg] + a.dtavg * v[2 * f];
      if (a.nreg > 1) acc[f * a.nreg + 1] = acc[f * a.nreg + 1] + a.dtavg * v[2 * f + 1];
    }
  }
}

template <int NC>
__global__ void __launch_bounds__(POP_RED_THREADS) k_moc_bnd(DevGrid g, MocArgs a) {
#pragma clang fp contract(off)
  const int l = blockIdx.x, k = blockIdx.y + 1, t = threadIdx.x;
  const MocList L = a.blists[l];
  const long long b2 = (long long)L.block * g.n2, b3 = (long long)L.block * g.n3 + (long long)(k - 1) * g.n2;
  double v[NC];
#pragma unroll
  for (int f = 0; f < NC; ++f) v[f] = 0.0;
  for (int c = t; c < L.cnt; c += POP_RED_THREADS) {
    const int p2 = a.bcells[L.off + c];   // a physical cell: column i - 1 is inside the block and holds its owner's value
    v[0] = v[0] + (0.5 * a.V[b3 + p2] * g.DXU[b2 + p2] + 0.5 * a.V[b3 + p2 - 1] * g.DXU[b2 + p2 - 1]);
    if constexpr (NC > 1) if (a.V2) v[1] = v[1] + a.V2[b3 + p2] * a.HTN[b2 + p2];
    if constexpr (NC > 2) v[2] = v[2] + a.V3[b3 + p2] * a.HTN[b2 + p2];
  }
  moc_wg_reduce<NC>(v);
  if (t == 0) {
    double *acc = a.BACC + ((long long)l * g.km + (k - 1)) * NC;
#pragma unroll
    for (int f = 0; f < NC; ++f) acc[f] = acc[f] + a.dtavg * v[f];
  }
}

}  // namespace pop
