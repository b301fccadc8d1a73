// kernels_transport.hpp -- northward heat and salt transports (compute_tracer_transports, diags_on_lat_aux_grid.F90:1294-1594)
// accumulated on the device.
//
// The routine is linear in its inputs, so the binned sums it forms from time means are formed here every step and weighted like a
// tavg entry.  Its per-column inputs of a step are
//   ADV, HDIF, VNF          written by the diagnostic form of the generic tracer kernel, k_tracer_rhs<., ., ., 2, false, true>
//                           (kernels_baroclinic.hpp): the step's own advective operator, mixing term and face flux velocity
//   ADV_I, VNF_I            k_trn_eddy from UISOP, VISOP (hmix_gm_share.F90:276-361)
//   ADV_SM, VNF_SM          k_trn_eddy from USUBM, VSUBM (mix_submeso.F90:679-748)
// all (nxb, nyb, nblocks) per tracer, columns no kernel visits staying 0.
//   k_trn_bin   one workgroup per (cell list, tracer): the cells of one block that lie in one latitude bin (host_lat_aux.cpp; the lists
//               of the MOC).  Thread t adds the cells t, t + 256, ... in that order, the workgroup reduces by the fixed tree of
//               moc_wg_reduce, and thread 0 does ACC = ACC + dtavg * sum for every term and region (the product rounded first).
//               Terms: -ADV TAREA, -HDIF TAREA, -ADV_I TAREA, -ADV_SM TAREA (:1412-1436).
//   k_trn_bnd   the same for the row south of region 2 (:1509-1520): VNF, VNF_I, VNF_SM.
// One writer per accumulator, no atomics, nothing leaves the device.
//
// The library is built with -ffp-contract=off; the pragma below says so again for this file.
#pragma once
#include "kernels_moc.hpp"

namespace pop {

constexpr int TRN_NBIN = 4, TRN_NBND = 3;   // terms per tracer of a bin / of the boundary row
// the column fields of one tracer, in the order of pop_get_field's names
enum TrnCol { TRN_C_ADV = 0, TRN_C_HDIF, TRN_C_VNF, TRN_C_ADV_I, TRN_C_VNF_I, TRN_C_ADV_SM, TRN_C_VNF_SM, TRN_NCOL };

struct TrnArgs {
  const double *TMIX[2];
  const double *UI, *VI, *US, *VS;   // UISOP, VISOP, USUBM, VSUBM; a null pair: its fields are not formed
  const double *HTE, *HTN;
  double *COL[2][TRN_NCOL];          // [tracer][TrnCol]
  const MocList *lists, *blists;     // block = LOCAL block index here
  const int *cells, *bcells;
  double *ACC, *BACC;                // [list][tracer][term][region], [blist][tracer][term]
  double dtavg;
  int nreg;
  int ntr, tr[2];                    // the requested tracers
};

// ADV_I / ADV_SM and VNF_I / VNF_SM of one physical column.  eoshift(.., shift=-1) is the value of column i - 1 / row j - 1, whose
// ghost copies are current here (the velocities were formed over the whole block, the mix-time tracers carry updated ghost cells).
__global__ void __launch_bounds__(POP_RED_THREADS) k_trn_eddy(DevGrid g, TrnArgs a) {
#pragma clang fp contract(off)
  const int p2 = blockIdx.x * POP_RED_THREADS + threadIdx.x, b = blockIdx.y, nxb = g.nxb, km = g.km;
  if (p2 >= g.n2 || !interior(g, b, p2 % nxb, p2 / nxb)) return;
  const long long q2 = (long long)b * g.n2 + p2, base3 = (long long)b * g.n3 + p2;
  const double hte = a.HTE[q2], htew = a.HTE[q2 - 1], htn = a.HTN[q2], htns = a.HTN[q2 - nxb];
  const double tarear = g.TAREA_R[q2], tarea = g.TAREA[q2];
  const int kmt = g.KMT[q2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const double *U = s ? a.US : a.UI, *V = s ? a.VS : a.VI;
    if (!U) continue;
    double adv[2] = {0.0, 0.0}, vnf[2] = {0.0, 0.0};
    for (int k = 1; k <= km; ++k) {
      const long long o = base3 + (long long)(k - 1) * g.n2;
      const double u0 = U[o], uw = U[o - 1], v0 = V[o], vs = V[o - nxb], dzk = g.dz[k];
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const double *TM = a.TMIX[n];
        const double t0 = TM[o], te = TM[o + 1], tw = TM[o - 1], tn = TM[o + nxb], ts = TM[o - nxb];
        double W3 = 0.5 * hte * u0 * (t0 + te) - 0.5 * htew * uw * (tw + t0);
        W3 = W3 + 0.5 * htn * v0 * (t0 + tn) - 0.5 * htns * vs * (ts + t0);
        if (k <= kmt) adv[n] = adv[n] + -(dzk * tarear * W3);
        vnf[n] = vnf[n] + 0.5 * v0 * htn * tarear * (t0 + tn) * tarea * dzk;
      }
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) { a.COL[n][s ? TRN_C_ADV_SM : TRN_C_ADV_I][q2] = adv[n]; a.COL[n][s ? TRN_C_VNF_SM : TRN_C_VNF_I][q2] = vnf[n]; }
  }
}

__global__ void __launch_bounds__(POP_RED_THREADS) k_trn_bin(DevGrid g, TrnArgs a) {
#pragma clang fp contract(off)
  const int l = blockIdx.x, n = a.tr[blockIdx.y], t = threadIdx.x;
  const MocList L = a.lists[l];
  const long long b2 = (long long)L.block * g.n2;
  const double *F[TRN_NBIN] = {a.COL[n][TRN_C_ADV], a.COL[n][TRN_C_HDIF], a.UI ? a.COL[n][TRN_C_ADV_I] : nullptr, a.US ? a.COL[n][TRN_C_ADV_SM] : nullptr};
  double v[2 * TRN_NBIN];
#pragma unroll
  for (int f = 0; f < 2 * TRN_NBIN; ++f) v[f] = 0.0;
  for (int c = t; c < L.cnt; c += POP_RED_THREADS) {
    const int w = a.cells[L.off + c], p2 = w & ((1 << MOC_FLAG_SHIFT) - 1), fl = w >> MOC_FLAG_SHIFT;
    const double tarea = g.TAREA[b2 + p2];
#pragma unroll
    for (int f = 0; f < TRN_NBIN; ++f) {
      const double x = F[f] ? -(F[f][b2 + p2] * tarea) : 0.0;
      if (fl & 1) v[2 * f] = v[2 * f] + x;
      if (fl & 2) v[2 * f + 1] = v[2 * f + 1] + x;
    }
  }
  moc_wg_reduce<2 * TRN_NBIN>(v);
  if (t == 0) {
    double *acc = a.ACC + ((long long)l * 2 + n) * TRN_NBIN * a.nreg;
#pragma unroll
    for (int f = 0; f < TRN_NBIN; ++f) {
      acc[f * a.nreg] = acc[f * a.nreg] + a.dtavg * v[2 * f];
      if (a.nreg > 1) acc[f * a.nreg + 1] = acc[f * a.nreg + 1] + a.dtavg * v[2 * f + 1];
    }
  }
}

__global__ void __launch_bounds__(POP_RED_THREADS) k_trn_bnd(DevGrid g, TrnArgs a) {
#pragma clang fp contract(off)
  const int l = blockIdx.x, n = a.tr[blockIdx.y], t = threadIdx.x;
  const MocList L = a.blists[l];
  const long long b2 = (long long)L.block * g.n2;
  const double *F[TRN_NBND] = {a.COL[n][TRN_C_VNF], a.UI ? a.COL[n][TRN_C_VNF_I] : nullptr, a.US ? a.COL[n][TRN_C_VNF_SM] : nullptr};
  double v[TRN_NBND];
#pragma unroll
  for (int f = 0; f < TRN_NBND; ++f) v[f] = 0.0;
  for (int c = t; c < L.cnt; c += POP_RED_THREADS) {
    const int p2 = a.bcells[L.off + c];
#pragma unroll
    for (int f = 0; f < TRN_NBND; ++f) if (F[f]) v[f] = v[f] + F[f][b2 + p2];
  }
  moc_wg_reduce<TRN_NBND>(v);
  if (t == 0) {
    double *acc = a.BACC + ((long long)l * 2 + n) * TRN_NBND;
#pragma unroll
    for (int f = 0; f < TRN_NBND; ++f) acc[f] = acc[f] + a.dtavg * v[f];
  }
}

}  // namespace pop
