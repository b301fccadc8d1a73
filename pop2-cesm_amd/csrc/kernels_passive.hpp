// kernels_passive.hpp -- the small kernels of the passive tracers n = 3 .. nt that have no (T, S) counterpart to instantiate.
//
// The right-hand side of a passive pair is k_tracer_rhs<., ., ., NP, true> (kernels_baroclinic.hpp), its implicit vertical mixing
// the standard k_impvmixt / k_impvmixt_reg over the pair; del4, lw_lim, Gent-McWilliams and the submesoscale flux run their (T, S)
// kernels once more per pair.  Here: KPP's non-local source of a passive tracer, the averaging step, the surface level of the Robert
// filter, and the surface reset of a tracer module.
#pragma once
#include "kernels_common.hpp"

namespace pop {

// add_kpp_sources (vmix_kpp.F90:2747-2790) for a passive tracer: KPP_SRC(k,n) = STF(n) / dz(k) * (VDC(k-1,2) GHAT(k-1) - VDC(k,2) GHAT(k)).
// The bracket is the same for every tracer of salinity's class; k_kpp_blmix<., ., ., true> leaves it in X while it forms salinity's
// source, and the product below is the one it forms there (stf / dzk * x), so a passive tracer given salinity's STF gets salinity's
// source bit for bit.  3-D parallel; blockIdx.z = block * np + slot.
struct KppSrcPassiveArgs { const double *STF[2]; double *SRC[2]; };
template <bool PBC = false>
__global__ void __launch_bounds__(256)
k_kpp_src_passive(DevGrid g, const double *__restrict__ X, KppSrcPassiveArgs a, int np) {
  const int p2 = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y + 1, b = blockIdx.z / np, n = blockIdx.z % np;
  if (p2 >= g.n2) return;
  const long long q2 = (long long)b * g.n2 + p2, o = (long long)b * g.n3 + (long long)(k - 1) * g.n2 + p2;
  const double dzk = (PBC && k > 1) ? pbc_dz(g, k, g.KMT[q2], g.DZBC[q2]) : g.dz[k];
  a.SRC[n][o] = a.STF[n][q2] / dzk * X[o];
}

// averaging step (step_mod.F90:663-796) of one passive tracer: the thickness-weighted surface level of k_avg2d and the levels
// k >= 2 of k_avg3d, same expressions.  Reads PSURF of the three time levels as they are before k_avg2d averages them: launched first.
struct AvgPassiveArgs { double *TO[2], *TC[2]; const double *TN[2]; const double *PO, *PC, *PN; double dz1, grav; };
__global__ void __launch_bounds__(256)
k_avg_passive(DevGrid g, AvgPassiveArgs a, int np) {
  const int p2 = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y + 1, b = blockIdx.z / np, n = blockIdx.z % np;
  if (p2 >= g.n2) return;
  const long long q = (long long)b * g.n2 + p2, o = (long long)b * g.n3 + (long long)(k - 1) * g.n2 + p2;
  const double to = a.TO[n][o], tc = a.TC[n][o], tn = a.TN[n][o];
  if (k >= 2) {
    a.TO[n][o] = 0.5 * (to + tc);
    a.TC[n][o] = 0.5 * (tc + tn);
    return;
  }
  const double po = a.PO[q], pc = a.PC[q], pn = a.PN[q];
  const double pfo = 0.5 * (po + pc), pfc = 0.5 * (pc + pn);
  double t = 0.5 * ((a.dz1 + po / a.grav) * to + (a.dz1 + pc / a.grav) * tc);
  t = t / (a.dz1 + pfo / a.grav);
  const double mn = fmin(to, tc), mx = fmax(to, tc);
  if (t < mn) t = mn;
  if (t > mx) t = mx;
  a.TO[n][o] = t;
  double t2 = 0.5 * ((a.dz1 + pc / a.grav) * tc + (a.dz1 + pn / a.grav) * tn);
  t2 = t2 / (a.dz1 + pfc / a.grav);
  const double mn2 = fmin(tc, tn), mx2 = fmax(tc, tn);
  if (t2 < mn2) t2 = mn2;
  if (t2 > mx2) t2 = mx2;
  a.TC[n][o] = t2;
}

// Robert filter, surface tracer = (tracer * thickness) / thickness (step_mod.F90:1121-1145) of one passive tracer with the adjusted
// PSURF: the division k_rf_psurf_adjust makes for T and S
__global__ void k_rf_surface_div(DevGrid g, RfParams p, const double *__restrict__ PC, const double *__restrict__ PN,
                                 double *__restrict__ TC, double *__restrict__ TN) {
  const long long q2 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q2 >= (long long)g.n2 * g.nblocks) return;
  const long long b = q2 / g.n2, q = b * g.n3 + (q2 - b * g.n2);
  if (p.nonzero_new) TN[q] = TN[q] / (p.dz1 + PN[q2] / p.grav);
  TC[q] = TC[q] / (p.dz1 + PC[q2] / p.grav);
}

}  // namespace pop
