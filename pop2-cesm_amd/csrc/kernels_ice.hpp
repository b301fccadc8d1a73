// kernels_ice.hpp -- frazil ice formation (ice.F90:357-717) on the device.
//
// k_ice_formation is ice_formation: one thread per column (i, j, block), i fastest, so every level's loads and stores are coalesced
// 2-D rows; every cell of every local block, ghost cells included (the kernel is pointwise: a ghost cell whose inputs equal its source
// cell's ends with the source cell's bits).  The march is k = kmxice .. 2, then the surface level with its two passes; POTICE and QICE
// stay in registers.  With kmxice = 1 the pass moves about ten 2-D words per column (T, S, PSURF, KMT, AQICE in; T, S, RHO, QICE,
// AQICE [, FW_FREEZE] out): memory-bound and small beside a step, so there is one form of it and no tuning switch.
// Arithmetic is in the reference's evaluation order (the library is built with -ffp-contract=off).
#pragma once
#include "kernels_common.hpp"

namespace pop {

// Freezing point of sea water [deg C] from salinity in model units [g/g]: tfreez (ice.F90:725-757), which calls shr_frz_freezetemp of
// CIME's shr_frz_mod with S * salt_to_ppt.  shr_frz_mod is not part of POP; the three forms below restate it from memory (DESIGN.md
// section 13) and are kept in this one function -- host and device -- so that a correction is a single line.
// option: 0 'minus1p8', 1 'linear_salt', 2 'mushy'; each bounded below by -2.
__host__ __device__ __forceinline__ double ice_tfreez(int option, double salt) {
  const double psu = salt * 1000.0;
  const double p = psu > 0.0 ? psu : 0.0;
  double t;
  if (option == 1) t = -0.0544 * p;
  else if (option == 2) t = p / (-18.48 + 0.01848 * p);
  else t = -1.8;
  return t > -2.0 ? t : -2.0;
}

struct IceArgs {
  double *T, *S, *RHO;             // TRACER(:,:,:,1 | 2, tl), RHO(:,:,:,tl)
  const double *PS;                // PSURF(:,:,tl)
  double *QICE, *AQICE, *FWF;      // FWF = FW_FREEZE: written in the fresh-water form only
  double cpl, salice, salref;      // cp_over_lhfusion; sea-ice and reference salinity [g/g]
  double time_weight, dt1, grav;   // dt1 = dt(1)
  int kmxice, tfz, salt_flx;       // salt_flx = lfw_as_salt_flx
};

template <bool PBC, bool SALT>
__global__ void __launch_bounds__(256) k_ice_formation(DevGrid g, IceArgs a) {
  const int p2 = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (p2 >= g.n2) return;
  const long long q2 = (long long)b * g.n2 + p2, base3 = (long long)b * g.n3 + p2;
  const int kmt = g.KMT[q2];
  double dzbot = 0.0;
  if (PBC) dzbot = g.DZBC[q2];
  const double ref_val = a.salref - a.salice;
  double qice = 0.0, potice = 0.0;
  // sub-surface levels (ice.F90:459-525): heat of a warm level melts ice formed below it (POTICE limited by QICE)
  for (int k = a.kmxice; k >= 2; --k) {
    const long long o = base3 + (long long)(k - 1) * g.n2;
    double t = a.T[o], s = a.S[o];
    const double dzk = PBC ? pbc_dz(g, k, kmt, dzbot) : g.dz[k];
    const double tfrz = ice_tfreez(a.tfz, s);
    if (k <= kmt) potice = (tfrz - t) * dzk;
    potice = fmax(potice, qice);
    t = t + potice / dzk;
    if (SALT) s = s + ref_val * potice * a.cpl / dzk;
    else s = (s * (dzk + a.cpl * qice) + a.cpl * (a.S[o - g.n2] * (potice - qice) - a.salice * potice)) / dzk;
    qice = qice - potice;
    a.T[o] = t; a.S[o] = s;
    a.RHO[o] = mwjf_rho<false>(mwjf_level(g.pressz[k]), t, s, nullptr, nullptr);
  }
  // surface level (:535-569): its thickness follows the surface height
  double t = a.T[base3], s = a.S[base3];
  double w = PBC ? pbc_dz(g, 1, kmt, dzbot) : g.dz[1];
  w = w + a.PS[q2] / a.grav + 1.0e-20;   // eps2
  double tfrz = ice_tfreez(a.tfz, s);
  if (1 <= kmt) potice = (tfrz - t) * w;
  potice = fmax(potice, qice);
  t = t + potice / w;
  if (SALT) s = s + ref_val * potice * a.cpl / w;
  else s = (s * (w + a.cpl * qice) - a.salice * qice * a.cpl) / w;
  qice = qice - potice;
  // residual heat of the surface level melts ice formed earlier (:577-614)
  double aq = a.AQICE[q2] + a.time_weight * qice;
  tfrz = ice_tfreez(a.tfz, s);
  if (1 <= kmt) potice = (tfrz - t) * w;
  potice = fmax(potice, aq);
  t = t + potice / w;
  if (SALT) s = s + ref_val * potice * a.cpl / w;
  else a.FWF[q2] = a.time_weight * fmin(potice, qice) * a.cpl / a.dt1;
  aq = aq - a.time_weight * potice;
  a.T[base3] = t; a.S[base3] = s;
  a.RHO[base3] = mwjf_rho<false>(mwjf_level(g.pressz[1]), t, s, nullptr, nullptr);
  a.QICE[q2] = qice; a.AQICE[q2] = aq;
}

inline void launch_ice_formation(const DevGrid &g, const IceArgs &a, hipStream_t st) {
  with_flags([&](auto PBC, auto SALT) {
    hipLaunchKernelGGL((k_ice_formation<PBC.value, SALT.value>), dim3((g.n2 + 255) / 256, g.nblocks), dim3(256), 0, st, g, a);
  }, g.pbc != 0, a.salt_flx != 0);
}

// ice_flx_to_coupler (ice.F90:625-717) on TRACER(cur), PSURF(cur); rlast = 0: QFLUX = 0 (tlast_ice = 0)
struct IceFlxArgs {
  const double *T, *S, *PS;
  double *QICE, *AQICE, *QFLUX;
  double grav, tlast_ice, hflux_factor;
  int tfz, halve;
};
template <bool PBC>
__global__ void __launch_bounds__(256) k_ice_flx_to_coupler(DevGrid g, IceFlxArgs a) {
  const int p2 = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (p2 >= g.n2) return;
  const long long q2 = (long long)b * g.n2 + p2, base3 = (long long)b * g.n3 + p2;
  const int kmt = g.KMT[q2];
  const double tfrz = ice_tfreez(a.tfz, a.S[base3]);
  double w = PBC ? pbc_dz(g, 1, kmt, g.DZBC[q2]) : g.dz[1];
  w = w + a.PS[q2] / a.grav + 1.0e-20;
  double melt = 0.0;
  if (1 <= kmt) melt = (tfrz - a.T[base3]) * w;
  double aq = a.AQICE[q2];
  if (a.halve) aq = 0.5 * aq;
  const double q = (aq < 0.0) ? -aq : melt;
  a.AQICE[q2] = aq; a.QICE[q2] = q;
  a.QFLUX[q2] = (a.tlast_ice == 0.0) ? 0.0 : q / a.tlast_ice / a.hflux_factor;
}

}  // namespace pop
