// kernels_forcing.hpp -- the coupled surface forcing on the device: ocn_import's unit conversions and rotate_wind_stress
// (drivers/mct/ocn_import_export.F90:171-239, forcing_coupled.F90:1495-1500), pop_set_coupled_forcing (forcing_coupled.F90:677-945)
// and the per-step tail of set_surface_forcing (forcing.F90:379-437).
//
// All three kernels stream over the n2 x nblocks cells of the 2-D plane, ghost cells included, one writer per cell, no atomics.  Grid
// (cells of the plane / (256 VEC), blocks); VEC = 2: two cells along i per thread through 16-byte accesses when the plane is even (every
// block's plane then starts on a 16-byte boundary), as k_tavg_cells does.  Every raw field is read once.  The arithmetic is pointwise
// and in the reference's order of operations (the library is built with -ffp-contract=off), so a ghost cell whose inputs equal its
// source cell's ends with the source cell's bits.  The rotation reads cos(ANGLET), sin(ANGLET) formed once on the host with libm: no
// kernel evaluates a trigonometric function.
#pragma once
#include "kernels_common.hpp"
#include "kernels_ice.hpp"
#include "kernels_barotropic.hpp"

namespace pop {

// the x2o fields as pop_x2o lists them, and the imported fields the library keeps
enum CplRaw { X_TAUX = 0, X_TAUY, X_SNOW, X_RAIN, X_EVAP, X_MELTW, X_ROFL, X_ROFI, X_SALT, X_SWNET, X_SEN, X_LWUP, X_LWDN, X_MELTH, X_IFRAC, X_PSLV, X_DUU10N, X_NF };
enum CplField { CF_SNOW = 0, CF_PREC, CF_EVAP, CF_MELT, CF_ROFF, CF_IOFF, CF_SALT, CF_SENH, CF_LWUP, CF_LWDN, CF_MELTH, CF_IFRAC, CF_PRESS, CF_U10, CF_NF };

template <int VEC> struct CplVec { double v[VEC]; };
template <int VEC> __device__ __forceinline__ CplVec<VEC> cpl_load(const double *p, long long q) {
  CplVec<VEC> r;
  if constexpr (VEC == 2) { const double2 t = *(const double2 *)(p + q); r.v[0] = t.x; r.v[1] = t.y; }
  else r.v[0] = p[q];
  return r;
}
// a field the caller did not give (NULL) reads as zeros
template <int VEC> __device__ __forceinline__ CplVec<VEC> cpl_load0(const double *p, long long q) {
  if (p) return cpl_load<VEC>(p, q);
  CplVec<VEC> r;
#pragma unroll
  for (int s = 0; s < VEC; ++s) r.v[s] = 0.0;
  return r;
}
template <int VEC> __device__ __forceinline__ void cpl_store(double *p, long long q, const CplVec<VEC> &r) {
  if constexpr (VEC == 2) *(double2 *)(p + q) = make_double2(r.v[0], r.v[1]);
  else p[q] = r.v[0];
}

// ---- k_cpl_import: unit conversion, land masking and the rotation of the wind stress into grid coordinates
struct CplImportArgs {
  const double *raw[X_NF];          // staged x2o fields, (n2, nblocks) each; null = zeros
  double *F[CF_NF];                 // the imported fields
  double *SHF_QSW, *SMFT1, *SMFT2;
  const double *COSA, *SINA;        // cos(ANGLET), sin(ANGLET)
  double hflux_factor, momentum_factor;
};
template <int VEC>
__global__ __launch_bounds__(256) void k_cpl_import(DevGrid g, CplImportArgs a) {
#pragma clang fp contract(off)
  const int p2 = (blockIdx.x * 256 + threadIdx.x) * VEC;
  if (p2 >= g.n2) return;
  const long long q = (long long)blockIdx.y * g.n2 + p2;
  typedef CplVec<VEC> V;
  const V rc = cpl_load<VEC>(g.RCALCT, q), ca = cpl_load<VEC>(a.COSA, q), sa = cpl_load<VEC>(a.SINA, q);
  const V taux = cpl_load0<VEC>(a.raw[X_TAUX], q), tauy = cpl_load0<VEC>(a.raw[X_TAUY], q);
  const V snow = cpl_load0<VEC>(a.raw[X_SNOW], q), rain = cpl_load0<VEC>(a.raw[X_RAIN], q);
  const V swnet = cpl_load0<VEC>(a.raw[X_SWNET], q), ifrac = cpl_load0<VEC>(a.raw[X_IFRAC], q);
  const V pslv = cpl_load0<VEC>(a.raw[X_PSLV], q), duu = cpl_load0<VEC>(a.raw[X_DUU10N], q);
  V prec, qsw, ifr, press, u10, s1, s2;
#pragma unroll
  for (int s = 0; s < VEC; ++s) {
    prec.v[s] = rain.v[s] + snow.v[s];                              // ocn_import_export.F90:220
    qsw.v[s] = swnet.v[s] * rc.v[s] * a.hflux_factor;               // :223-224
    ifr.v[s] = ifrac.v[s] * rc.v[s];                                // :231
    press.v[s] = 10.0 * pslv.v[s] * rc.v[s];                        // :235  Pa -> dyne/cm^2
    u10.v[s] = 100.0 * 100.0 * duu.v[s] * rc.v[s];                  // :239  m^2/s^2 -> cm^2/s^2
    s1.v[s] = (taux.v[s] * ca.v[s] + tauy.v[s] * sa.v[s]) * rc.v[s] * a.momentum_factor;   // forcing_coupled.F90:1495-1497
    s2.v[s] = (tauy.v[s] * ca.v[s] - taux.v[s] * sa.v[s]) * rc.v[s] * a.momentum_factor;   // :1498-1500
  }
  cpl_store<VEC>(a.F[CF_SNOW], q, snow); cpl_store<VEC>(a.F[CF_PREC], q, prec);
  cpl_store<VEC>(a.F[CF_EVAP], q, cpl_load0<VEC>(a.raw[X_EVAP], q)); cpl_store<VEC>(a.F[CF_MELT], q, cpl_load0<VEC>(a.raw[X_MELTW], q));
  cpl_store<VEC>(a.F[CF_ROFF], q, cpl_load0<VEC>(a.raw[X_ROFL], q)); cpl_store<VEC>(a.F[CF_IOFF], q, cpl_load0<VEC>(a.raw[X_ROFI], q));
  cpl_store<VEC>(a.F[CF_SALT], q, cpl_load0<VEC>(a.raw[X_SALT], q)); cpl_store<VEC>(a.F[CF_SENH], q, cpl_load0<VEC>(a.raw[X_SEN], q));
  cpl_store<VEC>(a.F[CF_LWUP], q, cpl_load0<VEC>(a.raw[X_LWUP], q)); cpl_store<VEC>(a.F[CF_LWDN], q, cpl_load0<VEC>(a.raw[X_LWDN], q));
  cpl_store<VEC>(a.F[CF_MELTH], q, cpl_load0<VEC>(a.raw[X_MELTH], q));
  cpl_store<VEC>(a.F[CF_IFRAC], q, ifr); cpl_store<VEC>(a.F[CF_PRESS], q, press); cpl_store<VEC>(a.F[CF_U10], q, u10);
  cpl_store<VEC>(a.SHF_QSW, q, qsw); cpl_store<VEC>(a.SMFT1, q, s1); cpl_store<VEC>(a.SMFT2, q, s2);
}

// ---- k_cpl_combine: SMF = tgrid_to_ugrid(SMFT), the heat flux, the fresh-water fluxes (FWF) or the virtual salt flux, the interval's
//      copies.  Reads the imported fields after their halo update; T, S: the surface level of TRACER(cur)
struct CplCombineArgs {
  const double *F[CF_NF];
  const double *SMFT1, *SMFT2, *T, *S;   // T, S: (n2, km, nblocks), level 1 read
  const double *SHF_QSW;
  double *SMF1, *SMF2, *STF1, *STF2, *FW, *TFW1, *TFW2;
  double *SHF_COMP_QSW, *SFWF_COMP, *TFW_COMP1, *TFW_COMP2;   // the last three: null unless ice formation is on (forcing_coupled.F90:886-890)
  double lhv, lhf, hflux_factor, salinity_factor, sflux_factor, fwmass_to_fwflux;
  int tfz, lactive_ice;
};
template <int VEC, bool FWF>
__global__ __launch_bounds__(256) void k_cpl_combine(DevGrid g, CplCombineArgs a) {
#pragma clang fp contract(off)
  const int p2 = (blockIdx.x * 256 + threadIdx.x) * VEC;
  if (p2 >= g.n2) return;
  const int b = blockIdx.y;
  const long long q = (long long)b * g.n2 + p2, q3 = (long long)b * g.n3 + p2;
  typedef CplVec<VEC> V;
  const V rc = cpl_load<VEC>(g.RCALCT, q);
  const V evap = cpl_load<VEC>(a.F[CF_EVAP], q), senh = cpl_load<VEC>(a.F[CF_SENH], q), lwup = cpl_load<VEC>(a.F[CF_LWUP], q);
  const V lwdn = cpl_load<VEC>(a.F[CF_LWDN], q), melth = cpl_load<VEC>(a.F[CF_MELTH], q), snow = cpl_load<VEC>(a.F[CF_SNOW], q);
  const V ioff = cpl_load<VEC>(a.F[CF_IOFF], q), prec = cpl_load<VEC>(a.F[CF_PREC], q), roff = cpl_load<VEC>(a.F[CF_ROFF], q);
  const V melt = cpl_load<VEC>(a.F[CF_MELT], q), salt = cpl_load<VEC>(a.F[CF_SALT], q);
  V stf1;
#pragma unroll
  for (int s = 0; s < VEC; ++s)   // forcing_coupled.F90:723-727
    stf1.v[s] = (evap.v[s] * a.lhv + senh.v[s] + lwup.v[s] + lwdn.v[s] + melth.v[s] - (snow.v[s] + ioff.v[s]) * a.lhf) * rc.v[s] * a.hflux_factor;
  cpl_store<VEC>(a.STF1, q, stf1);
  if constexpr (FWF) {   // :748-790
    const V t = cpl_load<VEC>(a.T, q3), sal = cpl_load<VEC>(a.S, q3);
    V fw, tfw1, tfw2;
#pragma unroll
    for (int s = 0; s < VEC; ++s) {
      const double fw0 = rc.v[s] * (prec.v[s] + evap.v[s] + roff.v[s] + ioff.v[s]) * a.fwmass_to_fwflux;
      const double w1 = rc.v[s] * melt.v[s] * a.fwmass_to_fwflux;
      const double w2 = a.lactive_ice ? 0.0 : ice_tfreez(a.tfz, sal.v[s]);   // tmelt (ice.F90:764-790)
      tfw1.v[s] = fw0 * t.v[s] + w1 * w2;
      fw.v[s] = fw0 + w1;
      const double sm = (melt.v[s] != 0.0) ? salt.v[s] / melt.v[s] : 0.0;   // salinity of the melt water
      tfw2.v[s] = rc.v[s] * melt.v[s] * a.fwmass_to_fwflux * sm;
    }
    cpl_store<VEC>(a.FW, q, fw); cpl_store<VEC>(a.TFW1, q, tfw1); cpl_store<VEC>(a.TFW2, q, tfw2);
    if (a.SFWF_COMP) { cpl_store<VEC>(a.SFWF_COMP, q, fw); cpl_store<VEC>(a.TFW_COMP1, q, tfw1); cpl_store<VEC>(a.TFW_COMP2, q, tfw2); }
  } else {               // :813-817 with MASK_ESTUARY = 0
    V stf2;
#pragma unroll
    for (int s = 0; s < VEC; ++s)
      stf2.v[s] = rc.v[s] * ((prec.v[s] + evap.v[s] + melt.v[s] + roff.v[s] + ioff.v[s]) * a.salinity_factor + salt.v[s] * a.sflux_factor);
    cpl_store<VEC>(a.STF2, q, stf2);
  }
  cpl_store<VEC>(a.SHF_COMP_QSW, q, cpl_load<VEC>(a.SHF_QSW, q));   // :856, :867
  // tgrid_to_ugrid (grid.F90:3399-3415): the northeast four-point average, 0 in the last row and column of the block array
  const V au0 = cpl_load<VEC>(g.AU0, q), aun = cpl_load<VEC>(g.AUN, q), aue = cpl_load<VEC>(g.AUE, q), aune = cpl_load<VEC>(g.AUNE, q);
  const V c1 = cpl_load<VEC>(a.SMFT1, q), c2 = cpl_load<VEC>(a.SMFT2, q);
  V smf1, smf2;
#pragma unroll
  for (int s = 0; s < VEC; ++s) {
    const int p = p2 + s, i = p % g.nxb, j = p / g.nxb;
    double u1 = 0.0, u2 = 0.0;
    if (i < g.nxb - 1 && j < g.nyb - 1) {
      const long long o = q + s;
      const double e1 = (s + 1 < VEC) ? c1.v[(s + 1) % VEC] : a.SMFT1[o + 1], e2 = (s + 1 < VEC) ? c2.v[(s + 1) % VEC] : a.SMFT2[o + 1];
      u1 = au0.v[s] * c1.v[s] + aun.v[s] * a.SMFT1[o + g.nxb] + aue.v[s] * e1 + aune.v[s] * a.SMFT1[o + g.nxb + 1];
      u2 = au0.v[s] * c2.v[s] + aun.v[s] * a.SMFT2[o + g.nxb] + aue.v[s] * e2 + aune.v[s] * a.SMFT2[o + g.nxb + 1];
    }
    smf1.v[s] = u1; smf2.v[s] = u2;
  }
  cpl_store<VEC>(a.SMF1, q, smf1); cpl_store<VEC>(a.SMF2, q, smf2);
}

// ---- k_sfc_forcing_step: the per-step tail of set_surface_forcing (forcing.F90:379-437).  The factor table is in device memory, the
//      index a kernel argument.  ICE: FW = SFWF_COMP + FW_FREEZE, TFW(1) = TFW_COMP(1) + FW_FREEZE TFRZ, TFW(2) = TFW_COMP(2) + FW_FREEZE salice
struct SfcStepArgs {
  const double *qsw_factor; int index_qsw;    // 0-based
  const double *SHF_COMP_QSW, *SFWF_COMP, *TFW_COMP1, *TFW_COMP2, *FW_FREEZE, *S;
  double *SHF_QSW, *FW, *TFW1, *TFW2;
  double salice; int tfz;
};
template <int VEC, bool ICE>
__global__ __launch_bounds__(256) void k_sfc_forcing_step(DevGrid g, SfcStepArgs a) {
#pragma clang fp contract(off)
  const int p2 = (blockIdx.x * 256 + threadIdx.x) * VEC;
  if (p2 >= g.n2) return;
  const int b = blockIdx.y;
  const long long q = (long long)b * g.n2 + p2, q3 = (long long)b * g.n3 + p2;
  typedef CplVec<VEC> V;
  const double f = a.qsw_factor[a.index_qsw];
  V qsw = cpl_load<VEC>(a.SHF_COMP_QSW, q);
#pragma unroll
  for (int s = 0; s < VEC; ++s) qsw.v[s] = f * qsw.v[s];            // forcing.F90:410
  cpl_store<VEC>(a.SHF_QSW, q, qsw);
  if constexpr (ICE) {                                               // :417-437
    const V fwf = cpl_load<VEC>(a.FW_FREEZE, q), sal = cpl_load<VEC>(a.S, q3);
    V fw = cpl_load<VEC>(a.SFWF_COMP, q), t1 = cpl_load<VEC>(a.TFW_COMP1, q), t2 = cpl_load<VEC>(a.TFW_COMP2, q);
#pragma unroll
    for (int s = 0; s < VEC; ++s) {
      fw.v[s] = fw.v[s] + fwf.v[s];
      t1.v[s] = t1.v[s] + fwf.v[s] * ice_tfreez(a.tfz, sal.v[s]);
      t2.v[s] = t2.v[s] + fwf.v[s] * a.salice;
    }
    cpl_store<VEC>(a.FW, q, fw); cpl_store<VEC>(a.TFW1, q, t1); cpl_store<VEC>(a.TFW2, q, t2);
  }
}

// ---- marginal-sea balance (ms_balancing, ms_balance.F90:577-642) in the virtual-salt-flux branch.
// k_ms_transport: inside every marginal sea the per-cell TRANSPORT term [kg/s of fresh water] and the overwrite of STF2 (:602-609);
// 0 elsewhere.  A cell lies in at most one sea; IND[s] is the indicator REGION_MASK == number of sea s.  QFLUX null: zeros
struct MsArgs {
  const double *F[CF_NF];
  const double *QFLUX, *DXT, *DYT;
  const double *IND[POP_MAX_MS], *MASK_FRAC[POP_MAX_MS];
  double *STF2, *TRANSPORT;
  const double *sums;               // the reduced transport of every sea, device memory (k_ms_distribute)
  double c_q, c_s, c_a, c_t;
  int nseas;
};
template <int VEC>
__global__ __launch_bounds__(256) void k_ms_transport(DevGrid g, MsArgs a) {
#pragma clang fp contract(off)
  const int p2 = (blockIdx.x * 256 + threadIdx.x) * VEC;
  if (p2 >= g.n2) return;
  const long long q = (long long)blockIdx.y * g.n2 + p2;
  typedef CplVec<VEC> V;
  V in;
#pragma unroll
  for (int s = 0; s < VEC; ++s) in.v[s] = 0.0;
  for (int m = 0; m < a.nseas; ++m) {
    const V x = cpl_load<VEC>(a.IND[m], q);
#pragma unroll
    for (int s = 0; s < VEC; ++s) in.v[s] = (x.v[s] != 0.0) ? 1.0 : in.v[s];
  }
  const V evap = cpl_load<VEC>(a.F[CF_EVAP], q), prec = cpl_load<VEC>(a.F[CF_PREC], q), melt = cpl_load<VEC>(a.F[CF_MELT], q);
  const V roff = cpl_load<VEC>(a.F[CF_ROFF], q), ioff = cpl_load<VEC>(a.F[CF_IOFF], q), salt = cpl_load<VEC>(a.F[CF_SALT], q);
  const V qf = cpl_load0<VEC>(a.QFLUX, q), dxt = cpl_load<VEC>(a.DXT, q), dyt = cpl_load<VEC>(a.DYT, q);
  V stf2 = cpl_load<VEC>(a.STF2, q), tr;
#pragma unroll
  for (int s = 0; s < VEC; ++s) {
    const double work = evap.v[s] + prec.v[s] + melt.v[s] + roff.v[s] + ioff.v[s];   // :577
    const double qpos = fmax(0.0, qf.v[s]);
    const double t = (qpos * a.c_q + work * 1.0 + salt.v[s] * a.c_s) * dxt.v[s] * dyt.v[s] * a.c_a;
    const double o = -qpos * a.c_q * a.c_t * 1.0e-4;
    tr.v[s] = (in.v[s] != 0.0) ? t : 0.0;
    stf2.v[s] = (in.v[s] != 0.0) ? o : stf2.v[s];
  }
  cpl_store<VEC>(a.TRANSPORT, q, tr); cpl_store<VEC>(a.STF2, q, stf2);
}
// the reduced sum of one sea from the scalars of the global sum into the vector of transports
__global__ void k_ms_keep(const SolverScalars *sc, double *sums, int sea) {
  if (threadIdx.x == 0 && blockIdx.x == 0) sums[sea] = sc->sum0;
}
// k_ms_distribute: STF2 += MASK_FRAC(sea) * transport(sea) * c_t / (DXT * DYT), seas in region order (:637-640)
template <int VEC>
__global__ __launch_bounds__(256) void k_ms_distribute(DevGrid g, MsArgs a) {
#pragma clang fp contract(off)
  const int p2 = (blockIdx.x * 256 + threadIdx.x) * VEC;
  if (p2 >= g.n2) return;
  const long long q = (long long)blockIdx.y * g.n2 + p2;
  typedef CplVec<VEC> V;
  const V dxt = cpl_load<VEC>(a.DXT, q), dyt = cpl_load<VEC>(a.DYT, q);
  V stf2 = cpl_load<VEC>(a.STF2, q);
  for (int m = 0; m < a.nseas; ++m) {
    const V mf = cpl_load<VEC>(a.MASK_FRAC[m], q);
    const double t = a.sums[m];
#pragma unroll
    for (int s = 0; s < VEC; ++s) stf2.v[s] = stf2.v[s] + mf.v[s] * t * a.c_t / (dxt.v[s] * dyt.v[s]);
  }
  cpl_store<VEC>(a.STF2, q, stf2);
}

}  // namespace pop
