// kernels_bckgrnd.hpp -- the latitude-varying KPP background diffusivity (lhoriz_varying_bckgrnd, vmix_kpp.F90:544-611) inside the
// interior coefficients: bckgrnd_vdc(i,j) and bckgrnd_vvc(i,j) where ri_iwmix reads the per-level background (:1886-1898).  The two
// 2-D fields come from host_bckgrnd.cpp.
//
// Arrangement (that of kernels_tidal.hpp): with the varying background on the interior kernels of kernels_kpp.hpp run with a
// background of zeros and write
//   VISC = rich_mix f3,  VDC = rich_mix f3 (+ double diffusion),  0 at k >= KMT,
// and k_kpp_bckgrnd, launched behind them on the same stream and before k_kpp_blmix, adds bckgrnd_vvc to VISC and bckgrnd_vdc to VDC.
// With tidal mixing on there is no such pass: k_kpp_tidal<PBC, true> reads the column's two values from the same fields.
// A sum of two terms does not depend on their order, so without double diffusion the result is bitwise the reference's
// bckgrnd + rich_mix f3 (0 + bckgrnd with lrich off), with it within a rounding of the three-term sum.
#pragma once

namespace pop {

struct BckDev {
  const double *VDC = nullptr, *VVC = nullptr, *VVC_PR = nullptr;   // bckgrnd_vdc, Prandtl bckgrnd_vdc, (Prandtl bckgrnd_vdc) / Prandtl: (nxb, nyb, nblocks)
};

// One thread per column, i fastest, marching k over the levels above the bottom (k < KMT: the interior kernels wrote 0 at and below it
// and nothing is added there).  The two 2-D values are loaded once; per level a read-modify-write of VISC and of VDC (of both VDC
// arrays when the tracer classes do not share one); the operands of level k + 1 are requested before level k is stored.  No
// thickness is read, so partial bottom cells need no form of their own.
struct BckRaw { double visc, vd1, vd2; };
__global__ void __launch_bounds__(POP_COL_THREADS)
k_kpp_bckgrnd(DevGrid g, BckDev bd, int vdc_same, double *__restrict__ VISC, double *__restrict__ VDC1, double *__restrict__ VDC2) {
  Col c;
  if (!col_setup(g, c, false)) return;
  const int km = g.km;
  const long long n2 = g.n2;
  const int kmt = g.KMT[c.q2];
  if (kmt < 2) return;
  const double bvdc = bd.VDC[c.q2], bvvc = bd.VVC[c.q2];
  const long long vb = ((long long)c.b * (km + 2)) * n2 + c.p2;
  auto load = [&](int k) {
    BckRaw r;
    r.visc = VISC[c.base3 + (long long)(k - 1) * n2]; r.vd1 = VDC1[vb + (long long)k * n2];
    r.vd2 = vdc_same ? 0.0 : VDC2[vb + (long long)k * n2];
    return r;
  };
  BckRaw cu = load(1);
#pragma unroll 1
  for (int k = 1; k < kmt; ++k) {                      // k <= km - 1
    const BckRaw nx = load(k + 1 < kmt ? k + 1 : k);
    VISC[c.base3 + (long long)(k - 1) * n2] = cu.visc + bvvc;
    VDC1[vb + (long long)k * n2] = cu.vd1 + bvdc;
    if (!vdc_same) VDC2[vb + (long long)k * n2] = cu.vd2 + bvdc;
    cu = nx;
  }
}

}  // namespace pop
