// kernels_aniso.hpp -- anisotropic horizontal viscosity (hmix_momentum = 3, 'anis'): hdiffu_aniso (hmix_aniso.F90:557-1062)
// for every level of every local block, into the 3-D fields HDU, HDV that the momentum right-hand side adds
// (k_momentum_rhs<true>, k_momentum_rhs_lds<R, PBC, true>).
//
// The friction at (i,j) is the divergence of the quarter-cell stresses of (i,j) and of its four neighbours (:940-1018); each
// stress needs the strain of its own point (:718-765), i.e. U, V on the radius-2 diamond of (i,j).  k_hdiffu_aniso forms every
// stress once per level in LDS and shares it with the four neighbours (below).  Every expression keeps the reference's operation
// order (the library is built with -ffp-contract=off), so a restatement in that order agrees to the last bit except where
// cos / sin differ.
//
// Geometry H1E ... K2S, AMAX_CFL, DSMIN, F_PERP_SMAG, ANGLE and the variable viscosities F_PARA, F_PERP (3-D) come from
// host_setup.cpp (init_aniso :372-533, compute_ccsm_var_viscosity :1069-1296).  Partial bottom cells: the ratios GW, GE, GS,
// GN (:689-710) of the thickness DZU that pbc_dz forms from KMU / DZUB.
#pragma once
#include "kernels_common.hpp"

namespace pop {

struct AnisoArgs {
  const double *UM, *VM;                    // U, V at the mix time level
  double *HDU, *HDV;                        // out: Hdiff(U), Hdiff(V), 3-D
  const double *H1E, *H1W, *H2N, *H2S, *K1E, *K1W, *K2N, *K2S;
  const double *AMAX, *DSMIN, *FPS, *ANGLE, *UAREA;   // AMAX_CFL; Smagorinsky: DSMIN, F_PERP_SMAG; 'east': ANGLE
  const double *FPARA, *FPERP;              // lvariable_hmix_aniso: 3-D, level k at (k-1)*n2
  double visc_para, visc_perp, c_para, c_perp;
  int east, variable, smag;                 // alignment 'east' (else 'grid'); F_PARA / F_PERP; Smagorinsky
};

// the quarter-cell stresses of one point: strain (:718-765), viscosities (:807-869), coefficients (:881-911), stress (:913-926)
struct AnisoPoint { double S11[4], S22[4], S12[4]; };

__device__ __forceinline__ AnisoPoint aniso_stress(const AnisoArgs &a, long long q, long long o, double u0, double uw_, double ue_, double us_,
                                                   double un_, double v0, double vw_, double ve_, double vs_, double vn_, double gw, double ge,
                                                   double gs, double gn) {
  const double uw = gw * uw_, ue = ge * ue_, us = gs * us_, un = gn * un_;
  const double vw = gw * vw_, ve = ge * ve_, vs = gs * vs_, vn = gn * vn_;
  const double h1w = a.H1W[q], h1e = a.H1E[q], h2s = a.H2S[q], h2n = a.H2N[q];
  const double k1w = a.K1W[q], k1e = a.K1E[q], k2s = a.K2S[q], k2n = a.K2N[q];
  double E11[4], E22[4], E12[4];
  {
    const double w1 = (u0 - uw) / h1w, w2 = (ue - u0) / h1e;
    const double w3 = 0.5 * k2s * (v0 + vs), w4 = 0.5 * k2n * (v0 + vn);
    E11[0] = w1 + w3; E11[1] = w1 + w4; E11[2] = w2 + w4; E11[3] = w2 + w3;
  }
  {
    const double w1 = (v0 - vs) / h2s, w2 = (vn - v0) / h2n;
    const double w3 = 0.5 * k1w * (u0 + uw), w4 = 0.5 * k1e * (u0 + ue);
    E22[0] = w1 + w3; E22[1] = w2 + w3; E22[2] = w2 + w4; E22[3] = w1 + w4;
  }
  {
    const double w1 = (u0 - us) / h2s, w2 = (un - u0) / h2n, w3 = (v0 - vw) / h1w, w4 = (ve - v0) / h1e;
    const double w5 = k2s * (u0 + us), w6 = k2n * (u0 + un), w7 = k1w * (v0 + vw), w8 = k1e * (v0 + ve);
    E12[0] = w1 + w3 - 0.5 * (w5 + w7); E12[1] = w2 + w3 - 0.5 * (w6 + w7);
    E12[2] = w2 + w4 - 0.5 * (w6 + w8); E12[3] = w1 + w4 - 0.5 * (w5 + w8);
  }
  double V1[4], V2[4];
  if (a.smag) {
    const double ds = a.DSMIN[q], fps = a.FPS[q], amax = a.AMAX[q];
    const double fpa = a.variable ? a.FPARA[o] : 0.0, fpe = a.variable ? a.FPERP[o] : 0.0;
#pragma unroll
    for (int iq = 0; iq < 4; ++iq) {
      const double w6 = sqrt(2.0 * (E11[iq] * E11[iq] + E22[iq] * E22[iq]) + E12[iq] * E12[iq]);   // |D|
      double t1 = a.c_para * 1.0 * w6 * ds * ds;   // F_PARA_SMAG = 1 (:515)
      double t2 = a.c_perp * fps * w6 * ds * ds;
      if (a.variable) { t1 = fmax(t1, fpa); t2 = fmax(t2, fpe); }
      V1[iq] = fmin(t1, amax); V2[iq] = fmin(t2, amax);
    }
  } else {
    const double t1 = a.variable ? a.FPARA[o] : a.visc_para, t2 = a.variable ? a.FPERP[o] : a.visc_perp;
#pragma unroll
    for (int iq = 0; iq < 4; ++iq) { V1[iq] = t1; V2[iq] = t2; }
  }
  AnisoPoint P;
  if (a.east) {
    const double ang = a.ANGLE[q];
    const double n1 = cos(ang), n2 = -sin(ang);
    const double nn = n1 * n2, nn2 = nn * nn, dn = n1 * n1 - n2 * n2;
#pragma unroll
    for (int iq = 0; iq < 4; ++iq) {
      const double A = 0.5 * (V1[iq] + V2[iq]) - 2.0 * (V1[iq] - V2[iq]) * nn2;
      const double B = A;
      const double C = (V1[iq] - V2[iq]) * n1 * n2 * dn;
      const double D = V2[iq] + 2.0 * (V1[iq] - V2[iq]) * nn2;
      P.S11[iq] = A * E11[iq] - B * E22[iq] + C * E12[iq];
      P.S22[iq] = -(B * E11[iq]) + A * E22[iq] - C * E12[iq];
      P.S12[iq] = C * (E11[iq] - E22[iq]) + D * E12[iq];
    }
  } else {
#pragma unroll
    for (int iq = 0; iq < 4; ++iq) {
      const double A = 0.5 * (V1[iq] + V2[iq]), B = A, C = 0.0, D = V2[iq];
      P.S11[iq] = A * E11[iq] - B * E22[iq] + C * E12[iq];
      P.S22[iq] = -(B * E11[iq]) + A * E22[iq] - C * E12[iq];
      P.S12[iq] = C * (E11[iq] - E22[iq]) + D * E12[iq];
    }
  }
  return P;
}

// LDS-tiled form: a workgroup owns a 64 x 4 tile of U columns and marches k.  Per level it stages U, V (and DZU) of the tile plus a
// 2-cell ring, forms the quarter-cell stresses of the tile plus a 1-cell ring ONCE into LDS (each thread one or two points), and
// then every thread forms the divergence of its own cell from LDS.  Two barriers per level, no double buffering: the staging of
// level k+1 starts after the second barrier of level k (nobody reads U, V after it), and the stresses of level k+1 are written after
// the first barrier of level k+1 (every thread has finished its divergence of level k).  The arithmetic of every point is
// aniso_stress, the divergence that of :943-1032: the same operations in the same order as the reference.
constexpr int ANI_TX = 64, ANI_TY = 4;
constexpr int ANI_SW = ANI_TX + 2, ANI_SN = ANI_SW * (ANI_TY + 2);   // stress points: tile + 1 ring
constexpr int ANI_UW = ANI_TX + 4, ANI_UN = ANI_UW * (ANI_TY + 4);   // U, V points: tile + 2 rings
static_assert(ANI_SN <= 2 * ANI_TX * ANI_TY && ANI_UN <= 3 * ANI_TX * ANI_TY, "points per thread");

template <bool PBC>
__global__ void __launch_bounds__(ANI_TX * ANI_TY) k_hdiffu_aniso(DevGrid g, AnisoArgs a) {
  __shared__ double su[ANI_UN], sv[ANI_UN], sz[PBC ? ANI_UN : 1];
  __shared__ double s11[4][ANI_SN], s22[4][ANI_SN], s12[4][ANI_SN];
  const int b = blockIdx.z;
  const int i0 = NGHOST + blockIdx.x * ANI_TX, j0 = NGHOST + blockIdx.y * ANI_TY;   // first cell of the tile, 0-based
  if (land_tile(g, b, i0, ANI_TX, j0, ANI_TY)) return;   // no ocean near the tile: HDU, HDV stay 0 there
  const int nxb = g.nxb, nyb = g.nyb, km = g.km;
  const long long n2 = g.n2;
  const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * ANI_TX + tx;
  const int i = i0 + tx, j = j0 + ty;
  const bool act = i + 1 <= blk_ie(g, b) && j + 1 <= blk_je(g, b);   // physical U point (i0, j0 >= ib, jb)
  const long long q = (long long)b * n2 + (long long)(act ? j * nxb + i : NGHOST * nxb + NGHOST);   // lanes without a cell read a valid one
  const long long base3 = (long long)b * g.n3 + (q - (long long)b * n2);
  const int kmu = g.KMU[q];
  const double uarea = a.UAREA[q];
  const long long qE = q + 1, qW = q - 1, qN = q + nxb, qS = q - nxb;
  const double h2s0 = a.H2S[q], h2n0 = a.H2N[q], h1w0 = a.H1W[q], h1e0 = a.H1E[q];
  const double k1w0 = a.K1W[q], k1e0 = a.K1E[q], k2s0 = a.K2S[q], k2n0 = a.K2N[q];
  const double h2sE = a.H2S[qE], h2nE = a.H2N[qE], h2sW = a.H2S[qW], h2nW = a.H2N[qW];
  const double h1wN = a.H1W[qN], h1eN = a.H1E[qN], h1wS = a.H1W[qS], h1eS = a.H1E[qS];
  const int lc = (ty + 1) * ANI_SW + tx + 1;                  // own cell among the stress points
  const int uc = (ty + 2) * ANI_UW + tx + 2;                  // own cell among the U, V points
  for (int k = 1; k <= km; ++k) {
    const long long ob = (long long)b * g.n3 + (long long)(k - 1) * n2;
    // stage U, V (DZU) of the tile + 2 rings; cells beyond the block array (overhanging tiles) hold 0 and feed no physical cell
    for (int p = tid; p < ANI_UN; p += ANI_TX * ANI_TY) {
      const int gi = i0 - 2 + p % ANI_UW, gj = j0 - 2 + p / ANI_UW;
      const bool in = gi < nxb && gj < nyb;
      const long long c2 = in ? (long long)gj * nxb + gi : 0;
      su[p] = in ? a.UM[ob + c2] : 0.0;
      sv[p] = in ? a.VM[ob + c2] : 0.0;
      if (PBC) sz[p] = in ? pbc_dz(g, k, g.KMU[(long long)b * n2 + c2], g.DZUB[(long long)b * n2 + c2]) : 1.0;
    }
    __syncthreads();
    // GW, GE, GS, GN (:694-701) of the point at U-tile position c; 1 without partial bottom cells
    auto gr = [&](int c, int e) { return PBC ? fmin(sz[c], sz[c + e]) / sz[c] : 1.0; };
    for (int p = tid; p < ANI_SN; p += ANI_TX * ANI_TY) {
      const int li = p % ANI_SW, lj = p / ANI_SW, gi = i0 - 1 + li, gj = j0 - 1 + lj;
      if (gi >= nxb - 1 || gj >= nyb - 1) continue;          // beyond the last ghost ring any physical cell reads
      const int c = (lj + 1) * ANI_UW + li + 1;
      const long long c2 = (long long)gj * nxb + gi;
      const AnisoPoint P = aniso_stress(a, (long long)b * n2 + c2, ob + c2, su[c], su[c - 1], su[c + 1], su[c - ANI_UW], su[c + ANI_UW],
                                        sv[c], sv[c - 1], sv[c + 1], sv[c - ANI_UW], sv[c + ANI_UW],
                                        gr(c, -1), gr(c, 1), gr(c, -ANI_UW), gr(c, ANI_UW));
#pragma unroll
      for (int iq = 0; iq < 4; ++iq) { s11[iq][p] = P.S11[iq]; s22[iq][p] = P.S22[iq]; s12[iq][p] = P.S12[iq]; }
    }
    const double GW = gr(uc, -1), GE = gr(uc, 1), GS = gr(uc, -ANI_UW), GN = gr(uc, ANI_UW);   // before the next level restages sz
    __syncthreads();
    if (!act) continue;
    const int cE = lc + 1, cW = lc - 1, cN = lc + ANI_SW, cS = lc - ANI_SW;
    double FX, FY, w1, w2, w3, w4;
    // x-component (:943-977)
    w1 = h2s0 * s11[0][lc] + h2n0 * s11[1][lc];
    w2 = h2s0 * s11[3][lc] + h2n0 * s11[2][lc];
    w3 = (h2sE * s11[0][cE] + h2nE * s11[1][cE]) * GE;
    w4 = (h2sW * s11[3][cW] + h2nW * s11[2][cW]) * GW;
    FX = 0.25 * (w2 + w3 - w1 - w4);
    w1 = h1w0 * s12[0][lc] + h1e0 * s12[3][lc];
    w2 = h1w0 * s12[1][lc] + h1e0 * s12[2][lc];
    w3 = (h1wN * s12[0][cN] + h1eN * s12[3][cN]) * GN;
    w4 = (h1wS * s12[1][cS] + h1eS * s12[2][cS]) * GS;
    FX = FX + 0.25 * ((w2 + w3) * (1.0 + 0.5 * h2n0 * k2n0) - (w1 + w4) * (1.0 - 0.5 * h2s0 * k2s0));
    w1 = h2s0 * s22[0][lc] + h2n0 * s22[1][lc];
    w2 = h2s0 * s22[3][lc] + h2n0 * s22[2][lc];
    w3 = (h2sE * s22[0][cE] + h2nE * s22[1][cE]) * GE;
    w4 = (h2sW * s22[3][cW] + h2nW * s22[2][cW]) * GW;
    FX = FX - 0.125 * ((w2 + w3) * h1e0 * k1e0 + (w1 + w4) * h1w0 * k1w0);
    // y-component (:985-1018)
    w1 = h1w0 * s22[0][lc] + h1e0 * s22[3][lc];
    w2 = h1w0 * s22[1][lc] + h1e0 * s22[2][lc];
    w3 = (h1wN * s22[0][cN] + h1eN * s22[3][cN]) * GN;
    w4 = (h1wS * s22[1][cS] + h1eS * s22[2][cS]) * GS;
    FY = 0.25 * (w2 + w3 - w1 - w4);
    w1 = h2s0 * s12[0][lc] + h2n0 * s12[1][lc];
    w2 = h2s0 * s12[3][lc] + h2n0 * s12[2][lc];
    w3 = (h2sE * s12[0][cE] + h2nE * s12[1][cE]) * GE;
    w4 = (h2sW * s12[3][cW] + h2nW * s12[2][cW]) * GW;
    FY = FY + 0.25 * ((w2 + w3) * (1.0 + 0.5 * h1e0 * k1e0) - (w1 + w4) * (1.0 - 0.5 * h1w0 * k1w0));
    w1 = h1w0 * s11[0][lc] + h1e0 * s11[3][lc];
    w2 = h1w0 * s11[1][lc] + h1e0 * s11[2][lc];
    w3 = (h1wN * s11[0][cN] + h1eN * s11[3][cN]) * GN;
    w4 = (h1wS * s11[1][cS] + h1eS * s11[2][cS]) * GS;
    FY = FY - 0.125 * ((w2 + w3) * h2n0 * k2n0 + (w1 + w4) * h2s0 * k2s0);
    // divided by the U-cell area where the level is wet (:1026-1032)
    const bool wet = kmu >= k;
    const long long o = base3 + (long long)(k - 1) * n2;
    a.HDU[o] = wet ? FX / uarea : 0.0;
    a.HDV[o] = wet ? FY / uarea : 0.0;
  }
}

inline void launch_hdiffu_aniso(const DevGrid &g, const AnisoArgs &a, hipStream_t st) {
  const dim3 B(ANI_TX, ANI_TY), G((g.nxb - 2 * NGHOST + ANI_TX - 1) / ANI_TX, (g.nyb - 2 * NGHOST + ANI_TY - 1) / ANI_TY, g.nblocks);
  with_flags([&](auto PBC) { hipLaunchKernelGGL((k_hdiffu_aniso<PBC.value>), G, B, 0, st, g, a); }, g.pbc);
}

}  // namespace pop
