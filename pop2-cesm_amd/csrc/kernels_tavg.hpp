// kernels_tavg.hpp -- time-averaged output (tavg.F90): the accumulation passes, reset and normalisation.
//
// accumulate_tavg_field (tavg.F90:3202-3240) is a whole-array statement per entry and level.  Here one launch per call site of
// the step ("site") serves every entry of the site: a thread loads each distinct source of the site once and then walks a table
// of descriptors, one per entry, that says which sources feed which expression, how the value enters the buffer (method) and
// where the buffer is.  The walk is the same in every lane (the table is a kernel argument, read by scalar loads), so there is
// no divergence, and every buffer cell has exactly one writer, so there are no atomics.  Every cell of every local block is
// updated -- ghost and land cells included, as the reference's statements do: no land elimination here.
//
// The product of `BUF + dtavg*ARRAY` is rounded before the sum (the library is built with -ffp-contract=off; the pragma below
// says so again for this file).
#pragma once
#include <utility>
#include "kernels_common.hpp"

namespace pop {

constexpr int TAVG_MAX_STREAMS = 9;    // tavg.F90:83 max_avail_tavg_streams
constexpr int TAVG_MAX_FIELDS = 64;    // POP_TAVG_MAX_FIELDS
constexpr int TAVG_MAX_SRC = 12;       // distinct sources of one launch
constexpr int TAVG_MAX_VINT = 6;       // 2-D entries fed from a range of levels, per launch
constexpr double TAVG_BIGNUM = 1.0e30; // tavg.F90 bignum

enum TavgMethod { TAVG_AVG = 1, TAVG_MIN = 2, TAVG_MAX = 3, TAVG_QFLUX = 4, TAVG_CONSTANT = 5 };   // tavg.F90:75-80
enum TavgExpr {
  TX_X = 0,        // x
  TX_SQR,          // x*x
  TX_XY,           // x*y
  TX_KE,           // 0.5*(x*x + y*y)
  TX_DPOS,         // max(x - y, 0)
  TX_DNEG,         // min(x - y, 0)
  TX_DIVC,         // x/c
  TX_DIVC_SQR,     // (x/c)*(x/c)
  TX_DIVC_SQSUM,   // (x/c)*(x/c) + (y/c)*(y/c)
  TX_M_DIVC,       // where KMT > 0: x/c, else 0             (columns only)
  TX_M_SUMDIVC,    // where KMT > 0: (x + y)/c, else 0
  TX_M_MULCC,      // where KMT > 0: x*c*c2, else 0
  TX_RHO_VINT,     // x*thickness of the T cell where k <= KMT, else 0 (baroclinic.F90:2392-2414; columns only)
  TX_MULCC         // x*c*c2 on every cell (TFW_S, forcing.F90:579)
};

// cell (q, k, b) of a source: p[((long long)b*nz + k + k0)*n2 + q]; nz = 1: a 2-D field
struct TavgSrc { const double *p; int nz, k0; };
// buffer of an entry.  cells: kmax levels per block (1: a 2-D entry taken from level 1); columns: a 2-D buffer, fed from the levels
// 1 .. kmax where the entry is one of those.  cst, cst2: the constants of the expression, or the const of method qflux
struct TavgDesc { double *buf; double cst, cst2; short kmax; unsigned char a, b, expr, method; };
struct TavgTable {
  TavgSrc src[TAVG_MAX_SRC];
  TavgDesc d[TAVG_MAX_FIELDS];
  int nsrc, n;          // cells: every entry; columns: entries [0, n2d) of 2-D sources, [n2d, n) fed from every level
  int n2d, kmax;        // the largest kmax of the table: levels the launch covers (cells) / the march covers (columns)
  double dtavg;
};
// what TX_RHO_VINT needs besides the density
struct TavgVint { const double *PSURF; double grav; };

// f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>): the indices are constants from the start, so the small
// per-thread arrays below are registers (a `#pragma unroll` loop is unrolled too late for that: the arrays went to scratch)
template <class F, int... I>
__device__ __forceinline__ void tavg_each_impl(F &&f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void tavg_each(F &&f) { tavg_each_impl(f, std::make_integer_sequence<int, N>{}); }
struct TavgRegs { double v[TAVG_MAX_SRC]; };
__device__ __forceinline__ double tavg_pick(const TavgRegs &s, int i) {   // s.v[i] for a wave-uniform i without indexing registers
  double x = s.v[0];
  tavg_each<TAVG_MAX_SRC>([&](auto J) { if constexpr (J.value > 0) x = (i == J.value) ? s.v[J.value] : x; });
  return x;
}
__device__ __forceinline__ double tavg_value(int expr, double x, double y, double c, double c2 = 0.0, bool ocean = true) {
#pragma clang fp contract(off)
  switch (expr) {
    case TX_M_DIVC: return ocean ? x / c : 0.0;
    case TX_M_SUMDIVC: return ocean ? (x + y) / c : 0.0;
    case TX_M_MULCC: return ocean ? x * c * c2 : 0.0;
    case TX_MULCC: return x * c * c2;
    case TX_SQR: return x * x;
    case TX_XY: return x * y;
    case TX_KE: return 0.5 * (x * x + y * y);
    case TX_DPOS: return fmax(x - y, 0.0);
    case TX_DNEG: return fmin(x - y, 0.0);
    case TX_DIVC: return x / c;
    case TX_DIVC_SQR: { const double w = x / c; return w * w; }
    case TX_DIVC_SQSUM: { const double w = x / c, z = y / c; return w * w + z * z; }
    default: return x;
  }
}
__device__ __forceinline__ double tavg_apply(int method, double buf, double v, double dtavg, double cst) {
#pragma clang fp contract(off)
  switch (method) {
    case TAVG_AVG: { const double w = dtavg * v; return buf + w; }
    case TAVG_MIN: return (v < buf) ? v : buf;
    case TAVG_MAX: return (v > buf) ? v : buf;
    case TAVG_QFLUX: { const double w = cst * fmax(0.0, v); return buf + w; }
    default: return v;   // constant
  }
}

// ------------------------------------------------------------------------------------------
// k_tavg_cells: the 3-D entries of a site and its 2-D entries taken from one level (kmax = 1).  Grid (cells of the level
// plane / (256 VEC), levels, blocks); VEC = 2: two cells along i per thread through 16-byte accesses (n2 even, so every level
// plane starts on a 16-byte boundary).
// ------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void k_tavg_cells(int n2, TavgTable t) {
  const int q = (blockIdx.x * 256 + threadIdx.x) * VEC;
  if (q >= n2) return;
  const int k = blockIdx.y, b = blockIdx.z;
  TavgRegs s0, s1;
  tavg_each<TAVG_MAX_SRC>([&](auto I) {
    constexpr int i = I.value;
    s0.v[i] = 0.0; s1.v[i] = 0.0;
    if (i < t.nsrc) {
      const double *p = t.src[i].p + ((long long)b * t.src[i].nz + k + t.src[i].k0) * n2 + q;
      if constexpr (VEC == 2) { const double2 v = *(const double2 *)p; s0.v[i] = v.x; s1.v[i] = v.y; }
      else s0.v[i] = *p;
    }
  });
  for (int e = 0; e < t.n; ++e) {
    const TavgDesc d = t.d[e];
    if (k >= d.kmax) continue;   // k > avail%km returns (tavg.F90:3193)
    double *bp = d.buf + ((long long)b * d.kmax + k) * n2 + q;
    if constexpr (VEC == 2) {
      const double2 o = *(const double2 *)bp;
      const double r0 = tavg_apply(d.method, o.x, tavg_value(d.expr, tavg_pick(s0, d.a), tavg_pick(s0, d.b), d.cst), t.dtavg, d.cst);
      const double r1 = tavg_apply(d.method, o.y, tavg_value(d.expr, tavg_pick(s1, d.a), tavg_pick(s1, d.b), d.cst), t.dtavg, d.cst);
      *(double2 *)bp = make_double2(r0, r1);
    } else
      *bp = tavg_apply(d.method, *bp, tavg_value(d.expr, tavg_pick(s0, d.a), tavg_pick(s0, d.b), d.cst), t.dtavg, d.cst);
  }
}

// ------------------------------------------------------------------------------------------
// k_tavg_columns: one thread per column.  The 2-D entries of 2-D sources, then the 2-D entries the reference feeds once per
// level k <= kmax (RHO_VINT, dTEMP_POS_2D, dTEMP_NEG_2D: every level; U1_8, T1_8 ...: levels 1 .. 8): the thread marches k and adds
// into the buffer value in that order, as the reference's k loop does.  Those are all method avg.
// ------------------------------------------------------------------------------------------
template <bool PBC>
__global__ __launch_bounds__(256) void k_tavg_columns(DevGrid g, TavgTable t, TavgVint w) {
#pragma clang fp contract(off)
  const int q = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (q >= g.n2) return;
  const long long q2 = (long long)b * g.n2 + q;
  TavgRegs s;
  tavg_each<TAVG_MAX_SRC>([&](auto I) { constexpr int i = I.value; s.v[i] = (i < t.nsrc && t.src[i].nz == 1) ? t.src[i].p[q2] : 0.0; });
  const int kmt = g.KMT[q2];
  for (int e = 0; e < t.n2d; ++e) {
    const TavgDesc d = t.d[e];
    d.buf[q2] = tavg_apply(d.method, d.buf[q2], tavg_value(d.expr, tavg_pick(s, d.a), tavg_pick(s, d.b), d.cst, d.cst2, kmt > 0), t.dtavg, d.cst);
  }
  const int nv = t.n - t.n2d;
  if (nv <= 0) return;
  double acc[TAVG_MAX_VINT];
  tavg_each<TAVG_MAX_VINT>([&](auto J) { constexpr int j = J.value; acc[j] = (j < nv) ? t.d[t.n2d + j].buf[q2] : 0.0; });
  const double dzbot = PBC ? g.DZBC[q2] : 0.0, eta = w.PSURF ? w.PSURF[q2] / w.grav : 0.0;
  for (int k = 1; k <= t.kmax; ++k) {
    tavg_each<TAVG_MAX_SRC>([&](auto I) {
      constexpr int i = I.value;
      if (i < t.nsrc && t.src[i].nz > 1) s.v[i] = t.src[i].p[((long long)b * t.src[i].nz + (k - 1) + t.src[i].k0) * g.n2 + q];
    });
    // thickness of the T cell: the variable-thickness surface layer at k = 1, the partial bottom cell at k = KMT
    const double thick = (k == 1) ? g.dz.u(1) + eta : (PBC ? pbc_dz(g, k, kmt, dzbot) : g.dz.u(k));
    tavg_each<TAVG_MAX_VINT>([&](auto J) {
      constexpr int j = J.value;
      if (j < nv && k <= t.d[t.n2d + j].kmax) {
        const TavgDesc d = t.d[t.n2d + j];
        const double x = tavg_pick(s, d.a);
        const double v = (d.expr == TX_RHO_VINT) ? ((k <= kmt) ? x * thick : 0.0) : tavg_value(d.expr, x, tavg_pick(s, d.b), d.cst);
        const double pr = t.dtavg * v;
        acc[j] = acc[j] + pr;
      }
    });
  }
  tavg_each<TAVG_MAX_VINT>([&](auto J) { constexpr int j = J.value; if (j < nv) t.d[t.n2d + j].buf[q2] = acc[j]; });
}

// reset (tavg_reset_field_stream: the value by method) and normalise-into-a-copy (tavg_norm_field_all)
__global__ void k_tavg_fill(double *__restrict__ p, long long n, double v) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
__global__ void k_tavg_scale(const double *__restrict__ in, double *__restrict__ out, long long n, double factor) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i] * factor;
}

}  // namespace pop
