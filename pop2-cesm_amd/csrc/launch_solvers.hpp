// launch_solvers.hpp -- host side of the barotropic solvers: the drivers, their shared launch helpers and the dispatch
// (part of pop_amd.hip, after launch_halo.hpp).
#pragma once

namespace {

SolverArgs solver_args(pop_ctx *c) {
  SolverArgs a{};
  a.X = c->PS[c->newt]; a.R = c->R; a.S0 = c->S0; a.S1 = c->S1; a.Q = c->Q; a.Z = c->Z; a.AZ = c->AZ;
  a.Bv = c->RHS; a.C = c->centerWgt; a.partial = c->partial; a.sc = c->sc;
  return a;
}

// preconditioner() with preconditionerChoice = 'evp' (:2331-2366): PX <- sub-block solves of X on the physical cells
// residual: X is a residual of a solver (zero on land): sub-blocks without an ocean cell are not read (k_evp_apply_wave3<true>)
int evp_apply(pop_ctx *c, const double *X, double *PX, bool residual = true) {
  const dim3 GW((unsigned)((c->evp.S + POP_EVP_SB - 1) / POP_EVP_SB));
  if (c->f.evp_wave == 0)   // a thread per sub-block, the plain statement in the reference's order
    hipLaunchKernelGGL(k_evp_apply, dim3((unsigned)((c->evp.S + POP_EVP_THREADS - 1) / POP_EVP_THREADS)), dim3(POP_EVP_THREADS), 0, c->stream,
                       c->evp, c->g.nxb, X, PX);
  else   // 3 (the default): anti-diagonal wavefronts, eight lanes per sub-block, eight sub-blocks per wave
    with_flags([&](auto RES) { hipLaunchKernelGGL(k_evp_apply_wave3<RES.value>, GW, dim3(64), 0, c->stream, c->evp, c->g.nxb, X, PX); }, residual);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// start of every solve: fresh device scalars (pcg starts its recurrence from eta0 = 1)
int solver_begin(pop_ctx *c, double eta0 = 0.0) {
  SolverScalars init{}; init.eta0 = eta0;
  HIPCHK(c, hipMemcpyAsync(c->sc, &init, sizeof(init), hipMemcpyHostToDevice, c->stream));
  return 0;
}
int not_converged(pop_ctx *c, const char *routine) { c->err = std::string(routine) + ": solver not converged"; return 2; }
// end of every solve that iterated on the host's count: the ghosts of the solution as POP_SolversRun leaves them -- copied from their source
// cells through srcmap (the fused forms; null: the form kept them current by halo updates) --, the residual norm, and the verdict
int solver_finish(pop_ctx *c, double *X, const int *srcmap, long long ncell, double rr, const char *routine) {
  if (srcmap) hipLaunchKernelGGL(k_halo_srcmap, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, c->stream, X, srcmap, ncell);
  c->rmsResidual = std::sqrt(rr * c->h.residualNorm);
  HIPCHK(c, hipGetLastError());
  if (c->numIterations == c->h.c.max_iterations && c->h.convergenceCriterion != 0.0) return not_converged(c, routine);
  return 0;
}

// POP_SolversRun -> pcg (POP_SolversMod.F90:1255-1503), diagonal or EVP preconditioner
int solver_pcg(pop_ctx *c) {
  const pop_config &cf = c->h.c;
  const dim3 G = grid_2d(c), B(POP_RED_THREADS);
  if (solver_begin(c, 1.0)) return 1;
  HIPCHK(c, hipMemsetAsync(c->S0, 0, sizeof(double) * c->g.n2 * c->g.nblocks, c->stream));
  SolverArgs a = solver_args(c);
  hipLaunchKernelGGL(k_residual<false>, grid_2d(c), B, 0, c->stream, c->g, a);
  if (halo_update(c, c->R, 1)) return 1;
  c->numIterations = cf.max_iterations;
  double rr = 0.0;
  bool pending = false;   // x,r update of the previous iteration not yet applied
  for (int m = 1; m <= cf.max_iterations; ++m) {
    a = solver_args(c);
    if (c->use_evp) {   // :1322-1362: z = M^-1 r by sub-block solves, (r,z), halo of z
      if (pending) hipLaunchKernelGGL(k_pcg_xr, G, B, 0, c->stream, c->g, a);
      if (evp_apply(c, c->R, c->Z)) return 1;
      hipLaunchKernelGGL(k_dot_partial, G, B, 0, c->stream, c->g, (const double *)c->R, (const double *)c->Z, c->g.mMask, c->partial);
      if (halo_update(c, c->Z, 1)) return 1;
    } else if (pending) hipLaunchKernelGGL(k_pcg_a<true>, G, B, 0, c->stream, c->g, a);
    else hipLaunchKernelGGL(k_pcg_a<false>, G, B, 0, c->stream, c->g, a);
    if (reduce_finish<1>(c, FIN_PCG_RZ)) return 1;
    hipLaunchKernelGGL(k_pcg_b, G, B, 0, c->stream, c->g, a);
    std::swap(c->S0, c->S1);
    if (halo_update(c, c->Q, 1)) return 1;
    if (reduce_finish<1>(c, FIN_PCG_SQ)) return 1;
    pending = true;
    if (m % cf.convergence_check_freq == 0) {
      a = solver_args(c);
      hipLaunchKernelGGL(k_pcg_xr, G, B, 0, c->stream, c->g, a);
      pending = false;
      hipLaunchKernelGGL(k_residual<true>, grid_2d(c), B, 0, c->stream, c->g, a);
      if (halo_update(c, c->R, 1)) return 1;
      if (reduce_finish<1>(c, FIN_RR)) return 1;
      SolverScalars s;
      if (read_scalars(c, &s)) return 1;
      rr = s.rr;
      if (rr < c->h.convergenceCriterion) { c->numIterations = m; break; }
    }
  }
  if (pending) { a = solver_args(c); hipLaunchKernelGGL(k_pcg_xr, G, B, 0, c->stream, c->g, a); }
  return solver_finish(c, nullptr, nullptr, 0, rr, "POP_SolversPCG");
}

// pcg, fused form: two launches per iteration, halo folded into the matvec through srcmap, final
// reduction stage recomputed by the consumer kernel, and one hipGraph replay per
// convergenceCheckFreq iterations (same arithmetic and summation order as solver_pcg).  It runs on a
// SolveView: the rank's own blocks (single rank), or -- replicated barotropic mode -- every block
// of the decomposition on every rank.
// The rules below depend on the solver view (the local and the replicated view differ in size): functions of the view that take the plan's
// switch values (Forms; presum_by_size and two_cell_shape are in forms.hpp, which applies them to the local view for P-CSI).
// which forms of step A / step B the fused pcg launches (launch_fpcg_a / launch_fpcg_b)
static bool fpcg_pair_ok(const Forms &f, const SolveView &v, const FusedArgs &a) {
  return v.g.red_act && a.presummed && !a.sendmap && (v.g.red_nact % 16) == 0 && f.fpcg_b2 && f.fpcg_a_pair;
}
// two cells per thread in the fused pcg / ChronGear kernels: the shape rule, unless the plan says one cell per thread even on large grids
static bool two_cell_ok(const Forms &f, const DevGrid &g, bool presummed) { return two_cell_shape(g.nxb, presummed) && f.fpcg_b2; }
FusedArgs fused_args(pop_ctx *c, const SolveView &v) {
  FusedArgs a{};
  a.X = v.X; a.R = v.R; a.Z = v.Z; a.S0 = v.S0; a.S1 = v.S1; a.Q = v.Q;
  a.Bv = v.RHS; a.C = v.C; a.partA = v.partial; a.partB = v.partial + (size_t)v.nchunk * v.g.nblocks;
  a.sc = c->sc; a.srcmap = v.srcmap; a.nchunk = v.nchunk; a.nblocks = v.g.nblocks;
  a.bsA = v.blocksum + 2 * v.nblocks_tot; a.bsB = v.blocksum + 3 * v.nblocks_tot;
  a.presummed = (presum_by_size(v.nchunk, v.g.nblocks) || c->f.presum_forced) ? 1 : 0;
  return a;
}
// large grids: ordered block sums of a partial array between solver kernels (view-local block order)
// (more than 64 terms per accumulator: the four-threads-per-accumulator form, one memory round trip instead of two or three)
constexpr int POP_RELAY_LMAX = 36;
static bool presum_relay(int relay, const SolveView &v) {   // relay: Forms::block_sums_relay
  const int terms = (v.nchunk + POP_RED_THREADS - 1) / POP_RED_THREADS;
  return (terms > 64 || relay == 2) && (terms + 3) / 4 <= POP_RELAY_LMAX && relay != 0;
}
// NF interleaved fields per chunk (pcg 1, ChronGear 2)
template <int NF = 1>
void presum(pop_ctx *c, const SolveView &v, const double *partial, double *bs) {
  if (presum_relay(c->f.block_sums_relay, v)) hipLaunchKernelGGL((k_block_sums_relay<NF, POP_RELAY_LMAX>), dim3(v.g.nblocks, NF), dim3(1024), 0, c->stream, partial, v.nchunk, (const int *)c->iota, bs);
  else hipLaunchKernelGGL(k_block_sums<NF>, dim3(v.g.nblocks), dim3(POP_RED_THREADS), 0, c->stream, partial, v.nchunk, (const int *)c->iota, bs);
}
dim3 view_grid(const SolveView &v) { return dim3(red_grid_x(v.g), v.g.nblocks); }
// r = b - A x (+ partial (r,r)) of the fused solvers: two cells per thread on large grids, else one
// (presummed: a.presummed, except where the distributed ChronGear applies the size rule alone)
template <bool WITH_RR>
void launch_fresidual(pop_ctx *c, const SolveView &v, const FusedArgs &a, bool presummed) {
  const dim3 G = view_grid(v);
  if (two_cell_ok(c->f, v.g, presummed)) hipLaunchKernelGGL(k_fresidual2<WITH_RR>, G, dim3(POP_RED_THREADS / 2), 0, c->stream, v.g, a);
  else hipLaunchKernelGGL(k_fresidual<WITH_RR>, G, dim3(POP_RED_THREADS), 0, c->stream, v.g, a);
}
template <bool WITH_RR>
void launch_fresidual(pop_ctx *c, const SolveView &v, const FusedArgs &a) { launch_fresidual<WITH_RR>(c, v, a, a.presummed != 0); }
// step A of the fused pcg: two chunks per workgroup on compacted launches (single rank), else one
void launch_fpcg_a(pop_ctx *c, const SolveView &v, const FusedArgs &a, bool update) {
  const dim3 G = view_grid(v), B(POP_RED_THREADS);
  const bool pair = fpcg_pair_ok(c->f, v, a);
  if (pair) {
    const dim3 GP(G.x / 2, G.y);
    if (update) hipLaunchKernelGGL(k_fpcg_a_pair<true>, GP, B, 0, c->stream, v.g, a);
    else hipLaunchKernelGGL(k_fpcg_a_pair<false>, GP, B, 0, c->stream, v.g, a);
  } else if (update) hipLaunchKernelGGL(k_fpcg_a<true>, G, B, 0, c->stream, v.g, a);
  else hipLaunchKernelGGL(k_fpcg_a<false>, G, B, 0, c->stream, v.g, a);
}
// step B of the fused pcg: two cells per thread on large grids (presummed block sums, even row pitch), else one
// xupd: the pending x += alpha s of the previous iteration is applied here (k_fpcg_a<true> ran before and published alpha)
void launch_fpcg_b(pop_ctx *c, const SolveView &v, const FusedArgs &a, bool xupd) {
  const dim3 G = view_grid(v);
  const bool two = two_cell_ok(c->f, v.g, a.presummed != 0);
  // (occupancy probe, profiles/r03_ab_b2_occupancy.txt: with dynamic LDS holding the kernel to 3 / 2 waves per SIMD instead of its 4
  // the step costs +2.2 / +7.1 ms; the two-cell form needs 108 VGPRs, a 96- or 80-register budget spills 84 / 140 B)
  if (two && xupd) hipLaunchKernelGGL(k_fpcg_b2<true>, G, dim3(POP_RED_THREADS / 2), 0, c->stream, v.g, a);
  else if (two) hipLaunchKernelGGL(k_fpcg_b2<false>, G, dim3(POP_RED_THREADS / 2), 0, c->stream, v.g, a);
  else if (xupd) hipLaunchKernelGGL(k_fpcg_b<true>, G, dim3(POP_RED_THREADS), 0, c->stream, v.g, a);
  else hipLaunchKernelGGL(k_fpcg_b<false>, G, dim3(POP_RED_THREADS), 0, c->stream, v.g, a);
}
// n iterations; pending: the x,r update of the iteration before is still to be applied.  Leaves the last one pending
void fused_iterations(pop_ctx *c, SolveView &v, int n, bool pending) {
  for (int it = 0; it < n; ++it) {
    FusedArgs a = fused_args(c, v);
    launch_fpcg_a(c, v, a, pending);
    if (a.presummed) presum(c, v, a.partA, (double *)a.bsA);
    launch_fpcg_b(c, v, a, pending);
    if (a.presummed) presum(c, v, a.partB, (double *)a.bsB);
    std::swap(v.S0, v.S1);
    pending = true;
  }
}
// one check interval: freq iterations, pending update, residual + (r,r) -> host
int fused_interval(pop_ctx *c, SolveView &v, int freq) {
  const dim3 G = view_grid(v), B(POP_RED_THREADS);
  fused_iterations(c, v, freq, false);
  FusedArgs a = fused_args(c, v);
  hipLaunchKernelGGL(k_fpcg_xr, G, B, 0, c->stream, v.g, a);
  launch_fresidual<true>(c, v, a);
  // the view holds every block it sums (single rank or replicated), in block-id order
  hipLaunchKernelGGL(k_rr_total, dim3(1), dim3(POP_RED_THREADS), 0, c->stream, (const double *)v.partial, v.nchunk, v.g.nblocks, c->sc, c->host_rr, c->h.convergenceCriterion);
  return 0;
}
// Check intervals with one interval of look-ahead.  `enqueue(i)` puts interval i on the stream (a hipGraph replay or
// plain launches) and returns whether it ends with a convergence check (k_rr_total).  The host keeps at most two checked
// intervals in flight and examines them in order; the check that meets the criterion raises the device stop flag, so the
// interval already enqueued behind it does nothing, and the GPU never idles while the host looks at a residual.
// Returns the index of the converged interval or -1; rr = last residual seen.
template <class Enqueue>
int run_intervals(pop_ctx *c, int nint, Enqueue enqueue, double &rr, int &err) {
  int next = 0, ring = 0, head = 0;          // ring: checks enqueued; head: checks examined
  int idx[8] = {};
  err = 0;
  auto fill = [&]() {
    while (next < nint && ring - head < 2) {
      const int chk = enqueue(next);
      if (chk < 0) { err = 1; return; }
      if (chk) {
        if (hipEventRecord(c->chk_ev[ring & 3], c->stream) != hipSuccess) { err = 1; return; }
        idx[ring & 7] = next; ++ring;
      }
      ++next;
    }
  };
  fill();
  while (!err && head < ring) {
    if (hipEventSynchronize(c->chk_ev[head & 3]) != hipSuccess) { err = 1; break; }
    rr = c->host_rr[head & 7];
    const int i = idx[head & 7];
    ++head;
    if (rr < c->h.convergenceCriterion) return i;
    fill();
  }
  return -1;
}

// The hipGraph of one check interval, captured from the launch stream the first time it is needed.  key: the solution array the launches
// carry (the time-level rotation cycles three of them); variant: which of the solver's interval forms (P-CSI: ping-pong half and check;
// pcg, ChronGear: 0).  capture() enqueues the interval and returns non-zero on failure.  Null: capture or instantiation failed.
template <class Capture>
hipGraphExec_t graph_for(pop_ctx *c, const double *key, int variant, Capture capture) {
  for (auto &g : c->graphs) if (g.key == key && g.variant == variant) return g.exec;
  hipGraph_t graph;
  hipGraphExec_t exec = nullptr;
  if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return nullptr;
  const int e = capture();
  const hipError_t ce = hipStreamEndCapture(c->stream, &graph);
  if (e || ce != hipSuccess) return nullptr;
  if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) return nullptr;
  hipGraphDestroy(graph);
  c->graphs.push_back({key, variant, exec});
  return exec;
}

// ---- the resident pcg of small grids (kernels_pcg_persist.hpp) ------------------------------------------------------------------
// Plan of one view: which chunks a workgroup owns, the window index of every stencil neighbour, the halo cells.  Built on the host
// from the view's source map (ghost -> source cell, -1 = fill), so block boundaries inside the view, the cyclic wrap, closed
// boundaries and a tripole fold need no case of their own.  Returns nullptr (with the reason kept) when the view does not qualify.
static pop_ctx::PersistPlan *persist_plan(pop_ctx *c, const SolveView &v) {
  for (auto &p : c->persist) if (p.key == (const void *)v.srcmap) return p.ok ? &p : nullptr;
  c->persist.emplace_back();
  pop_ctx::PersistPlan &pl = c->persist.back();
  pl.key = (const void *)v.srcmap;
  const HostModel &h = c->h;
  const int n2 = (int)h.n2, nxb = h.nxb, nchunk = v.nchunk, nb = v.g.nblocks, nslots = nchunk * nb;
  const bool global = v.srcmap != c->srcmap;                // the replicated view holds every block of the decomposition
  auto refuse = [&](const char *why) -> pop_ctx::PersistPlan * { pl.why = why; return nullptr; };
  if (nb * ((nchunk + POP_RED_THREADS - 1) / POP_RED_THREADS) > POP_PERSIST_MAXP) return refuse("too many partial slots per thread");
  // chunks per workgroup: the smallest of 1 / 2 / 4 / 8 that needs at most 250 workgroups (one per CU: the waits need every workgroup
  // resident).  gx1v7 in one block: 246 x 2 (10.7 us per iteration; 123 x 4: 12.0, 62 x 8: 14.1 on the same box, profiles/r04_ab_persist_shape.txt);
  // gx1v7 in the eight 48-row bands of the 8-rank decomposition (replicated solve): 144 x 4.
  // measurement only: Forms::persist = 2 | 4 | 8 forces that many chunks per workgroup
  std::vector<int> cand;
  if (c->f.persist > 1 && (nslots + c->f.persist - 1) / c->f.persist <= 250) cand.push_back(c->f.persist);
  if (cand.empty())
    for (int cp : {1, 2, 4, 8}) if ((nslots + cp - 1) / cp <= 250) { cand.push_back(cp); break; }
  if (cand.empty()) return refuse("more than 2000 chunks");
  const std::vector<int> sm = global ? global_srcmap(h) : c->h_srcmap;
  if ((long long)sm.size() != (long long)n2 * nb) return refuse("source map size");
  const int off[8] = {nxb, -nxb, 1, -1, nxb + 1, -nxb + 1, nxb - 1, -nxb - 1};
  int CP = 0, nwg = 0, nwin_max = 0;
  std::vector<int> own, hoff, hq;
  std::vector<unsigned short> nbr;
  const char *why = "";
  for (int cp : cand) {
    why = "";
    nwg = (nslots + cp - 1) / cp; nwin_max = 0;
    const int NOWN = cp * POP_RED_THREADS;
    own.assign((size_t)nwg * NOWN, -1); hoff.assign(nwg + 1, 0); hq.clear();
    nbr.assign((size_t)nwg * NOWN * 8, 0);
    for (int w = 0; w < nwg && !*why; ++w) {
      std::unordered_map<int, int> where;                    // cell -> window index
      for (int u = 0; u < cp; ++u) {
        const int slot = w * cp + u;
        if (slot >= nslots) break;
        const int b = slot / nchunk, ch = slot % nchunk;
        const BlockInfo &B = h.all_blocks[global ? b : h.local_ids[b] - 1];
        for (int t = 0; t < POP_RED_THREADS; ++t) {
          const int p2 = ch * POP_RED_THREADS + t;
          if (p2 >= n2) break;
          const int i = p2 % nxb + 1, j = p2 / nxb + 1;
          if (i < B.ib || i > B.ie || j < B.jb || j > B.je) continue;
          own[(size_t)w * NOWN + u * POP_RED_THREADS + t] = b * n2 + p2;
          where[b * n2 + p2] = u * POP_RED_THREADS + t;
        }
      }
      const size_t h0 = hq.size();
      for (int L = 0; L < NOWN; ++L) {
        const int q = own[(size_t)w * NOWN + L];
        if (q < 0) continue;
        for (int n = 0; n < 8; ++n) {
          const int m = sm[q + off[n]];
          int idx;
          if (m < 0) idx = -1;
          else {
            auto it = where.find(m);
            if (it != where.end()) idx = it->second;
            else { idx = NOWN + (int)(hq.size() - h0); where[m] = idx; hq.push_back(m); }
          }
          nbr[((size_t)w * NOWN + L) * 8 + n] = (unsigned short)(idx < 0 ? 0xFFFF : idx);
        }
      }
      const int nhalo = (int)(hq.size() - h0), nwin = NOWN + nhalo + 1;
      if ((nhalo + POP_RED_THREADS - 1) / POP_RED_THREADS > POP_PERSIST_MAXH) { why = "halo of a workgroup too large"; break; }
      if (nwin >= 0xFFFF) { why = "window too large"; break; }
      for (int L = 0; L < NOWN; ++L) for (int n = 0; n < 8; ++n) {
        unsigned short &x = nbr[((size_t)w * NOWN + L) * 8 + n];
        if (x == 0xFFFF) x = (unsigned short)(nwin - 1);     // the cell of zeros (fill value of closed boundaries)
      }
      hoff[w + 1] = (int)hq.size();
      nwin_max = std::max(nwin_max, nwin);
    }
    if (!*why && (size_t)3 * nwin_max * sizeof(double) > 60000) why = "window does not fit the LDS budget";
    if (!*why) { CP = cp; break; }
  }
  if (!CP) return refuse(why);
  if (hq.empty()) hq.push_back(0);
  if (dev_upload(c, &pl.own_q, own.data(), own.size()) || dev_upload(c, &pl.nbr, nbr.data(), nbr.size()) ||
      dev_upload(c, &pl.halo_off, hoff.data(), hoff.size()) || dev_upload(c, &pl.halo_q, hq.data(), hq.size())) return nullptr;
  const size_t nwords = 4 * (size_t)nslots + 2 * (size_t)n2 * nb;      // partials [2 buffers][2 fields (ChronGear)][nslots], then z [2][ncell]
  if (nwords * sizeof(PWord) >= (1ULL << 32)) return refuse("exchange buffer beyond 32-bit offsets");
  double *p = nullptr;
  if (dev_alloc(c, &p, 2 * nwords)) return nullptr;          // zero-filled: tag 0 is never waited for (epochs start at 1)
  pl.W = reinterpret_cast<PWord *>(p);
  if (dev_alloc(c, &pl.X0, (size_t)n2 * nb)) return nullptr;
  pl.CP = CP; pl.nwg = nwg; pl.nwin_max = nwin_max; pl.nslots = nslots; pl.ok = true;
  return &pl;
}
// the arguments every resident kernel takes, for one solve on view v
constexpr unsigned long long POP_PERSIST_WAIT_TICKS = 200000000ULL;   // bound of a wait for another workgroup's data: 2 s
PersistArgs persist_args(pop_ctx *c, const SolveView &v, const pop_ctx::PersistPlan &pl) {
  const pop_config &cf = c->h.c;
  PersistArgs a{};
  a.X = v.X; a.Bv = v.RHS; a.C = v.C; a.WNo = v.g.WNo; a.WEa = v.g.WEa; a.WNE = v.g.WNE; a.mMask8 = v.g.mMask8;
  a.nxb = v.g.nxb; a.nchunk = v.nchunk; a.nblocks = v.g.nblocks; a.nslots = pl.nslots; a.ncell = (long long)v.g.n2 * v.g.nblocks;
  a.own_q = pl.own_q; a.nbr = pl.nbr; a.halo_off = pl.halo_off; a.halo_q = pl.halo_q; a.W = pl.W;
  a.epoch = (++c->persist_epoch) << 32;                    // tags of this solve: no word of an earlier solve can carry one of them
  a.max_iter = cf.max_iterations; a.freq = cf.convergence_check_freq; a.criterion = c->h.convergenceCriterion; a.out = c->persist_out;
  a.wait_ticks = POP_PERSIST_WAIT_TICKS;
  return a;
}
// One resident solve: kern = the kernel for 1 / 2 / 4 / 8 chunks per workgroup (k_pcg_persist, k_cg_persist, k_pcsi_persist), a its arguments.
// Launches, waits for the result in pinned memory, and finishes the solve as solver_finish does.  0: solved; 2: not converged;
// 3: the launch did not complete its exchanges (c->err says what it left) -- the caller repeats the solve with the launches per iteration
template <class Args>
int persist_launch(pop_ctx *c, const SolveView &v, const pop_ctx::PersistPlan &pl, const Args &a, void (*const (&kern)[4])(Args), const char *what, const char *routine) {
  const long long ncell = (long long)v.g.n2 * v.g.nblocks;
  double *out = c->persist_out;                            // iterations, (r,r), status, checks
  out[0] = -1.0; out[1] = 0.0; out[2] = 0.0; out[3] = 0.0;
  const size_t lds = (size_t)3 * pl.nwin_max * sizeof(double);
  const dim3 G(pl.nwg), B(POP_RED_THREADS);
  switch (pl.CP) {
    case 1: hipLaunchKernelGGL(kern[0], G, B, lds, c->stream, a); break;
    case 2: hipLaunchKernelGGL(kern[1], G, B, lds, c->stream, a); break;
    case 4: hipLaunchKernelGGL(kern[2], G, B, lds, c->stream, a); break;
    default: hipLaunchKernelGGL(kern[3], G, B, lds, c->stream, a); break;
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->chk_ev[0], c->stream));
  HIPCHK(c, hipEventSynchronize(c->chk_ev[0]));
  if (out[2] != 0.0 || out[0] < 0.0) {
    char b[200];
    snprintf(b, sizeof b, " [iterations %g, status %g, checks %g, %d workgroups x %d chunks, %d blocks]", out[0], out[2], out[3], pl.nwg, pl.CP, v.g.nblocks);
    c->err = std::string(what) + (out[0] < 0.0 ? ": the launch left no result" : ": a wait for another workgroup's data gave up (kernels_pcg_persist.hpp)") + b;
    return 3;
  }
  c->numIterations = (int)out[0];
  c->rmsResidual = std::sqrt(out[1] * c->h.residualNorm);
  c->persist_used = 1; c->persist_nwg = pl.nwg; c->persist_cp = pl.CP;
  hipLaunchKernelGGL(k_halo_srcmap, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, c->stream, v.X, v.srcmap, ncell);
  HIPCHK(c, hipGetLastError());
  const bool conv = out[3] > 0.0 && out[1] < c->h.convergenceCriterion;
  if (!conv && c->h.convergenceCriterion != 0.0) return not_converged(c, routine);
  return 0;
}
// persist_launch returned 3 (its header: several processes on one GPU): no resident solve again in this model, and this one is repeated by
// the form named in `instead`.  X0: the copy of x taken before a launch that may have written x at its very end, restored here; null for
// P-CSI, whose launch writes the other half of the ping-pong pair.  Everything else the launch touched it only read.
int persist_give_up(pop_ctx *c, const char *instead, const SolveView &v, const double *X0) {
  c->persist_gave_up += 1;
  fprintf(stderr, "libpop_amd: %s -- continuing with %s\n", c->err.c_str(), instead);
  c->err.clear();
  if (X0) HIPCHK(c, hipMemcpyAsync(v.X, X0, sizeof(double) * v.g.n2 * v.g.nblocks, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}
// the copy persist_give_up restores
int persist_keep_x0(pop_ctx *c, const SolveView &v, const pop_ctx::PersistPlan &pl) {
  HIPCHK(c, hipMemcpyAsync(pl.X0, v.X, sizeof(double) * v.g.n2 * v.g.nblocks, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

int solver_pcg_fused(pop_ctx *c, SolveView &v) {
  const pop_config &cf = c->h.c;
  c->persist_used = 0;
  if (c->f.persist && !fused_args(c, v).presummed) {   // wherever the persist plan qualifies (small views)
    const pop_ctx::PersistPlan *pl = c->persist_gave_up ? nullptr : persist_plan(c, v);
    if (pl) {   // from the first guess; should it give up, the launches below repeat the solve from the same guess -- the same numbers
      static void (*const kern[4])(PersistArgs) = {k_pcg_persist<1>, k_pcg_persist<2>, k_pcg_persist<4>, k_pcg_persist<8>};
      if (persist_keep_x0(c, v, *pl)) return 1;
      const int e = persist_launch(c, v, *pl, persist_args(c, v, *pl), kern, "resident pcg", "POP_SolversPCG");
      if (e != 3) return e;
      if (persist_give_up(c, "the two-launch pcg", v, pl->X0)) return 1;
    }
  }
  const dim3 G = view_grid(v), B(POP_RED_THREADS);
  const int freq = cf.convergence_check_freq;
  if (solver_begin(c, 1.0)) return 1;
  HIPCHK(c, hipMemsetAsync(v.S0, 0, sizeof(double) * v.g.n2 * v.g.nblocks, c->stream));
  launch_fresidual<false>(c, v, fused_args(c, v));
  c->numIterations = cf.max_iterations;
  double rr = 0.0;
  const bool use_graph = (freq % 2 == 0) && c->f.graph;   // even: S0 / S1 end an interval where they started it
  int lerr = 0;
  const int nint = cf.max_iterations / freq;
  const int conv = run_intervals(c, nint, [&](int) -> int {
    if (use_graph) {
      hipGraphExec_t exec = graph_for(c, v.X, 0, [&]() { return fused_interval(c, v, freq); });
      if (!exec || hipGraphLaunch(exec, c->stream) != hipSuccess) return -1;
    } else if (fused_interval(c, v, freq)) return -1;
    return 1;
  }, rr, lerr);
  if (lerr) { c->err = "fused pcg: interval launch failed"; return 1; }
  if (conv >= 0) c->numIterations = (conv + 1) * freq;
  if (c->numIterations == cf.max_iterations && nint * freq < cf.max_iterations) {   // remainder without a check
    fused_iterations(c, v, cf.max_iterations - nint * freq, false);
    hipLaunchKernelGGL(k_fpcg_xr, G, B, 0, c->stream, v.g, fused_args(c, v));
  }
  // (every ghost of the solution has a source inside the view)
  return solver_finish(c, v.X, v.srcmap, (long long)v.g.n2 * v.g.nblocks, rr, "POP_SolversPCG");
}
SolveView local_view(pop_ctx *c) {
  SolveView v{};
  v.g = c->g; v.X = c->PS[c->newt]; v.R = c->R; v.Z = c->Z; v.S0 = c->S0; v.S1 = c->S1; v.Q = c->Q;
  v.RHS = c->RHS; v.C = c->centerWgt; v.partial = c->partial; v.blocksum = c->blocksum;
  v.srcmap = c->srcmap; v.gid = c->gid; v.nchunk = c->nchunk; v.nblocks_tot = c->h.nblocks_tot;
  return v;
}
// the same view for the fused pcg / ChronGear kernels: with land elimination active their launches cover only the chunks
// that hold an ocean cell (DevGrid::red_act); the partials of the chunks left out are zeroed once per solve
SolveView fused_view(pop_ctx *c) {
  SolveView v = local_view(c);
  if (c->g.skip && c->red_act) {
    v.g.red_act = c->red_act; v.g.red_cnt = c->red_cnt; v.g.red_nact = c->red_nact;
    hipMemsetAsync(v.partial, 0, (size_t)v.nchunk * v.g.nblocks * 2 * sizeof(double), c->stream);
  }
  return v;
}
// Replicated barotropic mode (small 2-D problems on several GPUs): the tropic distribution of the
// reference (domain.F90:433-543, POP_RedistributeBlocks around the solve, POP_SolversMod.F90:390-417,
// 481) taken to its limit -- every rank gathers RHS and the first guess of ALL blocks with one
// all-reduce of disjoint contributions, runs the fused solver on the whole 2-D domain with no
// per-iteration communication, and keeps its own blocks.  Arithmetic and iteration count equal the
// single-rank run (same blocks, same b4b sums).
// ---- fused solvers for blocks spread over ranks -------------------------------------------------------------------
// Ghosts with a source on this rank are read there (srcmap); ghosts owned by another rank need ONE exchange per
// iteration (z: the search direction and the solution at those ghosts are then advanced locally with the owner's
// arithmetic, so they never travel).  The message is packed by the kernel that produces z (FusedArgs::sendmap) and read
// in place from the receive buffer by the kernel that consumes it (rmap): no pack / unpack launches.  The dot products
// go through the b4b block-sum vector (own blocks' ordered sums, zeros elsewhere) and an all-reduce.  Forming the
// block sums in the producing kernel (last workgroup by atomic ticket) was measured and rejected: the agent-scope
// release every workgroup needs costs 20 ns per workgroup (profiles/probes/ticket_probe.hip: 77-88 us against 10 us
// for the two launches at 4 224 workgroups).
//   pcg       : k_fpcg_a(+pack) | block sums | all-reduce (launch stream)  ||  exchange z (side stream, own communicator)
//               k_fpcg_b(reads rbuf) | block sums | all-reduce            = 7 operations, 6 on the critical path
//   ChronGear : exchange z | k_fcg_a(reads rbuf) | block sums<2> | ONE all-reduce | k_fcg_b(+pack)   = 5 operations
// Convergence checks keep one interval of look-ahead (run_intervals): the residual lands in pinned host memory, the
// check that converges raises the device stop flag, and -- the all-reduced sums being the same bits on every rank --
// all ranks stop at the same check.  Bitwise the same results as the single-rank run.
struct DistSolve {
  pop_ctx *c; SolveView v; int nbt;
  FusedArgs args() const {
    FusedArgs a = fused_args(c, v);
    a.presummed = 1; a.nblocks = nbt; a.bsA = c->redbuf; a.bsB = c->redbuf + 2 * nbt;
    a.sendmap = c->sendmap; a.send_off = c->send_off; a.send_slot = c->send_slot; a.sendbuf = c->sendbuf;
    a.rmap = c->rmap; a.rbuf = c->recvbuf;
    return a;
  }
  // ordered block sums of every rank -> all ranks; NF interleaved fields at redbuf + off
  template <int NF> int allsum(const double *partial, long long off) {
    hipLaunchKernelGGL(k_block_sums_global<NF>, dim3(nbt), dim3(POP_RED_THREADS), 0, c->stream, partial, v.nchunk, c->loc_of_gid, c->redbuf + off);
    if (c->allred(c->comm_user, off, (long long)NF * nbt)) { c->err = "distributed solver: allreduce failed" + tr_err(c); return 1; }
    c->solver_ops += 2;
    return 0;
  }
  // the one-level exchange of the buffers the kernels packed: on the side stream beside the all-reduce when the
  // transport has a second communicator, else in line.  fork: the packed data is complete on the launch stream now.
  bool overlap = true;
  bool side() const { return overlap && c->xchg_side && c->comm_side && c->f.overlap; }
  int xchg_begin() {
    PeerSpans ps(c, 1);
    c->solver_ops += 1;
    if (side()) {
      if (hipEventRecord(c->ev_sa, c->stream) != hipSuccess || hipStreamWaitEvent(c->comm_side, c->ev_sa, 0) != hipSuccess) { c->err = "distributed solver: event failed"; return 1; }
      if (ps.exchange(c, c->xchg_side)) { c->err = "distributed solver: exchange failed" + tr_err(c); return 1; }
      if (hipEventRecord(c->ev_sx, c->comm_side) != hipSuccess) { c->err = "distributed solver: event failed"; return 1; }
      return 0;
    }
    if (ps.exchange(c, c->xchg)) { c->err = "distributed solver: exchange failed" + tr_err(c); return 1; }
    return 0;
  }
  int xchg_end() {   // the launch stream may read the receive buffer after this
    if (side() && hipStreamWaitEvent(c->stream, c->ev_sx, 0) != hipSuccess) { c->err = "distributed solver: event failed"; return 1; }
    return 0;
  }
  // residual + (r,r) of all ranks -> device scalars, pinned host ring, stop flag (the check of run_intervals)
  int check() {
    launch_fresidual<true>(c, v, args());
    if (allsum<1>(args().partA, 0)) return 1;
    hipLaunchKernelGGL(k_rr_blocks, dim3(1), dim3(1), 0, c->stream, (const double *)c->redbuf, nbt, c->sc, c->host_rr, c->h.convergenceCriterion);
    c->solver_ops += 2;
    return 0;
  }
};

int solver_pcg_fused_dist(pop_ctx *c) {
  const pop_config &cf = c->h.c;
  DistSolve D{c, fused_view(c), c->h.nblocks_tot};
  SolveView &v = D.v;
  const dim3 G = view_grid(v), B(POP_RED_THREADS);
  const int nbt = D.nbt, freq = cf.convergence_check_freq;
  if (!c->allred || !c->xchg || !c->redbuf || !c->sendbuf || c->red_doubles < 4LL * nbt) { c->err = "distributed pcg: no transport / reduce buffer"; return 1; }
  if (solver_begin(c, 1.0)) return 1;
  HIPCHK(c, hipMemsetAsync(v.S0, 0, sizeof(double) * v.g.n2 * v.g.nblocks, c->stream));
  launch_fresidual<false>(c, v, D.args());
  c->numIterations = cf.max_iterations;
  c->solver_ops = 0; c->solver_enq = 0;
  auto iterations = [&](int n, bool pending) -> int {
    for (int it = 0; it < n; ++it) {
      c->solver_enq += 1;
      FusedArgs a = D.args();
      if (pending) hipLaunchKernelGGL(k_fpcg_a<true>, G, B, 0, c->stream, v.g, a);
      else hipLaunchKernelGGL(k_fpcg_a<false>, G, B, 0, c->stream, v.g, a);
      c->solver_ops += 1;
      if (D.xchg_begin() || D.allsum<1>(a.partA, 0) || D.xchg_end()) return 1;
      launch_fpcg_b(c, v, a, pending);
      c->solver_ops += 1;
      if (D.allsum<1>(a.partB, 2 * nbt)) return 1;
      std::swap(v.S0, v.S1);
      pending = true;
    }
    return 0;
  };
  double rr = 0.0;
  int lerr = 0;
  const int nint = cf.max_iterations / freq;
  const int conv = run_intervals(c, nint, [&](int) -> int {
    if (iterations(freq, false)) return -1;
    hipLaunchKernelGGL(k_fpcg_xr, G, B, 0, c->stream, v.g, D.args());
    c->solver_ops += 1;
    if (D.check()) return -1;
    return 1;
  }, rr, lerr);
  if (lerr) { if (c->err.empty()) c->err = "distributed pcg: interval launch failed"; return 1; }
  if (conv >= 0) c->numIterations = (conv + 1) * freq;
  if (c->numIterations == cf.max_iterations && nint * freq < cf.max_iterations) {   // remainder without a check
    if (iterations(cf.max_iterations - nint * freq, false)) return 1;
    hipLaunchKernelGGL(k_fpcg_xr, G, B, 0, c->stream, v.g, D.args());
  }
  c->S0 = v.S0; c->S1 = v.S1;
  // ghosts of the solution: remote ones were advanced with their owners' arithmetic, the ones with a source on this rank
  // are copied now (srcmap is the identity on remote ghosts)
  return solver_finish(c, v.X, v.srcmap, (long long)v.g.n2 * v.g.nblocks, rr, "POP_SolversPCG");
}

int solver_pcg_replicated(pop_ctx *c) {
  SolveView &v = c->gv;
  const size_t n2 = c->g.n2, NG = n2 * c->h.nblocks_tot;
  double *PN = c->PS[c->newt];
  HIPCHK(c, hipMemsetAsync(c->redbuf, 0, sizeof(double) * 2 * NG, c->stream));
  for (int lb = 0; lb < c->g.nblocks; ++lb) {
    const size_t go = (size_t)(c->h.local_ids[lb] - 1) * n2;
    HIPCHK(c, hipMemcpyAsync(c->redbuf + go, c->RHS + lb * n2, n2 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->redbuf + NG + go, PN + lb * n2, n2 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  }
  if (c->allred(c->comm_user, 0, (long long)(2 * NG))) { c->err = "replicated solve: allreduce callback failed" + tr_err(c); return 1; }
  HIPCHK(c, hipMemcpyAsync(v.RHS, c->redbuf, NG * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(v.X, c->redbuf + NG, NG * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  hipLaunchKernelGGL(k_center_all, dim3((unsigned)((NG + 255) / 256)), dim3(256), 0, c->stream, v.g, step_params(c), c->gTAREA, c->gKMT, v.C, (long long)NG);
  const int e = solver_pcg_fused(c, v);
  if (e) return e;
  for (int lb = 0; lb < c->g.nblocks; ++lb) {
    const size_t go = (size_t)(c->h.local_ids[lb] - 1) * n2;
    HIPCHK(c, hipMemcpyAsync(PN + lb * n2, v.X + go, n2 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  }
  return 0;
}

// start-up pass of ChronGear (POP_SolversMod.F90:1990-2060): r0, z0 = M^-1 r0, the first dot products, x1.  fused: the fused forms
// (diagonal preconditioner only) also want 1/A0 in S1 for their kernels
int cg_startup(pop_ctx *c, bool fused) {
  const dim3 G = grid_2d(c), B(POP_RED_THREADS);
  if (solver_begin(c)) return 1;
  SolverArgs a = solver_args(c);
  hipLaunchKernelGGL(k_residual<false>, G, B, 0, c->stream, c->g, a);
  if (halo_update(c, c->R, 1)) return 1;
  if (c->use_evp && !fused) {   // :2009-2032
    if (evp_apply(c, c->R, c->Z) || halo_update(c, c->Z, 1)) return 1;
    hipLaunchKernelGGL(k_cg_init<true>, G, B, 0, c->stream, c->g, a);
  } else hipLaunchKernelGGL(k_cg_init<false>, G, B, 0, c->stream, c->g, a);
  if (halo_update(c, c->Q, 1)) return 1;
  if (reduce_finish<2>(c, FIN_CG_INIT)) return 1;
  hipLaunchKernelGGL(k_cg_update<true>, G, B, 0, c->stream, c->g, a);
  const long long a2 = (long long)c->g.n2 * c->g.nblocks;
  if (fused) hipLaunchKernelGGL(k_pcsi_a0r, dim3((unsigned)((a2 + 255) / 256)), dim3(256), 0, c->stream, (const double *)c->centerWgt, c->S1, a2);
  return 0;
}

// ChronGear (POP_SolversMod.F90:1960-2266), diagonal or EVP preconditioner
int solver_chrongear(pop_ctx *c) {
  const pop_config &cf = c->h.c;
  const dim3 G = grid_2d(c), B(POP_RED_THREADS);
  if (cg_startup(c, false)) return 1;
  SolverArgs a = solver_args(c);
  c->numIterations = cf.max_iterations;
  double rr = 0.0;
  for (int m = 1; m <= cf.max_iterations; ++m) {
    if (c->use_evp) { if (evp_apply(c, c->R, c->Z)) return 1; }
    else hipLaunchKernelGGL(k_cg_z, G, B, 0, c->stream, c->g, a);
    if (halo_update(c, c->Z, 1)) return 1;
    hipLaunchKernelGGL(k_cg_az, G, B, 0, c->stream, c->g, a);
    if (reduce_finish<2>(c, FIN_CG_ITER)) return 1;
    hipLaunchKernelGGL(k_cg_update<false>, grid_2d(c), B, 0, c->stream, c->g, a);
    if (m % cf.convergence_check_freq == 0) {
      hipLaunchKernelGGL(k_residual<true>, grid_2d(c), B, 0, c->stream, c->g, a);
      if (halo_update(c, c->R, 1)) return 1;
      if (reduce_finish<1>(c, FIN_RR)) return 1;
      SolverScalars s;
      if (read_scalars(c, &s)) return 1;
      rr = s.rr;
      if (rr < c->h.convergenceCriterion) { c->numIterations = m; break; }
    }
  }
  return solver_finish(c, nullptr, nullptr, 0, rr, "POP_SolversChronGear");
}

// ChronGear, fused form for one rank: the start-up pass as in solver_chrongear, then two launches per iteration
// (k_fcg_a, k_fcg_b: the z halo folded into the matvec through srcmap, scalar recurrences recomputed by every
// workgroup from the ordered totals) and one hipGraph replay per check interval.  Same arithmetic and summation
// order as solver_chrongear: bitwise the same solution and iteration count.
// compacted launches (DevGrid::red_act): the iterations store pairs of partials, the checks single ones, in the same slots;
// chunks that are not launched cannot zero theirs, so the slots are cleared whenever the layout changes
static void cg_clear_partials(pop_ctx *c, const SolveView &v) {
  if (v.g.red_act) hipMemsetAsync(v.partial, 0, (size_t)v.nchunk * v.g.nblocks * 2 * sizeof(double), c->stream);
}
// the arguments of the fused ChronGear kernels: those of the fused pcg plus the matvec of z and 1/A0 (cg_startup left it in S1)
static FusedArgs cg_args(pop_ctx *c, const SolveView &v, FusedArgs a) { a.AZ = c->AZ; a.A0R = v.S1; return a; }
// step A of the fused ChronGear: two cells per thread on large grids, else one
static void launch_fcg_a(pop_ctx *c, const SolveView &v, const FusedArgs &a, bool presummed) {
  if (two_cell_ok(c->f, v.g, presummed)) hipLaunchKernelGGL(k_fcg_a2, view_grid(v), dim3(POP_RED_THREADS / 2), 0, c->stream, v.g, a);
  else hipLaunchKernelGGL(k_fcg_a, view_grid(v), dim3(POP_RED_THREADS), 0, c->stream, v.g, a);
}
// n iterations; par: the (rho, sigma) ping-pong slot the first one reads
static void cg_fused_iterations(pop_ctx *c, SolveView &v, int n, int par) {
  for (int it = 0; it < n; ++it, par = 1 - par) {
    const FusedArgs a = cg_args(c, v, fused_args(c, v));
    launch_fcg_a(c, v, a, a.presummed != 0);
    if (a.presummed) presum<2>(c, v, a.partA, (double *)a.bsA);
    hipLaunchKernelGGL(k_fcg_b, view_grid(v), dim3(POP_RED_THREADS), 0, c->stream, v.g, a, par);
  }
}
// one check interval: freq iterations, residual + (r,r) -> host
static int cg_fused_interval(pop_ctx *c, SolveView &v, int freq, int par) {
  cg_fused_iterations(c, v, freq, par);
  cg_clear_partials(c, v);
  launch_fresidual<true>(c, v, fused_args(c, v));
  hipLaunchKernelGGL(k_rr_total, dim3(1), dim3(POP_RED_THREADS), 0, c->stream, (const double *)v.partial, v.nchunk, v.g.nblocks, c->sc, c->host_rr, c->h.convergenceCriterion);
  cg_clear_partials(c, v);
  return 0;
}
int solver_chrongear_fused(pop_ctx *c) {
  const pop_config &cf = c->h.c;
  SolveView v = fused_view(c);
  const int freq = cf.convergence_check_freq;
  if (cg_startup(c, true)) return 1;
  c->persist_used = 0;
  // small views: the iterations as one resident launch (k_cg_persist)
  if (c->f.persist &&!fused_args(c, v).presummed && !c->persist_gave_up &&
      v.g.nblocks * ((v.nchunk + POP_RED_THREADS - 1) / POP_RED_THREADS) <= POP_CGP_MAXP) {
    if (const pop_ctx::PersistPlan *pl = persist_plan(c, v)) {
      static void (*const kern[4])(CgPersistArgs) = {k_cg_persist<1>, k_cg_persist<2>, k_cg_persist<4>, k_cg_persist<8>};
      CgPersistArgs ca{};
      ca.p = persist_args(c, v, *pl);
      ca.R = v.R; ca.S = v.S0; ca.Q = v.Q; ca.A0R = v.S1; ca.sc = c->sc;
      if (persist_keep_x0(c, v, *pl)) return 1;   // x after the start-up pass
      const int e = persist_launch(c, v, *pl, ca, kern, "resident ChronGear", "POP_SolversChronGear");
      if (e != 3) return e;
      if (persist_give_up(c, "the two-launch ChronGear", v, pl->X0)) return 1;   // r, s, q and the scalars were only read
    }
  }
  c->numIterations = cf.max_iterations;
  double rr = 0.0;
  // a graph holds the ping-pong slots of its iterations: valid for every interval only when freq is even (each then starts at slot 0)
  const bool use_graph = (freq % 2 == 0) && c->f.graph;
  int lerr = 0;
  const int nint = cf.max_iterations / freq;
  const int conv = run_intervals(c, nint, [&](int i) -> int {
    const int par = (i * freq) & 1;   // odd freq: the slot carries over between intervals
    if (use_graph) {
      hipGraphExec_t exec = graph_for(c, v.X, 0, [&]() { return cg_fused_interval(c, v, freq, par); });
      if (!exec || hipGraphLaunch(exec, c->stream) != hipSuccess) return -1;
    } else cg_fused_interval(c, v, freq, par);
    return 1;
  }, rr, lerr);
  if (lerr) { c->err = "fused ChronGear: interval launch failed"; return 1; }
  if (conv >= 0) c->numIterations = (conv + 1) * freq;
  if (c->numIterations == cf.max_iterations && nint * freq < cf.max_iterations)   // remainder without a check
    cg_fused_iterations(c, v, cf.max_iterations - nint * freq, (nint * freq) & 1);
  return solver_finish(c, v.X, v.srcmap, (long long)v.g.n2 * v.g.nblocks, rr, "POP_SolversChronGear");
}

// ChronGear for blocks spread over ranks (see DistSolve): start-up pass as in solver_chrongear, then per iteration
// exchange z | k_fcg_a | block sums of (r,z), (az,z) | ONE all-reduce | k_fcg_b, which also packs the next z
int solver_chrongear_fused_dist(pop_ctx *c) {
  const pop_config &cf = c->h.c;
  DistSolve D{c, local_view(c), c->h.nblocks_tot};   // whole launches: the (r,r) partials of the checks and the pairs of the iterations share slots
  D.overlap = false;   // nothing runs beside the exchange here: the next kernel needs it
  SolveView &v = D.v;
  const dim3 G = view_grid(v), B(POP_RED_THREADS);
  const int nbt = D.nbt, freq = cf.convergence_check_freq;
  if (!c->allred || !c->xchg || !c->redbuf || !c->sendbuf || c->red_doubles < 4LL * nbt) { c->err = "distributed ChronGear: no transport / reduce buffer"; return 1; }
  if (cg_startup(c, true)) return 1;
  // z of the first iteration at the neighbours' ghosts: z = r*A0R on the whole array, packed and exchanged once
  hipLaunchKernelGGL(k_cg_z, grid_2d(c), B, 0, c->stream, c->g, solver_args(c));
  if (c->nsend_all) hipLaunchKernelGGL(k_halo_pack_all, dim3((c->nsend_all + 255) / 256, 1), dim3(256), 0, c->stream, (const double *)c->Z, c->sa_src, c->sa_start, c->sa_cnt, c->nsend_all, c->sendbuf, 1, c->g.n2);
  if (D.xchg_begin()) return 1;
  c->numIterations = cf.max_iterations;
  c->solver_ops = 0; c->solver_enq = 0;
  // Two cells per thread by the SIZE rule alone: DistSolve::args() sets presummed = 1 on every grid (the sums go through the all-reduce), and
  // pop_tuning.solver_presum forces it too; neither makes a small grid a large one, and k_fcg_a2 / k_fresidual2 are the large-grid forms
  const bool large = presum_by_size(v.nchunk, v.g.nblocks);
  auto iterations = [&](int n, int par) -> int {
    for (int it = 0; it < n; ++it, par = 1 - par) {
      c->solver_enq += 1;
      const FusedArgs a = cg_args(c, v, D.args());
      launch_fcg_a(c, v, a, large);
      c->solver_ops += 1;
      if (D.allsum<2>(a.partA, 0)) return 1;
      hipLaunchKernelGGL(k_fcg_b, G, B, 0, c->stream, v.g, a, par);
      c->solver_ops += 1;
      if (D.xchg_begin()) return 1;
    }
    return 0;
  };
  double rr = 0.0;
  int lerr = 0;
  const int nint = cf.max_iterations / freq;
  const int conv = run_intervals(c, nint, [&](int i) -> int {
    if (iterations(freq, (i * freq) & 1)) return -1;
    // r = b - A x; its z = r*A0R is packed by the residual kernel and exchanged for the next interval
    const FusedArgs a = cg_args(c, v, D.args());
    launch_fresidual<true>(c, v, a, large);
    if (D.allsum<1>(a.partA, 0)) return -1;
    hipLaunchKernelGGL(k_rr_blocks, dim3(1), dim3(1), 0, c->stream, (const double *)c->redbuf, nbt, c->sc, c->host_rr, c->h.convergenceCriterion);
    if (D.xchg_begin()) return -1;
    c->solver_ops += 2;
    return 1;
  }, rr, lerr);
  if (lerr) { if (c->err.empty()) c->err = "distributed ChronGear: interval launch failed"; return 1; }
  if (conv >= 0) c->numIterations = (conv + 1) * freq;
  if (c->numIterations == cf.max_iterations && nint * freq < cf.max_iterations &&   // remainder without a check
      iterations(cf.max_iterations - nint * freq, (nint * freq) & 1)) return 1;
  return solver_finish(c, v.X, v.srcmap, (long long)v.g.n2 * v.g.nblocks, rr, "POP_SolversChronGear");
}

// ---------------------------------------------------------------------------------------------
// P-CSI (POP_SolversMod.F90:1510-1835), diagonal or EVP preconditioner (EVP: operation-by-operation form only).  kernels_pcsi.hpp describes the
// fused one-launch-per-iteration form; solver_pcsi is the operation-by-operation form that also
// serves multi-rank runs (one halo update per iteration, no collective except at the checks).
// ---------------------------------------------------------------------------------------------
__global__ void k_set_int(int *p, int v) { *p = v; }

int pcsi_check_start(const pop_ctx *c) { return c->h.c.convergence_check_start > 0 ? c->h.c.convergence_check_start : 60; }   // convergenceCheckStart :636

int solver_pcsi(pop_ctx *c) {
  const pop_config &cf = c->h.c;
  const dim3 B(POP_RED_THREADS);
  const long long a2 = (long long)c->g.n2 * c->g.nblocks;
  const dim3 G1((unsigned)((a2 + 255) / 256)), B1(256);
  if (solver_begin(c)) return 1;
  SolverArgs a = solver_args(c);
  hipLaunchKernelGGL(k_residual<false>, grid_2d(c), B, 0, c->stream, c->g, a);
  auto precond = [&]() -> int {   // r' = M^-1 r in place (:1646-1660, :1738-1752)
    if (c->use_evp) {
      if (evp_apply(c, c->R, c->Z)) return 1;
      HIPCHK(c, hipMemcpyAsync(c->R, c->Z, sizeof(double) * a2, hipMemcpyDeviceToDevice, c->stream));
    } else hipLaunchKernelGGL(k_pcsi_precond, G1, B1, 0, c->stream, c->g, c->R, (const double *)c->centerWgt, a2);
    return 0;
  };
  if (precond()) return 1;
  if (halo_update(c, c->R, 1)) return 1;
  hipLaunchKernelGGL(k_pcsi_update<true>, G1, B1, 0, c->stream, (const double *)c->R, c->Q, a.X, a2, (const double *)c->pcsi_omega,
                     (const int *)c->pcsi_base, 0, c->pcsi_csy);
  hipLaunchKernelGGL(k_residual<false>, grid_2d(c), B, 0, c->stream, c->g, a);
  c->numIterations = cf.max_iterations;
  double rr = 0.0;
  const int start = pcsi_check_start(c);
  for (int m = 1; m <= cf.max_iterations; ++m) {
    hipLaunchKernelGGL(k_set_int, dim3(1), dim3(1), 0, c->stream, c->pcsi_base, m - 1);
    if (precond()) return 1;
    if (halo_update(c, c->R, 1)) return 1;
    hipLaunchKernelGGL(k_pcsi_update<false>, G1, B1, 0, c->stream, (const double *)c->R, c->Q, a.X, a2, (const double *)c->pcsi_omega,
                       (const int *)c->pcsi_base, 1, c->pcsi_csy);
    const bool check = (m % cf.convergence_check_freq == 0) && m >= start;
    if (check) hipLaunchKernelGGL(k_residual<true>, grid_2d(c), B, 0, c->stream, c->g, a);
    else hipLaunchKernelGGL(k_residual<false>, grid_2d(c), B, 0, c->stream, c->g, a);
    if (check) {
      if (reduce_finish<1>(c, FIN_RR)) return 1;
      SolverScalars s;
      if (read_scalars(c, &s)) return 1;
      rr = s.rr;
      if (rr < c->h.convergenceCriterion) { c->numIterations = m; break; }
    }
  }
  return solver_finish(c, nullptr, nullptr, 0, rr, "POP_SolversPCSI");
}

// fused form; state ping-pongs between (X, R, Q) and (Z, AZ, S1)
struct PcsiBufs { double *X[2], *R[2], *Q[2]; };
static PcsiArgs pcsi_args(pop_ctx *c, const PcsiBufs &bf, int in, int j) {
  PcsiArgs a{};
  a.Xi = bf.X[in]; a.Ri = bf.R[in]; a.Qi = bf.Q[in]; a.Xo = bf.X[1 - in]; a.Ro = bf.R[1 - in]; a.Qo = bf.Q[1 - in];
  a.Bv = c->RHS; a.C = c->centerWgt; a.A0R = c->S0; a.omega = c->pcsi_omega; a.base = c->pcsi_base; a.srcmap = c->srcmap; a.partial = c->partial; a.sc = c->sc;
  a.csy = c->pcsi_csy; a.j = j; a.nchunk = c->nchunk;
  if (c->use_evp) { a.raw_r = 1; a.Ri = c->R; a.Ro = c->AZ; }   // r' = M^-1 r in R (read), the residual itself to AZ (written): evp_apply(AZ -> R) follows every step
  return a;
}
// DevGrid of the single-rank fused P-CSI launches: with land elimination active, the compacted chunk list (DevGrid::red_act)
static DevGrid pcsi_grid(const pop_ctx *c) {
  DevGrid g = c->g;
  if (c->g.skip && c->red_act && c->peers.empty()) { g.red_act = c->red_act; g.red_cnt = c->red_cnt; g.red_nact = c->red_nact; }
  return g;
}
// `freq` steps starting from buffer `in`; the last one also forms (r,r) -> host when with_rr
// two iterations per launch (k_pcsi_step_x2): how many of the n iterations of an interval go in pairs -- the last two stay single (the check
// needs the chunk partials of (r, r) of k_pcsi_step2, and a single step before it keeps the pairs aligned for every n)
// An interval of an even number of iterations goes in pairs throughout: the pair before a check leaves the residual itself in a scratch field
// and k_pcsi_rr_chunks forms the chunk partials of (r, r) from it.  An odd interval: pairs, then one single step (which carries the check).
static int pcsi_pairs(const pop_ctx *c, int n) { return c->f.pcsi_two_step ? n / 2 : 0; }
// one pair; with_raw: the residual itself to pcsi_raw as well, and the chunk partials of (r, r) from it
static void pcsi_launch_pair(pop_ctx *c, const DevGrid &gg, PcsiArgs a, bool with_raw) {
  const int tiles_i = (gg.nxb - 2 * NGHOST + 63) / 64, tiles_j = (gg.nyb - 2 * NGHOST + 7) / 8;
  const dim3 GT(lds_launch_x<8>(gg, tiles_i, tiles_j), gg.nblocks), TB(64, 8);
  a.jfold = c->pcsi_jfold;
  double *raw = with_raw ? c->pcsi_raw : nullptr;
  if (a.jfold) {
    if (with_raw) hipLaunchKernelGGL((k_pcsi_step_x2<true, true>), GT, TB, 0, c->stream, gg, a, raw);
    else hipLaunchKernelGGL((k_pcsi_step_x2<false, true>), GT, TB, 0, c->stream, gg, a, raw);
  } else if (with_raw) hipLaunchKernelGGL((k_pcsi_step_x2<true, false>), GT, TB, 0, c->stream, gg, a, raw);
  else hipLaunchKernelGGL((k_pcsi_step_x2<false, false>), GT, TB, 0, c->stream, gg, a, raw);
  if (with_raw) hipLaunchKernelGGL(k_pcsi_rr_chunks, dim3(red_grid_x(gg), gg.nblocks), dim3(POP_RED_THREADS), 0, c->stream, gg, a, (const double *)raw);
}
static int pcsi_launches(const pop_ctx *c, int n) { return n - pcsi_pairs(c, n); }
static void pcsi_interval(pop_ctx *c, const PcsiBufs &bf, int in, int freq, bool with_rr) {
  const DevGrid gg = pcsi_grid(c);
  const dim3 G(red_grid_x(gg), gg.nblocks), B(POP_RED_THREADS);
  int j0 = 1;
  const int npairs = pcsi_pairs(c, freq);
  for (int p = 0; p < npairs; ++p, j0 += 2) {
    pcsi_launch_pair(c, gg, pcsi_args(c, bf, in, j0), with_rr && j0 + 1 == freq);   // (the last pair of an even interval that ends in a check)
    in = 1 - in;
  }
  for (int j = j0; j <= freq; ++j) {
    const PcsiArgs a = pcsi_args(c, bf, in, j);
    if (c->f.pcsi_two_cell) {
      const bool rr = j == freq && with_rr;
      if (rr && c->use_evp) hipLaunchKernelGGL((k_pcsi_step2<true, true>), G, dim3(POP_RED_THREADS / 2), 0, c->stream, gg, a);
      else if (c->use_evp) hipLaunchKernelGGL((k_pcsi_step2<false, true>), G, dim3(POP_RED_THREADS / 2), 0, c->stream, gg, a);
      else if (rr) hipLaunchKernelGGL((k_pcsi_step2<true>), G, dim3(POP_RED_THREADS / 2), 0, c->stream, gg, a);
      else hipLaunchKernelGGL((k_pcsi_step2<false>), G, dim3(POP_RED_THREADS / 2), 0, c->stream, gg, a);
    } else if (j == freq && with_rr) hipLaunchKernelGGL((k_pcsi_step<false, true>), G, B, 0, c->stream, gg, a);
    else hipLaunchKernelGGL((k_pcsi_step<false, false>), G, B, 0, c->stream, gg, a);
    if (c->use_evp) evp_apply(c, c->AZ, c->R);
    in = 1 - in;
  }
  if (with_rr) {
    hipLaunchKernelGGL(k_rr_total, dim3(1), dim3(POP_RED_THREADS), 0, c->stream, (const double *)c->partial, c->nchunk, c->g.nblocks, c->sc, c->host_rr, c->h.convergenceCriterion);
  }
}
int solver_pcsi_fused(pop_ctx *c) {
  const pop_config &cf = c->h.c;
  const dim3 G = grid_2d(c), B(POP_RED_THREADS);
  const int freq = cf.convergence_check_freq, start = pcsi_check_start(c);
  PcsiBufs bf{{c->PS[c->newt], c->Z}, {c->R, c->AZ}, {c->Q, c->S1}};   // (with EVP the residual pair is fixed: pcsi_args)
  if (solver_begin(c)) return 1;
  // r0 = b - A x0 (ghosts of x0 read at their sources), then the start-up step x1 = x0 + r0'/gamma, r1 = b - A x1
  {
    SolveView v = local_view(c);
    const long long a2 = (long long)c->g.n2 * c->g.nblocks;
    hipLaunchKernelGGL(k_pcsi_a0r, dim3((unsigned)((a2 + 255) / 256)), dim3(256), 0, c->stream, (const double *)c->centerWgt, c->S0, a2);
    if (c->use_evp) {   // r0 into AZ, r0' = M^-1 r0 by the sub-block solves into R; both start from zero (cells no kernel writes are never read)
      HIPCHK(c, hipMemsetAsync(c->AZ, 0, sizeof(double) * a2, c->stream));
      HIPCHK(c, hipMemsetAsync(c->R, 0, sizeof(double) * a2, c->stream));
      v.R = c->AZ;
      hipLaunchKernelGGL(k_fresidual<false>, G, B, 0, c->stream, c->g, fused_args(c, v));
      if (evp_apply(c, c->AZ, c->R)) return 1;
    } else {
      hipLaunchKernelGGL(k_fresidual<false>, G, B, 0, c->stream, c->g, fused_args(c, v));
      hipLaunchKernelGGL(k_pcsi_scale, dim3((c->g.n2 + 255) / 256, c->g.nblocks), dim3(256), 0, c->stream, c->g, c->R, (const double *)c->S0);
    }
  }
  hipLaunchKernelGGL((k_pcsi_step<true, false>), G, B, 0, c->stream, c->g, pcsi_args(c, bf, 0, 0));
  if (c->use_evp && evp_apply(c, c->AZ, c->R)) return 1;
  c->persist_used = 0;
  if (!c->use_evp && c->f.persist && !c->persist_gave_up) {
    // small views: the iterations as one resident launch (k_pcsi_persist: neighbour waits only, grid-wide exchanges at the checks)
    const SolveView v = local_view(c);   // (v.X is bf.X[0])
    const pop_ctx::PersistPlan *pl = fused_args(c, v).presummed ? nullptr : persist_plan(c, v);
    if (pl) {
      static void (*const kern[4])(PcsiPersistArgs) = {k_pcsi_persist<1>, k_pcsi_persist<2>, k_pcsi_persist<4>, k_pcsi_persist<8>};
      PcsiPersistArgs pa{};
      pa.p = persist_args(c, v, *pl);
      pa.Xin = bf.X[1]; pa.Rin = bf.R[1]; pa.Qin = bf.Q[1]; pa.A0R = c->S0; pa.omega = c->pcsi_omega; pa.csy = c->pcsi_csy; pa.start = start;
      const int e = persist_launch(c, v, *pl, pa, kern, "resident P-CSI", "POP_SolversPCSI");
      if (e != 3) return e;
      // the launch wrote its solution array only at its end (x of the start-up step is still in the other half of the pair; r', dx
      // were only read): nothing to restore, the launches below repeat the iterations
      if (persist_give_up(c, "one launch per iteration", v, nullptr)) return 1;
    }
  }
  if (pcsi_grid(c).red_act)   // compacted launches from here on: the partials of the chunks that are left out must read as zero
    HIPCHK(c, hipMemsetAsync(c->partial, 0, (size_t)c->nchunk * c->g.nblocks * 2 * sizeof(double), c->stream));
  int in = 1;
  c->numIterations = cf.max_iterations;
  double rr = 0.0;
  // intervals of `freq` steps (the last one may be shorter); those that end on a multiple of freq at or after
  // convergenceCheckStart carry a check.  in_before[i]: ping-pong half interval i starts from
  const int nint = (cf.max_iterations + freq - 1) / freq;
  std::vector<int> in_after(nint + 1, in);
  int lerr = 0;
  const int conv = run_intervals(c, nint, [&](int i) -> int {
    const int m = i * freq, n = std::min(freq, cf.max_iterations - m);
    const bool with_rr = (n == freq) && (m + n >= start);
    hipLaunchKernelGGL(k_set_int, dim3(1), dim3(1), 0, c->stream, c->pcsi_base, m);
    if (c->f.graph && n == freq) {   // one graph per ping-pong half the interval starts from, with and without the check
      hipGraphExec_t exec = graph_for(c, bf.X[0], in * 2 + (with_rr ? 1 : 0), [&]() { pcsi_interval(c, bf, in, n, with_rr); return 0; });
      if (!exec || hipGraphLaunch(exec, c->stream) != hipSuccess) return -1;
    } else pcsi_interval(c, bf, in, n, with_rr);
    if (pcsi_launches(c, n) % 2) in = 1 - in;
    in_after[i] = in;
    return with_rr ? 1 : 0;
  }, rr, lerr);
  if (lerr) { c->err = "fused P-CSI: interval launch failed"; return 1; }
  if (conv >= 0) { c->numIterations = (conv + 1) * freq; in = in_after[conv]; }   // later intervals did nothing on the device
  const long long ncell = (long long)c->g.n2 * c->g.nblocks;
  if (in == 1) HIPCHK(c, hipMemcpyAsync(bf.X[0], bf.X[1], sizeof(double) * ncell, hipMemcpyDeviceToDevice, c->stream));
  return solver_finish(c, bf.X[0], c->srcmap, ncell, rr, "POP_SolversPCSI");
}

// fused P-CSI with blocks spread over ranks: one halo exchange (r') and one launch per iteration, a block-sum
// all-reduce only at the convergence checks
int solver_pcsi_fused_dist(pop_ctx *c) {
  const pop_config &cf = c->h.c;
  const dim3 G = grid_2d(c), B(POP_RED_THREADS);
  const int freq = cf.convergence_check_freq, start = pcsi_check_start(c), nbt = c->h.nblocks_tot;
  if (!c->allred || !c->redbuf || c->red_doubles < nbt) { c->err = "distributed P-CSI: no transport / reduce buffer"; return 1; }
  PcsiBufs bf{{c->PS[c->newt], c->Z}, {c->R, c->AZ}, {c->Q, c->S1}};
  if (solver_begin(c)) return 1;
  const long long a2 = (long long)c->g.n2 * c->g.nblocks;
  {
    SolveView v = local_view(c);
    hipLaunchKernelGGL(k_pcsi_a0r, dim3((unsigned)((a2 + 255) / 256)), dim3(256), 0, c->stream, (const double *)c->centerWgt, c->S0, a2);
    hipLaunchKernelGGL(k_fresidual<false>, G, B, 0, c->stream, c->g, fused_args(c, v));
    hipLaunchKernelGGL(k_pcsi_scale, dim3((c->g.n2 + 255) / 256, c->g.nblocks), dim3(256), 0, c->stream, c->g, c->R, (const double *)c->S0);
  }
  auto step = [&](int in, int j, bool first, bool rr) -> int {
    if (halo_remote(c, bf.R[in], 1)) return 1;
    PcsiArgs a = pcsi_args(c, bf, in, j);
    a.remote_ghosts = 1;
    if (first) hipLaunchKernelGGL((k_pcsi_step<true, false>), G, B, 0, c->stream, c->g, a);
    else if (c->f.pcsi_two_cell && rr) hipLaunchKernelGGL((k_pcsi_step2<true>), G, dim3(POP_RED_THREADS / 2), 0, c->stream, c->g, a);
    else if (c->f.pcsi_two_cell) hipLaunchKernelGGL((k_pcsi_step2<false>), G, dim3(POP_RED_THREADS / 2), 0, c->stream, c->g, a);
    else if (rr) hipLaunchKernelGGL((k_pcsi_step<false, true>), G, B, 0, c->stream, c->g, a);
    else hipLaunchKernelGGL((k_pcsi_step<false, false>), G, B, 0, c->stream, c->g, a);
    return 0;
  };
  if (step(0, 0, true, false)) return 1;
  int in = 1;
  c->numIterations = cf.max_iterations;
  double rr = 0.0;
  if (c->f.pcsi_two_step_dist && halo_update_many(c, {{c->RHS, 1}})) return 1;   // the pairs form r at the first ring of ghost cells
  // two iterations per launch across ranks (k_pcsi_step_x2): x, dx and r' travel two rings wide once per PAIR instead of r' once per
  // iteration -- half the messages per iteration
  const bool pairs = c->f.pcsi_two_step_dist;
  const DevGrid gg = c->g;
  for (int m = 1; m <= cf.max_iterations; ++m) {
    bool check = (m % freq == 0) && m >= start;
    hipLaunchKernelGGL(k_set_int, dim3(1), dim3(1), 0, c->stream, c->pcsi_base, m - 1);
    if (pairs && !check && m + 1 <= cf.max_iterations) {
      if (halo_update_many(c, {{bf.X[in], 1}, {bf.Q[in], 1}, {bf.R[in], 1}})) return 1;
      const bool check2 = ((m + 1) % freq == 0) && m + 1 >= start;
      pcsi_launch_pair(c, gg, pcsi_args(c, bf, in, 1), check2);
      ++m; check = check2;
    } else {
      if (pairs && halo_update_many(c, {{bf.X[in], 1}, {bf.Q[in], 1}})) return 1;   // (the pairs do not advance x, dx at the ghosts of other ranks)
      if (step(in, 1, false, check)) return 1;
    }
    in = 1 - in;
    if (check) {
      hipLaunchKernelGGL(k_block_sums_global<1>, dim3(nbt), dim3(POP_RED_THREADS), 0, c->stream, (const double *)c->partial, c->nchunk, c->loc_of_gid, c->redbuf);
      if (c->allred(c->comm_user, 0, nbt)) { c->err = "distributed P-CSI: allreduce failed" + tr_err(c); return 1; }
      hipLaunchKernelGGL(k_finalize<1>, dim3(1), dim3(1), 0, c->stream, c->redbuf, nbt, c->sc, (int)FIN_RR);
      SolverScalars s;
      if (read_scalars(c, &s)) return 1;
      rr = s.rr;
      if (rr < c->h.convergenceCriterion) { c->numIterations = m; break; }
    }
  }
  if (in == 1) HIPCHK(c, hipMemcpyAsync(bf.X[0], bf.X[1], sizeof(double) * a2, hipMemcpyDeviceToDevice, c->stream));
  if (pairs && halo_remote(c, bf.X[0], 1)) return 1;   // (the single steps keep x current at the ghosts of other ranks; the pairs do not)
  return solver_finish(c, bf.X[0], c->srcmap, a2, rr, "POP_SolversPCSI");
}

// elapsed time of the last bracketed solve into the totals (waits for its closing event: at the next solve that is long past)
void solve_collect(pop_ctx *c) {
  if (!c->solve_pending) return;
  c->solve_pending = false;
  float ms = 0;
  if (hipEventSynchronize(c->ev_solve[1]) == hipSuccess && hipEventElapsedTime(&ms, c->ev_solve[0], c->ev_solve[1]) == hipSuccess) {
    c->solver_ms_total += ms; c->solver_iters_total += c->solve_iters_pending; c->solver_calls_total += 1;
  }
}

// POP_SolversRun: the driver of the configured solver (1 pcg, 2 ChronGear, 3 P-CSI) in the form the plan names (Forms::path: 1 operation
// by operation, 2 fused on one rank, 3 fused with the blocks spread over ranks, 4 replicated fused solve on every rank)
int solver_run(pop_ctx *c) {
  const int path = c->f.path, choice = c->h.c.solver_choice;
  if (choice == 2) return path == 2 ? solver_chrongear_fused(c) : path == 3 ? solver_chrongear_fused_dist(c) : solver_chrongear(c);
  if (choice == 3) return path == 2 ? solver_pcsi_fused(c) : path == 3 ? solver_pcsi_fused_dist(c) : solver_pcsi(c);
  switch (path) {
    case 4:
      if (!c->allred || !c->redbuf || c->red_doubles < 2LL * c->g.n2 * c->h.nblocks_tot) { c->err = "replicated solve needs pop_set_comm with a reduce buffer of pop_reduce_buffer_doubles()"; return 1; }
      return solver_pcg_replicated(c);
    case 2: { SolveView v = fused_view(c); const int e = solver_pcg_fused(c, v); c->S0 = v.S0; c->S1 = v.S1; return e; }
    case 3: return solver_pcg_fused_dist(c);
    default: return solver_pcg(c);
  }
}

}  // namespace
