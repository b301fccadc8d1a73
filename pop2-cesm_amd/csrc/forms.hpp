// forms.hpp -- the plan: every choice the library makes about kernel forms and schedule, resolved ONCE at pop_create* by
// resolve_forms and read everywhere else (pop_ctx::f).  Plain host C++: no HIP call, nothing that needs a device, so a host-only
// context carries the same plan.  Order of every entry: the library's rule, then the caller's pop_tuning / the POP_* environment
// (pop_amd.hip tuning_resolve has merged the two into HostModel::tun, which nothing but this file reads).  pop_get_tuning returns
// that request; pop_get_dim("form_<entry>") returns the outcome below.
#pragma once
#include <algorithm>
#include "pop_internal.hpp"

namespace pop {

// ---- the entries (type, name): one list, which declares the struct and serves pop_get_dim("form_<name>")
enum { VMIXU_INLINE = 0, VMIXU_SIDE = 1, VMIXU_DEFERRED = 2 };                      // Forms::vmixu
enum { KPP_BUOY_MARCH = 0, KPP_BUOY_FUSED_LDS, KPP_BUOY_LDS, KPP_BUOY_PLAIN };      // Forms::kpp_buoy; MARCH and FUSED_LDS form the interior coefficients too
enum { KPP_INTERIOR_FUSED = 0, KPP_INTERIOR_REG, KPP_INTERIOR_GENERIC };            // Forms::kpp_interior
#define POP_FORMS(X)                                                                                                                 \
  /* workgroup orders (kernels_common.hpp; copied into DevGrid) */                                                                 \
  X(int, xcd_remap) X(int, red_band) X(int, lds_order)                                                                              \
  /* land elimination: skip workgroups without an ocean cell; steps after set-up / a restart / a new state that run them all */   \
  X(bool, land_skip) X(int, land_full_steps)                                                                                        \
  /* right-hand-side kernels: LDS tile rows (0 = the direct-load kernel), Gent-McWilliams through the tiled forms, KPP_SRC read at \
     every level, predictor with the forward elimination inside the tracer kernel (the part that does not depend on the step) */   \
  X(int, momentum_lds_rows) X(int, tracer_lds_rows) X(bool, gm_lds) X(bool, kpp_src_full) X(bool, tracer_fwd)                       \
  /* Thomas kernels: column in registers for U, V / the tracers (level count included), both tracers in one thread, waves per      \
     workgroup of the velocity solve */                                                                                             \
  X(bool, reg_thomas_u) X(bool, reg_thomas_t) X(bool, thomas_pair) X(int, impvmixu_waves)                                           \
  /* shared arrays and streams */                                                                                                   \
  X(bool, vdc_shared) X(bool, side_stream) X(bool, del4_side) X(bool, mom_side) X(bool, aniso_side)                                 \
  /* del4: patch rows of the first Laplacians (and of k_kpp_vvc; 0 = 256 consecutive cells), the previous step's tracer / momentum \
     launch forms them */                                                                                                           \
  X(int, del4_tile_rows) X(bool, d2t_fuse) X(bool, d2u_fuse)                                                                        \
  /* implicit vertical mixing of U, V: VMIXU_*; the barotropic velocity added in the step tail (the reference's order) */           \
  X(int, vmixu) X(bool, btrop_inline)                                                                                               \
  /* KPP: the next step's coefficients beside the barotropic solver; the mask of kernel forms and what kpp_vmix_coeffs selects     \
     from it before it knows the step (kernels_kpp.hpp) */                                                                          \
  X(bool, kpp_ahead) X(int, kpp_col) X(bool, kpp_lazy) X(bool, kpp_lazy20) X(bool, kpp_march) X(bool, kpp_pbc_generic)              \
  X(bool, kpp_shear_col) X(int, kpp_buoy) X(int, kpp_buoy_kr) X(bool, kpp_buoy_sfc) X(bool, kpp_depth_lazy) X(int, kpp_depth_kr)    \
  X(int, kpp_interior) X(bool, kpp_sparse) X(bool, kpp_side) X(bool, kpp_wuk) X(int, kpp_wuk_margin)                                \
  /* other 3-D switches */                                                                                                          \
  X(int, state3d_levels) X(bool, gm_sf_stored) X(bool, submeso_all_levels)                                                          \
  /* barotropic solver: path 1 per operation, 2 fused, 3 fused with the blocks spread over ranks, 4 replicated fused; the switch   \
     values the per-view rules of launch_solvers.hpp take (persist: 0 off | 1 the rule | 2 | 4 | 8 chunks per workgroup) */        \
  X(int, path) X(bool, fused_ok) X(bool, evp_fused_ok) X(bool, replicated) X(int, evp_wave) X(bool, graph) X(bool, overlap)         \
  X(bool, presum_forced) X(bool, fpcg_b2) X(bool, fpcg_a_pair) X(int, block_sums_relay) X(int, persist)                             \
  /* P-CSI: two cells per thread, two iterations per launch on one rank / with the blocks spread over ranks */                     \
  X(bool, pcsi_two_cell) X(bool, pcsi_two_step) X(bool, pcsi_two_step_dist)                                                         \
  /* halo updates and the RCCL transport */                                                                                         \
  X(bool, halo_separate) X(bool, halo_overlap) X(int, rccl_overlap)
struct Forms {
#define X(type, name) type name = 0;
  POP_FORMS(X)
#undef X
};
// pop_get_dim("form_<name>"): the entry as an int, -1 for a name that is none
inline int forms_get(const Forms &f, const std::string &name) {
#define X(type, member) if (name == #member) return (int)f.member;
  POP_FORMS(X)
#undef X
  return -1;
}

// ---- host facts the rules read
// kref of KPP (vmix_kpp.F90: the level whose bottom reaches the surface layer epssfc * zt(k)), 1-based with slots 0, km + 1, km + 2
constexpr double KPP_EPSSFC = 0.1;
inline std::vector<int> kpp_kref(const HostModel &h) {
  std::vector<int> kref(h.km + 3, 1);
  for (int k = 1; k <= h.km; ++k) {
    const double surfthick = KPP_EPSSFC * h.zt[k];
    kref[k] = k;
    for (int kt = 1; kt <= k; ++kt) if (h.zw[kt] >= surfthick) { kref[k] = kt; break; }
  }
  return kref;
}
// over all ranks: choices between collective code paths must not depend on the rank
inline int max_blocks_per_rank(const HostModel &h) {
  std::vector<int> per(h.nranks, 0);
  for (int o : h.block_owner) if (o >= 0 && o < h.nranks) per[o]++;
  return per.empty() ? 0 : *std::max_element(per.begin(), per.end());
}
// source map of the fused solver path on the rank's own blocks: ghost cell -> local source cell, -1 = fill value
inline std::vector<int> local_srcmap(const HostModel &h) {
  std::vector<int> sm(h.n2 * h.nblocks);
  for (size_t p = 0; p < sm.size(); ++p) sm[p] = (int)p;
  for (size_t i = 0; i < h.halo.copy_dst.size(); ++i) sm[h.halo.copy_dst[i]] = h.halo.copy_src[i];
  for (int d : h.halo.fill_dst) sm[d] = -1;
  if (h.c.ns_boundary == 2) {   // centre scalars beyond the fold are plain mirrored copies of physical cells (TripolePlan loc 0: no symmetrised row)
    const TripolePlan &T = h.halo.tripole[0];
    for (size_t e = 0; e < T.dst.size(); ++e) sm[T.dst[e]] = T.a[e];
  }
  return sm;
}
// two P-CSI iterations per launch with a tripole fold: the ghost cells beyond the fold are formed as mirror images of their source cells, which
// must be cells of this rank (true of any decomposition into bands of whole rows, and of one rank).  jfold: per local block, the first array
// row beyond the fold (nyb: none)
inline bool pcsi_fold_local(const HostModel &h, const std::vector<int> &srcmap, std::vector<int> &jfold) {
  bool local = true;
  jfold.assign(h.nblocks, h.nyb);
  if (h.c.ns_boundary != 2) return true;
  for (int lb = 0; lb < h.nblocks; ++lb) {
    const BlockInfo &B = h.all_blocks[h.local_ids[lb] - 1];
    if (!(B.j_glob[B.je] < 0)) continue;
    jfold[lb] = B.je;
    for (int j = B.je; j < h.nyb; ++j) for (int i = 0; i < h.nxb; ++i) {
      const int cell = lb * (int)h.n2 + j * h.nxb + i;
      if (srcmap[cell] == cell) local = false;
    }
  }
  return local;
}
// 256-cell chunks of a block in the full launch of the 2-D reduction / solver kernels (red_band: a multiple of the eight XCDs)
inline int chunks_per_block(long long n2, int red_band) {
  const int nc = (int)((n2 + 255) / 256);
  return red_band ? 8 * ((nc + 7) / 8) : nc;
}
// rules of the solver that depend on the view (the local and the replicated view differ in size): functions of the view that take the
// plan's switch value (launch_solvers.hpp).  The size rule of the large-grid forms: more chunk partials than a consumer workgroup should
// sum -> block sums by a launch of their own; two cells per thread: where the block sums are presummed, the row pitch is even and the
// launch is not tiled
inline bool presum_by_size(long long nchunk, long long nblocks) { return nchunk * nblocks > 2048; }
inline bool two_cell_shape(int nxb, bool presummed) { return presummed && (nxb & 1) == 0; }

// ---- the resolver
// the size rule: below ~2^19 columns on the rank the launch-parallel forms win, above it the kernels are bandwidth-bound
inline bool bandwidth_bound(const HostModel &h) { return (long long)h.n2 * h.nblocks > (1LL << 19); }
// register kernels exist for the level counts of the production grids (the with_value<60, 62> dispatches)
inline bool register_levels(const HostModel &h) { return h.km == 60 || h.km == 62; }

inline int resolve_forms(const HostModel &h, Forms &f, std::string &err) {
  const pop_config &c = h.c;
  const pop_tuning &t = h.tun;
  const bool big = bandwidth_bound(h), reg_km = register_levels(h), evp = use_evp(c), tripole = c.ns_boundary == 2;
  const bool single = h.halo.peers.empty();   // no block of another rank borders this rank's
  auto rule_or = [](int v, bool rule) { return (tun_set(v) && v >= 0) ? v != 0 : rule; };   // 0 | 1 overrides the rule
  // the switches whose other values named kernel forms that no longer exist
  if (tun_set(t.xcd_remap) && t.xcd_remap != 0 && t.xcd_remap != 1) { err = "pop_create: pop_tuning.xcd_remap is " + std::to_string(t.xcd_remap) + ": 0 linear or 1 XCD bands"; return 1; }
  if (tun_set(t.evp_wave) && t.evp_wave != 0 && t.evp_wave != 3) { err = "pop_create: pop_tuning.evp_wave is " + std::to_string(t.evp_wave) + ": 0 one thread per sub-block or 3 wavefronts"; return 1; }

  // ---- workgroup orders.  Measured on MI355X: the XCD-banded order cuts fabric re-fetch of the stencil kernels from 3.2x to 1.3x of the
  // algorithmic reads at gx1v7 (-6% time) but costs +20% at tx0.1v3, where the 256 MB infinity cache already absorbs the re-fetch
  // (row-aligned 2-D tile columns, tried for both the column and the reduction kernels, lost 128-B alignment of the rows and cost +10% /
  // +2% there).  Large grids therefore keep the natural linear order; either order stays selectable and tested.
  f.xcd_remap = tun_or(t.xcd_remap, big ? 0 : 1);
  // 2-D solver / reduction kernels: XCD-banded chunk order (same chunks, same partial order, only the workgroup -> chunk assignment
  // changes, so results are bitwise unchanged): gx1v7 4.31 -> 4.01 ms per step (the 9-point matvec finds its j+-1 rows in the XCD's own
  // L2), tx0.1v3 177.1 -> 175.2
  f.red_band = tun_or(t.red_band, 1);
  f.lds_order = tun_or(t.lds_order, 1);
  f.land_skip = !tun_off(t.land_skip);
  f.land_full_steps = tun_or(t.land_full_steps, 4);

  // ---- right-hand-side kernels
  // momentum: 3x3 stencils staged through LDS (kernels_momentum_lds.hpp): 64x8 tiles measured -11 % (tx0.1v3) / -12 % (gx1v7) against the
  // direct-load kernel
  f.momentum_lds_rows = tun_or(t.momentum_lds, 4);
  // tracers (kernels_tracer_lds.hpp).  Measured against the direct-load kernel: tx0.1v3 15.0 ms -> 12.8 (64x4 tiles) / 13.6 (64x8); gx1v7
  // 0.260 ms -> 0.208 (64x4) / 0.192 (64x8); round 3 (branch-free kernels, two waves per SIMD): 64 x 4 tiles at every size (gx1v7 0.149 vs
  // 0.156 ms, tx0.1v3 7.6 vs 8.0)
  f.tracer_lds_rows = tun_or(t.tracer_lds, 4);
  // Gent-McWilliams: straight-line flux functions, every horizontal face flux formed once (64 x 8 patches computing 63 x 7 cells; 64 x 4
  // measured 2 % of the step slower), and the LDS tracer kernel with the mixing tendency given; 0: the cell-by-cell / generic kernels
  f.gm_lds = !tun_off(t.gm_flux_tile);
  f.kpp_src_full = tun_on(t.kpp_src_full);

  // ---- Thomas kernels.  The register kernel keeps the elimination coefficients of a column in VGPRs instead of writing them to scratch
  // fields and reading them back (the generic corrector moves 46 GB at the L2 for 19 GB of algorithmic traffic).  gx1v7: 0.19 vs 0.30 ms.
  // tx0.1v3: round 1 measured the generic march faster for the predictor (9.9 vs 11.6 ms, whole grid); with land elimination the register
  // form wins for both (same box, A/B twice: corrector 6.3 vs 8.1-8.6 ms, predictor 7.2 vs 7.5-8.1, step -1.2 .. -1.6 ms).  The velocity
  // solve is faster in registers at both sizes.  Partial bottom cells: every form carries the PBC branches; pbc_generic_thomas = 1 keeps
  // the scratch-staged ones (the cross-check of the register instantiations)
  const bool pbc_generic = c.partial_bottom_cells && tun_on(t.pbc_generic_thomas);
  const bool want_u = !tun_on(t.generic_thomas) && !pbc_generic;
  const bool want_t = (tun_set(t.reg_thomas_t) ? t.reg_thomas_t != 0 : !tun_on(t.generic_thomas)) && !pbc_generic;
  f.reg_thomas_u = want_u && reg_km;
  f.reg_thomas_t = want_t && reg_km;
  // both tracers in one thread when they share the diffusivity array (corrector form only: the predictor's three full register columns +
  // its up-front loads spill ~ 900 B per lane)
  f.thomas_pair = f.reg_thomas_t && rule_or(t.thomas_pair, big);
  // two waves per workgroup on small grids, never with partial bottom cells
  f.impvmixu_waves = (!c.partial_bottom_cells && !big) ? 2 : 1;
  // predictor with the forward elimination inside the right-hand-side kernel: centred advection through the LDS kernel, pressure averaging,
  // and the register tracer solve not asked for (whatever the level count)
  f.tracer_fwd = c.tadvect == 1 && c.hmix_tracer != 3 && (f.tracer_lds_rows == 4 || f.tracer_lds_rows == 8) && c.lpressure_avg &&
                 (tun_set(t.tracer_fwd) ? t.tracer_fwd != 0 : !want_t);

  // ---- shared arrays and streams
  // KPP without double diffusion gives both tracer classes the same diffusivity, value for value (vmix_kpp.F90 ri_iwmix: VDC(:,:,k,2) =
  // VDC(:,:,k,1); blmix applies the same shape function to both): one array then serves both, so the KPP kernels write it once and the
  // tracer kernels find the second read in cache
  f.vdc_shared = c.vmix_choice == 3 && !c.ldbl_diff && !tun_off(t.vdc_shared);
  f.side_stream = !tun_off(t.side_stream);
  // del4: the first Laplacians need only the mix-time fields, so they run on the side stream beside the vertical-mixing coefficients (own
  // output buffers instead of the shared scratch); anis: the friction likewise
  f.del4_side = f.side_stream && (c.hmix_tracer == 4 || c.hmix_momentum == 4) && !tun_off(t.del4_side);
  f.aniso_side = f.side_stream && c.hmix_momentum == 3 && !tun_off(t.aniso_side);
  f.mom_side = c.hmix_momentum == 3 ? f.aniso_side : f.del4_side;

  // ---- del4.  Bandwidth-bound grids: 64 x 4 patches (tx0.1v3: -0.5 ms per step); k_kpp_vvc takes the same patches (the row j + 1 of its
  // four-point average is read by the same workgroup; 64 x 2 / 8 / 16 measured: vmix 7.54 / 7.65 / 7.97 ms against 7.57)
  f.del4_tile_rows = big ? 4 : 0;
  if (tun_set(t.del4_tile)) f.del4_tile_rows = (t.del4_tile == 2 || t.del4_tile == 4 || t.del4_tile == 8 || t.del4_tile == 16) ? t.del4_tile : 0;
  // the tracer / momentum kernel of a step also forms the first Laplacian of the next step from the tile it has in LDS: no tripole fold (the
  // ghost ring of the field comes from a halo update, which is the same arithmetic only where ghost cells are plain copies), centred
  // advection through the LDS kernel, bandwidth-bound grids.  d2t_fuse = 0 | 1 overrides the size rule of both; d2u_fuse = 0 switches the
  // momentum one off
  const bool fuse = f.del4_side && !tripole && rule_or(t.d2t_fuse, big);
  f.d2t_fuse = fuse && c.hmix_tracer == 4 && c.tadvect == 1;
  f.d2u_fuse = fuse && c.hmix_momentum == 4 && !tun_off(t.d2u_fuse);

  // ---- velocity mixing schedule.  The barotropic velocity is added to U, V(new) on the side stream while the tracer corrector runs; not
  // beyond a tripole fold (the halo update symmetrises |U| of the degenerate top row there, which does not commute with the sum).
  f.btrop_inline = !f.side_stream || tripole || tun_on(t.btrop_inline);
  // The implicit vertical mixing of U, V is not needed before the step tail: with the register kernel (no shared scratch) it runs on the
  // side stream beside the barotropic solver, whose one-workgroup reduction kernels leave the GPU idle.  Bandwidth-bound grids: held back
  // until the solve has finished and launched then with the barotropic velocity added on the way out (k_impvmixu_reg<., ., true>): the
  // separate k_add_barotropic pass over U, V(new) is gone
  const bool off_stream = f.side_stream && f.reg_thomas_u && !tun_on(t.vmixu_inline);
  f.vmixu = (off_stream && !f.btrop_inline && rule_or(t.vmixu_defer, big)) ? VMIXU_DEFERRED : off_stream ? VMIXU_SIDE : VMIXU_INLINE;

  // ---- barotropic solver
  f.evp_wave = tun_or(t.evp_wave, 3);
  f.graph = !tun_on(t.solver_nograph);
  f.overlap = !tun_on(t.solver_overlap_off);
  f.presum_forced = tun_on(t.solver_presum);
  f.fpcg_b2 = !tun_off(t.fpcg_b2);
  f.fpcg_a_pair = !tun_off(t.fpcg_a_pair);
  f.block_sums_relay = tun_or(t.block_sums_relay, 1);   // 2: wherever it can run (the cross-check on small grids)
  // small views: the iterations as one resident launch wherever the persist plan qualifies (launch_solvers.hpp persist_plan); 2 | 4 | 8 force
  // that many chunks per workgroup (measurement only)
  f.persist = !tun_set(t.pcg_persist) ? 1 : (t.pcg_persist == 0 || t.pcg_persist == 2 || t.pcg_persist == 4 || t.pcg_persist == 8) ? t.pcg_persist : 1;
  const bool unfused = tun_on(t.solver_unfused);
  f.fused_ok = single && h.nblocks <= 8 && !unfused;
  if (evp) {   // P-CSI + EVP: step kernel + sub-block solves, two launches per iteration; pcg / ChronGear + EVP: operation by operation
    f.evp_fused_ok = f.fused_ok && c.solver_choice == 3;
    f.fused_ok = false;
  }
  f.replicated = !single && c.solver_choice == 1 && !evp && h.nblocks_tot <= 8 && (long long)h.n2 * h.nblocks_tot <= (4LL << 20) &&
                 !tun_on(t.solver_distributed);
  const bool spread = h.nranks > 1 && !unfused, few = max_blocks_per_rank(h) <= 16;
  if (c.solver_choice == 2) f.path = (f.fused_ok && !evp) ? 2 : (spread && few && !evp) ? 3 : 1;
  else if (c.solver_choice == 3) f.path = evp ? (f.evp_fused_ok ? 2 : 1) : f.fused_ok ? 2 : spread ? 3 : 1;
  else f.path = evp ? 1 : f.replicated ? 4 : f.fused_ok ? 2 : (spread && few) ? 3 : 1;
  // P-CSI: two cells per thread follows the shape rule of the local view (pcsi_step2 = 0 | 1 stands in for "presummed"); two iterations per
  // launch (k_pcsi_step_x2) where that rule holds, with the diagonal preconditioner, through a fold whose partners are on the rank
  const int nchunk = chunks_per_block((long long)h.n2, f.red_band);
  const bool two_cell_rule = two_cell_shape(h.nxb, presum_by_size(nchunk, h.nblocks));
  f.pcsi_two_cell = tun_set(t.pcsi_step2) ? two_cell_shape(h.nxb, t.pcsi_step2 != 0) : two_cell_rule;
  if (!evp && (tun_set(t.pcsi_two_step) ? t.pcsi_two_step != 0 : two_cell_rule)) {
    std::vector<int> jfold;
    const bool fold_ok = !tripole || pcsi_fold_local(h, local_srcmap(h), jfold);
    f.pcsi_two_step = fold_ok && single;
    f.pcsi_two_step_dist = fold_ok && !single;
  }

  // ---- KPP
  if (c.vmix_choice == 3) {
    // the next step's coefficients on a third stream beside the barotropic solver (VALU-bound work beside bandwidth-bound work):
    // bandwidth-bound grids, and (round 4) small grids whose pcg / P-CSI solve is the one resident launch: that launch keeps at most one
    // workgroup per CU busy waiting on memory for 2 ms, the KPP kernels of the next step fill the rest (gx1v7: 3.26 -> 3.09, 3.36 -> 3.18 ms
    // per step, A/B on one box; P-CSI 1.85 -> 1.81 ms; beside the resident ChronGear the look-ahead costs more than it hides: 3.08 -> 3.34)
    const bool resident_solve = (c.solver_choice == 1 || c.solver_choice == 3) && !evp && f.persist != 0 && h.nranks == 1 && h.nblocks <= 8 &&
                                h.n2 * h.nblocks <= 250u * 8u * 256u;
    f.kpp_ahead = f.side_stream && (tun_set(t.kpp_ahead) ? t.kpp_ahead != 0 : (big || resident_solve));
    // column (register) forms: bandwidth-bound grids only -- below ~2^19 columns the 3-D-parallel forms win on parallelism.  Measured at
    // tx0.1v3: ushear 11.2 -> 2.7 ms; ushear in column form at every size (gx1v7 vmix 0.716 -> 0.692 ms).  Bit 0 ushear column form, bit 1
    // unused, bit 2 buoydiff LDS form, bit 3 buoydiff + interior fused, bit 4 as one column march
    const std::vector<int> kref = kpp_kref(h);
    const int max_kref = *std::max_element(kref.begin(), kref.end());
    f.kpp_col = (max_kref <= 24) ? tun_or(t.kpp_col, big ? 31 : 1) : 0;
    // bit 3: buoydiff and the interior coefficients in ONE level-parallel launch; bit 2: the level-parallel LDS form of buoydiff
    const bool fused_bi = (f.kpp_col & 8) && max_kref <= 20 && h.km <= 64, lds = (f.kpp_col & 4) && max_kref <= 28;
    // the surface-layer buoyancy difference on demand inside the boundary-layer-depth march (k_kpp_bldepth<true, .>), with the level-parallel
    // fused kernel and with the plain 3-D buoydiff kernel; the LDS buoydiff form keeps the full field
    f.kpp_lazy = (fused_bi || !lds) && max_kref <= 28 && !c.lcheckekmo && c.kpp_ml_diagnostics != 1 && !tun_off(t.kpp_lazy);
    f.kpp_lazy20 = f.kpp_lazy && max_kref <= 20;
    // bit 4: buoydiff + interior coefficients as one column march (one smoothing pass, no double diffusion)
    f.kpp_march = f.kpp_lazy && fused_bi && (f.kpp_col & 16) && c.num_v_smooth_Ri == 1 && !c.ldbl_diff && h.km >= 3;
    // partial bottom cells: the PBC instantiations of the production (column-march) selection where it applies (r3), else the 3-D-parallel /
    // scratch-staged forms, which carry the PBC branches: every level of the surface-layer buoyancy difference and of the shear formed (no
    // on-demand march), one stream, no sparse mask
    f.kpp_pbc_generic = c.partial_bottom_cells && !(f.kpp_march && f.kpp_lazy20 && (f.kpp_col & 1) && !tun_on(t.pbc_generic_kpp));
    const bool gen = f.kpp_pbc_generic;
    f.kpp_shear_col = !gen && (f.kpp_col & 1);
    f.kpp_buoy = gen ? KPP_BUOY_PLAIN : f.kpp_march ? KPP_BUOY_MARCH : fused_bi ? KPP_BUOY_FUSED_LDS : lds ? KPP_BUOY_LDS : KPP_BUOY_PLAIN;
    f.kpp_buoy_kr = max_kref <= 20 ? 20 : 28;
    f.kpp_buoy_sfc = gen || !f.kpp_lazy;
    f.kpp_depth_lazy = !gen && f.kpp_lazy;
    f.kpp_depth_kr = (f.kpp_depth_lazy && !f.kpp_lazy20) ? 28 : 20;
    f.kpp_interior = gen ? KPP_INTERIOR_GENERIC : fused_bi ? KPP_INTERIOR_FUSED : (!tun_on(t.kpp_interior_generic) && reg_km) ? KPP_INTERIOR_REG : KPP_INTERIOR_GENERIC;
    f.kpp_sparse = !gen && f.kpp_march && h.km <= 64 && !tun_off(t.kpp_sparse);
    // the shear of the velocity against its surface-layer reference needs only U and V: on KPP's own side stream it overlaps the (VALU-bound)
    // buoydiff and the interior kernel; bldepth waits for it
    f.kpp_side = !tun_off(t.kpp_side_stream) && !gen;
    // shear kernel limited by the previous evaluation's KBL (k_kpp_ushear_col): only with the on-demand march, which can form a level that is
    // missing itself; the margin: levels beyond the hint
    f.kpp_wuk = f.kpp_depth_lazy && (f.kpp_col & 1) && !tun_off(t.kpp_ushear_hint);
    f.kpp_wuk_margin = tun_or(t.kpp_ushear_margin, 3);
  }

  // ---- other 3-D switches
  f.state3d_levels = tun_or(t.state3d_levels, 4);
  f.gm_sf_stored = !tun_off(t.gm_sf_stored);
  f.submeso_all_levels = tun_on(t.submeso_all_levels);

  // ---- halo updates: one message per neighbour for several fields; the mid-step tracer halo beside interior tiles; the second communicator
  // for exchanges on the side stream (0 none, 1 own stream with several ranks, 2 on a single rank too: the set-up against the real librccl)
  f.halo_separate = tun_on(t.halo_separate);
  f.halo_overlap = !tun_on(t.halo_overlap_off);
  f.rccl_overlap = tun_or(t.rccl_overlap, 1);
  return 0;
}

}  // namespace pop
