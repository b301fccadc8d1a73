// pop_amd.hip -- launch orchestration (the step_mod.F90 call sequence) and the C ABI of
// libpop_amd.so.  gfx950 only.  See include/pop_amd.h for the boundary and DESIGN.md for the
// kernel list.  The product path has no CPU fallback: every compute entry point fails loudly
// when the context was created host-only or no HIP device is usable.  The context is declared in
// pop_ctx.hpp; pop_create_tuned fills it through the steps of create_device.hpp, and pop_destroy
// releases what the context's ownership lists hold.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <unordered_map>
#include "kernels_baroclinic.hpp"
#include "kernels_barotropic.hpp"
#include "kernels_mix.hpp"
#include "kernels_thomas_reg.hpp"
#include "kernels_momentum_lds.hpp"
#include "kernels_aniso.hpp"
#include "kernels_submeso.hpp"
#include "kernels_tracer_lds.hpp"
#include "kernels_rf.hpp"
#include "kernels_pcsi.hpp"
#include "kernels_evp.hpp"
#include "kernels_lwlim.hpp"
#include "kernels_gm.hpp"
#include "kernels_passive.hpp"
#include "kernels_ice.hpp"
#include "kernels_pcg_persist.hpp"
#include "kernels_tavg.hpp"
#include "kernels_diag.hpp"
#include "kernels_moc.hpp"
#include "kernels_transport.hpp"
#include "kernels_forcing.hpp"
#include "rccl_transport.hpp"

using namespace pop;

#include "pop_ctx.hpp"
#include "launch_halo.hpp"
#include "launch_solvers.hpp"
#include "launch_moc.hpp"
#include "launch_transport.hpp"
#include "launch_tavg.hpp"
#include "launch_diag.hpp"
#include "launch_forcing.hpp"
#include "create_device.hpp"

namespace {

int need_device(pop_ctx *c) {
  if (!c) return 1;
  if (c->host_only) { c->err = "context was created host-only: no GPU path available (there is no CPU fallback)"; return 1; }
  return 0;
}

// time level of the ABI (0 old, 1 cur, 2 new) -> index of the rotating arrays
int time_index(const pop_ctx *c, int tl) { return tl == 0 ? c->oldt : tl == 1 ? c->curt : c->newt; }
// resolve a named field: device pointer, element count (local), whether tl / n apply
int resolve(pop_ctx *c, const std::string &name, int tl, int n, double **ptr, long long *count) {
  const long long a2 = (long long)c->g.n2 * c->g.nblocks, a3 = (long long)c->g.n3 * c->g.nblocks;
  const int t = time_index(c, tl);
  auto ok = [&](double *p, long long cnt) { *ptr = p; *count = cnt; return p ? 0 : 1; };
  if (name == "TRACER") return (n >= 0 && n < c->h.nt) ? ok(c->TR[n][t], a3) : 1;
  if (name == "UVEL") return ok(c->U[t], a3);
  if (name == "VVEL") return ok(c->V[t], a3);
  if (name == "RHO") return ok(c->RHO[t], a3);
  if (name == "PSURF") return ok(c->PS[t], a2);
  if (name == "GRADPX") return ok(c->GX[t], a2);
  if (name == "GRADPY") return ok(c->GY[t], a2);
  if (name == "UBTROP") return ok(c->UB[t], a2);
  if (name == "VBTROP") return ok(c->VB[t], a2);
  if (name == "PGUESS") return ok(c->PGUESS, a2);
  if (name == "FW") return ok(c->FW, a2);
  if (name == "FW_OLD") return ok(c->FW_OLD, a2);
  if (name == "SHF_QSW") return ok(c->SHF_QSW, a2);
  if (name == "CHL") return ok(c->CHL, a2);                   // chlorophyll, mg/m^3 (sw_absorption_type 'chlorophyll')
  if (name == "STF") return (n >= 0 && n < c->h.nt) ? ok(c->STF[n], a2) : 1;
  if (name == "TFW") return (n >= 0 && n < c->h.nt) ? ok(c->TFW[n], a2) : 1;
  if (name == "KPP_SRC") return (n >= 0 && n < c->h.nt) ? ok(c->KPP_SRC[n], a3) : 1;
  if (name == "VDC") return (n == 0 || n == 1) ? ok(c->VDC[n], (long long)c->g.n2 * (c->g.km + 2) * c->g.nblocks) : 1;
  if (name == "VVC") return ok(c->VVC, a3);
  if (name == "DH") return ok(c->DH, a2);
  if (name == "DHU") return ok(c->DHU, a2);
  if (name == "ZX") return ok(c->ZX, a2);
  if (name == "ZY") return ok(c->ZY, a2);
  if (name == "UH") return ok(c->UH, a2);
  if (name == "VH") return ok(c->VH, a2);
  if (name == "RHS") return ok(c->RHS, a2);
  if (name == "centerWgt") return ok(c->centerWgt, a2);
  if (name == "HBLT") return ok(c->HBLT, a2);
  if (name == "HMXL") return ok(c->HMXL, a2);
  if (name == "HMXL_DR") return ok(c->HMXL_DR, a2);
  if (name == "UISOP") return ok(c->gm.UISOP, a3);           // diag_gm_bolus (hmix_tracer = 3): eddy-induced velocity, east / north face and top of the T cell
  if (name == "VISOP") return ok(c->gm.VISOP, a3);
  if (name == "WISOP") return ok(c->gm.WISOP, a3);
  // work fields of Gent-McWilliams mixing, for the pins of tests/pins.py: the merged stream function of the half cells (stored in the branch
  // without cancellation: n = 2 face + half, face 0 east / north, half 0 top) and the transition layer's depths
  if (name == "GM_SF_SLX") return (n >= 0 && n < 4) ? ok(c->gm.SF[n], a3) : 1;
  if (name == "GM_SF_SLY") return (n >= 0 && n < 4) ? ok(c->gm.SF[4 + n], a3) : 1;
  if (name == "KAPPA_ISOP") return (n == 0 || n == 1) ? ok(c->gm.KI[n], a3) : 1;   // the tapered isopycnal diffusivity of the top / bottom half (cfl_hdiff of hdifft_gm reads it)
  if (name == "TLT_DIABATIC_DEPTH") return ok(c->gm.DD, a2);
  if (name == "TLT_THICKNESS") return ok(c->gm.TH, a2);
  if (name == "TLT_INTERIOR_DEPTH") return ok(c->gm.ID, a2);
  // lsubmesoscale_mixing: the mixed-layer depth and length scale of submeso_sf; with submeso_diag the tendency on its own and the velocities
  if (name == "SUBM_ML_DEPTH") return ok(c->subm.ML, a2);
  if (name == "HLS_SUBM") return ok(c->subm.HLS, a2);
  if (name == "SUBM_BX") return (n == 0 || n == 1) ? ok(c->subm.B[n], a2) : 1;
  if (name == "SUBM_BY") return (n == 0 || n == 1) ? ok(c->subm.B[2 + n], a2) : 1;
  if (name == "SUBM_ADV_TEND") return (n == 0 || n == 1) ? ok(c->subm.TD[n], a3) : (n >= 2 && n < c->h.nt) ? ok(c->PTD[n], a3) : 1;
  if (name == "USUBM") return ok(c->subm.US, a3);
  if (name == "VSUBM") return ok(c->subm.VS, a3);
  if (name == "WSUBM") return ok(c->subm.WS, a3);
  // pop_transport_request: the per-column terms of the last accumulated step, by tracer index (kernels_transport.hpp TrnCol)
  if (name.compare(0, 4, "TRN_") == 0) {
    const char *const col[TRN_NCOL] = {"TRN_ADV", "TRN_HDIF", "TRN_VNF", "TRN_ADV_ISOP", "TRN_VNF_ISOP", "TRN_ADV_SUBM", "TRN_VNF_SUBM"};
    for (int f = 0; f < TRN_NCOL; ++f) if (name == col[f]) return (n == 0 || n == 1) ? ok(c->trn.COL[n][f], a2) : 1;
  }
  if (c->tidal.on && c->mix.kpp) {   // tidal_diag: the last evaluation's TIDAL_DIFF, TIDAL_N2, KVMIX, KVMIX_M
    const TidalDev &td = ((const KppHost *)c->mix.kpp)->tidal;
    if (name == "TIDAL_DIFF") return ok(td.DIFF, a3);
    if (name == "TIDAL_N2") return ok(td.N2, a3);
    if (name == "KVMIX") return ok(td.KV, a3);
    if (name == "KVMIX_M") return ok(td.KVM, a3);
  }
  if (name == "GM_GTK") return (n == 0 || n == 1) ? ok(c->gm.GTK[n], a3) : (n >= 2 && n < c->h.nt && c->h.c.hmix_tracer == 3) ? ok(c->PW[n], a3) : 1;   // the mixing tendency the tracer right-hand side reads (hmix_tracer = 3)
  if (name == "HDU") return ok(c->HDU, a3);                   // hmix_momentum = 3: Hdiff(U), Hdiff(V) of hdiffu_aniso at every level
  if (name == "HDV") return ok(c->HDV, a3);
  if (name == "F_PARA") return ok(c->FPARA, a3);              // ... with lvariable_hmix_aniso
  if (name == "F_PERP") return ok(c->FPERP, a3);
  if (name == "QICE") return ok(c->ice.QICE, a2);             // pop_init_ice: this call's and the accumulated heat debt, the coupler's flux, the fresh-water flux
  if (name == "AQICE") return ok(c->ice.AQICE, a2);
  if (name == "QFLUX") return ok(c->ice.QFLUX, a2);
  if (name == "FW_FREEZE") return ok(c->ice.FWF, a2);
  if (double *p = cpl_field(c, name, n)) return ok(p, a2);   // pop_init_coupled_forcing: the imported fields and the interval's copies
  if (name == "SMF") return ok(c->d2[n == 0 ? "SMF1" : "SMF2"], a2);
  if (name == "SMFT") return ok(c->d2[n == 0 ? "SMFT1" : "SMFT2"], a2);
  auto it = c->d2.find(name);
  if (it != c->d2.end()) return ok(it->second, a2);
  return 1;
}

// ---- what the entry points do with a named-field argument, stated once
int unknown(pop_ctx *c, const char *what, const char *name) { c->err = std::string(what) + name; return 1; }
int field_arg(pop_ctx *c, const char *name, int tl, int n, double **ptr, long long *count) {
  if (!resolve(c, name, tl, n, ptr, count)) return 0;
  for (const char *f : {"TRACER", "STF", "TFW", "KPP_SRC", "GM_GTK", "SUBM_ADV_TEND"})
    if (!strcmp(name, f) && (n < 0 || n >= c->h.nt)) { c->err = std::string(name) + ": tracer index " + std::to_string(n) + " is outside 0 .. nt-1 = " + std::to_string(c->h.nt - 1); return 1; }
  return unknown(c, "unknown field ", name);
}
int mask_arg(pop_ctx *c, const char *name, double **ptr) {   // optional: no name, no mask
  long long cnt;
  *ptr = nullptr;
  return name && resolve(c, name, 0, 0, ptr, &cnt) ? unknown(c, "unknown mask ", name) : 0;
}
int count_is(pop_ctx *c, long long have, long long want, const char *name) {
  if (have == want) return 0;
  c->err = name ? std::string("count mismatch for ") + name : std::string("count mismatch");
  return 1;
}
// ---- how every pop_init_* opens, stated once: a context, the namelist struct of this library's size (nml = null: the call takes
// none), a context with fields, the first call.  `twice` is the entry point's own wording of the last
int init_arg(pop_ctx *c, const char *fn, const char *nml, size_t want, const int *struct_bytes, bool inited, const char *twice = "called a second time (once per context)") {
  if (!c) return 1;
  const std::string who = std::string(fn) + ": ";
  if (nml && (!struct_bytes || *struct_bytes != (int)want)) { c->err = who + nml + ".struct_bytes is not sizeof(" + nml + ") of this library (" + std::to_string(want) + ")"; return 1; }
  if (c->h.plan_only) { c->err = who + "the context has no fields (POP_CREATE_PLAN_ONLY)"; return 1; }
  if (inited) { c->err = who + twice; return 1; }
  return 0;
}
// ... and closes its checks: nothing has run yet (a restart file that was read counts as a run)
int init_before_steps(pop_ctx *c, const char *fn, const char *hint = "call it right after pop_create") {
  if (!c->ran && c->nsteps_total <= 0) return 0;
  c->err = std::string(fn) + ": a step or a phase has already run (" + hint + ")";
  return 1;
}
template <class V, class T>
int copy_out(pop_ctx *c, const V &v, T *host, long long count, const char *name) {   // a host vector to the caller's array
  if (count_is(c, (long long)v.size(), count, name)) return 1;
  std::copy(v.begin(), v.end(), host);
  return 0;
}
// The caller has written this field (pop_set_field) or may write it (pop_field_device_ptr): ghost cells and the non-local
// source are no longer known to be current, and a new prognostic state may carry other values on land, so the next steps
// run every workgroup again (land elimination).
void mark_written(pop_ctx *c, const char *name, int tl) {
  const std::string nm(name);
  if (nm == "KPP_SRC") { c->kpp_src_user = true; c->src_dirty = true; c->src_dirty_alt = true; }
  if (nm == "TRACER") c->tr_ghosts_ok[time_index(c, tl)] = false;
  if (nm == "UVEL" || nm == "VVEL") c->uv_ghosts_ok[time_index(c, tl)] = false;
  for (const char *f : {"TRACER", "UVEL", "VVEL", "RHO", "PSURF", "GRADPX", "GRADPY", "UBTROP", "VBTROP", "PGUESS", "FW_OLD"})
    if (nm == f) c->full_left = c->f.land_full_steps;
}
// guards of the host-array halo updates
int loc_kind_ok(pop_ctx *c, int loc, int kind, const char *text) {
  if (loc >= 0 && loc <= 3 && kind >= 0 && kind <= 2) return 0;
  c->err = text;
  return 1;
}
int single_rank_only(pop_ctx *c) {
  if (c->h.nranks == 1) return 0;
  c->err = "host halo update needs all blocks on one rank";
  return 1;
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

int pop_create(const pop_config *cfg, int rank, int nranks, int flags, pop_ctx **out) { return pop_create_tuned(cfg, nullptr, nullptr, rank, nranks, flags, out); }
int pop_create_with_grid(const pop_config *cfg, const pop_grid_input *grid, int rank, int nranks, int flags, pop_ctx **out) {
  return pop_create_tuned(cfg, grid, nullptr, rank, nranks, flags, out);
}

// ---- tuning switches (include/pop_amd.h pop_tuning): one table of (field, environment variable).  What is merged here is the REQUEST;
// forms.hpp resolve_forms turns it into the plan (pop_ctx::f), once, in pop_create_tuned
#define POP_TUNING_FIELDS(X)                                                                                                            \
  X(land_skip, "POP_LAND_SKIP") X(land_full_steps, "POP_LAND_FULL_STEPS") X(xcd_remap, "POP_XCD_REMAP")   \
  X(red_band, "POP_RED_BAND") X(lds_order, "POP_LDS_ORDER") X(momentum_lds, "POP_MOMENTUM_LDS") X(tracer_lds, "POP_TRACER_LDS")         \
  X(generic_thomas, "POP_GENERIC_THOMAS") X(reg_thomas_t, "POP_REG_THOMAS_T") X(thomas_pair, "POP_THOMAS_PAIR")                         \
  X(tracer_fwd, "POP_TRACER_FWD") X(vdc_shared, "POP_VDC_SHARED") X(side_stream, "POP_SIDE_STREAM") X(del4_side, "POP_DEL4_SIDE")       \
  X(del4_tile, "POP_DEL4_TILE") X(d2t_fuse, "POP_D2T_FUSE") X(d2u_fuse, "POP_D2U_FUSE") X(vmixu_defer, "POP_VMIXU_DEFER")               \
  X(vmixu_inline, "POP_VMIXU_INLINE") X(btrop_inline, "POP_BTROP_INLINE") X(kpp_ahead, "POP_KPP_AHEAD") X(kpp_col, "POP_KPP_COL")       \
  X(kpp_lazy, "POP_KPP_LAZY") X(kpp_ushear_hint, "POP_KPP_USHEAR_HINT") X(kpp_ushear_margin, "POP_KPP_USHEAR_MARGIN")                   \
  X(kpp_side_stream, "POP_KPP_SIDE_STREAM") X(kpp_interior_generic, "POP_KPP_INTERIOR_GENERIC") \
  X(kpp_src_full, "POP_KPP_SRC_FULL") X(solver_unfused, "POP_SOLVER_UNFUSED") X(solver_nograph, "POP_SOLVER_NOGRAPH")                   \
  X(solver_presum, "POP_SOLVER_PRESUM") X(solver_distributed, "POP_SOLVER_DISTRIBUTED") X(solver_overlap_off, "POP_SOLVER_OVERLAP_OFF") \
  X(fpcg_b2, "POP_FPCG_B2") X(pcsi_step2, "POP_PCSI_STEP2") X(halo_separate, "POP_HALO_SEPARATE")                                       \
  X(halo_overlap_off, "POP_HALO_OVERLAP_OFF") X(rccl_overlap, "POP_RCCL_OVERLAP") X(evp_wave, "POP_EVP_WAVE") X(fpcg_a_pair, "POP_FPCG_A_PAIR") X(kpp_sparse, "POP_KPP_SPARSE") X(pbc_generic_thomas, "POP_PBC_GENERIC_THOMAS") X(pbc_generic_kpp, "POP_PBC_GENERIC_KPP") X(state3d_levels, "POP_STATE3D_LEVELS") X(gm_sf_stored, "POP_GM_SF_STORED") X(pcg_persist, "POP_PCG_PERSIST") X(gm_flux_tile, "POP_GM_FLUX_TILE") X(pcsi_two_step, "POP_PCSI_TWO_STEP") X(block_sums_relay, "POP_BLOCK_SUMS_RELAY") X(aniso_side, "POP_ANISO_SIDE") X(submeso_all_levels, "POP_SUBMESO_ALL_LEVELS")
void pop_tuning_init(pop_tuning *t) {
  if (!t) return;
  t->struct_bytes = (int)sizeof(pop_tuning);
#define X(f, e) t->f = POP_TUNING_UNSET;
  POP_TUNING_FIELDS(X)
#undef X
}
// caller's struct, then the environment (a variable that is set but not a number counts as 1, as the older on/off switches did)
static void tuning_resolve(pop_tuning &t, const pop_tuning *user) {
  pop_tuning_init(&t);
  if (user && user->struct_bytes == (int)sizeof(pop_tuning)) t = *user;
  auto env = [](const char *name, int &v) {
    const char *e = getenv(name);
    if (!e) return;
    char *end = nullptr;
    const long x = strtol(e, &end, 10);
    v = (end == e) ? 1 : (int)x;
  };
#define X(f, e) env(e, t.f);
  POP_TUNING_FIELDS(X)
#undef X
}
int pop_get_tuning(const pop_ctx *c, pop_tuning *resolved) {
  if (!c || !resolved) return 1;
  *resolved = c->h.tun;
  return 0;
}

// the reference's direct-access binary grid files (grid.F90:1362-1380, :2066-2085): whole records, native byte order
int pop_read_grid_files(const char *horiz_grid_file, const char *topography_file, int nx_global, int ny_global, double *seven_records, int *kmt) {
  const size_t n = (size_t)nx_global * ny_global;
  auto slurp = [&](const char *path, void *dst, size_t bytes) {
    FILE *f = fopen(path, "rb");
    if (!f) return 1;
    const size_t got = fread(dst, 1, bytes, f);
    fclose(f);
    return got == bytes ? 0 : 1;
  };
  if (horiz_grid_file && seven_records && slurp(horiz_grid_file, seven_records, 7 * n * sizeof(double))) return 1;
  if (topography_file && kmt && slurp(topography_file, kmt, n * sizeof(int))) return 2;
  return 0;
}

// The host model first (configuration, blocks, grid, halo plan: host_setup.cpp), then the plan (forms.hpp), then the device half as
// the steps of create_device.hpp in their order
int pop_create_tuned(const pop_config *cfg_in, const pop_grid_input *grid, const pop_tuning *tuning, int rank, int nranks, int flags, pop_ctx **out) {
  if (!cfg_in || !out || nranks < 1 || rank < 0 || rank >= nranks) return 1;
  pop_ctx *c = new pop_ctx();
  *out = c;
  c->h.rank = rank; c->h.nranks = nranks;
  if (tuning && tuning->struct_bytes != (int)sizeof(pop_tuning)) { c->err = "pop_create_tuned: pop_tuning.struct_bytes does not match this library (use pop_tuning_init)"; return 1; }
  tuning_resolve(c->h.tun, tuning);
  c->grid_from_input = grid != nullptr;
  if (grid && !(grid->ULAT && grid->ULON && grid->HTN && grid->HTE && grid->HUS && grid->HUW)) { c->err = "pop_create_with_grid: ULAT, ULON, HTN, HTE, HUS, HUW are required"; return 1; }
  if (config_read_check(cfg_in, grid, c->h.c, c->err)) return 1;
  c->h.gin = grid;
  c->h.plan_only = (flags & POP_CREATE_PLAN_ONLY) != 0;
  const int hb = host_build(c->h);
  c->h.gin = nullptr;
  if (hb) { c->err = c->h.err; return 1; }
  c->host_only = (flags & (POP_CREATE_HOST_ONLY | POP_CREATE_PLAN_ONLY)) != 0;
  // the plan: every kernel-form and schedule choice, once (a plan-only context has no vertical grid and no plan)
  if (!c->h.plan_only && resolve_forms(c->h, c->f, c->err)) return 1;
  if (c->host_only) return 0;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { c->err = "no HIP device available; libpop_amd has no CPU fallback"; return 1; }
  HIPCHK(c, hipStreamCreate(&c->stream));
  c->own_stream = true;
  return create_grid_device(c) || create_land_lists(c) || create_hmix_advect(c) || create_gm(c) || create_submeso(c) || create_state_fields(c) ||
         create_solver_lists(c) || create_halo_device(c) || create_solver_device(c) || create_mix_and_ahead(c) || create_initial_state(c);
}

// Everything the context owns is in its four lists (pop_ctx.hpp); KPP keeps its own stream and events (kpp_destroy)
int pop_destroy(pop_ctx *c) {
  if (!c) return 0;
  // copies into pinned buffers (an armed step's diagnostics, an import's upload) and exchanges may still be in flight
  if (c->stream) hipStreamSynchronize(c->stream);
  for (hipStream_t s : c->streams) hipStreamSynchronize(s);
  for (auto &g : c->graphs) hipGraphExecDestroy(g.exec);
  for (void *p : c->pinned) hipHostFree(p);
  for (hipEvent_t e : c->events) hipEventDestroy(e);
  if (c->rccl_tr) {
    if (c->rccl_tr->comm2) rccl().CommDestroy(c->rccl_tr->comm2);
    if (c->rccl_tr->comm) rccl().CommDestroy(c->rccl_tr->comm);
    delete c->rccl_tr;
  }
  for (hipStream_t s : c->streams) hipStreamDestroy(s);
  kpp_destroy(c->mix);
  for (void *p : c->allocs) hipFree(p);
  if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
  delete c;
  return 0;
}
const char *pop_last_error(const pop_ctx *c) { return c ? c->err.c_str() : "null context"; }

int pop_get_dim(const pop_ctx *c, const char *name) {
  const std::string n(name);
  if (n == "nx_block") return c->h.nxb;
  if (n == "ny_block") return c->h.nyb;
  if (n == "km") return c->h.km;
  if (n == "nt") return c->h.nt;
  if (n == "nblocks") return c->h.nblocks;
  if (n == "nblocks_tot") return c->h.nblocks_tot;
  if (n == "cpl_nsteps_per_interval") return c->cpl.inited ? c->cpl.nml.nsteps_per_interval : 0;   // pop_init_coupled_forcing: the length of qsw_12hr_factor
  if (n == "nblocks_x") return c->h.nbx;
  if (n == "nblocks_y") return c->h.nby;
  if (n == "nghost") return NGHOST;
  if (n == "oldtime") return c->oldt;
  if (n == "curtime") return c->curt;
  if (n == "newtime") return c->newt;
  if (n == "leapfrogts") return c->leapfrogts;
  if (n == "land_skip_active") return c->g.skip;
  if (n == "kpp_ahead_used") return c->ahead_swaps;   // steps whose KPP coefficients were those of the look-ahead (phase_vmix)
  if (n == "d2t_fused") return c->f.d2t_fuse;   // the tracer / momentum kernels also form the next step's del4 first Laplacian
  if (n == "d2u_fused") return c->f.d2u_fuse;
  if (n == "d2t_last_formed") return c->d2t_last_formed;   // ... and whether the last such launch did (not on averaging steps)
  if (n == "d2u_last_formed") return c->d2u_last_formed;
  if (n == "avg_ts") return c->avg_ts;
  if (n == "eod") return c->eod;             // time_management.F90: the step just taken ended a day / the one before it did
  if (n == "eod_last") return c->eod_last;
  if (n == "nsteps_total") return c->nsteps_total;
  if (n == "nsteps_per_interval") return c->h.nsteps_per_interval;
  if (n == "solver_stream_ops") return (int)c->solver_ops;
  if (n == "solver_iterations_enqueued") return (int)c->solver_enq;
  if (n == "rank") return c->h.rank;
  if (n == "nranks") return c->h.nranks;
  if (n == "solver_chunks_per_block") return c->nchunk;                 // 256-cell chunks of a block (the full launch of the fused solver kernels)
  if (n == "solver_chunks_listed") return c->red_act ? c->red_nact : -1;  // compacted launch: workgroups per block (-1: no list, every chunk is launched)
  if (n == "solver_chunks_active") return c->red_active_total;          // chunks with an ocean cell (or work for another rank), all local blocks
  if (n == "pcg_persist_used") return c->persist_used;
  if (n == "pcg_persist_gave_up") return c->persist_gave_up;
  if (n == "pcsi_two_step") return (c->f.pcsi_two_step || c->f.pcsi_two_step_dist) ? 1 : 0;   // P-CSI: two iterations per launch (k_pcsi_step_x2) in use
  if (n == "pcg_persist_workgroups") return c->persist_nwg;
  if (n == "pcg_persist_chunks_per_workgroup") return c->persist_cp;
  if (n == "solver_path") return c->h.plan_only ? 0 : c->f.path;   // 1 per operation, 2 fused, 3 fused distributed, 4 replicated fused
  if (n == "thomas_register_tracers") return c->f.reg_thomas_t;    // column-in-registers Thomas kernels in use
  if (n == "thomas_register_velocity") return c->f.reg_thomas_u;
  if (n == "max_blocks_per_rank") return max_blocks_per_rank(c->h);
  if (n == "ocean_columns_local") return (int)c->h.ocean_cols_local;     // POP_CREATE_PLAN_ONLY contexts (-1 otherwise)
  if (n == "ocean_columns_total") return (int)c->h.ocean_cols_total;
  if (n == "lat_aux_region_start") return (c->moc.aux.inited && c->moc.aux.n_reg > 1) ? c->moc.aux.region_start[1] : 0;   // pop_init_transports
  if (n == "moc_stream") return c->moc.requested ? c->moc.stream : 0;
  if (n == "transport_stream") return c->trn.requested ? c->trn.stream : 0;
  if (n == "n_transport_comp") return c->moc.aux.inited ? trn_n_comp(c->h.c) : 0;   // pop_init_transports
  if (n.compare(0, 5, "form_") == 0 && !c->h.plan_only) return forms_get(c->f, n.substr(5));   // any entry of the plan (forms.hpp)
  return -1;
}
double pop_get_scalar(const pop_ctx *c, const char *name) {
  const std::string n(name);
  if (n == "dtt") return c->h.dtt;
  if (n == "dtu") return c->h.dtu;
  if (n == "dtp") return c->h.dtp;
  if (n == "residualNorm") return c->h.residualNorm;
  if (n == "convergenceCriterion") return c->h.convergenceCriterion;
  if (n == "rcheck") return c->h.rcheck;
  if (n == "rconst") return c->h.rconst;
  if (n == "uarea_equator") return c->h.uarea_equator;
  if (n == "rmsResidual") return c->rmsResidual;
  if (n == "land_tile_fraction") return c->land_fraction;     // 64-column row segments without an ocean cell nearby (land elimination)
  if (n == "PcsiMaxEigs") return c->h.pcsi_max_eig;
  if (n == "PcsiMinEigs") return c->h.pcsi_min_eig;
  if (n == "lanczos_steps") return (double)c->h.pcsi_lanczos_steps;
  if (n == "robert_curtime") return c->h.robert_curtime;
  if (n == "robert_newtime") return c->h.robert_newtime;
  if (n == "rf_volume_2_km") return c->h.rf_volume_2_km;
  if (n == "open_ocean_volume_2_km") return c->h.open_ocean_volume_2_km;
  if (n == "bgtarea_t_1") return c->h.bgtarea_t_1;
  if (n == "persist_iterations") return c->persist_out ? c->persist_out[0] : NAN;   // what the last resident pcg launch reported (kernels_pcg_persist.hpp)
  if (n == "persist_rr") return c->persist_out ? c->persist_out[1] : NAN;
  if (n == "persist_status") return c->persist_out ? c->persist_out[2] : NAN;
  if (n == "persist_checks") return c->persist_out ? c->persist_out[3] : NAN;
  if (n == "tlast_ice") return c->ice.inited ? c->ice.tlast_ice : NAN;               // pop_init_ice: time since the coupler last took QFLUX
  if (n == "time_weight") return ice_time_weight(c);
  if (n == "cp_over_lhfusion") return c->ice.inited ? c->ice.k.cp_over_lhfusion : NAN;
  if (n == "rf_S1") return c->rf_S[0];
  if (n == "rf_S2") return c->rf_S[1];
  if (n == "rf_S_prev1") return c->rf_S_prev_valid[0] ? c->rf_S_prev[0] : NAN;   // NAN: not valid (no filtered step yet, or a restart file without it)
  if (n == "rf_S_prev2") return c->rf_S_prev_valid[1] ? c->rf_S_prev[1] : NAN;
  // HIP-event time of the barotropic solves (POP_SolversRun) since "solver_ms_reset", the iterations they took and their number
  if (n == "solver_ms_total") { solve_collect(const_cast<pop_ctx *>(c)); return c->solver_ms_total; }
  if (n == "solver_iterations_total") { solve_collect(const_cast<pop_ctx *>(c)); return (double)c->solver_iters_total; }
  if (n == "solver_calls_total") { solve_collect(const_cast<pop_ctx *>(c)); return (double)c->solver_calls_total; }
  if (n == "solver_ms_reset") { pop_ctx *m = const_cast<pop_ctx *>(c); solve_collect(m); m->solver_ms_total = 0; m->solver_iters_total = 0; m->solver_calls_total = 0; return 0.0; }
  return NAN;
}
int pop_get_block(const pop_ctx *c, int block_id, int *out8, int *i_glob, int *j_glob) {
  if (block_id < 1 || block_id > c->h.nblocks_tot) return 1;   // get_block: invalid block_id (blocks.F90:309-311)
  const BlockInfo &B = c->h.all_blocks[block_id - 1];
  if (out8) { int v[8] = {B.block_id, B.local_id, B.ib, B.ie, B.jb, B.je, B.iblock, B.jblock}; std::copy(v, v + 8, out8); }
  if (i_glob) std::copy(B.i_glob.begin(), B.i_glob.end(), i_glob);
  if (j_glob) std::copy(B.j_glob.begin(), B.j_glob.end(), j_glob);
  return 0;
}
int pop_local_block_ids(const pop_ctx *c, int *ids) { std::copy(c->h.local_ids.begin(), c->h.local_ids.end(), ids); return 0; }

long long pop_field_count(const pop_ctx *c, const char *name) {
  const std::string n(name);
  const long long a2 = (long long)c->h.n2 * c->h.nblocks, a3 = (long long)c->h.n3 * c->h.nblocks;
  for (const char *s : {"TRACER", "UVEL", "VVEL", "RHO", "KPP_SRC", "VVC", "UISOP", "VISOP", "WISOP", "GM_SF_SLX", "GM_SF_SLY", "HDU", "HDV", "F_PARA", "F_PERP",
                        "SUBM_ADV_TEND", "USUBM", "VSUBM", "WSUBM", "GM_GTK", "KAPPA_ISOP", "TIDAL_COEF_3D", "TIDAL_DIFF", "TIDAL_N2", "KVMIX", "KVMIX_M"}) if (n == s) return a3;
  if (n == "VDC") return (long long)c->h.n2 * (c->h.km + 2) * c->h.nblocks;
  return a2;
}
// wait for side-stream work whose results the launch stream (or the host) is about to use
// drop a KPP look-ahead in flight: whatever follows on the launch stream is ordered after it, and the next step computes
// its coefficients itself.  Every entry point through which a caller may read or change fields (join_side) does this, so
// only an uninterrupted sequence of pop_step calls uses the look-ahead.
static int ahead_cancel(pop_ctx *c) {
  if (c->ahead_valid) { HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_ahead, 0)); c->ahead_valid = false; }
  c->d2t_next_valid = false;   // same rule for the first Laplacians the tracer / momentum kernels formed for the next step
  c->d2u_next_valid = false;
  return 0;
}
static int phase_impvmixu(pop_ctx *c, hipStream_t st);
static int join_side(pop_ctx *c, bool keep_ahead = false) {
  // implicit vertical mixing of U, V held back for the fused form of baroclinic_correct_adjust: a caller that looks at (or changes)
  // fields in between gets the plain kernel now, and the barotropic velocity is added by its own launch later
  if (c->vmixu_deferred) { c->vmixu_deferred = false; if (phase_impvmixu(c, nullptr)) return 1; }
  if (c->vmixu_pending) { HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_vmixu, 0)); c->vmixu_pending = false; }
  if (!keep_ahead && ahead_cancel(c)) return 1;
  return 0;
}
int pop_get_field(pop_ctx *c, const char *name, int tl, int n, double *host, long long count) {
  const std::string nm(name);
  if (nm == "BCKGRND_VDC" || nm == "BCKGRND_VVC" || (nm == "TLON" && !c->tlon.empty())) {   // init-time fields of pop_init_kpp_bckgrnd (host copies); TLON of either init call
    if (nm != "TLON" && !c->bck.on) { c->err = nm + " exists after pop_init_kpp_bckgrnd with lhoriz_varying_bckgrnd only"; return 1; }
    return copy_out(c, nm == "TLON" ? c->tlon : nm == "BCKGRND_VDC" ? c->bck.f.vdc : c->bck.f.vvc, host, count, name);
  }
  if (nm == "ANGLET" || nm == "COS_ANGLET" || nm == "SIN_ANGLET") {   // grid.F90:660-735 and the rotation's cosine / sine (host copies)
    if (c->h.plan_only) { c->err = nm + ": the context has no fields (POP_CREATE_PLAN_ONLY)"; return 1; }
    cpl_anglet(c);
    return copy_out(c, nm == "ANGLET" ? c->anglet : nm == "COS_ANGLET" ? c->cos_anglet : c->sin_anglet, host, count, name);
  }
  if (nm == "MASK_FRAC" && c->msb.inited) {   // pop_init_ms_balance: by sea (host copy)
    const size_t a2 = c->h.n2 * c->h.nblocks;
    if (n < 0 || n >= (int)c->msb.seas.size()) { c->err = "MASK_FRAC: sea index " + std::to_string(n) + " is outside 0 .. n_marginal_seas - 1"; return 1; }
    return copy_out(c, std::vector<double>(c->msb.mask_frac.begin() + n * a2, c->msb.mask_frac.begin() + (n + 1) * a2), host, count, name);
  }
  if (nm == "TIDAL_ENERGY_FLUX" || nm == "TIDAL_COEF_3D") {   // init-time fields of pop_init_tidal_mixing (host copies)
    if (!c->tidal.on) { c->err = nm + " exists after pop_init_tidal_mixing with ltidal_mixing only"; return 1; }
    return copy_out(c, nm == "TIDAL_COEF_3D" ? c->tidal.f.coef : c->tidal.f.flux, host, count, name);
  }
  if (nm == "TIDAL_DIFF" || nm == "TIDAL_N2" || nm == "KVMIX" || nm == "KVMIX_M") {
    if (!c->tidal.on || !c->tidal.nml.tidal_diag) { c->err = nm + " exists after pop_init_tidal_mixing with ltidal_mixing and tidal_diag only"; return 1; }
    if (need_device(c)) return 1;
  }
  if (c->host_only) {   // host-only contexts expose the init-time 2-D fields of the local blocks (and F_PARA, F_PERP)
    if (nm == "F_PARA" || nm == "F_PERP") {
      const std::vector<double> &all = c->h.aniso_f[nm == "F_PARA" ? 0 : 1];
      if (all.empty()) { c->err = nm + " exists with hmix_momentum = 3 and lvariable_hmix_aniso only"; return 1; }
      return copy_out(c, local_part3(c->h, all), host, count, name);
    }
    std::string key = nm;
    if (nm == "SMF") key = n == 0 ? "SMF1" : "SMF2";
    if (nm == "SMFT") key = n == 0 ? "SMFT1" : "SMFT2";
    auto it = c->h.f2.find(key);
    if (it == c->h.f2.end()) { c->err = "unknown field " + nm; return 1; }
    return copy_out(c, local_part(c->h, it->second), host, count, name);
  }
  double *p; long long cnt;
  if (field_arg(c, name, tl, n, &p, &cnt) || count_is(c, cnt, count, name)) return 1;
  if (join_side(c)) return 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(host, p, cnt * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
int pop_set_field(pop_ctx *c, const char *name, int tl, int n, const double *host, long long count) {
  if (need_device(c)) return 1;
  double *p; long long cnt;
  if (field_arg(c, name, tl, n, &p, &cnt) || count_is(c, cnt, count, name)) return 1;
  if (join_side(c)) return 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(p, host, cnt * sizeof(double), hipMemcpyHostToDevice));
  if ((!strcmp(name, "F_PARA") || !strcmp(name, "F_PERP")) && !c->h.c.lsmag_aniso) {
    // var_viscosity_infile: init_aniso tapers what it read to AMAX_CFL (hmix_aniso.F90:444-464); a min, so writing back what was read changes nothing
    const std::vector<double> amax = local_part(c->h, c->h.f2.at("AMAX_CFL"));
    std::vector<double> f(host, host + cnt);
    for (int lb = 0; lb < c->h.nblocks; ++lb)
      for (int k = 0; k < c->h.km; ++k)
        for (size_t p2 = 0; p2 < c->h.n2; ++p2) {
          double &v = f[(size_t)lb * c->h.n3 + (size_t)k * c->h.n2 + p2];
          const double m = amax[(size_t)lb * c->h.n2 + p2];
          if (v > m) v = m;
        }
    HIPCHK(c, hipMemcpy(p, f.data(), cnt * sizeof(double), hipMemcpyHostToDevice));
  }
  if (!strcmp(name, "CHL") && c->h.sw.CHLI) {   // set_chl (sw_absorption.F90:500-512): the column of the transmission table per cell
    std::vector<int> idx((size_t)cnt);
    for (long long q = 0; q < cnt; ++q) idx[q] = sw_chl_index(c->h.sw, host[q]);
    HIPCHK(c, hipMemcpy(c->h.sw.CHLI, idx.data(), (size_t)cnt * sizeof(int), hipMemcpyHostToDevice));
  }
  mark_written(c, name, tl);
  return 0;
}
int pop_get_ifield(pop_ctx *c, const char *name, int *host, long long count) {
  if (!strcmp(name, "KBL")) {   // KPP: level of the boundary-layer depth that belongs to the current KPP_SRC (device-resident)
    if (need_device(c) || join_side(c)) return 1;
    if (!c->KBL) { c->err = "KBL exists with vmix_choice = 3 only"; return 1; }
    if (count_is(c, count, (long long)c->g.n2 * c->g.nblocks, nullptr)) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(host, c->KBL, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
  }
  if (!strcmp(name, "TIDAL_REGION_BOX2D")) {   // REGION_BOX2D of ltidal_min_regions (0 everywhere without it)
    if (!c->tidal.on) { c->err = "TIDAL_REGION_BOX2D exists after pop_init_tidal_mixing with ltidal_mixing only"; return 1; }
    return copy_out(c, c->tidal.f.box, host, count, nullptr);
  }
  auto it = c->h.i2.find(name);
  if (it == c->h.i2.end()) { c->err = std::string("unknown integer field ") + name; return 1; }
  return copy_out(c, local_part(c->h, it->second), host, count, nullptr);
}
void *pop_field_device_ptr(pop_ctx *c, const char *name, int tl, int n) {
  if (c->host_only) return nullptr;
  join_side(c);               // the caller may read the field on the launch stream
  mark_written(c, name, tl);  // ... or write it
  double *p; long long cnt;
  return resolve(c, name, tl, n, &p, &cnt) ? nullptr : (void *)p;
}

// ---- restart files (restart.F90 write_restart :1095-1715, read_restart :184-1088; 'bin' format of io_binary.F90)
// The files themselves -- header text, records, each rank's place in them -- are host_restart.cpp's (slab_file_write, slab_file_read); here is
// what a field is on the device and what state goes with it.
// device pointer and size of restart field f, checked against what its records hold
static int restart_field_ptr(pop_ctx *c, const RestartField &f, double **p, size_t *bytes) {
  long long n;
  if (resolve(c, f.dev, f.tl, f.n, p, &n) || n != (long long)f.nlev * c->g.n2 * c->g.nblocks) { c->err = "restart: unknown field " + f.dev; return 1; }
  *bytes = (size_t)n * sizeof(double);
  return 0;
}
int pop_write_restart(pop_ctx *c, const char *path) {
  if (need_device(c) || join_side(c)) return 1;
  const HostModel &h = c->h;
  const std::vector<RestartField> fields = restart_fields(h);
  // calendar of a run that starts 0001-01-01 00:00 with 365-day years (time_management.F90 defaults)
  const double secs = (double)c->nsteps_total * h.dtt;
  const long long day = (long long)(secs / 86400.0);
  const int sod = (int)(secs - 86400.0 * (double)day);
  static const int mdays[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
  int doy = (int)(day % 365), month = 1;
  while (doy >= mdays[month - 1]) { doy -= mdays[month - 1]; ++month; }
  std::vector<RestartAttr> at = {
    {"title", "char", "POP restart"}, {"history", "char", "written by libpop_amd"}, {"conventions", "char", "POP binary restart"},
    {"runid", "char", "pop_amd"}, {"iyear", "int", std::to_string(1 + day / 365)}, {"imonth", "int", std::to_string(month)},
    {"iday", "int", std::to_string(doy + 1)}, {"ihour", "int", std::to_string(sod / 3600)}, {"iminute", "int", std::to_string(sod % 3600 / 60)},
    {"isecond", "int", std::to_string(sod % 60)}, {"iyear0", "int", "1"}, {"imonth0", "int", "1"}, {"iday0", "int", "1"},
    {"ihour0", "int", "0"}, {"iminute0", "int", "0"}, {"isecond0", "int", "0"}, {"dtt", "r8", fmt_r8(h.dtt)},
    {"elapsed_days", "int", std::to_string(day)}, {"seconds_this_day", "r8", fmt_r8((double)sod)},
    {"nsteps_total", "int", std::to_string(c->nsteps_total)},
    {"nsteps_this_interval", "int", std::to_string(c->nsteps_this_interval)},   // extension: exact restart inside an averaging interval
    // restart.F90:1313-1314: both flags as they stand after the step that has just finished.  The next time_manager copies eod into
    // eod_last (time_management.F90:1809) before it resets eod (:2110), so the file's eod decides the first step after the restart
    {"eod", "log", c->eod ? "T" : "F"}, {"eod_last", "log", c->eod_last ? "T" : "F"},
    {"lcoupled_ts", "log", "F"},   // restart.F90:1333: never a coupled time step here, so the ice record is AQICE, not QFLUX (:1477-1489)
  };
  if (h.ice) at.push_back({"tlast_ice", "r8", fmt_r8(c->ice.tlast_ice)});   // restart.F90:1332
  if (h.c.tmix_opt == 3)
    for (int n = 0; n < h.nt; ++n) if (c->rf_S_prev_valid[n]) at.push_back({"rf_S_prev_" + restart_tracer_name(h, n), "r8", fmt_r8(c->rf_S_prev[n])});
  HIPCHK(c, hipStreamSynchronize(c->stream));
  auto fetch = [&](size_t i, double *buf) {
    const RestartField &f = fields[i];
    if (f.dev.empty()) return 0;   // FW_FREEZE without pop_init_ice: the zeros the buffer holds
    double *p; size_t bytes;
    if (restart_field_ptr(c, f, &p, &bytes)) return 1;
    if (hipMemcpy(buf, p, bytes, hipMemcpyDeviceToHost) != hipSuccess) { c->err = "restart: device copy failed"; return 1; }
    return 0;
  };
  return slab_file_write(h, path, at, fields, fetch, "restart", c->err);
}

int pop_read_restart(pop_ctx *c, const char *path, int flags) {
  if (need_device(c) || join_side(c)) return 1;
  const HostModel &h = c->h;
  RestartHeader hd;
  if (restart_parse_header(path, hd, c->err)) return 1;
  std::vector<RestartField> fields = restart_fields(h);
  // restart.F90:679-697: a file written at a coupled time step (lcoupled_ts, when CESM writes its restarts) carries QFLUX where the
  // others carry AQICE.  QFLUX is read, masked and halo-updated as AQICE would be (:886-896, 1041-1055); AQICE is what init_ice left: 0
  const bool coupled_ts = h.ice && hd.logical("lcoupled_ts");
  if (coupled_ts)
    for (RestartField &f : fields) if (f.name == "AQICE") { f.name = "QFLUX"; f.dev = "QFLUX"; }
  // Everything the header must give is checked before the first record is read: a header that lacks some of it leaves the context as it was.
  for (RestartField &f : fields) {   // record of each field from the header (define_field_binary :1075-1080), not from our own order
    int ndims;
    if (!hd.find(f.name, RestartHeader::PREFIX, &f.id, &ndims)) {
      if (f.dev.empty()) continue;                                   // FW_FREEZE is not used here
      c->err = "could not find field in binary header file: " + f.name; return 1;
    }
    if (ndims && ndims != f.ndims) { c->err = "restart: wrong rank for " + f.name; return 1; }
  }
  fields.erase(std::remove_if(fields.begin(), fields.end(), [](const RestartField &f) { return f.dev.empty(); }), fields.end());   // ... and not read
  if (!hd.has("nsteps_total")) { c->err = "restart: header has no nsteps_total"; return 1; }
  if (h.ice && !hd.has("tlast_ice")) { c->err = "restart: header has no tlast_ice (the file was written without pop_init_ice)"; return 1; }
  const std::vector<int> KMT = local_part(h, c->h.i2["KMT"]), KMU = local_part(h, c->h.i2["KMU"]);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  auto store = [&](size_t i, double *buf) {
    const RestartField &f = fields[i];
    restart_mask(h, f, buf, KMT, KMU);
    double *p; size_t bytes;
    if (restart_field_ptr(c, f, &p, &bytes)) return 1;
    if (hipMemcpy(p, buf, bytes, hipMemcpyHostToDevice) != hipSuccess) { c->err = "restart: device copy failed"; return 1; }
    const int uv = (f.mask == 1 || f.mask == 3) ? 1 : 0;             // U-grid fields: NE corner, vector (restart.F90:969-1014)
    return halo_update(c, p, f.nlev, 0.0, uv, uv);                   // read_restart :960-1040 (fillValue 0)
  };
  // a failure during the walk (a short file) leaves the fields stored before it in place, as in the reference: there is no rollback
  if (slab_file_read(h, path, fields, (flags & 1) != 0, store, c->err)) return 1;
  c->full_left = c->f.land_full_steps;   // land elimination: the state just read is new
  for (bool &b : c->tr_ghosts_ok) b = false;
  for (bool &b : c->uv_ghosts_ok) b = false;
  // init_ts :1665-1681: density of both time levels from the tracers just read
  launch_state3d(c->g, c->TR[0][c->curt], c->TR[1][c->curt], c->RHO[c->curt], c->stream);
  launch_state3d(c->g, c->TR[0][c->oldt], c->TR[1][c->oldt], c->RHO[c->oldt], c->stream);
  HIPCHK(c, hipGetLastError());
  // scalars: initial.F90:1088 first_step = .false.; time_management.F90:1426 nsteps_this_interval = 0 unless the file says otherwise
  if (coupled_ts) HIPCHK(c, hipMemsetAsync(c->ice.AQICE, 0, (size_t)c->g.n2 * c->g.nblocks * sizeof(double), c->stream));
  c->nsteps_total = hd.integer("nsteps_total", 0);
  c->nsteps_this_interval = hd.integer("nsteps_this_interval", 0);
  c->first_step = 0;
  // restart.F90:467-468: eod and eod_last each from its own attribute (list-directed logicals); one the file lacks keeps the default,
  // false.  time_manager of the next step copies eod into eod_last (time_management.F90:1809): the file's eod decides that step.
  c->eod = hd.logical("eod");
  c->eod_last = hd.logical("eod_last");
  // files this library wrote before it wrote eod: their eod_last held eod
  if (!hd.has("eod") && hd.text("history").find("written by libpop_amd") != std::string::npos) { c->eod = c->eod_last; c->eod_last = 0; }
  // module state of hmix_gm that no restart file carries: KAPPA_VERTICAL is 1 until compute_kappa runs again (init_gm, hmix_gm.F90:860) -- with
  // 'once_a_day' that is the first step of a restart written at the end of a day (eod_last), with 'never' it stays 1 (the reference's behaviour too)
  if (c->gm.KV) {
    std::vector<double> ones((size_t)c->g.n3 * c->g.nblocks, 1.0);
    HIPCHK(c, hipMemcpy(c->gm.KV, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (h.ice) c->ice.tlast_ice = hd.real("tlast_ice");   // restart.F90:489; QICE belongs to the step that formed it and is not in the file
  if (h.c.tmix_opt == 3) {
    for (int n = 0; n < h.nt; ++n) {
      const std::string key = "rf_S_prev_" + restart_tracer_name(h, n);
      c->rf_S_prev_valid[n] = hd.has(key);                           // extract_attrib_file(..., from_file=rf_S_prev_valid) :516-519
      if (c->rf_S_prev_valid[n]) c->rf_S_prev[n] = hd.real(key);
    }
  }
  return 0;
}

// ---- time_manager + set_switches (time_management.F90:1823-1847, 2139-2234) ----------------
// DevGrid::skip for the step that starts now; cached solver graphs hold the flag by value
static void land_skip_for_step(pop_ctx *c) {
  // every one of the three rotating time levels must have been the `new` one in a step that ran every workgroup (averaging
  // steps do not rotate: with a short averaging period four steps may not get round), and POP_LAND_FULL_STEPS steps at least
  if (c->full_left == c->f.land_full_steps) c->full_seen = 0;      // a reset (set-up, restart, new state) starts the count again
  const int want = (c->f.land_skip && c->full_left == 0 && (c->full_seen == 7 || c->f.land_full_steps == 0)) ? 1 : 0;
  if (!want) c->full_seen |= 1 << c->newt;
  if (c->full_left > 0) --c->full_left;
  if (want == c->g.skip) return;
  c->g.skip = want;
  if (c->stream) hipStreamSynchronize(c->stream);
  for (auto &g : c->graphs) hipGraphExecDestroy(g.exec);
  c->graphs.clear();
}
int pop_time_manager(pop_ctx *c) {
  const pop_config &cf = c->h.c;
  c->ran = true;
  if (!c->host_only) land_skip_for_step(c);
  c->leapfrogts = 1; c->f_euler_ts = 0; c->avg_ts = 0;
  c->nsteps_total += 1;
  if (c->cpl.inited) c->cpl.nsteps += 1;   // the coupling interval's count: pop_set_coupled_forcing resets it
  if (cf.tmix_opt == 2) { c->nsteps_this_interval += 1; if (c->nsteps_this_interval > c->h.nsteps_per_interval) c->nsteps_this_interval = 1; }
  c->eod_last = c->eod;
  c->eod = (cf.tmix_opt == 2) ? (c->nsteps_this_interval == c->h.nsteps_per_interval) : (c->nsteps_total % cf.steps_per_day == 0);
  if (c->first_step) { c->leapfrogts = 0; c->f_euler_ts = 1; c->first_step = 0; }
  if (cf.tmix_opt == 1 && c->nsteps_total % cf.time_mix_freq == 0) c->avg_ts = 1;
  if (cf.tmix_opt == 2) {
    const int n = c->nsteps_this_interval;
    if (n == 2) c->avg_ts = 1;
    else if (n != 1 && (n + 1) % cf.time_mix_freq != 0 && n % cf.time_mix_freq == 0) c->avg_ts = 1;
  }
  // step_mod.F90:302-320
  if (c->leapfrogts) { c->mixt = c->oldt; c->beta = 1.0 / 3.0; c->c2dtt = 2.0 * c->h.dt[1]; c->c2dtu = 2.0 * c->h.dtu; c->c2dtp = 2.0 * c->h.dtp; }
  else { c->mixt = c->curt; c->beta = 0.5; c->c2dtt = c->h.dt[1]; c->c2dtu = c->h.dtu; c->c2dtp = c->h.dtp; }
  tavg_set_flag(c);   // step_mod.F90:260-274: right after time_manager
  c->tavg.in_step = !c->host_only;
  // diag_init_sums (step_mod.F90:353): the arming of pop_diag_arm holds for this step only
  c->diag.run_global = c->diag.arm_global; c->diag.run_cfl = c->diag.arm_cfl;
  c->diag.arm_global = c->diag.arm_cfl = false;
  return 0;
}

int pop_dhdt(pop_ctx *c) {
  if (need_device(c)) return 1;
  ScopedPhase ph(c, "DHDT");
  hipLaunchKernelGGL(k_dhdt, dim3(col_grid(c->g, 256), c->g.nblocks), dim3(256), 0, c->stream, c->g, step_params(c),
                     c->PS[c->curt], c->PS[c->oldt], c->FW_OLD, c->DH, c->DHU);
  HIPCHK(c, hipGetLastError());
  if (c->tavg.active && tavg_site(c, TS_FORCING)) return 1;
  return 0;
}

// launchers of the individual baroclinic phases (also used by pop_time_phase)
static MixState kpp_mix_state(pop_ctx *c, int slot, bool into_alt) {
  MixState ms{};
  for (int n = 0; n < 2; ++n) {
    ms.TMIX[n] = c->TR[n][slot]; ms.STF[n] = c->STF[n];
    ms.KPP_SRC[n] = into_alt ? c->KPPa[n] : c->KPP_SRC[n]; ms.VDC[n] = into_alt ? c->VDCa[n] : c->VDC[n];
  }
  ms.UMIX = c->U[slot]; ms.VMIX = c->V[slot]; ms.UCUR = c->U[c->curt]; ms.VCUR = c->V[c->curt]; ms.RHOMIX = c->RHO[slot];
  ms.VVC = into_alt ? c->VVCa : c->VVC; ms.SHF_QSW = c->SHF_QSW; ms.HBLT = into_alt ? c->HBLTa : c->HBLT;
  ms.HMXL = (into_alt && c->HMXLa) ? c->HMXLa : c->HMXL; ms.HMXL_DR = (into_alt && c->HMXL_DRa) ? c->HMXL_DRa : c->HMXL_DR;
  ms.KBL = into_alt ? c->KBLa : c->KBL;
  ms.KPP_SRCX = into_alt ? c->KPPXa : c->KPPX;
  ms.src_clear_all = (into_alt ? c->src_dirty_alt : c->src_dirty) ? 1 : 0;
  (into_alt ? c->src_dirty_alt : c->src_dirty) = false;   // the evaluation that follows clears the set
  ms.S3a = c->S3a; ms.S3b = c->S3b; ms.S3c = c->S3c; ms.S3d = c->S3d; ms.E3 = c->E3; ms.F3 = c->F3;
  return ms;
}
// KPP's non-local source of the passive tracers from the bracket k_kpp_blmix left in KPPX (kernels_passive.hpp), on the launch stream
// once the coefficients of this step are in place -- computed here or swapped in from the look-ahead
static int phase_kpp_src_passive(pop_ctx *c) {
  for (int n = 2; n < c->h.nt; n += 2) {
    const int np = std::min(2, c->h.nt - n);
    KppSrcPassiveArgs a{};
    for (int s = 0; s < np; ++s) { a.STF[s] = c->STF[n + s]; a.SRC[s] = c->KPP_SRC[n + s]; }
    const dim3 G((c->g.n2 + 255) / 256, c->g.km, c->g.nblocks * np);
    with_flags([&](auto PBC) { hipLaunchKernelGGL(k_kpp_src_passive<PBC.value>, G, dim3(256), 0, c->stream, c->g, (const double *)c->KPPX, a, np); }, c->g.pbc);
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}
static int phase_vmix(pop_ctx *c) {
  const pop_config &cf = c->h.c;
  const StepParams sp = step_params(c);
  if (cf.vmix_choice == 1)
    hipLaunchKernelGGL(k_vmix_const, grid_3d(c), dim3(256), 0, c->stream, c->g, sp, c->TR[0][c->mixt], c->TR[1][c->mixt], c->VDC[0], c->VVC);
  else {
    if (c->ahead_valid && c->ahead_slot == c->mixt) {   // computed beside the previous step's solver: swap the output sets in
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_ahead, 0));
      c->ahead_valid = false; c->kpp_src_user = false; ++c->ahead_swaps;
      for (int n = 0; n < 2; ++n) { std::swap(c->VDC[n], c->VDCa[n]); std::swap(c->KPP_SRC[n], c->KPPa[n]); }
      std::swap(c->VVC, c->VVCa); std::swap(c->HBLT, c->HBLTa); std::swap(c->KBL, c->KBLa); std::swap(c->src_dirty, c->src_dirty_alt);
      if (c->HMXLa) { std::swap(c->HMXL, c->HMXLa); std::swap(c->HMXL_DR, c->HMXL_DRa); }
      std::swap(c->KPPX, c->KPPXa);
      return c->h.nt > 2 ? phase_kpp_src_passive(c) : 0;
    }
    if (ahead_cancel(c)) return 1;
    const MixState ms = kpp_mix_state(c, c->mixt, false);
    if (mix_vmix_coeffs(c->h, c->f, c->g, sp, c->mix, ms, c->stream, c->err)) return 1;
    c->kpp_src_user = false;
    if (cf.vmix_choice == 3 && c->h.nt > 2) return phase_kpp_src_passive(c);
  }
  return 0;
}
// KPP of the next step on the look-ahead stream.  Valid when the next step is a leapfrog step (mixtime = its oldtime = this
// step's curtime) and nothing rewrites the curtime fields before then (no averaging step, no Robert filter).  Inputs:
// T, S, U, V at curtime and the surface fluxes; scratch: the 3-D work fields, idle between baroclinic_driver and the
// next step; outputs: the second set of VDC / VVC / KPP_SRC / HBLT.
static int kpp_look_ahead(pop_ctx *c) {
  // an averaging step rewrites oldtime and curtime in its tail and does not rotate; the Robert filter rewrites curtime
  // (with the mixed-layer-depth diagnostics on, HMXL / HMXL_DR of the step that just ran stay where they are: the look-ahead writes the second pair)
  // tidal_diag: TIDAL_DIFF ... KVMIX_M have one set of arrays, which holds the step that has run
  if (!c->f.kpp_ahead || c->avg_ts || c->h.c.tmix_opt == 3 || (c->h.c.kpp_ml_diagnostics == 1 && !c->HMXLa) ||
      (c->tidal.on && c->tidal.nml.tidal_diag)) return 0;
  HIPCHK(c, hipEventRecord(c->ev_ahead_fork, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->ahead, c->ev_ahead_fork, 0));
  const MixState ms = kpp_mix_state(c, c->curt, true);
  if (mix_vmix_coeffs(c->h, c->f, c->g, step_params(c), c->mix, ms, c->ahead, c->err)) return 1;
  HIPCHK(c, hipEventRecord(c->ev_ahead, c->ahead));
  c->ahead_valid = true; c->ahead_slot = c->curt;
  return 0;
}
// lsubmesoscale_mixing (horizontal_mix.F90:566-581, mix_submeso.F90:341-1005): the column fields of submeso_sf from the mix-time tracers and this
// step's HMXL, then the tendency of submeso_flux added to GTK, which k_gm_flux has just written on the same stream
static SubmDev submeso_dev(pop_ctx *c) {
  SubmDev W = c->subm;
  W.HMXL = (c->h.c.vmix_choice == 3) ? c->HMXL : nullptr;    // ML_DEPTH = HMXL | zw(1) (:424-426)
  W.grav = step_params(c).grav; W.sqrt_grav = std::sqrt(W.grav);
  return W;
}
// submeso_flux of the tracer pair (X0, X1) added to W.GTK, from the column fields k_submeso_column formed
static int submeso_flux_launch(pop_ctx *c, const SubmDev &W, const double *X0, const double *X1, bool tz0 = false) {
  if (W.TD[0]) {   // the levels below the march hold 0
    const size_t bytes = (size_t)c->g.n3 * c->g.nblocks * sizeof(double);
    HIPCHK(c, hipMemsetAsync(W.TD[0], 0, bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(W.TD[1], 0, bytes, c->stream));
  }
  const dim3 GT(((c->g.nxb + POP_SUBM_TX - 1) / POP_SUBM_TX) * ((c->g.nyb + POP_SUBM_TY - 1) / POP_SUBM_TY), c->g.nblocks);
  with_flags([&](auto TZ0) { hipLaunchKernelGGL(k_submeso_flux<TZ0.value>, GT, dim3(POP_SUBM_TX, POP_SUBM_TY), 0, c->stream, c->g, W, X0, X1); }, tz0);
  return 0;
}
static int phase_submeso(pop_ctx *c, const double *T, const double *S) {
  const SubmDev W = submeso_dev(c);
  const dim3 G2((c->g.n2 + 255) / 256, c->g.nblocks);
  hipLaunchKernelGGL(k_submeso_column, G2, dim3(256), 0, c->stream, c->g, W, T, S);
  if (submeso_flux_launch(c, W, T, S)) return 1;
  if (W.US) hipLaunchKernelGGL(k_submeso_vel, G2, dim3(256), 0, c->stream, c->g, W);
  HIPCHK(c, hipGetLastError());
  return 0;
}
// hmix_tracer = 3 (horizontal_mix.F90:549-554, hmix_gm.F90:1102-2226): slopes and tapered diffusivities of the mix-time tracers, the
// isopycnal part added to VDC (after vmix_coeffs, before the tracer right-hand side reads it), and the tendency GTK of both tracers
// the tendency of the tracer pair (X0, X1) into G.GTK from the slopes and diffusivities in G; add: with the isopycnal part added to VDC
static void gm_flux_launch(pop_ctx *c, const GmDev &G, const double *X0, const double *X1, bool add) {
  const dim3 G3((c->g.n2 + 255) / 256, c->g.km, c->g.nblocks);
  const StepParams sp = step_params(c);
  double *v1 = (sp.nvdc == 2 && c->VDC[1] != c->VDC[0]) ? c->VDC[1] : nullptr;   // one shared array is added to once
  if (c->f.gm_lds && (G.cancellation || G.SF[0])) {   // every horizontal face flux formed once in 64 x 8 patches; else (or the stream-function terms not stored) cell by cell
    constexpr int R = 8;     // rows of the patch
    const dim3 GT(((c->g.nxb + 62) / 63) * ((c->g.nyb + R - 2) / (R - 1)), (c->g.km + POP_GM_KC - 1) / POP_GM_KC, G3.z);
    with_flags([&](auto CANC, auto ADD) {
      hipLaunchKernelGGL((k_gm_flux_tile<R, CANC.value, ADD.value>), GT, dim3(64, R), 0, c->stream, c->g, G, X0, X1, c->VDC[0], v1);
    }, G.cancellation, add);
  } else
  with_flags([&](auto ADD) {
    hipLaunchKernelGGL(k_gm_flux<ADD.value>, dim3(G3.x, (c->g.km + POP_GM_KC - 1) / POP_GM_KC, G3.z), dim3(256), 0, c->stream, c->g, G, X0, X1, c->VDC[0], v1);
  }, add);
}
static GmDev gm_dev(pop_ctx *c) {
  GmDev G = c->gm;
  G.HBLT = (c->h.c.vmix_choice == 3) ? c->HBLT : nullptr;            // BL_DEPTH = KPP_HBLT | zw(1) (:1210-1212)
  if (G.tlt) G.HMXL = (c->h.c.vmix_choice == 3) ? c->HMXL : nullptr;
  return G;
}
static int phase_hmix_gm(pop_ctx *c) {
  const double *T = c->TR[0][c->mixt], *S = c->TR[1][c->mixt];
  const GmDev G = gm_dev(c);
  const dim3 G3((c->g.n2 + 255) / 256, c->g.km, c->g.nblocks);
  const dim3 G2(G3.x, c->g.nblocks);
  const bool kappa_now = G.KV && (c->h.c.gm_kappa_freq == 1 || c->nsteps_total == 1 || (c->h.c.gm_kappa_freq == 2 && c->eod_last));   // compute_kappa (:1258-1332): the first step of the run, or every step
  if (G.tlt) {   // :1222-1250, then the tapering with the layer's rules, then merged_streamfunction / apply_vertical_profile (:1668-1674)
    hipLaunchKernelGGL(k_gm_diabatic_depth, G2, dim3(256), 0, c->stream, c->g, G);
    hipLaunchKernelGGL(k_gm_coeffs<1>, G3, dim3(256), 0, c->stream, c->g, G, T, S);
    hipLaunchKernelGGL(k_gm_transition_layer, G2, dim3(256), 0, c->stream, c->g, G);
    if (kappa_now) hipLaunchKernelGGL(k_gm_kappa_vertical, G2, dim3(256), 0, c->stream, c->g, G, T, S, step_params(c).grav);
    hipLaunchKernelGGL(k_gm_coeffs<2>, G3, dim3(256), 0, c->stream, c->g, G, T, S);
    hipLaunchKernelGGL(k_gm_msf_column, G2, dim3(256), 0, c->stream, c->g, G);
  } else {
    if (kappa_now) hipLaunchKernelGGL(k_gm_kappa_vertical, G2, dim3(256), 0, c->stream, c->g, G, T, S, step_params(c).grav);
    hipLaunchKernelGGL(k_gm_coeffs<0>, G3, dim3(256), 0, c->stream, c->g, G, T, S);
  }
  if (G.SF[0]) hipLaunchKernelGGL(k_gm_sf, G3, dim3(256), 0, c->stream, c->g, G);   // without cancellation: SF_SLX, SF_SLY once per half cell
  if (G.UISOP) hipLaunchKernelGGL(k_gm_bolus, G2, dim3(256), 0, c->stream, c->g, G);   // diag_gm_bolus
  gm_flux_launch(c, G, T, S, true);
  HIPCHK(c, hipGetLastError());
  if (c->h.c.lsubmesoscale_mixing) return phase_submeso(c, T, S);
  return 0;
}
static int phase_hmix_tracer(pop_ctx *c, hipStream_t st = nullptr) {   // del4: first Laplacian of the tracers into d2t; gm: the whole tendency
  if (c->h.c.hmix_tracer == 3) return phase_hmix_gm(c);
  if (c->h.c.hmix_tracer != 4) return 0;
  if (c->d2t_next_valid && c->d2t_next_slot == c->mixt) {   // formed by the previous step's tracer kernel (ghost ring already updated)
    c->d2t_next_valid = false;
    std::swap(c->d2t[0], c->d2t_next[0]); std::swap(c->d2t[1], c->d2t_next[1]);
    return 0;
  }
  c->d2t_next_valid = false;
  return mix_hdifft_del4(c->f.del4_tile_rows, c->g, step_params(c), c->mix, c->TR[0][c->mixt], c->TR[1][c->mixt], c->d2t[0], c->d2t[1], c->S3c, c->S3d, st ? st : c->stream, c->err);
}
// advt with tadvect = 3 (advection.F90:1667-1708, 2684-3280; comp_flux_vel_ghost :1014-1120): L(T) of both tracers into lw.XOUT
static int phase_advt_lw_lim(pop_ctx *c) {
  const int km = c->g.km;
  const double *X0 = c->TR[0][c->mixt], *X1 = c->TR[1][c->mixt];
  with_flags([&](auto PBC) {
    hipLaunchKernelGGL(k_lw_flux<PBC.value>, grid_cols(c), dim3(POP_COL_THREADS), 0, c->stream, c->g, c->lw, (const double *)c->U[c->curt], (const double *)c->V[c->curt], (const double *)c->DH);
  }, c->g.pbc);
  // UTE: E face, vector; WTKB: centre (comp_flux_vel_ghost :1080-1100).  VTN is not exchanged by the reference: it forms it in
  // the ghost rows from the ghost velocities.  Beyond a tripole fold those are the mirrored velocities with the sign of a
  // vector, so the N-face mirror of VTN with that sign is the same number (the two products are added in the other order);
  // the degenerate top row stays as computed (location 4: N face, ghost rows only).
  if (halo_update_many(c, {{c->lw.UTE, km, 3, 1}, {c->lw.VTN, km, 4, 1}, {c->lw.WTKB, km}})) return 1;
  const dim3 G3((c->g.n2 + 255) / 256, km, c->g.nblocks * 2);
  with_flags([&](auto PBC) {
    hipLaunchKernelGGL(k_lw_z<PBC.value>, G3, dim3(256), 0, c->stream, c->g, c->lw, X0, X1, c->c2dtt);
    hipLaunchKernelGGL(k_lw_x<PBC.value>, G3, dim3(256), 0, c->stream, c->g, c->lw, X0, X1, c->c2dtt);
    hipLaunchKernelGGL(k_lw_y<PBC.value>, G3, dim3(256), 0, c->stream, c->g, c->lw, X0, X1, c->c2dtt);
  }, c->g.pbc);
  HIPCHK(c, hipGetLastError());
  return 0;
}
// the arguments of the (T, S) right-hand side that do not depend on the kernel form
static TracerRhsArgs tracer_rhs_args(pop_ctx *c, const StepParams &sp) {
  TracerRhsArgs a{};
  if (c->h.c.tadvect == 3) { a.LTK[0] = c->lw.XOUT[0]; a.LTK[1] = c->lw.XOUT[1]; }
  a.E[0] = c->E3; a.F[0] = c->F3; a.E[1] = c->S3c; a.F[1] = c->S3d;
  for (int n = 0; n < 2; ++n) {
    a.TCUR[n] = c->TR[n][c->curt]; a.TOLD[n] = c->TR[n][c->oldt]; a.TMIX[n] = c->TR[n][c->mixt]; a.TNEW[n] = c->TR[n][c->newt];
    a.VDC[n] = c->VDC[sp.nvdc == 2 ? n : 0]; a.KPP_SRC[n] = c->KPP_SRC[n]; a.STF[n] = c->STF[n]; a.TFW[n] = c->TFW[n];
  }
  if (c->h.c.hmix_tracer == 4) { a.TMIX[0] = c->d2t[0]; a.TMIX[1] = c->d2t[1]; }   // del4: second Laplacian acts on D2T
  a.UCUR = c->U[c->curt]; a.VCUR = c->V[c->curt]; a.DH = c->DH; a.PCUR = c->PS[c->curt]; a.POLD = c->PS[c->oldt];
  a.c2dtt = c->c2dtt; a.use_kpp_src = (c->h.c.vmix_choice == 3);
  if (a.use_kpp_src && !c->kpp_src_user && !c->f.kpp_src_full) a.KBL = c->KBL;
  if (c->h.c.lsw_absorb != 0) {   // lsw_absorb: penetrating short wave (add_sw_absorb)
    a.sw_on = 1; a.sw_type = c->h.c.sw_absorption_type; a.sw_ksol = c->h.sw.ksol;
    a.QSW = c->SHF_QSW; a.swabs = c->h.sw.swabs; a.swTr = c->h.sw.Tr; a.swCHLI = c->h.sw.CHLI;
  }
  return a;
}
// site "tavg_transport" (launch_transport.hpp): the step's launch has been made; not inside pop_time_phase, which times kernels only
static int trn_after_rhs(pop_ctx *c, const TracerRhsArgs &a) { return (c->trn.active && !c->phase_timing) ? trn_site(c, a) : 0; }
static int phase_tracer_rhs(pop_ctx *c, bool fwd = false) {
  const StepParams sp = step_params(c);
  if (c->h.c.tadvect == 3 && phase_advt_lw_lim(c)) return 1;
  TracerRhsArgs a = tracer_rhs_args(c, sp);
  // the next step's first Laplacian: valid when that step is a leapfrog step whose mix time is this step's current time and nothing
  // rewrites the current tracers before then (no averaging step, no Robert filter) -- the rule of the KPP look-ahead
  // Gent-McWilliams (r4): the LDS kernel with the mixing tendency given (k_tracer_rhs_lds<., ., false, true>)
  const bool gm_lds = c->h.c.hmix_tracer == 3 && !c->g.pbc && c->f.gm_lds;
  const bool lds_kernel = c->h.c.tadvect == 1 && (c->h.c.hmix_tracer != 3 || gm_lds) && (c->f.tracer_lds_rows == 8 || c->f.tracer_lds_rows == 4);
  if (lds_kernel && gm_lds) { a.HDT[0] = c->gm.GTK[0]; a.HDT[1] = c->gm.GTK[1]; }
  const bool form_next = lds_kernel && !gm_lds && c->f.d2t_fuse && !c->avg_ts && c->h.c.tmix_opt != 3 && c->tr_ghosts_ok[c->curt];
  if (form_next) { a.D2N[0] = c->d2t_next[0]; a.D2N[1] = c->d2t_next[1]; a.AHF = c->mix.D4AHF; }
  c->d2t_last_formed = form_next;
  if (lds_kernel) {
    with_value<4, 8>(c->f.tracer_lds_rows, [&](auto R) { launch_tracer_lds<R.value>(c->g, sp, a, c->stream, fwd); });
    if (form_next && !c->phase_timing) {
      if (halo_update_many(c, {{c->d2t_next[0], c->g.km}, {c->d2t_next[1], c->g.km}})) return 1;
      c->d2t_next_valid = true; c->d2t_next_slot = c->curt;
    }
    return trn_after_rhs(c, a);
  }
  if (fwd) { c->err = "fused forward elimination needs the LDS tracer kernel"; return 1; }
  const bool gm = c->h.c.hmix_tracer == 3, up3 = c->h.c.tadvect == 2;
  if (gm) { a.HDT[0] = c->gm.GTK[0]; a.HDT[1] = c->gm.GTK[1]; }   // Gent-McWilliams: the tendency formed by phase_hmix_gm in place of del2 mixing
  if (up3) a.up = c->upw3;
  with_flags([&](auto GM, auto UP3, auto PBC) {
    hipLaunchKernelGGL((k_tracer_rhs<GM.value, UP3.value, PBC.value>), grid_stencil(c), block_stencil(), 0, c->stream, c->g, sp, a);
  }, gm, up3, c->g.pbc);
  return trn_after_rhs(c, a);
}
// pop_run_phase / pop_time_phase: the site on its own, from the fields the last right-hand side launch read
static int trn_phase(pop_ctx *c) {
  if (!c->trn.requested) { c->err = "tavg_transport: pop_transport_request has not been called"; return 1; }
  return trn_site(c, tracer_rhs_args(c, step_params(c)));
}
// tracer_update (baroclinic.F90:1981-2300) for the passive tracers n = 3 .. nt, a pair per launch and one launch of one for an odd count,
// on the launch stream after the (T, S) right-hand side: k_tracer_rhs<., ., ., NP, true>.  Every tracer uses cfg.tadvect and the (T, S)
// mixing scheme; the schemes that form a field per tracer ahead of the right-hand side run their (T, S) kernels once more per pair into
// the passive work fields, from the flux velocities (lw_lim), slopes and diffusivities (Gent-McWilliams) and stream function (submeso)
// already formed for this step.  No predictor follows (impvmixt(.., 1, 2, ..), baroclinic.F90:885-893, is for T and S).
static int phase_passive_rhs(pop_ctx *c) {
  const int nt = c->h.nt;
  if (nt <= 2) return 0;
  const pop_config &cf = c->h.c;
  const StepParams sp = step_params(c);
  const bool gm = cf.hmix_tracer == 3, up3 = cf.tadvect == 2;
  for (int n = 2; n < nt; n += 2) {
    const int np = std::min(2, nt - n);
    const int m[2] = {n, n + np - 1};   // slot -> tracer; with one tracer slot 1 repeats it as an input and has spare outputs
    const double *X0 = c->TR[m[0]][c->mixt], *X1 = c->TR[m[1]][c->mixt];
    double *W[2] = {c->PW[n], np == 2 ? c->PW[n + 1] : c->PWX};
    TracerRhsArgs a{};
    if (gm) {
      GmDev G = gm_dev(c);
      G.GTK[0] = W[0]; G.GTK[1] = W[1];
      gm_flux_launch(c, G, X0, X1, false);
      if (cf.lsubmesoscale_mixing) {
        SubmDev S = submeso_dev(c);
        S.GTK[0] = W[0]; S.GTK[1] = W[1];
        if (S.TD[0]) { S.TD[0] = c->PTD[n]; S.TD[1] = np == 2 ? c->PTD[n + 1] : c->PTDX; }
        if (submeso_flux_launch(c, S, X0, X1, G.cancellation != 0)) return 1;   // k_submeso_flux<TZ0>: what the reference's TZ holds for n > 2
      }
      a.HDT[0] = W[0]; a.HDT[1] = W[1];
    }
    if (cf.hmix_tracer == 4 && mix_hdifft_del4(c->f.del4_tile_rows, c->g, sp, c->mix, X0, X1, W[0], W[1], nullptr, nullptr, c->stream, c->err)) return 1;
    if (cf.tadvect == 3) {   // the three direction passes of phase_advt_lw_lim on this pair; UTE, VTN, WTKB are those of the step
      LwDev L = c->lw;
      L.XOUT[0] = c->PL[0]; L.XOUT[1] = c->PL[1];
      const dim3 G3((c->g.n2 + 255) / 256, c->g.km, c->g.nblocks * 2);
      with_flags([&](auto PBC) {
        hipLaunchKernelGGL(k_lw_z<PBC.value>, G3, dim3(256), 0, c->stream, c->g, L, X0, X1, c->c2dtt);
        hipLaunchKernelGGL(k_lw_x<PBC.value>, G3, dim3(256), 0, c->stream, c->g, L, X0, X1, c->c2dtt);
        hipLaunchKernelGGL(k_lw_y<PBC.value>, G3, dim3(256), 0, c->stream, c->g, L, X0, X1, c->c2dtt);
      }, c->g.pbc);
      a.LTK[0] = c->PL[0]; a.LTK[1] = c->PL[1];
    }
    for (int s = 0; s < 2; ++s) {
      const int t = m[s];
      a.TCUR[s] = c->TR[t][c->curt]; a.TOLD[s] = c->TR[t][c->oldt]; a.TMIX[s] = c->TR[t][c->mixt]; a.TNEW[s] = c->TR[t][c->newt];
      a.VDC[s] = c->VDC[sp.nvdc == 2 ? 1 : 0];   // VDC(:,:,:,min(n, size(VDC,4))): salinity's, or the only one (vertical_mix.F90:1260)
      a.KPP_SRC[s] = c->KPP_SRC[t]; a.STF[s] = c->STF[t]; a.TFW[s] = c->TFW[t];
      a.isrc[s] = c->h.iage[t] ? 1.0 / (365.0 * 86400.0) : 0.0;   // c1 / seconds_in_year (iage_mod.F90:352-353)
    }
    if (cf.hmix_tracer == 4) { a.TMIX[0] = W[0]; a.TMIX[1] = W[1]; }   // del4: second Laplacian acts on D2T
    a.UCUR = c->U[c->curt]; a.VCUR = c->V[c->curt]; a.DH = c->DH; a.PCUR = c->PS[c->curt]; a.POLD = c->PS[c->oldt];
    a.c2dtt = c->c2dtt; a.use_kpp_src = (cf.vmix_choice == 3);
    if (up3) a.up = c->upw3;
    with_flags([&](auto GM, auto UP3, auto PBC, auto TWO) {
      hipLaunchKernelGGL((k_tracer_rhs<GM.value, UP3.value, PBC.value, TWO.value ? 2 : 1, true>), grid_stencil(c), block_stencil(), 0, c->stream, c->g, sp, a);
    }, gm, up3, c->g.pbc, np == 2);
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}
// the surface reset of the tracer modules (reset_passive_tracers; ideal age: TRACER(:,:,1) = 0 over the whole slab, iage_mod.F90:386-415)
static int passive_reset(pop_ctx *c, int slot) {
  for (int n = 2; n < c->h.nt; ++n)
    if (c->h.iage[n]) HIPCHK(c, hipMemset2DAsync(c->TR[n][slot], (size_t)c->g.n3 * sizeof(double), 0, (size_t)c->g.n2 * sizeof(double), c->g.nblocks, c->stream));
  return 0;
}
static ImpvmixtArgs impvmixt_args(pop_ctx *c, const double *psfc) {
  const StepParams sp = step_params(c);
  ImpvmixtArgs a{};
  for (int n = 0; n < 2; ++n) { a.TNEW[n] = c->TR[n][c->newt]; a.TOLD[n] = c->TR[n][c->oldt]; a.TCUR[n] = c->TR[n][c->curt]; a.VDC[n] = c->VDC[sp.nvdc == 2 ? n : 0]; }
  a.PSFC = psfc; a.POLD = c->PS[c->oldt]; a.PCUR = c->PS[c->curt]; a.PNEW = c->PS[c->newt]; a.PMIX = c->PS[c->mixt];
  a.E = c->E3; a.F = c->F3; a.RHO = c->RHO[c->newt]; a.c2dtt = c->c2dtt; a.nfirst = 1; a.nlast = 2;
  return a;
}
// predictor with the forward elimination inside the right-hand-side kernel (Forms::tracer_fwd) on a leapfrog step
static bool tracer_fwd_fused(const pop_ctx *c) { return c->f.tracer_fwd && c->leapfrogts; }
static int phase_impvmixt_back(pop_ctx *c) {
  ImpvmixtBackArgs b{};
  for (int n = 0; n < 2; ++n) { b.TNEW[n] = c->TR[n][c->newt]; b.TOLD[n] = c->TR[n][c->oldt]; }
  b.E[0] = c->E3; b.F[0] = c->F3; b.E[1] = c->S3c; b.F[1] = c->S3d;
  const dim3 G = grid_cols(c);
  hipLaunchKernelGGL(k_impvmixt_back, dim3(G.x, G.y, 2), dim3(POP_COL_THREADS), 0, c->stream, c->g, b);
  return 0;
}
static int phase_impvmixt_pred(pop_ctx *c) {
  launch_impvmixt<0, false, false>(c->g, step_params(c), impvmixt_args(c, c->PS[c->curt]), grid_cols(c), c->stream, c->f.reg_thomas_t, c->f.thomas_pair);
  return 0;
}
static int phase_state_new(pop_ctx *c) {
  launch_state3d(c->g, c->TR[0][c->newt], c->TR[1][c->newt], c->RHO[c->newt], c->stream);
  return 0;
}
// density of the new tracers on the rows j_first <= j < j_end (0-based) of every block
static void state_new_rows(pop_ctx *c, int j_first, int j_end) {
  const int p0 = j_first * c->g.nxb, p1 = j_end * c->g.nxb;
  if (p1 <= p0) return;
  hipLaunchKernelGGL(k_state3d_rows, dim3((p1 - p0 + 255) / 256, c->g.km, c->g.nblocks), dim3(256), 0, c->stream, c->g,
                     (const double *)c->TR[0][c->newt], (const double *)c->TR[1][c->newt], c->RHO[c->newt], p0, p1);
}
// anis: hdiffu_aniso of the mix-time velocity into HDU, HDV (every level)
static AnisoArgs aniso_args(pop_ctx *c) {
  const pop_config &cf = c->h.c;
  AnisoArgs a{};
  a.UM = c->U[c->mixt]; a.VM = c->V[c->mixt]; a.HDU = c->HDU; a.HDV = c->HDV;
  a.H1E = c->d2["H1E"]; a.H1W = c->d2["H1W"]; a.H2N = c->d2["H2N"]; a.H2S = c->d2["H2S"];
  a.K1E = c->d2["K1E"]; a.K1W = c->d2["K1W"]; a.K2N = c->d2["K2N"]; a.K2S = c->d2["K2S"];
  a.AMAX = c->d2["AMAX_CFL"]; a.ANGLE = c->d2["ANGLE"]; a.UAREA = c->d2["UAREA"];
  if (cf.lsmag_aniso) { a.DSMIN = c->d2["DSMIN"]; a.FPS = c->d2["F_PERP_SMAG"]; }
  a.FPARA = c->FPARA; a.FPERP = c->FPERP;
  a.visc_para = cf.visc_para; a.visc_perp = cf.visc_perp; a.c_para = cf.c_para; a.c_perp = cf.c_perp;
  a.east = cf.aniso_alignment == 1; a.variable = cf.lvariable_hmix_aniso; a.smag = cf.lsmag_aniso;
  return a;
}
static int phase_hmix_momentum(pop_ctx *c, hipStream_t st = nullptr) {   // del4: first Laplacian of the velocity into d2u; anis: HDU, HDV
  if (c->h.c.hmix_momentum == 3) { launch_hdiffu_aniso(c->g, aniso_args(c), st ? st : c->stream); return 0; }
  if (c->h.c.hmix_momentum != 4) return 0;
  if (c->d2u_next_valid && c->d2u_next_slot == c->mixt) {   // formed by the previous step's momentum kernel (ghost ring already updated)
    c->d2u_next_valid = false;
    std::swap(c->d2u[0], c->d2u_next[0]); std::swap(c->d2u[1], c->d2u_next[1]);
    return 0;
  }
  c->d2u_next_valid = false;
  return mix_hdiffu_del4(c->f.del4_tile_rows, c->g, step_params(c), c->mix, c->U[c->mixt], c->V[c->mixt], c->d2u[0], c->d2u[1], c->S3c, c->S3d, st ? st : c->stream, c->err);
}
static int phase_momentum_rhs(pop_ctx *c, int tj_first = 0, int tj_count = -1, bool last_piece = true) {
  MomentumRhsArgs a{};
  a.UCUR = c->U[c->curt]; a.VCUR = c->V[c->curt]; a.UOLD = c->U[c->oldt]; a.VOLD = c->V[c->oldt]; a.UMIX = c->U[c->mixt]; a.VMIX = c->V[c->mixt];
  a.RHOOLD = c->RHO[c->oldt]; a.RHOCUR = c->RHO[c->curt]; a.RHONEW = c->RHO[c->newt]; a.VVC = c->VVC; a.DHU = c->DHU;
  if (c->h.c.hmix_momentum == 4) { a.UMIX = c->d2u[0]; a.VMIX = c->d2u[1]; }   // del4: second Laplacian acts on D2U, D2V
  a.UNEW = c->U[c->newt]; a.VNEW = c->V[c->newt]; a.ZX = c->ZX; a.ZY = c->ZY;
  // 3x3 stencils staged through LDS (kernels_momentum_lds.hpp; Forms::momentum_lds_rows)
  // the next step's first Laplacian of the velocity (see phase_tracer_rhs; whole-domain launches of the LDS kernel only)
  // (several ranks launch the kernel in three pieces -- interior tile rows, then the rim rows: every piece writes its tiles, the halo
  // update follows the last one)
  const bool form_next = (c->f.momentum_lds_rows == 8 || c->f.momentum_lds_rows == 4) && c->f.d2u_fuse && !c->avg_ts &&
                         c->h.c.tmix_opt != 3 && c->uv_ghosts_ok[c->curt];
  if (form_next) { a.D2N[0] = c->d2u_next[0]; a.D2N[1] = c->d2u_next[1]; a.AMF = c->mix.D4AMF; }
  c->d2u_last_formed = form_next;
  const bool pre = c->h.c.hmix_momentum == 3;   // anis: the friction phase_hmix_momentum formed
  if (pre) { a.HDU = c->HDU; a.HDV = c->HDV; }
  const bool lds = with_value<4, 8>(c->f.momentum_lds_rows, [&](auto R) { launch_momentum_lds<R.value>(c->g, step_params(c), a, c->stream, tj_first, tj_count, pre); });
  if (!lds) with_flags([&](auto PRE, auto PBC) {
    hipLaunchKernelGGL((k_momentum_rhs<PRE.value, PBC.value>), grid_stencil(c), block_stencil(), 0, c->stream, c->g, step_params(c), a);
  }, pre, c->g.pbc);
  if (form_next && last_piece && !c->phase_timing) {
    if (halo_update_many(c, {{c->d2u_next[0], c->g.km, 1, 1}, {c->d2u_next[1], c->g.km, 1, 1}})) return 1;
    c->d2u_next_valid = true; c->d2u_next_slot = c->curt;
  }
  return 0;
}
static int phase_impvmixu(pop_ctx *c, hipStream_t st) {
  ImpvmixuArgs a{c->U[c->newt], c->V[c->newt], c->E3, c->U[c->oldt], c->V[c->oldt], c->VVC};
  launch_impvmixu(c->g, step_params(c), a, grid_cols(c), st ? st : c->stream, c->f.reg_thomas_u, c->f.impvmixu_waves);
  return 0;
}

static int phase_correct(pop_ctx *c) {
  const StepParams sp = step_params(c);
  // the generic Thomas kernel stages E, F through the shared 3-D scratch (E3, F3), which a KPP look-ahead in flight on its own
  // stream also uses (E3 = the Richardson column of the generic k_kpp_interior): the corrector then follows the look-ahead.
  // The register kernels touch no scratch and run beside it.
  if (!c->f.reg_thomas_t && c->ahead_valid) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_ahead, 0));
  if (sp.pavg) launch_impvmixt<1, false, true>(c->g, sp, impvmixt_args(c, c->PS[c->newt]), grid_cols(c), c->stream, c->f.reg_thomas_t, c->f.thomas_pair);
  else launch_impvmixt<0, true, true>(c->g, sp, impvmixt_args(c, c->PS[c->newt]), grid_cols(c), c->stream, c->f.reg_thomas_t, c->f.thomas_pair);
  // passive tracers: TNEW(1) -= TOLD(1) (PSURF(new) - PSURF(old)) / (grav dz(1)) and the standard solve with PSURF(new) on the left-hand
  // side, under pressure averaging (baroclinic.F90:1303-1321) as without it (:1328-1344: mixtime = oldtime on a leapfrog step, curtime on
  // the Euler step, which is what PMIX is) -- the all-tracer form k_impvmixt<0, PRE>, a pair per launch; then reset_passive_tracers (:1458-1460)
  for (int n = 2; n < c->h.nt; n += 2) {
    ImpvmixtArgs a = impvmixt_args(c, c->PS[c->newt]);
    a.nfirst = 1; a.nlast = std::min(2, c->h.nt - n);
    for (int s = 0; s < a.nlast; ++s) {
      a.TNEW[s] = c->TR[n + s][c->newt]; a.TOLD[s] = c->TR[n + s][c->oldt]; a.TCUR[s] = c->TR[n + s][c->curt];
      a.VDC[s] = c->VDC[sp.nvdc == 2 ? 1 : 0];
    }
    launch_impvmixt<0, true, false>(c->g, sp, a, grid_cols(c), c->stream, c->f.reg_thomas_t, c->f.thomas_pair);
  }
  return passive_reset(c, c->newt);
}
// ice_formation (ice.F90:357-621) on the tracers, surface pressure and density of one time slot
static int phase_ice(pop_ctx *c, int slot) {
  if (!c->ice.inited) { c->err = "ice formation needs pop_init_ice"; return 1; }
  const pop_ctx::Ice &I = c->ice;
  IceArgs a{};
  a.T = c->TR[0][slot]; a.S = c->TR[1][slot]; a.RHO = c->RHO[slot]; a.PS = c->PS[slot];
  a.QICE = I.QICE; a.AQICE = I.AQICE; a.FWF = I.FWF;
  a.cpl = I.k.cp_over_lhfusion; a.salice = I.k.salice; a.salref = I.k.salref;
  a.time_weight = ice_time_weight(c); a.dt1 = c->h.dt[1]; a.grav = GRAV;
  a.kmxice = I.nml.kmxice; a.tfz = I.nml.tfreeze_option; a.salt_flx = I.nml.lfw_as_salt_flx;
  launch_ice_formation(c->g, a, c->stream);
  return 0;
}
static int phase_add_btrop(pop_ctx *c, hipStream_t st = nullptr) {
  hipLaunchKernelGGL(k_add_barotropic, grid_3d(c), dim3(256), 0, st ? st : c->stream, c->g, c->U[c->newt], c->V[c->newt], c->UB[c->newt], c->VB[c->newt]);
  return 0;
}

int pop_baroclinic_driver(pop_ctx *c) {
  if (need_device(c)) return 1;
  ScopedPhase ph(c, "BAROCLINIC");
  if (c->vmixu_deferred) { c->vmixu_deferred = false; if (phase_impvmixu(c, nullptr)) return 1; }   // a driver call that was never followed by its correct_adjust
  const StepParams sp = step_params(c);
  // tavg: the velocities and, unless the Robert filter takes them in step_rf, the tracers of the cur level (baroclinic.F90:772-816)
  if (c->tavg.active && (tavg_site(c, TS_STATE) || (c->h.c.tmix_opt != 3 && tavg_site(c, TS_TRACER)))) return 1;
  // del4 first Laplacians / the anisotropic friction beside the vertical-mixing coefficients: they read only mix-time fields
  const bool tr_side = c->f.del4_side && c->h.c.hmix_tracer != 3;
  const bool fork = c->f.mom_side || tr_side;
  if (fork) {
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
    if (tr_side && phase_hmix_tracer(c, c->side)) return 1;
    HIPCHK(c, hipEventRecord(c->ev_d2t, c->side));
    if (c->f.mom_side && phase_hmix_momentum(c, c->side)) return 1;
    HIPCHK(c, hipEventRecord(c->ev_d2u, c->side));
  }
  if (phase_vmix(c)) return 1;
  if (c->tavg.active && tavg_site(c, TS_VMIX)) return 1;   // this step's coefficients, computed or swapped in, before K33 is added
  if (fork) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_d2t, 0));
  if (!tr_side && phase_hmix_tracer(c)) return 1;   // Gent-McWilliams reads and adds to the coefficients vmix just formed
  if (c->tavg.active && tavg_site(c, TS_HMIX)) return 1;
  const bool fwd = sp.pavg && tracer_fwd_fused(c);
  if (phase_tracer_rhs(c, fwd) || phase_passive_rhs(c)) return 1;
  // several ranks: the exchange of the new tracers' ghost rows runs on the communication stream while the launch stream
  // forms the density and the momentum right-hand side of every tile that reads no ghost row of another rank; the first
  // and last tile rows follow once the rows have arrived (same kernels on disjoint tiles: bitwise the serial result)
  const int mrows = c->f.momentum_lds_rows;
  const bool overlap = sp.pavg && halo_async_ok(c) && (mrows == 4 || mrows == 8) && !c->h.c.ns_boundary;
  const int mtiles_j = overlap ? (c->g.nyb - 2 * NGHOST + mrows - 1) / mrows : 0;
  if (sp.pavg) {
    if (fwd ? phase_impvmixt_back(c) : phase_impvmixt_pred(c)) return 1;
    if (overlap && mtiles_j >= 3) {
      HaloAsync HA;
      if (halo_many_begin(c, {{c->TR[0][c->newt], c->g.km}, {c->TR[1][c->newt], c->g.km}}, HA)) return 1;
      state_new_rows(c, NGHOST, c->g.nyb - NGHOST);                      // physical rows: own cells + ghosts copied inside the rank
      if (c->f.mom_side) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_d2u, 0));
      else if (phase_hmix_momentum(c)) return 1;
      if (phase_momentum_rhs(c, 1, mtiles_j - 2, false)) return 1;      // interior tile rows
      if (halo_many_end(c, HA)) return 1;
      state_new_rows(c, 0, NGHOST); state_new_rows(c, c->g.nyb - NGHOST, c->g.nyb);   // ghost rows
      if (phase_momentum_rhs(c, 0, 1, false) || phase_momentum_rhs(c, mtiles_j - 1, 1, true)) return 1;   // rim tile rows
    } else {
      if (halo_update_many(c, {{c->TR[0][c->newt], c->g.km}, {c->TR[1][c->newt], c->g.km}})) return 1;
      if (phase_state_new(c)) return 1;
      if (c->f.mom_side) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_d2u, 0));
      else if (phase_hmix_momentum(c)) return 1;
      if (phase_momentum_rhs(c)) return 1;
    }
  } else {
    if (c->f.mom_side) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_d2u, 0));
    else if (phase_hmix_momentum(c)) return 1;
    if (phase_momentum_rhs(c)) return 1;
  }
  // the implicit vertical mixing of U, V is not needed before the step tail (Forms::vmixu): on the side stream beside the barotropic solver,
  // or held back until the solve has finished and launched then with the barotropic velocity added on the way out.  Nothing between here and
  // baroclinic_correct_adjust reads U, V(new); a caller that does (any field access: join_side) gets the plain kernel first.
  if (c->f.vmixu == VMIXU_DEFERRED) c->vmixu_deferred = true;
  else if (c->f.vmixu == VMIXU_SIDE) {
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
    if (phase_impvmixu(c, c->side)) return 1;
    HIPCHK(c, hipEventRecord(c->ev_vmixu, c->side));
    c->vmixu_pending = true;
  } else if (phase_impvmixu(c, nullptr)) return 1;
  if (c->diag.run_cfl && diag_cfl(c)) return 1;   // cfl_check (baroclinic.F90:1203)
  if (c->moc.active && moc_site(c)) return 1;     // the binned sums of compute_moc from the U, V, DH advt saw
  HIPCHK(c, hipGetLastError());
  return 0;
}

int pop_solver_run(pop_ctx *c) {
  if (need_device(c)) return 1;
  return solver_run(c);
}
int pop_solver_preconditioner(pop_ctx *c, const char *x_name, int x_tl, const char *px_name, int px_tl) {
  if (need_device(c)) return 1;
  if (join_side(c)) return 1;
  double *x, *px; long long cnt, a2 = (long long)c->g.n2 * c->g.nblocks;
  if (resolve(c, x_name, x_tl, 0, &x, &cnt) || cnt != a2) return unknown(c, "unknown 2-D field ", x_name);
  if (resolve(c, px_name, px_tl, 0, &px, &cnt) || cnt != a2 || px == x) return unknown(c, "unknown 2-D field ", px_name);
  HIPCHK(c, hipMemsetAsync(px, 0, sizeof(double) * a2, c->stream));
  if (c->use_evp) return evp_apply(c, x, px, false);   // (any field the caller names: no assumption about its land values)
  HIPCHK(c, hipMemcpyAsync(px, x, sizeof(double) * a2, hipMemcpyDeviceToDevice, c->stream));
  hipLaunchKernelGGL(k_pcsi_precond, dim3((unsigned)((a2 + 255) / 256)), dim3(256), 0, c->stream, c->g, px, (const double *)c->centerWgt, a2);
  HIPCHK(c, hipGetLastError());
  return 0;
}
// grad / div / zcurl of operators.F90 on device fields.  A 3-D field name selects its level-k slab.
int pop_operator(pop_ctx *c, int op, int k, const char *a_name, const char *b_name, int tl, const char *o1_name, const char *o2_name) {
  if (need_device(c)) return 1;
  if (join_side(c)) return 1;
  if (op < 0 || op > 2 || k < 1 || k > c->g.km) { c->err = "pop_operator: op 0 grad, 1 div, 2 zcurl; 1 <= k <= km"; return 1; }
  const long long a2 = (long long)c->g.n2 * c->g.nblocks, a3 = (long long)c->g.n3 * c->g.nblocks;
  auto slab = [&](const char *name, int t, double **p, long long *stride) -> int {
    long long cnt;
    if (!name || resolve(c, name, t, 0, p, &cnt) || (cnt != a2 && cnt != a3)) return unknown(c, "pop_operator: unknown field ", name ? name : "(null)");
    *stride = cnt == a3 ? c->g.n3 : c->g.n2;
    if (cnt == a3) *p += (long long)(k - 1) * c->g.n2;
    return 0;
  };
  double *A, *B, *O1, *O2 = nullptr; long long sa, sb, so1, so2 = 0;
  if (slab(a_name, tl, &A, &sa)) return 1;
  B = A; sb = sa;
  if (op != 0 && slab(b_name, tl, &B, &sb)) return 1;
  if (slab(o1_name, tl, &O1, &so1)) return 1;
  if (op == 0 && slab(o2_name, tl, &O2, &so2)) return 1;
  if (sb != sa || (op == 0 && so2 != so1)) { c->err = "pop_operator: the two inputs (outputs) must have the same rank"; return 1; }
  hipLaunchKernelGGL(k_operator, dim3((c->g.n2 + 255) / 256, c->g.nblocks), dim3(256), 0, c->stream, c->g, op, k,
                     (const double *)A, (const double *)B, O1, O2 ? O2 : O1, sa, so1, 0);
  HIPCHK(c, hipGetLastError());
  return 0;
}
int pop_operator_host(pop_ctx *c, int op, int k, int block_local, const double *a, const double *b, double *o1, double *o2) {
  if (need_device(c)) return 1;
  if (join_side(c)) return 1;
  if (op < 0 || op > 2 || k < 1 || k > c->g.km) { c->err = "pop_operator_host: op 0 grad, 1 div, 2 zcurl; 1 <= k <= km"; return 1; }
  if (block_local < 1 || block_local > c->g.nblocks) { c->err = "pop_operator_host: block_local is this_block%local_id, 1 .. nblocks"; return 1; }
  if (!a || !o1 || (op != 0 && !b) || (op == 0 && !o2)) { c->err = "pop_operator_host: grad(F -> GRADX, GRADY), div / zcurl(UX, UY -> one field)"; return 1; }
  const size_t n2 = (size_t)c->g.n2;
  if (!c->op_scratch && dev_alloc(c, &c->op_scratch, 4 * n2)) return 1;
  double *A = c->op_scratch, *B = A + n2, *O1 = B + n2, *O2 = O1 + n2;
  HIPCHK(c, hipMemcpyAsync(A, a, n2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (op != 0) HIPCHK(c, hipMemcpyAsync(B, b, n2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_operator, dim3((c->g.n2 + 255) / 256, 1), dim3(256), 0, c->stream, c->g, op, k,
                     (const double *)A, (const double *)(op != 0 ? B : A), O1, O2, 0LL, 0LL, block_local - 1);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(o1, O1, n2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (op == 0) HIPCHK(c, hipMemcpyAsync(o2, O2, n2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
int pop_solver_get_diagnostics(const pop_ctx *c, int *it, double *rms) {
  if (it) *it = c->numIterations;
  if (rms) *rms = c->rmsResidual;
  return 0;
}

static int barotropic_driver(pop_ctx *c, bool update_zx_zy);
int pop_barotropic_driver(pop_ctx *c) { return barotropic_driver(c, true); }
// barotropic.F90:267 on its own: the caller has already updated the halos of ZX, ZY (step_mod.F90:405-423).  Beyond a tripole
// fold a second update would not be a no-op (the symmetrised top row takes each sign from the partner point).
int pop_barotropic_driver_updated(pop_ctx *c) { return barotropic_driver(c, false); }
static int barotropic_driver(pop_ctx *c, bool update_zx_zy) {
  if (need_device(c)) return 1;
  ScopedPhase ph(c, "BAROTROPIC");
  const StepParams sp = step_params(c);
  if (update_zx_zy && halo_update_many(c, {{c->ZX, 1, 1, 1}, {c->ZY, 1, 1, 1}})) return 1;   // NE corner, vector (step_mod.F90:405-423)
  BtropArgs a{};
  a.ZX = c->ZX; a.ZY = c->ZY; a.GXC = c->GX[c->curt]; a.GXO = c->GX[c->oldt]; a.GYC = c->GY[c->curt]; a.GYO = c->GY[c->oldt];
  a.UBO = c->UB[c->oldt]; a.VBO = c->VB[c->oldt]; a.PCUR = c->PS[c->curt]; a.FW = c->FW; a.PGUESS = c->PGUESS;
  a.UH = c->UH; a.VH = c->VH; a.W3 = c->W3; a.W4 = c->W4; a.RHS = c->RHS; a.centerWgt = c->centerWgt; a.PNEW = c->PS[c->newt];
  a.GXN = c->GX[c->newt]; a.GYN = c->GY[c->newt]; a.UBN = c->UB[c->newt]; a.VBN = c->VB[c->newt];
  a.GXR = c->leapfrogts ? c->GX[c->oldt] : c->GX[c->curt]; a.GYR = c->leapfrogts ? c->GY[c->oldt] : c->GY[c->curt];
  a.scal = &c->sc->xcheck; a.rcheck = c->h.rcheck; a.rconst = c->h.rconst;
  const dim3 G(col_grid(c->g, 256), c->g.nblocks), B(256);
  hipLaunchKernelGGL(k_btrop_rhs1, G, B, 0, c->stream, c->g, sp, a);
  hipLaunchKernelGGL(k_btrop_rhs2, G, B, 0, c->stream, c->g, sp, a);
  if (halo_update(c, c->RHS, 1)) return 1;
  solve_collect(c);
  if (!c->ev_solve[0] && (new_event(c, &c->ev_solve[0], hipEventDefault) || new_event(c, &c->ev_solve[1], hipEventDefault))) return 1;
  HIPCHK(c, hipEventRecord(c->ev_solve[0], c->stream));
  const int e = pop_solver_run(c);
  if (e) return e;
  HIPCHK(c, hipEventRecord(c->ev_solve[1], c->stream));
  c->solve_pending = true; c->solve_iters_pending = c->numIterations;
  hipLaunchKernelGGL(k_dot_partial, grid_2d(c), dim3(POP_RED_THREADS), 0, c->stream, c->g, c->PS[c->newt], c->g.CHECKER, (const double *)nullptr, c->partial);
  if (reduce_finish<1>(c, FIN_XCHECK)) return 1;
  hipLaunchKernelGGL(k_btrop_fin1, G, B, 0, c->stream, c->g, a);
  hipLaunchKernelGGL(k_btrop_fin2, G, B, 0, c->stream, c->g, sp, a);
  if (halo_update_many(c, {{c->PS[c->newt], 1}, {c->GX[c->newt], 1, 1, 1}, {c->GY[c->newt], 1, 1, 1}})) return 1;   // barotropic.F90:699-729
  if (c->tavg.active && tavg_site(c, TS_BTROP)) return 1;   // barotropic.F90:687-693
  HIPCHK(c, hipGetLastError());
  return 0;
}

int pop_baroclinic_correct_adjust(pop_ctx *c) {
  if (need_device(c)) return 1;
  ScopedPhase ph(c, "CORRECT_ADJUST");
  // the barotropic velocity is added to U, V(new) (step_mod.F90:572-600) on the side stream while the tracer corrector runs:
  // same sum at every cell; the halo update of U, V in the step tail then carries it to the ghost cells.  Not beyond a
  // tripole fold: there the update symmetrises |U| of the degenerate top row, which does not commute with the sum, so the
  // reference's order (halo updates first, step_mod.F90:467-513, then the sum over whole blocks) is kept.
  if (c->vmixu_deferred) {   // implicit vertical mixing of U, V and the sum in one launch (see pop_baroclinic_driver)
    c->vmixu_deferred = false;
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
    ImpvmixuArgs a{c->U[c->newt], c->V[c->newt], c->E3, c->U[c->oldt], c->V[c->oldt], c->VVC, c->UB[c->newt], c->VB[c->newt]};
    launch_impvmixu_add(c->g, step_params(c), a, grid_cols(c), c->side, c->f.impvmixu_waves);
    HIPCHK(c, hipEventRecord(c->ev_vmixu, c->side));
    c->vmixu_pending = true; c->btrop_added = true;
  } else if (!c->f.btrop_inline) {
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
    if (phase_add_btrop(c, c->side)) return 1;
    HIPCHK(c, hipEventRecord(c->ev_vmixu, c->side));
    c->vmixu_pending = true; c->btrop_added = true;
  }
  if (phase_correct(c)) return 1;
  // increment_tlast_ice (baroclinic.F90:1253: on every step, whatever ice_freq_opt says), then ice on the new tracers once the corrector
  // has solved (:1442-1450; under the Robert filter step_rf forms it).  The kernel also leaves the final density of the levels it
  // changed; reset_passive_tracers, which phase_correct has already done, touches no tracer that ice formation touches.
  if (c->ice.inited) c->ice.tlast_ice = c->ice.tlast_ice + c->h.dtt * ice_time_weight(c);
  if (c->ice.liceform && c->h.c.tmix_opt != 3 && phase_ice(c, c->newt)) return 1;
  HIPCHK(c, hipGetLastError());
  return 0;
}

// step_RF (step_mod.F90:919-1350): Robert-Asselin-Williams filter of curtime (and newtime) with the
// volume-conserving adjustment of PSURF and the tracers, then the leapfrog index rotation
static int step_rf(pop_ctx *c) {
  const HostModel &h = c->h;
  const int o = c->oldt, cu = c->curt, nw = c->newt, nt = h.nt;
  const long long a2 = (long long)c->g.n2 * c->g.nblocks, a3 = (long long)c->g.n3 * c->g.nblocks;
  RfParams p{h.robert_newtime, h.robert_curtime, h.rf_nonzero_newtime, h.dz[1], GRAV};
  auto filt = [&](double *const F[3], long long n) {
    hipLaunchKernelGGL(k_rf_filter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, (const double *)F[o], F[cu], F[nw], p);
  };
  filt(c->UB, a2); filt(c->VB, a2); filt(c->GX, a2); filt(c->GY, a2); filt(c->U, a3); filt(c->V, a3);
  double *WORKN[2] = {c->W3, c->W4}, *WB = c->UH;          // 2-D work arrays free at this point of the step
  RfTracerArgs ta{};
  RfSurfArgs sa{};
  sa.PO = c->PS[o]; sa.PC = c->PS[cu]; sa.PN = c->PS[nw];
  const dim3 GC = grid_cols(c);
  double svol[MAXNT] = {};
  auto sum = [&](const double *F, const double *mask, double *result) { return masked_sum(c, F, nullptr, mask, false, result); };
  // a pair of tracers per pass through the two work arrays: (T, S), then the passive tracers; every pass reads PSURF as it is before its filter
  for (int n0 = 0; n0 < nt; n0 += 2) {
    const int np = std::min(2, nt - n0);
    for (int s = 0; s < np; ++s) {
      const int n = n0 + s;
      ta.TO[s] = c->TR[n][o]; ta.TC[s] = c->TR[n][cu]; ta.TN[s] = c->TR[n][nw]; ta.WORKN[s] = WORKN[s];
      sa.TO[s] = c->TR[n][o]; sa.TC[s] = c->TR[n][cu]; sa.TN[s] = c->TR[n][nw]; sa.WORKN[s] = WORKN[s];
    }
    hipLaunchKernelGGL(k_rf_tracer_interior, dim3(GC.x, GC.y, np), dim3(POP_COL_THREADS), 0, c->stream, c->g, p, ta);
    for (int s = 0; s < np; ++s) if (sum(WORKN[s], nullptr, &svol[n0 + s])) return 1;
    hipLaunchKernelGGL(k_rf_surface, dim3((unsigned)((a2 + 255) / 256), np), dim3(256), 0, c->stream, c->g, p, sa);
    for (int s = 0; s < np; ++s) { double s1; if (sum(WORKN[s], nullptr, &s1)) return 1; svol[n0 + s] = svol[n0 + s] + s1; }
  }
  hipLaunchKernelGGL(k_rf_psurf, dim3((unsigned)((a2 + 255) / 256)), dim3(256), 0, c->stream, c->g, p, (const double *)c->PS[o], c->PS[cu], c->PS[nw], WB);
  double rf_sump;
  if (sum(WB, c->g.CONSTNT, &rf_sump)) return 1;      // MASK_TRBUDGET(:,:,1) = (KMT >= 1) = CONSTNT
  rf_sump = rf_sump / h.bgtarea_t_1;
  hipLaunchKernelGGL(k_rf_psurf_adjust, dim3((unsigned)((a2 + 255) / 256)), dim3(256), 0, c->stream, c->g, p, rf_sump, c->PS[cu], c->PS[nw],
                     c->TR[0][cu], c->TR[0][nw], c->TR[1][cu], c->TR[1][nw], WB);
  for (int n = 2; n < nt; ++n)
    hipLaunchKernelGGL(k_rf_surface_div, dim3((unsigned)((a2 + 255) / 256)), dim3(256), 0, c->stream, c->g, p, (const double *)c->PS[cu], (const double *)c->PS[nw], c->TR[n][cu], c->TR[n][nw]);
  double vsurf, vsurf_oo;
  if (sum(WB, c->g.CONSTNT, &vsurf) || sum(WB, c->g.RCALCT, &vsurf_oo)) return 1;
  const double rf_ocean_norm = h.open_ocean_volume_2_km + vsurf_oo;   // fully coupled normalisation (:1166-1172)
  (void)vsurf;
  for (int n = 0; n < nt; ++n) {
    c->rf_S[n] = svol[n] / rf_ocean_norm;
    const double factor = (!c->rf_S_prev_valid[n] || h.rf_nonzero_newtime) ? c->rf_S[n] : 0.5 * (c->rf_S[n] + c->rf_S_prev[n]);
    hipLaunchKernelGGL(k_rf_conserve, grid_3d(c), dim3(256), 0, c->stream, c->g, p, factor * h.robert_newtime, factor * h.robert_curtime,
                       c->TR[n][cu], c->TR[n][nw]);
  }
  // reset_passive_tracers on TRACER(cur) after the filter, on TRACER(new) when it was filtered too (step_mod.F90:1259-1279)
  if (passive_reset(c, cu) || (h.rf_nonzero_newtime && passive_reset(c, nw))) return 1;
  // ice from the filtered TRACER(cur), then from TRACER(new); AQICE carries from the first call to the second (:1250-1273).  The halo
  // updates of the tail have run, so every ghost cell holds its source cell's inputs and ends with its bits
  if (c->ice.liceform && (phase_ice(c, cu) || phase_ice(c, nw))) return 1;
  HIPCHK(c, hipMemcpyAsync(c->FW_OLD, c->FW, a2 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  launch_state3d(c->g, (const double *)c->TR[0][cu], (const double *)c->TR[1][cu], c->RHO[cu], c->stream);
  launch_state3d(c->g, (const double *)c->TR[0][nw], (const double *)c->TR[1][nw], c->RHO[nw], c->stream);
  if (c->tavg.active && tavg_site(c, TS_TRACER)) return 1;   // step_mod.F90:1290-1298: the tracers after the filter, ice and the new density
  hipLaunchKernelGGL(k_pguess, dim3((unsigned)((a2 + 255) / 256)), dim3(256), 0, c->stream, a2, c->PGUESS, c->PS[nw], c->PS[cu], c->PS[o]);
  c->oldt = cu; c->curt = nw; c->newt = o;                              // step_mod.F90:1318-1322
  if (!h.rf_nonzero_newtime) for (int n = 0; n < nt; ++n) { c->rf_S_prev[n] = c->rf_S[n]; c->rf_S_prev_valid[n] = true; }
  HIPCHK(c, hipGetLastError());
  return 0;
}

int pop_step_tail(pop_ctx *c) {
  if (need_device(c)) return 1;
  ScopedPhase ph(c, "3D-UPDATE");
  const int km = c->g.km;
  if (join_side(c, true)) return 1;
  {   // the seven updates of step_mod.F90:467-560 as one message per neighbour
    std::vector<HaloItem> items = {{c->UB[c->newt], 1, 1, 1}, {c->VB[c->newt], 1, 1, 1}, {c->U[c->newt], km, 1, 1}, {c->V[c->newt], km, 1, 1}, {c->RHO[c->newt], km}};
    for (int n = 0; n < c->h.nt; ++n) items.push_back({c->TR[n][c->newt], km});
    // ice formed on the new tracers before this update (no Robert filter) worked on ghost cells that were not yet current
    if (c->ice.inited && c->h.c.tmix_opt != 3) { items.push_back({c->ice.QICE, 1}); items.push_back({c->ice.AQICE, 1}); items.push_back({c->ice.FWF, 1}); }
    if (halo_update_many(c, items)) return 1;
    c->tr_ghosts_ok[c->newt] = true; c->uv_ghosts_ok[c->newt] = true;
  }
  if (!c->btrop_added && phase_add_btrop(c)) return 1;
  c->btrop_added = false;
  const long long a2 = (long long)c->g.n2 * c->g.nblocks;
  hipLaunchKernelGGL(k_pguess, dim3((a2 + 255) / 256), dim3(256), 0, c->stream, a2, c->PGUESS, c->PS[c->newt], c->PS[c->curt], c->PS[c->oldt]);
  if (c->diag.run_global && diag_global_pre(c)) return 1;   // step_mod.F90:649
  if (c->avg_ts) {
    const int o = c->oldt, cu = c->curt, nw = c->newt;
    Avg2dArgs a{};
    a.UBO = c->UB[o]; a.UBC = c->UB[cu]; a.VBO = c->VB[o]; a.VBC = c->VB[cu]; a.GXO = c->GX[o]; a.GXC = c->GX[cu]; a.GYO = c->GY[o]; a.GYC = c->GY[cu];
    a.PO = c->PS[o]; a.PC = c->PS[cu]; a.PG = c->PGUESS; a.FW_OLD = c->FW_OLD;
    a.UBN = c->UB[nw]; a.VBN = c->VB[nw]; a.GXN = c->GX[nw]; a.GYN = c->GY[nw]; a.PN = c->PS[nw]; a.FW = c->FW;
    for (int n = 0; n < 2; ++n) { a.T1O[n] = c->TR[n][o]; a.T1C[n] = c->TR[n][cu]; a.T1N[n] = c->TR[n][nw]; }
    a.dz1 = c->h.dz[1]; a.grav = GRAV;
    for (int n = 2; n < c->h.nt; n += 2) {   // passive tracers, ahead of k_avg2d, which averages PSURF in place
      const int np = std::min(2, c->h.nt - n);
      AvgPassiveArgs pa{};
      for (int s = 0; s < np; ++s) { pa.TO[s] = c->TR[n + s][o]; pa.TC[s] = c->TR[n + s][cu]; pa.TN[s] = c->TR[n + s][nw]; }
      pa.PO = c->PS[o]; pa.PC = c->PS[cu]; pa.PN = c->PS[nw]; pa.dz1 = a.dz1; pa.grav = a.grav;
      hipLaunchKernelGGL(k_avg_passive, dim3((c->g.n2 + 255) / 256, km, c->g.nblocks * np), dim3(256), 0, c->stream, c->g, pa, np);
    }
    hipLaunchKernelGGL(k_avg2d, dim3(col_grid(c->g, 256), c->g.nblocks), dim3(256), 0, c->stream, c->g, a);
    Avg3dArgs b{};
    b.UO = c->U[o]; b.UC = c->U[cu]; b.VO = c->V[o]; b.VC = c->V[cu]; b.RO = c->RHO[o]; b.RC = c->RHO[cu]; b.UN = c->U[nw]; b.VN = c->V[nw];
    for (int n = 0; n < 2; ++n) { b.TO[n] = c->TR[n][o]; b.TC[n] = c->TR[n][cu]; b.TN[n] = c->TR[n][nw]; }
    hipLaunchKernelGGL(k_avg3d, grid_3d(c), dim3(256), 0, c->stream, c->g, b);
  } else if (c->h.c.tmix_opt == 3) {                                   // step_mod.F90:798-802
    if (step_rf(c)) return 1;
  } else {
    HIPCHK(c, hipMemcpyAsync(c->FW_OLD, c->FW, a2 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    const int tmp = c->oldt; c->oldt = c->curt; c->curt = c->newt; c->newt = tmp;   // step_mod.F90:827-830
  }
  if (c->diag.run_global && diag_global_after(c)) return 1;   // step_mod.F90:860
  HIPCHK(c, hipGetLastError());
  c->tavg.in_step = false;
  c->diag.run_global = c->diag.run_cfl = false;
  return 0;
}

int pop_step(pop_ctx *c) {
  if (need_device(c)) return 1;
  if (c->h.c.ns_boundary == 2 && !c->grid_from_input) { c->err = "time stepping on a tripole decomposition needs the caller's grid (pop_create_with_grid): the internal lat-lon grid has no values beyond the fold"; return 1; }
  ScopedPhase ph(c, "STEP");
  int e;
  if ((e = pop_set_surface_forcing(c)) || (e = pop_time_manager(c)) || (e = pop_dhdt(c)) || (e = pop_baroclinic_driver(c)) || (e = kpp_look_ahead(c)) ||
      (e = pop_barotropic_driver(c)) || (e = pop_baroclinic_correct_adjust(c)) || (e = pop_step_tail(c))) return e;
  return 0;
}

int pop_halo_update(pop_ctx *c, const char *name, int tl, int n) {
  if (need_device(c)) return 1;
  if (join_side(c)) return 1;
  double *p; long long cnt;
  if (n < 0) {   // POP_HaloUpdate4DR8 (mpi/POP_HaloMod.F90:4122-4585): every tracer of a (nx,ny,km,nt,block) field
    if (std::string(name) != "TRACER" && std::string(name) != "KPP_SRC" && std::string(name) != "STF" && std::string(name) != "TFW") {
      c->err = std::string("pop_halo_update: field has no tracer dimension: ") + name; return 1;
    }
    for (int m = 0; m < c->h.nt; ++m) if (pop_halo_update(c, name, tl, m)) return 1;
    return 0;
  }
  if (field_arg(c, name, tl, n, &p, &cnt)) return 1;
  const int nz = (int)(cnt / ((long long)c->g.n2 * c->g.nblocks));
  return halo_update(c, p, nz);
}
int pop_halo_update_loc(pop_ctx *c, const char *name, int tl, int n, int field_loc, int field_kind) {
  if (need_device(c)) return 1;
  if (join_side(c)) return 1;
  if (loc_kind_ok(c, field_loc, field_kind, "pop_halo_update_loc: unknown field location / kind")) return 1;
  double *p; long long cnt;
  if (field_arg(c, name, tl, n < 0 ? 0 : n, &p, &cnt)) return 1;
  const int nz = (int)(cnt / ((long long)c->g.n2 * c->g.nblocks));
  return halo_update(c, p, nz, 0.0, field_loc, field_kind);
}
// host array (nx_block, ny_block, nz, local blocks) staged through a device work field: the update then runs through
// the same plan, kernels and transport as a device-resident field, so it also serves decompositions over several ranks
static int halo_host_staged(pop_ctx *c, double *array, int nz, double fill, int field_loc, int field_kind) {
  if (need_device(c) || join_side(c)) return 1;
  if (nz < 1 || nz > c->g.km) { c->err = "host halo update over several ranks: 1 <= nz <= km (update a 4-D field tracer by tracer)"; return 1; }
  const size_t cnt = (size_t)c->g.n2 * nz * c->g.nblocks;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->S3a, array, cnt * sizeof(double), hipMemcpyHostToDevice));
  if (halo_update(c, c->S3a, nz, fill, field_loc, field_kind)) return 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(array, c->S3a, cnt * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
int pop_halo_update_host_r8_loc(pop_ctx *c, double *array, int nz, double fill, int field_loc, int field_kind) {
  if (loc_kind_ok(c, field_loc, field_kind, "unknown field location / kind")) return 1;
  if (c->h.nranks != 1) return halo_host_staged(c, array, nz, fill, field_loc, field_kind);
  host_halo_r8_loc(c->h, array, nz, fill, field_loc, field_kind);
  return 0;
}
// POP_GlobalSum(array, dist, fieldLoc, errorCode, mMask) on HOST arrays of the local blocks (mpi/POP_ReductionsMod.F90:144-389):
// array and the optional multiplicative mask are staged into 2-D device work fields and summed by the same b4b kernels
// as a device-resident field (field_loc as in pop_global_sum_loc)
int pop_global_sum_host(pop_ctx *c, const double *array, const double *mask, int field_loc, double *result) {
  if (need_device(c) || join_side(c)) return 1;
  if (!array || !result) { c->err = "pop_global_sum_host: null argument"; return 1; }
  const size_t a2 = (size_t)c->g.n2 * c->g.nblocks;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->W3, array, a2 * sizeof(double), hipMemcpyHostToDevice));
  if (mask) HIPCHK(c, hipMemcpy(c->W4, mask, a2 * sizeof(double), hipMemcpyHostToDevice));
  return masked_sum(c, c->W3, nullptr, mask ? c->W4 : nullptr, top_row_once(c, field_loc), result);
}
int pop_halo_update_host_i4_loc(pop_ctx *c, int *array, int nz, int fill, int field_loc, int field_kind) {
  if (single_rank_only(c) || loc_kind_ok(c, field_loc, field_kind, "unknown field location / kind")) return 1;
  host_halo_i4_loc(c->h, array, nz, fill, field_loc, field_kind);
  return 0;
}
// host-array halo: valid for single-rank decompositions (all blocks local), used at init time
int pop_halo_update_host_r8(pop_ctx *c, double *array, int nz, double fill) {
  if (single_rank_only(c)) return 1;
  host_halo_r8(c->h, array, nz, fill);
  return 0;
}
int pop_halo_update_host_i4(pop_ctx *c, int *array, int nz, int fill) {
  if (single_rank_only(c)) return 1;
  host_halo_i4(c->h, array, nz, fill);
  return 0;
}
// POP_GlobalSum with fieldLoc on a tripole grid (mpi/POP_ReductionsMod.F90:308-341): N-face / NE-corner fields count
// the redundant half of the top row once
int pop_global_sum_loc(pop_ctx *c, const char *name, int tl, int n, const char *mask_name, int field_loc, double *result) {
  if (need_device(c)) return 1;
  if (join_side(c)) return 1;
  double *p, *mk; long long cnt;
  if (field_arg(c, name, tl, n, &p, &cnt) || mask_arg(c, mask_name, &mk)) return 1;
  return masked_sum(c, p, nullptr, mk, top_row_once(c, field_loc), result);
}
int pop_global_sum(pop_ctx *c, const char *name, int tl, int n, const char *mask_name, double *result) {
  return pop_global_sum_loc(c, name, tl, n, mask_name, 0, result);
}
// every rank's `nv` values side by side (slot vector + sum all-reduce; exact because the other slots are zero)
static int gather_slots(pop_ctx *c, const double *local, int nv, std::vector<double> &all, const char *who = "global reduction") {
  const int nr = c->h.nranks;
  all.assign((size_t)nv * nr, 0.0);
  if (nr == 1) { std::copy(local, local + nv, all.begin()); return 0; }
  if (!c->allred || !c->redbuf || c->red_doubles < (long long)nv * nr) { c->err = std::string(who) + ": multi-rank run without a transport"; return 1; }
  std::copy(local, local + nv, all.begin() + (size_t)nv * c->h.rank);
  HIPCHK(c, hipMemcpyAsync(c->redbuf, all.data(), sizeof(double) * all.size(), hipMemcpyHostToDevice, c->stream));
  if (c->allred(c->comm_user, 0, (long long)all.size())) { c->err = std::string(who) + ": allreduce failed" + tr_err(c); return 1; }
  HIPCHK(c, hipMemcpyAsync(all.data(), c->redbuf, sizeof(double) * all.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
// POP_GlobalMaxval/Minval (:2670-3223) and Maxloc/Minloc (:4002-4400): value, and the global (i,j) of the first cell
// (block order, then j, then i) that attains it; mask_name selects cells with a non-zero mask value
int pop_global_extreme(pop_ctx *c, const char *name, int tl, int n, const char *mask_name, int want_max, double *value, int *iloc, int *jloc) {
  if (need_device(c)) return 1;
  if (join_side(c)) return 1;
  double *p, *mk; long long cnt;
  if (field_arg(c, name, tl, n, &p, &cnt) || mask_arg(c, mask_name, &mk)) return 1;
  const dim3 G = grid_2d(c);
  with_flags([&](auto MAX) {
    hipLaunchKernelGGL(k_extreme_partial<MAX.value>, G, dim3(POP_RED_THREADS), 0, c->stream, c->g, (const double *)p, (const double *)mk, c->partial);
  }, want_max);
  const size_t np = (size_t)G.x * G.y;
  std::vector<double> part(2 * np);
  HIPCHK(c, hipMemcpyAsync(part.data(), c->partial, sizeof(double) * part.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double best = 0.0, bidx = -1.0;
  for (size_t s = 0; s < np; ++s) {
    const double v = part[2 * s], ix = part[2 * s + 1];
    if (ix < 0.0) continue;
    if (bidx < 0.0 || (want_max ? v > best : v < best) || (v == best && ix < bidx)) { best = v; bidx = ix; }
  }
  // local cell -> global block id, global (i,j)
  double loc3[4] = {0.0, -1.0, 0.0, 0.0};   // value, global block id (ordering key), iGlobal, jGlobal
  if (bidx >= 0.0) {
    const long long q = (long long)bidx;
    const int lb = (int)(q / c->g.n2), p2 = (int)(q % c->g.n2), gb = c->h.local_ids[lb] - 1;
    const BlockInfo &B = c->h.all_blocks[gb];
    loc3[0] = best; loc3[1] = gb; loc3[2] = B.i_glob[p2 % c->g.nxb]; loc3[3] = B.j_glob[p2 / c->g.nxb];
  }
  std::vector<double> all;
  if (gather_slots(c, loc3, 4, all)) return 1;
  int win = -1;
  for (int r = 0; r < c->h.nranks; ++r) {
    if (all[4 * r + 1] < 0.0) continue;
    if (win < 0 || (want_max ? all[4 * r] > all[4 * win] : all[4 * r] < all[4 * win]) || (all[4 * r] == all[4 * win] && all[4 * r + 1] < all[4 * win + 1])) win = r;
  }
  if (win < 0) { c->err = "pop_global_extreme: the mask selects no physical cell"; return 1; }
  if (value) *value = all[4 * win];
  if (iloc) *iloc = (int)all[4 * win + 2];
  if (jloc) *jloc = (int)all[4 * win + 3];
  return 0;
}
// POP_GlobalCount (:2062-2207): non-zero cells of the physical domain (tripole: redundant top-row points of N-face /
// NE-corner fields counted once)
int pop_global_count(pop_ctx *c, const char *name, int tl, int n, int field_loc, long long *count) {
  if (need_device(c)) return 1;
  if (join_side(c)) return 1;
  double *p; long long cnt;
  if (field_arg(c, name, tl, n, &p, &cnt)) return 1;
  const double *dup = top_row_once(c, field_loc) ? c->d2["TRIPOLE_DUP"] : nullptr;
  hipLaunchKernelGGL(k_count_partial, grid_2d(c), dim3(POP_RED_THREADS), 0, c->stream, c->g, (const double *)p, dup, c->partial);
  double ones;
  if (finish_sum<1>(c, FIN_PLAIN, &ones)) return 1;
  *count = (long long)ones;
  return 0;
}
// POP_GlobalSumProd2DR8 (mpi/POP_ReductionsMod.F90:1395-1618): sum of A*B[*mask] over the physical domain
int pop_global_sum_prod(pop_ctx *c, const char *name_a, int tl_a, int n_a, const char *name_b, int tl_b, int n_b,
                        const char *mask_name, double *result) {
  if (need_device(c)) return 1;
  if (join_side(c)) return 1;
  double *pa, *pb, *mk; long long cnt;
  if (field_arg(c, name_a, tl_a, n_a, &pa, &cnt) || field_arg(c, name_b, tl_b, n_b, &pb, &cnt) || mask_arg(c, mask_name, &mk)) return 1;
  return masked_sum(c, pa, pb, mk, false, result);
}
// POP_GlobalSumNfields2DR8 (mpi/POP_ReductionsMod.F90:823-1084): several fields, one result each
int pop_global_sum_nfields(pop_ctx *c, int nf, const char *const *names, const int *tl, const int *n, const char *mask_name, double *results) {
  for (int f = 0; f < nf; ++f)
    if (pop_global_sum(c, names[f], tl ? tl[f] : 1, n ? n[f] : 0, mask_name, results + f)) return 1;
  return 0;
}
// POP_GlobalSumScalarR8 (mpi/POP_ReductionsMod.F90:1091-1191): every rank's value lands in
// its own slot of a zeroed vector, the vector is all-reduced, and the slots are added in rank order
int pop_global_sum_scalar(pop_ctx *c, double local, double *result) {
  const int nr = c->h.nranks;
  if (nr == 1) { *result = local; return 0; }
  if (need_device(c)) return 1;
  std::vector<double> v;
  if (gather_slots(c, &local, 1, v, "pop_global_sum_scalar")) return 1;
  double t = 0.0;
  for (int r = 0; r < nr; ++r) t = t + v[r];
  *result = t;
  return 0;
}
// POP_GlobalSum2DI4 (mpi/POP_ReductionsMod.F90:621-816): init-time integer fields live
// on the host; integer addition is exact in any order, ranks are combined through the scalar sum
int pop_global_sum_i4(pop_ctx *c, const char *name, long long *result) {
  auto it = c->h.i2.find(name);
  if (it == c->h.i2.end()) { c->err = std::string("unknown integer field ") + name; return 1; }
  const HostModel &h = c->h;
  long long s = 0;
  for (int lb = 0; lb < h.nblocks; ++lb) {
    const int *a = it->second.data() + (size_t)(h.local_ids[lb] - 1) * h.n2;
    const BlockInfo &B = h.all_blocks[h.local_ids[lb] - 1];
    for (int j = B.jb - 1; j < B.je; ++j) for (int i = B.ib - 1; i < B.ie; ++i) s += a[(size_t)j * h.nxb + i];
  }
  double tot = 0.0;
  if (pop_global_sum_scalar(c, (double)s, &tot)) return 1;
  *result = (long long)tot;
  return 0;
}
// POP_SolversDiagonal(diagonalCorrection, blockIndx, errorCode) POP_SolversMod.F90:1110-1151
int pop_solver_diagonal(pop_ctx *c, int block_local, const double *diagonal_correction) {
  if (need_device(c)) return 1;
  if (block_local < 1 || block_local > c->h.nblocks) { c->err = "pop_solver_diagonal: block index out of range"; return 1; }
  const int n = (int)c->h.n2;
  const size_t off = (size_t)(block_local - 1) * n;
  HIPCHK(c, hipMemcpyAsync(c->Q + off, diagonal_correction, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));   // Q: solver work array
  hipLaunchKernelGGL(k_solver_diagonal, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->g.WC0 + off, c->Q + off, c->centerWgt + off, n);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
int pop_state_host(pop_ctx *c, int kk, const double *T, const double *S, double *rho, double *drhodt, double *drhods, long long n) {
  if (need_device(c)) return 1;
  return mix_state_host(c->h, c->g, kk, T, S, rho, drhodt, drhods, n, c->stream, c->err);
}

int pop_set_comm(pop_ctx *c, void *sb, void *rb, void *red, long long buf_doubles, pop_exchange_fn x, pop_allreduce_fn ar, void *user) {
  c->sendbuf = (double *)sb; c->recvbuf = (double *)rb; c->comm_doubles = buf_doubles;
  if (red) { c->redbuf = (double *)red; if (c->red_doubles == 0) c->red_doubles = 4LL * c->h.nblocks_tot; }
  c->xchg = x; c->allred = ar; c->comm_user = user;
  return 0;
}
// ---- in-library RCCL transport ------------------------------------------------------------------
int pop_rccl_unique_id(unsigned char *id128) {
  std::string err;
  if (rccl().load(err)) return 1;
  RcclApi::UniqueId id;
  if (rccl().GetUniqueId(&id)) return 1;
  std::memcpy(id128, id.internal, 128);
  return 0;
}
int pop_comm_init_rccl(pop_ctx *c, const unsigned char *id128) {
  if (need_device(c)) return 1;
  if (c->rccl_tr) { c->err = "pop_comm_init_rccl: transport already initialised"; return 1; }
  if (rccl().load(c->err)) return 1;
  RcclApi::UniqueId id;
  std::memcpy(id.internal, id128, 128);
  RcclTransport *t = new RcclTransport();
  const int rc = rccl().CommInitRank(&t->comm, c->h.nranks, id, c->h.rank);
  if (rc) { c->err = "pop_comm_init_rccl: ncclCommInitRank: " + rccl().what(rc); delete t; return 1; }
  c->rccl_tr = t;
  t->stream = &c->stream;
  const long long nb = pop_comm_buffer_doubles(c), nr = std::max<long long>(pop_reduce_buffer_doubles(c), 128);
  if (dev_alloc(c, &t->send, (size_t)nb) || dev_alloc(c, &t->recv, (size_t)nb) || dev_alloc(c, &t->red, (size_t)nr)) return 1;
  c->sendbuf = t->send; c->recvbuf = t->recv; c->comm_doubles = nb;
  c->redbuf = t->red; c->red_doubles = nr;
  c->xchg = rccl_exchange; c->allred = rccl_allreduce; c->comm_user = t;
  // second communicator for exchanges on the side stream (beside an all-reduce on the first).  Its id is made by
  // rank 0 and travels over the first communicator, one byte per double (exact under the sum with the other ranks'
  // zeros), so the host has nothing more to broadcast.  POP_RCCL_OVERLAP=0 keeps everything on one communicator.
  // (POP_RCCL_OVERLAP=2 also creates it on a single rank, so that the whole set-up can be checked against the real librccl)
  const int want2 = c->f.rccl_overlap;
  if (c->f.side_stream && want2 != 0 && (c->h.nranks > 1 || want2 == 2)) {
    std::vector<double> enc(128, 0.0);
    RcclApi::UniqueId id2;
    if (c->h.rank == 0) {
      if (rccl().GetUniqueId(&id2)) { c->err = "pop_comm_init_rccl: ncclGetUniqueId for the second communicator failed"; return 1; }
      for (int b = 0; b < 128; ++b) enc[b] = (double)(unsigned char)id2.internal[b];
    }
    HIPCHK(c, hipMemcpyAsync(t->red, enc.data(), 128 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (rccl_allreduce(t, 0, 128)) { c->err = "pop_comm_init_rccl: broadcasting the second id failed: " + t->err; return 1; }
    HIPCHK(c, hipMemcpyAsync(enc.data(), t->red, 128 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int b = 0; b < 128; ++b) id2.internal[b] = (char)(unsigned char)enc[b];
    const int rc2 = rccl().CommInitRank(&t->comm2, c->h.nranks, id2, c->h.rank);
    if (rc2) { c->err = "pop_comm_init_rccl: second communicator: " + rccl().what(rc2); return 1; }
    if (new_stream(c, &c->comm_side)) return 1;
    t->side = &c->comm_side;
    c->xchg_side = rccl_exchange_side;
  }
  return 0;
}
int pop_comm_info(const pop_ctx *c, int *out6, char *lib_path, int lib_path_bytes) {
  if (!c || !out6) return 1;
  for (int i = 0; i < 6; ++i) out6[i] = 0;
  if (lib_path && lib_path_bytes > 0) lib_path[0] = 0;
  out6[4] = (int)c->peers.size();
  out6[5] = halo_async_ok(c) ? 1 : 0;
  if (c->rccl_tr) {
    out6[0] = 2; out6[1] = out6[2] = -1; out6[3] = c->rccl_tr->comm2 ? -1 : 0;
    RcclApi &a = rccl();
    if (a.CommCount) { a.CommCount(c->rccl_tr->comm, &out6[1]); if (c->rccl_tr->comm2) a.CommCount(c->rccl_tr->comm2, &out6[3]); }
    if (a.CommUserRank) a.CommUserRank(c->rccl_tr->comm, &out6[2]);
    if (lib_path && lib_path_bytes > 0) snprintf(lib_path, (size_t)lib_path_bytes, "%s", a.path.c_str());
  } else if (c->xchg) out6[0] = 1;
  return 0;
}
// transport self-test (also the single-rank check of the RCCL binding): every rank contributes
// rank+1 in slot `rank` of the reduce buffer and passes one value round the ring of ranks
int pop_comm_selftest(pop_ctx *c) {
  if (need_device(c)) return 1;
  if (!c->xchg || !c->allred || !c->redbuf || !c->sendbuf) { c->err = "pop_comm_selftest: no transport installed"; return 1; }
  const int nr = c->h.nranks;
  if (c->red_doubles < nr) { c->err = "pop_comm_selftest: reduce buffer too small"; return 1; }
  std::vector<double> v(nr, 0.0);
  v[c->h.rank] = c->h.rank + 1.0;
  // pageable host memory: blocking copies bracketed by stream synchronisation (an asynchronous copy from / to a std::vector is
  // only ordered with the stream once its staging has happened)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->redbuf, v.data(), sizeof(double) * nr, hipMemcpyHostToDevice));
  if (c->allred(c->comm_user, 0, nr)) { c->err = "pop_comm_selftest: allreduce failed" + (c->rccl_tr ? ": " + c->rccl_tr->err : std::string()); return 1; }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(v.data(), c->redbuf, sizeof(double) * nr, hipMemcpyDeviceToHost));
  const double probe = 1000.0 + c->h.rank;
  double back = 0.0;
  HIPCHK(c, hipMemcpy(c->sendbuf, &probe, sizeof(double), hipMemcpyHostToDevice));
  // ring: one value to rank+1, one from rank-1 (a self message on one rank)
  const int nxt = (c->h.rank + 1) % nr, prv = (c->h.rank + nr - 1) % nr;
  const int peer[2] = {nxt, prv};
  const long long z2[2] = {0, 0}, sc1[2] = {1, 0}, rc1[2] = {nxt == prv ? 1 : 0, 1};
  if (c->xchg(c->comm_user, nxt == prv ? 1 : 2, peer, z2, sc1, z2, rc1)) { c->err = "pop_comm_selftest: exchange failed" + (c->rccl_tr ? ": " + c->rccl_tr->err : std::string()); return 1; }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(&back, c->recvbuf, sizeof(double), hipMemcpyDeviceToHost));
  for (int r = 0; r < nr; ++r) if (v[r] != r + 1.0) {
    char msg[160]; snprintf(msg, sizeof msg, "pop_comm_selftest: all-reduce returned a wrong sum (slot %d holds %.17g, expected %d)", r, v[r], r + 1);
    c->err = msg; return 1;
  }
  if (back != 1000.0 + prv) { c->err = "pop_comm_selftest: ring send/recv returned a wrong value"; return 1; }
  if (c->xchg_side && c->comm_side) {   // the same ring through the second communicator on its own stream, beside an all-reduce on the first
    const double probe2 = 2000.0 + c->h.rank;
    double back2 = 0.0;
    HIPCHK(c, hipMemcpyAsync(c->sendbuf, &probe2, sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->comm_side, c->ev_fork, 0));
    if (c->xchg_side(c->comm_user, nxt == prv ? 1 : 2, peer, z2, sc1, z2, rc1)) { c->err = "pop_comm_selftest: side-stream exchange failed" + tr_err(c); return 1; }
    if (c->allred(c->comm_user, 0, nr)) { c->err = "pop_comm_selftest: allreduce beside the side-stream exchange failed" + tr_err(c); return 1; }
    HIPCHK(c, hipStreamSynchronize(c->comm_side));
    HIPCHK(c, hipMemcpyAsync(&back2, c->recvbuf, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (back2 != 2000.0 + prv) { c->err = "pop_comm_selftest: side-stream ring send/recv returned a wrong value"; return 1; }
  }
  return 0;
}

int pop_set_reduce_buffer(pop_ctx *c, void *dev_redbuf, long long doubles) { c->redbuf = (double *)dev_redbuf; c->red_doubles = doubles; return 0; }
long long pop_reduce_buffer_doubles(const pop_ctx *c) {
  long long n = 4LL * c->h.nblocks_tot;
  if (c->f.replicated) n = std::max(n, 2LL * (long long)c->h.n2 * c->h.nblocks_tot);
  return n;
}
int pop_set_stream(pop_ctx *c, void *hip_stream) {   // run on the host framework's stream (e.g. torch's current stream)
  if (need_device(c)) return 1;
  if (c->own_stream && c->stream) { hipStreamSynchronize(c->stream); hipStreamDestroy(c->stream); }
  c->stream = (hipStream_t)hip_stream; c->own_stream = false;
  return 0;
}
long long pop_comm_buffer_doubles(const pop_ctx *c) {
  long long cells = 0;
  for (auto &p : c->h.halo.peers) cells += (long long)std::max(p.send_src.size(), p.recv_dst.size());
  // the largest message: the end-of-step update of UBTROP, VBTROP, U, V, RHO and the tracers in one piece
  return std::max<long long>(cells * (long long)(2 + (3 + c->h.nt) * std::max(c->h.km, 1)), 4LL * c->h.nblocks_tot);
}
int pop_halo_plan_counts(const pop_ctx *c, int *nl, int *nf, int *np) {
  if (nl) *nl = (int)c->h.halo.copy_dst.size();
  if (nf) *nf = (int)c->h.halo.fill_dst.size();
  if (np) *np = (int)c->h.halo.peers.size();
  return 0;
}
int pop_halo_plan_peer(const pop_ctx *c, int ip, int *rank, int *ns, int *nr) {
  if (ip < 0 || ip >= (int)c->h.halo.peers.size()) return 1;
  const PeerPlan &p = c->h.halo.peers[ip];
  if (rank) *rank = p.rank;
  if (ns) *ns = (int)p.send_src.size();
  if (nr) *nr = (int)p.recv_dst.size();
  return 0;
}
int pop_halo_plan_lists(const pop_ctx *c, int ip, int *send_src, int *recv_dst) {
  if (ip < 0 || ip >= (int)c->h.halo.peers.size()) return 1;
  const PeerPlan &p = c->h.halo.peers[ip];
  if (send_src) std::copy(p.send_src.begin(), p.send_src.end(), send_src);
  if (recv_dst) std::copy(p.recv_dst.begin(), p.recv_dst.end(), recv_dst);
  return 0;
}
int pop_halo_plan_local(const pop_ctx *c, int *dst, int *src, int *fill_dst) {
  const HaloPlan &P = c->h.halo;
  if (dst) std::copy(P.copy_dst.begin(), P.copy_dst.end(), dst);
  if (src) std::copy(P.copy_src.begin(), P.copy_src.end(), src);
  if (fill_dst) std::copy(P.fill_dst.begin(), P.fill_dst.end(), fill_dst);
  return 0;
}

// ---- tidal mixing: tidal_nml and the energy-flux record through an entry point of their own (tidal_mixing.F90 init_tidal_mixing1 / 2)
void pop_tidal_nml_init(pop_tidal_nml *nml) { if (nml) tidal_nml_defaults(*nml); }
int pop_init_tidal_mixing(pop_ctx *c, const pop_tidal_nml *nml, const double *energy_flux, long long count) {
  if (init_arg(c, "pop_init_tidal_mixing", "pop_tidal_nml", sizeof(pop_tidal_nml), nml ? &nml->struct_bytes : nullptr, c && c->tidal.inited) || init_before_steps(c, "pop_init_tidal_mixing")) return 1;
  if (!nml->ltidal_mixing) { c->tidal.inited = true; c->tidal.nml = *nml; return 0; }   // builds nothing
  const pop_config &cf = c->h.c;
  if (cf.vmix_choice != 3) { c->err = "tidal mixing needs vmix_choice = 3 (kpp) (initial.F90:1962)"; return 1; }
  if (cf.bckgrnd_vdc2 != 0.0) { c->err = "tidal mixing needs bckgrnd_vdc2 = 0 (initial.F90:1975)"; return 1; }
  pop_tidal_nml n = *nml;
  if (tidal_nml_resolve(n, c->err)) return 1;
  const size_t a2 = c->h.n2 * c->h.nblocks, a3 = c->h.n3 * c->h.nblocks;
  if (!energy_flux || count != (long long)a2) { c->err = "pop_init_tidal_mixing: count mismatch for the energy flux (nx_block * ny_block * nblocks)"; return 1; }
  std::vector<double> flux(energy_flux, energy_flux + a2);
  if (pop_halo_update_host_r8_loc(c, flux.data(), 1, 0.0, 0, 0)) return 1;   // centre, scalar: the record is read into the physical cells
  if (c->tlon.empty()) host_tlon_build(c->h, c->tlon);
  host_tidal_build(c->h, n, flux.data(), c->tlon, c->tidal.f);
  if (!c->host_only) {
    KppHost *K = (KppHost *)c->mix.kpp;
    TidalDev &td = K->tidal;
    const int km = c->h.km;
    double *p; int *pi;
    if (dev_upload(c, &p, c->tidal.f.coef.data(), a3)) return 1;
    td.COEF = p;
    if (n.ltidal_min_regions) { if (dev_upload(c, &pi, c->tidal.f.box.data(), a2)) return 1; td.BOX = pi; }
    std::vector<double> bvdc(km + 3, 0.0), bvvc_pr(km + 3, 0.0), minval(POP_MAX_TIDAL_MIN_REGIONS + 1, 0.0), zero(km + 3, 0.0);
    std::vector<int> klev(POP_MAX_TIDAL_MIN_REGIONS + 1, 0);
    for (int k = 1; k <= km; ++k) {   // as kpp_create forms them (bckgrnd_vdc2 = 0)
      bvdc[k] = cf.bckgrnd_vdc1 + cf.bckgrnd_vdc2 * std::atan(cf.bckgrnd_vdc_linv * (c->h.zw[k] - cf.bckgrnd_vdc_dpth));
      bvvc_pr[k] = (cf.Prandtl * bvdc[k]) / cf.Prandtl;   // bckgrnd_vvc(k) / Prandtl (vmix_kpp.F90:1826)
    }
    for (int r = 0; r < n.num_tidal_min_regions; ++r) { minval[r + 1] = n.tidal_min_values[r]; klev[r + 1] = n.tidal_min_regions_klevels[r]; }
    if (dev_upload(c, &p, bvdc.data(), bvdc.size())) return 1;
    td.bvdc = p;
    if (dev_upload(c, &p, bvvc_pr.data(), bvvc_pr.size())) return 1;
    td.bvvc_pr = p;
    if (dev_upload(c, &p, minval.data(), minval.size())) return 1;
    td.minval = p;
    if (dev_upload(c, &pi, klev.data(), klev.size())) return 1;
    td.klev = pi;
    if (!K->zero_bck) { if (dev_upload(c, &p, zero.data(), zero.size())) return 1; K->zero_bck = p; }   // pop_init_kpp_bckgrnd may have made it
    td.zgrid = K->dev.zgrid;
    td.mix_max = n.tidal_mix_max; td.prandtl = cf.Prandtl;
    td.lmax = n.ltidal_max ? 1 : 0; td.stabc = (n.ltidal_stabc && !n.lccsm_control_compatible) ? 1 : 0;
    if (n.tidal_diag) {
      if (dev_alloc(c, &td.DIFF, a3) || dev_alloc(c, &td.N2, a3) || dev_alloc(c, &td.KV, a3) || dev_alloc(c, &td.KVM, a3)) return 1;
    }
    K->tidal_on = true;
  }
  c->tidal.nml = n; c->tidal.inited = true; c->tidal.on = true;
  return 0;
}

// ---- latitude-varying KPP background diffusivity (the lhoriz_varying_bckgrnd branch of init_vmix_kpp, vmix_kpp.F90:544-611)
void pop_kpp_bckgrnd_nml_init(pop_kpp_bckgrnd_nml *nml) { if (nml) kpp_bckgrnd_nml_defaults(*nml); }
int pop_init_kpp_bckgrnd(pop_ctx *c, const pop_kpp_bckgrnd_nml *nml) {
  if (init_arg(c, "pop_init_kpp_bckgrnd", "pop_kpp_bckgrnd_nml", sizeof(pop_kpp_bckgrnd_nml), nml ? &nml->struct_bytes : nullptr, c && c->bck.inited) || init_before_steps(c, "pop_init_kpp_bckgrnd")) return 1;
  if (!nml->lhoriz_varying_bckgrnd) { c->bck.inited = true; c->bck.nml = *nml; return 0; }   // builds nothing
  const pop_config &cf = c->h.c;
  if (cf.vmix_choice != 3) { c->err = "lhoriz_varying_bckgrnd needs vmix_choice = 3 (kpp): it is a switch of vmix_kpp_nml"; return 1; }
  if (cf.bckgrnd_vdc2 != 0.0) { c->err = "lhoriz_varying_bckgrnd needs bckgrnd_vdc2 = 0 (vmix_kpp.F90:518)"; return 1; }
  if (nml->bckgrnd_vdc_eq < 0.0 || nml->bckgrnd_vdc_psim < 0.0 || nml->bckgrnd_vdc_ban < 0.0) {
    c->err = "lhoriz_varying_bckgrnd: negative parameter (bckgrnd_vdc_eq, bckgrnd_vdc_psim, bckgrnd_vdc_ban)"; return 1;
  }
  const bool own_tlon = c->tlon.empty();
  if (own_tlon) host_tlon_build(c->h, c->tlon);
  host_bckgrnd_build(c->h, *nml, c->tlon, c->bck.f);
  if (!c->host_only) {
    KppHost *K = (KppHost *)c->mix.kpp;
    const size_t a2 = c->h.n2 * c->h.nblocks;
    // a failed upload leaves the context as it was before the call: no host field readable, nothing of KppHost::bck set
    BckDev bd;
    const double *zero_bck = K->zero_bck;   // pop_init_tidal_mixing may have made it
    double *p = nullptr;
    bool bad = dev_upload(c, &p, c->bck.f.vdc.data(), a2) != 0;
    bd.VDC = p;
    bad = bad || dev_upload(c, &p, c->bck.f.vvc.data(), a2);
    bd.VVC = p;
    bad = bad || dev_upload(c, &p, c->bck.f.vvc_pr.data(), a2);
    bd.VVC_PR = p;
    if (!bad && !zero_bck) {
      std::vector<double> zero(c->h.km + 3, 0.0);
      bad = dev_upload(c, &p, zero.data(), zero.size()) != 0;
      zero_bck = p;
    }
    if (bad) {
      c->bck.f = BckgrndFields();
      if (own_tlon) c->tlon.clear();
      return 1;
    }
    K->bck = bd; K->zero_bck = zero_bck; K->bck_on = true;
  }
  c->bck.nml = *nml; c->bck.inited = true; c->bck.on = true;
  return 0;
}

// ---- ideal age (iage_mod.F90): tracer n (1-based, 3 .. nt) gets the module's interior source and surface reset, and starts from 0
int pop_init_iage(pop_ctx *c, int n) {
  if (init_arg(c, "pop_init_iage", nullptr, 0, nullptr, false)) return 1;
  if (n < 3 || n > c->h.nt) { c->err = "pop_init_iage: n is the 1-based number of a passive tracer, 3 .. nt = " + std::to_string(c->h.nt) + " (got " + std::to_string(n) + ")"; return 1; }
  if (c->h.iage[n - 1]) { c->err = "pop_init_iage: tracer " + std::to_string(n) + " is ideal age already (once per tracer)"; return 1; }
  if (init_before_steps(c, "pop_init_iage")) return 1;
  if (!c->host_only) {   // init_iage with init_iage_option 'startup' (iage_mod.F90:176-180): 0 at every time level
    const size_t bytes = (size_t)c->g.n3 * c->g.nblocks * sizeof(double);
    for (int t = 0; t < 3; ++t) HIPCHK(c, hipMemsetAsync(c->TR[n - 1][t], 0, bytes, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  c->h.iage[n - 1] = true;
  return 0;
}

// ---- frazil ice formation (ice.F90)
void pop_ice_nml_init(pop_ice_nml *nml) { if (nml) ice_nml_defaults(*nml); }
int pop_init_ice(pop_ctx *c, const pop_ice_nml *nml) {
  if (init_arg(c, "pop_init_ice", "pop_ice_nml", sizeof(pop_ice_nml), nml ? &nml->struct_bytes : nullptr, c && c->ice.inited)) return 1;
  if (c->cpl.inited) { c->err = "pop_init_ice: after pop_init_coupled_forcing, which took its constants and branches from the ice set-up (call pop_init_ice first)"; return 1; }
  if (init_before_steps(c, "pop_init_ice")) return 1;
  if (ice_nml_check(c->h, *nml, c->err)) return 1;
  pop_ctx::Ice I;
  if (!c->host_only) {
    const size_t a2 = (size_t)c->g.n2 * c->g.nblocks;
    if (dev_alloc(c, &I.QICE, a2) || dev_alloc(c, &I.AQICE, a2) || dev_alloc(c, &I.QFLUX, a2) || dev_alloc(c, &I.FWF, a2)) return 1;
  }
  I.nml = *nml; I.k = ice_consts(*nml); I.tlast_ice = 0.0;
  I.liceform = nml->ice_freq_opt != 0; I.inited = true;
  c->ice = I; c->h.ice = true;
  return 0;
}
int pop_ice_formation(pop_ctx *c, int tl) {
  if (need_device(c)) return 1;
  if (!c->ice.inited) { c->err = "pop_ice_formation needs pop_init_ice"; return 1; }
  if (tl < 0 || tl > 2) { c->err = "pop_ice_formation: tl is 0 old, 1 cur or 2 new"; return 1; }
  // work formed ahead (KPP look-ahead, del4 first Laplacians) read the cur level: it survives ice on the new one only
  if (join_side(c, tl == 2)) return 1;
  c->ran = true;
  if (phase_ice(c, time_index(c, tl))) return 1;
  HIPCHK(c, hipGetLastError());
  return 0;
}
int pop_ice_flx_to_coupler(pop_ctx *c) {
  if (need_device(c)) return 1;
  if (!c->ice.inited) { c->err = "pop_ice_flx_to_coupler needs pop_init_ice"; return 1; }
  if (join_side(c, true)) return 1;
  const pop_ctx::Ice &I = c->ice;
  IceFlxArgs a{};
  a.T = c->TR[0][c->curt]; a.S = c->TR[1][c->curt]; a.PS = c->PS[c->curt];
  a.QICE = I.QICE; a.AQICE = I.AQICE; a.QFLUX = I.QFLUX;
  a.grav = GRAV; a.tlast_ice = I.tlast_ice; a.hflux_factor = I.k.hflux_factor; a.tfz = I.nml.tfreeze_option;
  a.halve = (c->h.c.tmix_opt >= 1 && c->h.c.tmix_opt <= 3) ? 1 : 0;   // avg, avgfit, robert (ice.F90:693-697)
  with_flags([&](auto PBC) {
    hipLaunchKernelGGL(k_ice_flx_to_coupler<PBC.value>, dim3((c->g.n2 + 255) / 256, c->g.nblocks), dim3(256), 0, c->stream, c->g, a);
  }, c->g.pbc != 0);
  HIPCHK(c, hipGetLastError());
  if (c->tavg.active) {   // step_mod.F90:844-849: tavg_increment_sum_qflux(const=tlast_ice), then QFLUX once the flux has been formed
    if (c->tavg.dirty && tavg_build(c)) return 1;
    if (c->tavg.site[TS_QFLUX].cols.n) {
      for (int ns = 1; ns <= TAVG_MAX_STREAMS; ++ns) if (c->tavg.on[ns] && c->tavg.has_qflux[ns]) c->tavg.sum_qflux[ns] = c->tavg.sum_qflux[ns] + I.tlast_ice;
      if (tavg_site(c, TS_QFLUX)) return 1;
    }
  }
  return 0;
}
int pop_ice_export_reset(pop_ctx *c) {   // ocn_import_export.F90:715-717
  if (need_device(c)) return 1;
  if (!c->ice.inited) { c->err = "pop_ice_export_reset needs pop_init_ice"; return 1; }
  const size_t bytes = (size_t)c->g.n2 * c->g.nblocks * sizeof(double);
  c->ice.tlast_ice = 0.0;
  HIPCHK(c, hipMemsetAsync(c->ice.AQICE, 0, bytes, c->stream));
  HIPCHK(c, hipMemsetAsync(c->ice.QICE, 0, bytes, c->stream));
  return 0;
}
int pop_tfreez_host(pop_ctx *c, const double *S, double *TFRZ, long long count) {
  if (!c) return 1;
  if (!c->ice.inited) { c->err = "pop_tfreez_host needs pop_init_ice (tfreeze_option)"; return 1; }
  if (count < 0 || (count > 0 && (!S || !TFRZ))) { c->err = "pop_tfreez_host: bad arguments"; return 1; }
  for (long long q = 0; q < count; ++q) TFRZ[q] = ice_tfreez(c->ice.nml.tfreeze_option, S[q]);
  return 0;
}

// ---- coupled surface forcing (forcing_coupled.F90; launch_forcing.hpp)
void pop_coupled_nml_init(pop_coupled_nml *nml) { if (nml) coupled_nml_defaults(*nml); }
int pop_init_coupled_forcing(pop_ctx *c, const pop_coupled_nml *nml) {
  if (init_arg(c, "pop_init_coupled_forcing", "pop_coupled_nml", sizeof(pop_coupled_nml), nml ? &nml->struct_bytes : nullptr, c && c->cpl.inited) ||
      init_before_steps(c, "pop_init_coupled_forcing", "call it right after pop_create, after pop_init_ice")) return 1;
  CplState s;
  s.nml = *nml;
  if (coupled_nml_resolve(c->h, s.nml, c->err)) return 1;
  const double ocn_ref_salinity = c->ice.inited ? c->ice.nml.ocn_ref_salinity : 34.7;
  s.k = coupled_consts(s.nml, hflux_factor_of(c), ocn_ref_salinity);
  s.fwf = !(c->ice.inited && c->ice.nml.lfw_as_salt_flx);   // sfc_layer_type is 'varthick' throughout (forcing_coupled.F90:740-741)
  s.icefw = s.fwf && c->ice.liceform;                        // :886-887, forcing.F90:417-426
  if (host_qsw_12hr_factor(c->h, s.nml.qsw_distrb_opt, s.nml.nsteps_per_interval, s.qsw, c->err)) return 1;
  if (s.nml.lms_balance) {   // forcing_coupled.F90:845-848: inside the virtual-salt-flux branch only
    if (!c->msb.inited) { c->err = "pop_init_coupled_forcing: lms_balance needs pop_init_ms_balance first (the region table and REGION_MASK)"; return 1; }
    if (s.fwf) { c->err = "pop_init_coupled_forcing: lms_balance needs lfw_as_salt_flx (pop_init_ice): the reference balances the marginal seas in the virtual-salt-flux branch only (forcing_coupled.F90:800-850)"; return 1; }
    s.ms = !c->msb.seas.empty(); s.nseas = (int)c->msb.seas.size();
    const pop_ice_nml &in = c->ice.nml;
    const double sea_ice_salinity = s.nml.sea_ice_salinity != 0.0 ? s.nml.sea_ice_salinity : 4.0, rho_fw = s.nml.rho_fw != 0.0 ? s.nml.rho_fw : 1.0;
    s.c_q = -(1.0e4 / in.latent_heat_fusion) * (ocn_ref_salinity - sea_ice_salinity) / ocn_ref_salinity;   // ms_balance.F90:558-566
    s.c_s = -(1.0e3 / ocn_ref_salinity) * (rho_fw / in.rho_sw);
    s.c_a = 1.0e-4; s.c_t = -ocn_ref_salinity;
  }
  cpl_anglet(c);
  if (!c->host_only && cpl_init_device(c, s)) return 1;
  s.inited = true;
  c->cpl = s;
  return 0;
}
static int region_mask_keep(pop_ctx *c, const int *region_mask_global, const char *who);
int pop_init_ms_balance(pop_ctx *c, const pop_ms_balance_nml *nml, const int *region_mask_global) {
  if (init_arg(c, "pop_init_ms_balance", "pop_ms_balance_nml", sizeof(pop_ms_balance_nml), nml ? &nml->struct_bytes : nullptr, c && c->msb.inited)) return 1;
  if (c->cpl.inited) { c->err = "pop_init_ms_balance: after pop_init_coupled_forcing (call it before)"; return 1; }
  if (init_before_steps(c, "pop_init_ms_balance")) return 1;
  MsBalance M;
  const bool had_mask = !c->region_mask.empty();
  if (region_mask_keep(c, region_mask_global, "pop_init_ms_balance")) return 1;
  if (host_ms_balance_build(c->h, *nml, region_mask_global, M, c->err)) { if (!had_mask) c->region_mask.clear(); return 1; }
  M.region_mask.clear();   // one stored copy: pop_ctx::region_mask
  c->msb = M;
  if (c->tlon.empty()) host_tlon_build(c->h, c->tlon);   // pop_get_field("TLON"): the longitudes the search compared
  return 0;
}
// REGION_MASK as pop_init_transports and pop_init_ms_balance take it: the first call's array is kept, the second call's must equal it
static int region_mask_keep(pop_ctx *c, const int *region_mask_global, const char *who) {
  if (!region_mask_global) return 0;
  const size_t ng = (size_t)c->h.c.nx_global * c->h.c.ny_global;
  if (c->region_mask.empty()) { c->region_mask.assign(region_mask_global, region_mask_global + ng); return 0; }
  for (size_t g = 0; g < ng; ++g)
    if (c->region_mask[g] != region_mask_global[g]) {
      c->err = std::string(who) + ": REGION_MASK differs from the one the earlier init call was given, first at global (i, j) = (" + std::to_string(g % c->h.c.nx_global + 1) + ", " +
               std::to_string(g / c->h.c.nx_global + 1) + "): " + std::to_string(region_mask_global[g]) + " against " + std::to_string(c->region_mask[g]);
      return 1;
    }
  return 0;
}
static int ms_sea_arg(pop_ctx *c, int sea, const char *who) {
  if (!c->msb.inited) { c->err = std::string(who) + " needs pop_init_ms_balance"; return 1; }
  if (sea < 0 || sea >= (int)c->msb.seas.size()) { c->err = std::string(who) + ": sea is 0 .. n_marginal_seas - 1 = " + std::to_string((int)c->msb.seas.size() - 1); return 1; }
  return 0;
}
int pop_ms_balance_info(pop_ctx *c, int sea, int *number, int *npts, double *area, int *warnings, double *transport) {
  if (!c) return 1;
  if (ms_sea_arg(c, sea, "pop_ms_balance_info")) return 1;
  const MsSea &S = c->msb.seas[sea];
  if (number) *number = S.number;
  if (npts) *npts = (int)S.ipts.size();
  if (area) *area = S.area;
  if (warnings) *warnings = S.warn;
  if (transport) {
    *transport = 0.0;
    if (c->cpl.ms && c->cpl.imported) {   // the only call of the coupled forcing that waits for the device
      HIPCHK(c, hipStreamSynchronize(c->stream));
      HIPCHK(c, hipMemcpy(transport, c->cpl.ms_sums + sea, sizeof(double), hipMemcpyDeviceToHost));
    }
  }
  return 0;
}
int pop_ms_balance_points(pop_ctx *c, int sea, int *ipts, int *jpts, double *fracs, long long count) {
  if (!c) return 1;
  if (ms_sea_arg(c, sea, "pop_ms_balance_points")) return 1;
  const MsSea &S = c->msb.seas[sea];
  if (count_is(c, count, (long long)S.ipts.size(), "pop_ms_balance_points")) return 1;
  if (ipts) std::copy(S.ipts.begin(), S.ipts.end(), ipts);
  if (jpts) std::copy(S.jpts.begin(), S.jpts.end(), jpts);
  if (fracs) std::copy(S.fracs.begin(), S.fracs.end(), fracs);
  return 0;
}
int pop_coupled_qsw_factor(pop_ctx *c, double *factor, long long count) {
  if (!c) return 1;
  if (!c->cpl.inited) { c->err = "pop_coupled_qsw_factor needs pop_init_coupled_forcing"; return 1; }
  return copy_out(c, c->cpl.qsw, factor, count, "qsw_12hr_factor");
}
int pop_set_coupled_forcing(pop_ctx *c, const pop_x2o *x2o, long long count) {
  if (need_device(c)) return 1;
  if (!c->cpl.inited) { c->err = "pop_set_coupled_forcing needs pop_init_coupled_forcing"; return 1; }
  if (!x2o || x2o->struct_bytes != (int)sizeof(pop_x2o)) { c->err = "pop_set_coupled_forcing: pop_x2o.struct_bytes is not sizeof(pop_x2o) of this library (" + std::to_string(sizeof(pop_x2o)) + ")"; return 1; }
  if (c->tavg.in_step) { c->err = "pop_set_coupled_forcing: between pop_time_manager and pop_step_tail of a step (the forcing of a step in hand does not change)"; return 1; }
  if (count_is(c, count, (long long)c->g.n2 * c->g.nblocks, "pop_set_coupled_forcing")) return 1;
  if (join_side(c)) return 1;   // work formed ahead (the KPP look-ahead) read the old STF and SHF_QSW
  return cpl_import(c, x2o);
}
int pop_set_surface_forcing(pop_ctx *c) {
  if (!c) return 1;
  if (c->host_only || !cpl_step_active(c)) return 0;
  if (c->tavg.in_step) { c->err = "pop_set_surface_forcing: between pop_time_manager and pop_step_tail of a step (it is the head of a step, step_mod.F90:231)"; return 1; }
  if (join_side(c)) return 1;   // the KPP look-ahead read the SHF_QSW of the step before
  return cpl_step(c);
}
int pop_coupled_info(pop_ctx *c, int *out4, int *n_marginal_seas) {
  if (!c) return 1;
  if (out4) { out4[0] = c->cpl.inited ? 1 : 0; out4[1] = c->cpl.nml.qsw_distrb_opt; out4[2] = c->cpl.nml.nsteps_per_interval; out4[3] = c->cpl.nsteps; }
  if (n_marginal_seas) *n_marginal_seas = (int)c->msb.seas.size();
  return 0;
}

int pop_timers_reset(pop_ctx *c) { c->timers.clear(); c->timing = true; return 0; }
int pop_timer_ms(pop_ctx *c, const char *name, double *ms, int *calls) {
  auto it = c->timers.find(name);
  if (it == c->timers.end()) { if (ms) *ms = 0; if (calls) *calls = 0; return 1; }
  if (ms) *ms = it->second.ms;
  if (calls) *calls = it->second.calls;
  return 0;
}
int pop_device_sync(pop_ctx *c) {
  if (need_device(c)) return 1;
  if (join_side(c)) return 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
// time `reps` launches of one kernel phase with HIP events on the launch stream (state is left as
// the phase leaves it; callers use it between steps for roofline measurement only)
typedef int (*phase_fn_t)(pop_ctx *);
static phase_fn_t phase_by_name(const std::string &p) {
  if (p == "vmix") return phase_vmix;
  if (p == "tracer_rhs") return [](pop_ctx *x) { return phase_tracer_rhs(x); };
  if (p == "passive_rhs") return phase_passive_rhs;
  if (p == "tracer_rhs_fwd") return [](pop_ctx *x) { return phase_tracer_rhs(x, true); };
  if (p == "impvmixt_back") return phase_impvmixt_back;
  if (p == "impvmixt") return phase_impvmixt_pred;
  if (p == "state") return phase_state_new;
  if (p == "momentum_rhs") return [](pop_ctx *x) { return phase_momentum_rhs(x); };
  if (p == "impvmixu") return [](pop_ctx *x) { return phase_impvmixu(x, nullptr); };
  if (p == "correct") return phase_correct;
  if (p == "add_btrop") return [](pop_ctx *x) { return phase_add_btrop(x); };
  if (p == "ice") return [](pop_ctx *x) { return phase_ice(x, x->newt); };   // ice_formation on the new tracers (after pop_init_ice)
  if (p == "hmix_tracer") return [](pop_ctx *x) { return phase_hmix_tracer(x); };
  if (p == "hmix_momentum") return [](pop_ctx *x) { return phase_hmix_momentum(x); };
  // the ordered block sums between the two kernels of a fused pcg iteration (k_block_sums<1>, one workgroup per block), as the
  // solver launches it: timing only (the partial array holds whatever the last solve left)
  // the tavg sites on their own, each once with the weight of the last pop_time_manager (launch_tavg.hpp)
  if (p == "tavg_forcing") return [](pop_ctx *x) { return tavg_site(x, TS_FORCING); };
  if (p == "tavg_state") return [](pop_ctx *x) { return tavg_site(x, TS_STATE); };
  if (p == "tavg_tracer") return [](pop_ctx *x) { return tavg_site(x, TS_TRACER); };
  if (p == "tavg_vmix") return [](pop_ctx *x) { return tavg_site(x, TS_VMIX); };
  if (p == "tavg_hmix") return [](pop_ctx *x) { return tavg_site(x, TS_HMIX); };
  if (p == "tavg_btrop") return [](pop_ctx *x) { return tavg_site(x, TS_BTROP); };
  // the diagnostic sites on their own (launch_diag.hpp): they run when the context is armed or inside an armed step
  if (p == "diag_global_preupdate") return diag_phase_pre;
  if (p == "diag_global_afterupdate") return diag_phase_after;
  if (p == "diag_cfl") return diag_phase_cfl;
  if (p == "tavg_moc") return moc_phase;   // the MOC site on its own, with the weight of the last pop_time_manager (launch_moc.hpp)
  if (p == "tavg_transport") return trn_phase;   // the same for the tracer transports (launch_transport.hpp)
  if (p == "block_sums") return [](pop_ctx *x) { SolveView v = local_view(x); presum(x, v, v.partial, v.blocksum + 2 * v.nblocks_tot); return 0; };
  return nullptr;
}
// one phase of baroclinic_driver / baroclinic_correct_adjust on its own, once, on the launch stream with the step
// parameters pop_time_manager set: the public routines the reference's drivers call (vmix_coeffs vertical_mix.F90:518,
// tracer_update baroclinic.F90:1902 [tracer_rhs for T and S, passive_rhs for n = 3 .. nt; hmix_tracer = the first Laplacian of hdifft_del4], impvmixt
// vertical_mix.F90:1164, state state_mod.F90:258 on the new tracers, clinic baroclinic.F90:1635 [momentum_rhs;
// hmix_momentum = first Laplacian of hdiffu_del4], impvmixu vertical_mix.F90:1679 + baroclinic.F90:1077-1129,
// impvmixt_correct :1460 [correct]).  Lets a caller -- and the parity tests -- drive and check the phases one by one.
int pop_run_phase(pop_ctx *c, const char *phase) {
  if (need_device(c) || join_side(c)) return 1;
  phase_fn_t fn = phase_by_name(phase ? phase : "");
  if (!fn) { c->err = std::string("unknown phase ") + (phase ? phase : "(null)"); return 1; }
  c->ran = true;
  if (fn(c)) return 1;
  HIPCHK(c, hipGetLastError());
  return 0;
}
int pop_time_phase(pop_ctx *c, const char *phase, int reps, double *avg_ms) {
  if (need_device(c) || join_side(c)) return 1;
  const std::string p(phase);
  phase_fn_t fn = phase_by_name(p);
  if (!fn) { c->err = "unknown phase " + p; return 1; }
  c->ran = true;
  struct Events {   // destroyed on every return path
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() { if (e0) hipEventDestroy(e0); if (e1) hipEventDestroy(e1); }
  } ev;
  HIPCHK(c, hipEventCreate(&ev.e0)); HIPCHK(c, hipEventCreate(&ev.e1));
  // the launches of the phase only: the halo update of a first Laplacian formed for the next step (del4, large grids) belongs to
  // the step, not to the kernel, and the fields formed here are not kept
  struct Flag { bool &f; Flag(bool &x) : f(x) { f = true; } ~Flag() { f = false; } } timing(c->phase_timing);
  if (fn(c)) return 1;   // warm
  HIPCHK(c, hipEventRecord(ev.e0, c->stream));
  for (int r = 0; r < reps; ++r) if (fn(c)) return 1;
  HIPCHK(c, hipEventRecord(ev.e1, c->stream));
  HIPCHK(c, hipEventSynchronize(ev.e1));
  float ms = 0; HIPCHK(c, hipEventElapsedTime(&ms, ev.e0, ev.e1));
  c->d2t_next_valid = false; c->d2u_next_valid = false;
  *avg_ms = ms / std::max(reps, 1);
  return 0;
}

// ---- time-averaged output (tavg.F90; kernels_tavg.hpp, launch_tavg.hpp)
static std::string tavg_left_out_hint(const std::string &nm) {   // the slab entries stay left out; the transports have their own request
  return (nm == "N_HEAT" || nm == "N_SALT") ? ".  The northward transports are requested with pop_transport_request and read with pop_transport_get" : "";
}
int pop_tavg_request(pop_ctx *c, int ns, const char *name) {
  if (!c) return 1;
  if (!name) { c->err = "pop_tavg_request: no name"; return 1; }
  if (c->h.plan_only) { c->err = "pop_tavg_request: the context has no fields (POP_CREATE_PLAN_ONLY)"; return 1; }
  if (tavg_stream_ok(c, ns, "pop_tavg_request") || tavg_between_steps(c, "pop_tavg_request")) return 1;
  const std::string nm(name);
  if (nm == "MOC") { c->err = "pop_tavg_request: MOC is not a slab field: it is requested with pop_moc_request(stream) and read with pop_moc_get"; return 1; }
  if (const TavgEntry *e = tavg_find(c, name)) { c->err = "pop_tavg_request: " + nm + " is already requested, in stream " + std::to_string(e->stream) + " (a name belongs to one stream)"; return 1; }
  for (const char *l : tavg_left_out) if (nm == l) { c->err = "pop_tavg_request: " + nm + " is known to the reference, not built (DESIGN.md section 14)" + tavg_left_out_hint(nm); return 1; }
  const std::vector<TavgAvail> avail = tavg_avail(c);
  const TavgAvail *a = nullptr;
  for (const TavgAvail &x : avail) if (x.name == nm) a = &x;
  if (!a) { c->err = "pop_tavg_request: unknown tavg field " + nm; return 1; }
  const std::string miss = tavg_missing(c, a->need);
  if (!miss.empty()) { c->err = "pop_tavg_request: " + nm + " needs " + miss + ": this configuration does not produce its source"; return 1; }
  if ((int)c->tavg.req.size() >= TAVG_MAX_FIELDS) { c->err = "pop_tavg_request: more than POP_TAVG_MAX_FIELDS = " + std::to_string(TAVG_MAX_FIELDS) + " entries (" + nm + ")"; return 1; }
  TavgEntry e;
  e.name = nm; e.stream = ns; e.site = a->site; e.ndims = a->ndims; e.method = a->method; e.kmax = a->kmax;
  e.nlev = a->ndims == 3 ? a->kmax : 1;
  e.expr = a->expr; e.a = a->a; e.b = a->b; e.cst = a->cst; e.cst2 = a->cst2; e.cells = a->cells; e.vint = a->vint;
  if (!c->host_only) {
    if (join_side(c, true)) return 1;
    if (dev_alloc(c, &e.buf, tavg_count(c, e), false) || tavg_fill(c, e)) return 1;
  }
  const bool first = !c->tavg.used[ns];
  c->tavg.req.push_back(e);
  if (first) c->tavg.on[ns] = true;   // tavg_start_opt 'nstep', 0: on from the request
  tavg_refresh_flags(c);
  return 0;
}
int pop_tavg_set_on(pop_ctx *c, int ns, int on) {
  if (!c) return 1;
  if (tavg_stream_ok(c, ns, "pop_tavg_set_on") || tavg_between_steps(c, "pop_tavg_set_on")) return 1;
  c->tavg.on[ns] = on != 0;
  tavg_refresh_flags(c);
  return 0;
}
int pop_tavg_info(pop_ctx *c, const char *name, int *stream, int *ndims, int *nlevels, int *method) {
  if (!c) return 1;
  const std::string nm(name ? name : "");
  if (nm == "MOC") { c->err = "pop_tavg_info: MOC is not a slab field: it is requested with pop_moc_request(stream) and read with pop_moc_get"; return 1; }
  for (const char *l : tavg_left_out) if (nm == l) { c->err = "pop_tavg_info: " + nm + " is known to the reference, not built (DESIGN.md section 14)" + tavg_left_out_hint(nm); return 1; }
  for (const TavgAvail &a : tavg_avail(c)) {
    if (a.name != nm) continue;
    const TavgEntry *e = tavg_find(c, name);
    if (stream) *stream = e ? e->stream : 0;
    if (ndims) *ndims = a.ndims;
    if (nlevels) *nlevels = a.ndims == 3 ? a.kmax : 1;
    if (method) *method = a.method;
    return 0;
  }
  c->err = "pop_tavg_info: unknown tavg field " + nm;
  return 1;
}
int pop_tavg_sums(pop_ctx *c, int ns, double *tavg_sum, double *tavg_sum_qflux) {
  if (!c) return 1;
  if (tavg_stream_ok(c, ns, "pop_tavg_sums")) return 1;
  if (tavg_sum) *tavg_sum = c->tavg.sum[ns];
  if (tavg_sum_qflux) *tavg_sum_qflux = c->tavg.sum_qflux[ns];
  return 0;
}
int pop_tavg_get(pop_ctx *c, const char *name, int normalize, double *host, long long count) {
  if (need_device(c)) return 1;
  const TavgEntry *e = tavg_find(c, name ? name : "");
  if (!e) return unknown(c, "pop_tavg_get: not a requested tavg field: ", name ? name : "(null)");
  if (count_is(c, (long long)tavg_count(c, *e), count, name) || join_side(c, true)) return 1;
  return tavg_to_host(c, *e, normalize != 0, host);
}
void *pop_tavg_device_ptr(pop_ctx *c, const char *name) {
  if (!c || c->host_only) return nullptr;
  const TavgEntry *e = tavg_find(c, name ? name : "");
  return e ? (void *)e->buf : nullptr;
}
int pop_tavg_reset(pop_ctx *c, int ns) {
  if (!c) return 1;
  if (tavg_stream_ok(c, ns, "pop_tavg_reset") || tavg_between_steps(c, "pop_tavg_reset")) return 1;
  return tavg_reset_stream(c, ns);
}
int pop_tavg_write(pop_ctx *c, int ns, const char *path, int restart_type) {
  if (need_device(c) || tavg_stream_ok(c, ns, "pop_tavg_write") || tavg_between_steps(c, "pop_tavg_write") || join_side(c, true)) return 1;
  if (restart_type != 0 && restart_type != 1) { c->err = "pop_tavg_write: restart_type 0 (normalise, write, reset) or 1 (the sums as they are)"; return 1; }
  TavgState &T = c->tavg;
  std::vector<RestartField> fields;
  std::vector<const TavgEntry *> ent;
  int rec = 1;
  for (const TavgEntry &e : T.req) {
    if (e.stream != ns) continue;
    fields.push_back(RestartField{e.name, e.ndims, e.nlev, rec});
    ent.push_back(&e);
    rec += e.nlev;
  }
  if (ent.empty()) { c->err = "pop_tavg_write: stream " + std::to_string(ns) + " holds no entry"; return 1; }
  if (restart_type == 0) { double f; for (const TavgEntry *e : ent) if (tavg_factor(c, *e, &f)) return 1; }   // before anything is written
  const std::vector<RestartAttr> at = {{"title", "char", "POP tavg"}, {"history", "char", "written by libpop_amd"}, {"conventions", "char", "POP binary tavg"},
                                       {"restart_type", "int", std::to_string(restart_type)},
                                       {"tavg_sum", "r8", fmt_r8(T.sum[ns])}, {"tavg_sum_qflux", "r8", fmt_r8(T.sum_qflux[ns])},
                                       {"nsteps_total", "int", std::to_string(c->nsteps_total)}};   // tavg.F90:2003-2007
  auto fetch = [&](size_t i, double *buf) { return tavg_to_host(c, *ent[i], restart_type == 0, buf); };
  if (slab_file_write(c->h, path, at, fields, fetch, "tavg", c->err)) return 1;
  if (restart_type == 0 && c->moc.requested && c->moc.stream == ns && moc_snapshot(c)) return 1;   // write, then reset: the MOC of the interval stays readable
  if (restart_type == 0 && c->trn.requested && c->trn.stream == ns && trn_snapshot(c)) return 1;   // ... and the tracer transports
  return restart_type == 0 ? tavg_reset_stream(c, ns) : 0;
}
int pop_tavg_read(pop_ctx *c, int ns, const char *path) {
  if (need_device(c) || tavg_stream_ok(c, ns, "pop_tavg_read") || tavg_between_steps(c, "pop_tavg_read") || join_side(c, true)) return 1;
  TavgState &T = c->tavg;
  RestartHeader hd;
  if (restart_parse_header(path, hd, c->err)) return 1;
  if (!hd.has("tavg_sum") || !hd.has("tavg_sum_qflux")) { c->err = "pop_tavg_read: header has no tavg_sum / tavg_sum_qflux"; return 1; }
  if (hd.integer("restart_type", 1) != 1) { c->err = "pop_tavg_read: the file holds normalised fields (restart_type 0), not the sums"; return 1; }
  std::vector<RestartField> fields;
  std::vector<const TavgEntry *> ent;
  for (const TavgEntry &e : T.req) {
    if (e.stream != ns) continue;
    int id, ndims;
    if (!hd.find(e.name, RestartHeader::EXACT, &id, &ndims)) { c->err = "could not find field in binary header file: " + e.name; return 1; }
    fields.push_back(RestartField{e.name, e.ndims, e.nlev, id});
    ent.push_back(&e);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  auto store = [&](size_t i, double *buf) {
    const TavgEntry &e = *ent[i];
    if (hipMemcpy(e.buf, buf, tavg_count(c, e) * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { c->err = "tavg: device copy failed"; return 1; }
    return halo_update(c, e.buf, e.nlev, 0.0);
  };
  if (slab_file_read(c->h, path, fields, false, store, c->err)) return 1;
  T.sum[ns] = hd.real("tavg_sum");   // the sums only once every field is in place
  T.sum_qflux[ns] = hd.real("tavg_sum_qflux");
  return 0;
}

// ---- global and CFL diagnostics (diagnostics.F90; kernels_diag.hpp, launch_diag.hpp)
int pop_diag_arm(pop_ctx *c, int want_global, int want_cfl) {
  if (!c) return 1;
  if (c->h.plan_only) { c->err = "pop_diag_arm: the context has no fields (POP_CREATE_PLAN_ONLY)"; return 1; }
  if (c->tavg.in_step) { c->err = "pop_diag_arm: refused between pop_time_manager and pop_step_tail of a step (it arms the next step: call it between steps)"; return 1; }
  c->diag.arm_global = want_global != 0; c->diag.arm_cfl = want_cfl != 0;
  return 0;
}
int pop_diag_global_get(pop_ctx *c, pop_diag_global *out, double *avg_tracer_k, long long count) {
  if (need_device(c)) return 1;
  if (!out || out->struct_bytes != (int)sizeof(pop_diag_global)) { c->err = "pop_diag_global_get: struct_bytes is not sizeof(pop_diag_global)"; return 1; }
  DiagGlobalOut o;
  o.g.struct_bytes = out->struct_bytes;
  if (diag_finish_global(c, "pop_diag_global_get", o)) return 1;
  if (avg_tracer_k && copy_out(c, o.avg_tracer_k, avg_tracer_k, count, "avg_tracer_k")) return 1;
  *out = o.g;
  return 0;
}
int pop_diag_value(pop_ctx *c, const char *name, int n, double *value) {
  if (!c) return 1;
  const std::string nm(name ? name : "");
  for (const char *l : diag_left_out) if (nm == l) { c->err = "pop_diag_value: " + nm + " is known to the reference, not built (DESIGN.md section 15)"; return 1; }
  if (need_device(c)) return 1;
  DiagGlobalOut o;
  if (diag_finish_global(c, "pop_diag_value", o)) return 1;
  const pop_diag_global &g = o.g;
  const struct { const char *name; const double *p; } arrays[] = {{"avg_tracer", g.avg_tracer}, {"sfc_tracer_flux", g.sfc_tracer_flux},
                                                                   {"dtracer_avg", g.dtracer_avg}, {"dtracer_abs", g.dtracer_abs}};
  for (const auto &a : arrays)
    if (nm == a.name) {
      if (n < 0 || n >= c->h.nt) { c->err = "pop_diag_value: " + nm + ": tracer index " + std::to_string(n) + " is outside 0 .. nt-1 = " + std::to_string(c->h.nt - 1); return 1; }
      *value = a.p[n];
      return 0;
    }
  const struct { const char *name; double v; } scalars[] = {{"diag_sealevel", g.diag_sealevel}, {"diag_ke", g.diag_ke}, {"diag_ws", g.diag_ws},
    {"diag_press_free", g.diag_press_free}, {"diag_ke_free", g.diag_ke_free}, {"diag_ke_psfc", g.diag_ke_psfc}, {"rmsResidual", g.rmsResidual},
    {"iterationCount", (double)g.iterationCount}};
  for (const auto &s : scalars) if (nm == s.name) { *value = s.v; return 0; }
  return unknown(c, "pop_diag_value: unknown diagnostic ", nm.c_str());
}
int pop_diag_cfl(pop_ctx *c, const char *name, double *value, int *ijk, double *value_k, int *ij_k, int *nsteps_total) {
  if (need_device(c)) return 1;
  const int q = diag_cfl_index(name ? name : "");
  if (q < 0) return unknown(c, "pop_diag_cfl: unknown CFL number (advu, advv, advw, advt, hdifft, hdiffu, vdifft, vdiffu): ", name ? name : "(null)");
  DiagCflOut o;
  if (diag_finish_cfl(c, q, o)) return 1;
  if (value) *value = o.value;
  if (ijk) std::copy(o.ijk, o.ijk + 3, ijk);
  if (value_k) std::copy(o.value_k.begin(), o.value_k.end(), value_k);
  if (ij_k) std::copy(o.ij_k.begin(), o.ij_k.end(), ij_k);
  if (nsteps_total) *nsteps_total = c->diag.step_cfl;
  return 0;
}
int pop_check_ke(pop_ctx *c, double ke_thresh, int *exceeded) {
  if (!c) return 1;
  if (diag_need_site(c, "pop_check_ke", c->diag.step_after >= 0)) return 1;
  DiagGlobalOut o;
  if (diag_finish_global(c, "pop_check_ke", o)) return 1;
  if (exceeded) *exceeded = (o.g.diag_ke > ke_thresh || o.g.diag_ke < 0) ? 1 : 0;
  return 0;
}
int pop_grid_volumes(pop_ctx *c, double *area_t, double *volume_t, double *volume_u, double *area_t_k, double *volume_t_k) {
  if (!c) return 1;
  if (c->h.plan_only) { c->err = "pop_grid_volumes: the context has no fields (POP_CREATE_PLAN_ONLY)"; return 1; }
  const HostModel &h = c->h;
  if (area_t) *area_t = h.area_t;
  if (volume_t) *volume_t = h.volume_t;
  if (volume_u) *volume_u = h.volume_u;
  if (area_t_k) std::copy(h.area_t_k.begin() + 1, h.area_t_k.end(), area_t_k);
  if (volume_t_k) std::copy(h.volume_t_k.begin() + 1, h.volume_t_k.end(), volume_t_k);
  return 0;
}

// ---- meridional overturning circulation (diags_on_lat_aux_grid.F90; host_lat_aux.cpp, kernels_moc.hpp, launch_moc.hpp)
void pop_transports_nml_init(pop_transports_nml *nml) { if (nml) transports_nml_defaults(*nml); }
int pop_init_transports(pop_ctx *c, const pop_transports_nml *nml, const int *region_mask_global) {
  if (init_arg(c, "pop_init_transports", "pop_transports_nml", sizeof(pop_transports_nml), nml ? &nml->struct_bytes : nullptr, c && c->moc.aux.inited, "called twice")) return 1;
  if (c->ran) { c->err = "pop_init_transports: call it before the first step or phase"; return 1; }
  LatAux aux;
  const bool had_mask = !c->region_mask.empty();
  if (region_mask_keep(c, region_mask_global, "pop_init_transports")) return 1;
  if (host_lat_aux_build(c->h, *nml, region_mask_global, aux, c->err)) { if (!had_mask) c->region_mask.clear(); return 1; }
  c->moc.aux = std::move(aux);
  return 0;
}
int pop_lat_aux_grid(pop_ctx *c, int *n, double *edge, double *center) {
  if (!c || moc_inited(c, "pop_lat_aux_grid")) return 1;
  const LatAux &A = c->moc.aux;
  if (n) *n = A.n_lat;
  if (edge) std::copy(A.edge.begin(), A.edge.end(), edge);
  if (center) std::copy(A.center.begin(), A.center.end(), center);
  return 0;
}
int pop_moc_info(pop_ctx *c, int *n_lat, int *km1, int *n_comp, int *n_reg) {
  if (!c || moc_inited(c, "pop_moc_info")) return 1;
  if (n_lat) *n_lat = c->moc.aux.n_lat;
  if (km1) *km1 = c->h.km + 1;
  if (n_comp) *n_comp = c->moc.aux.n_comp;
  if (n_reg) *n_reg = c->moc.aux.n_reg;
  return 0;
}
int pop_moc_mask(pop_ctx *c, int *mask, long long count) {
  if (!c || moc_inited(c, "pop_moc_mask")) return 1;
  return copy_out(c, c->moc.aux.mask, mask, count, "MASK_LAT_DEPTH");
}
int pop_moc_bin_map(pop_ctx *c, int *bins, long long count) {
  if (!c || moc_inited(c, "pop_moc_bin_map")) return 1;
  return copy_out(c, c->moc.aux.bin_map, bins, count, "the bin map");
}
int pop_moc_request(pop_ctx *c, int ns) {
  if (!c) return 1;
  if (c->h.plan_only) { c->err = "pop_moc_request: the context has no fields (POP_CREATE_PLAN_ONLY)"; return 1; }
  if (tavg_stream_ok(c, ns, "pop_moc_request") || tavg_between_steps(c, "pop_moc_request") || moc_inited(c, "pop_moc_request")) return 1;
  if (c->moc.requested) { c->err = "pop_moc_request: MOC is already requested, in stream " + std::to_string(c->moc.stream); return 1; }
  if (!c->host_only && (join_side(c, true) || moc_alloc(c))) return 1;
  const bool first = !c->tavg.used[ns];
  c->moc.requested = true; c->moc.stream = ns;
  if (first) c->tavg.on[ns] = true;   // as the first pop_tavg_request of a stream
  tavg_refresh_flags(c);
  return 0;
}
int pop_moc_get(pop_ctx *c, int normalize, int which, double *out, long long count) {
  if (need_device(c) || moc_inited(c, "pop_moc_get")) return 1;
  if (!c->moc.requested) { c->err = "pop_moc_get: pop_moc_request has not been called"; return 1; }
  if (which != 0 && which != 1) { c->err = "pop_moc_get: which 0 (the running interval) or 1 (the snapshot of pop_tavg_write)"; return 1; }
  if (count_is(c, (long long)moc_n_out(c), count, "MOC")) return 1;
  if (which == 1) {
    if (!c->moc.have_snap) { c->err = "pop_moc_get: no snapshot yet: pop_tavg_write(stream, path, 0) of the MOC's stream takes it"; return 1; }
    std::copy(c->moc.snap.begin(), c->moc.snap.end(), out);
    return 0;
  }
  double factor;
  std::vector<double> sums;
  if (moc_factor(c, normalize, &factor) || join_side(c, true) || moc_reduce(c, sums)) return 1;
  moc_finish(c, sums, factor, out);
  return 0;
}
long long pop_moc_sums_count(pop_ctx *c) { return (c && c->moc.aux.inited) ? (long long)moc_n_sums(c) : -1; }
int pop_moc_sums_get(pop_ctx *c, double *sums, long long count) {
  if (need_device(c) || moc_inited(c, "pop_moc_sums_get")) return 1;
  if (!c->moc.requested) { c->err = "pop_moc_sums_get: pop_moc_request has not been called"; return 1; }
  std::vector<double> s;
  if (count_is(c, (long long)moc_n_sums(c), count, "the MOC sums") || join_side(c, true) || moc_reduce(c, s)) return 1;
  std::copy(s.begin(), s.end(), sums);
  return 0;
}
int pop_moc_sums_set(pop_ctx *c, const double *sums, long long count) {
  if (need_device(c) || moc_inited(c, "pop_moc_sums_set")) return 1;
  if (!c->moc.requested) { c->err = "pop_moc_sums_set: pop_moc_request has not been called"; return 1; }
  if (tavg_between_steps(c, "pop_moc_sums_set") || count_is(c, (long long)moc_n_sums(c), count, "the MOC sums")) return 1;
  if (moc_reset(c)) return 1;   // the vector replaces the sums of the interval
  c->moc.set_sums.assign(sums, sums + count);
  return 0;
}

// ---- northward heat and salt transports (compute_tracer_transports; kernels_transport.hpp, launch_transport.hpp)
int pop_transport_request(pop_ctx *c, int ns, int heat, int salt) {
  if (!c) return 1;
  if (c->h.plan_only) { c->err = "pop_transport_request: the context has no fields (POP_CREATE_PLAN_ONLY)"; return 1; }
  if (tavg_stream_ok(c, ns, "pop_transport_request") || tavg_between_steps(c, "pop_transport_request") || moc_inited(c, "pop_transport_request")) return 1;
  if (c->trn.requested) { c->err = "pop_transport_request: the transports are already requested, in stream " + std::to_string(c->trn.stream); return 1; }
  if (!heat && !salt) { c->err = "pop_transport_request: neither heat nor salt is asked for"; return 1; }
  if (c->h.c.tadvect == 3 && c->moc.aux.n_reg > 1) {
    c->err = "pop_transport_request: tadvect = 3 (lw_lim) with n_transport_reg = 2: the north-face value of lw_lim is not kept, so the southern-boundary transport of region 2 cannot be formed (one region is built)";
    return 1;
  }
  c->trn.n_comp = trn_n_comp(c->h.c);
  if (!c->host_only && (join_side(c, true) || trn_alloc(c))) return 1;
  const bool first = !c->tavg.used[ns];
  c->trn.requested = true; c->trn.stream = ns; c->trn.want[0] = heat != 0; c->trn.want[1] = salt != 0;
  if (first) c->tavg.on[ns] = true;   // as the first pop_tavg_request of a stream
  tavg_refresh_flags(c);
  return 0;
}
int pop_transport_info(pop_ctx *c, int *n_lat, int *n_comp, int *n_reg, int *stream, int *heat, int *salt) {
  if (!c || moc_inited(c, "pop_transport_info")) return 1;
  if (n_lat) *n_lat = c->moc.aux.n_lat;
  if (n_comp) *n_comp = trn_n_comp(c->h.c);
  if (n_reg) *n_reg = c->moc.aux.n_reg;
  if (stream) *stream = c->trn.requested ? c->trn.stream : 0;
  if (heat) *heat = c->trn.want[0];
  if (salt) *salt = c->trn.want[1];
  return 0;
}
static int trn_requested(pop_ctx *c, const char *who) {
  if (need_device(c) || moc_inited(c, who)) return 1;
  if (!c->trn.requested) { c->err = std::string(who) + ": pop_transport_request has not been called"; return 1; }
  return 0;
}
int pop_transport_get(pop_ctx *c, int tracer, int normalize, int which, double *out, long long count) {
  if (trn_requested(c, "pop_transport_get")) return 1;
  if ((tracer != 1 && tracer != 2) || !c->trn.want[tracer - 1]) { c->err = "pop_transport_get: tracer 1 (heat) or 2 (salt), as pop_transport_request asked for"; return 1; }
  if (which != 0 && which != 1) { c->err = "pop_transport_get: which 0 (the running interval) or 1 (the snapshot of pop_tavg_write)"; return 1; }
  if (count_is(c, (long long)trn_n_out(c), count, tracer == 1 ? "N_HEAT" : "N_SALT")) return 1;
  if (which == 1) {
    if (!c->trn.have_snap) { c->err = "pop_transport_get: no snapshot yet: pop_tavg_write(stream, path, 0) of the transports' stream takes it"; return 1; }
    std::copy(c->trn.snap[tracer - 1].begin(), c->trn.snap[tracer - 1].end(), out);
    return 0;
  }
  double factor;
  std::vector<double> sums;
  if (trn_factor(c, normalize, &factor) || join_side(c, true) || trn_reduce(c, sums)) return 1;
  trn_finish(c, sums, factor, tracer - 1, out);
  return 0;
}
long long pop_transport_sums_count(pop_ctx *c) { return (c && c->moc.aux.inited) ? (long long)trn_n_sums(c) : -1; }
int pop_transport_sums_get(pop_ctx *c, double *sums, long long count) {
  if (trn_requested(c, "pop_transport_sums_get")) return 1;
  std::vector<double> s;
  if (count_is(c, (long long)trn_n_sums(c), count, "the transport sums") || join_side(c, true) || trn_reduce(c, s)) return 1;
  std::copy(s.begin(), s.end(), sums);
  return 0;
}
int pop_transport_sums_set(pop_ctx *c, const double *sums, long long count) {
  if (trn_requested(c, "pop_transport_sums_set")) return 1;
  if (tavg_between_steps(c, "pop_transport_sums_set") || count_is(c, (long long)trn_n_sums(c), count, "the transport sums")) return 1;
  if (trn_reset(c)) return 1;   // the vector replaces the sums of the interval
  c->trn.set_sums.assign(sums, sums + count);
  return 0;
}

}  // extern "C"
