// pop_ctx.hpp -- the context of one model instance and the small helpers every launch file uses: the ownership helpers
// (device memory, events, streams, pinned host memory: each recorded in the context where it is made), launch shapes and
// step parameters.  Part of the single translation unit pop_amd.hip (included after the kernel headers).
#pragma once

#define HIPCHK(ctx, call)                                                                       \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess) {                                                                     \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                           \
      return 1;                                                                                 \
    }                                                                                           \
  } while (0)

struct PhaseTimer { double ms = 0; int calls = 0; };

struct DevPeer { int rank; int *send_src = nullptr, *recv_dst = nullptr; int nsend = 0, nrecv = 0; };

// ---- time-averaged output (tavg.F90; launch_tavg.hpp): the requested entries, the streams and the launch tables of the sites
enum TavgSite { TS_FORCING = 0, TS_STATE, TS_TRACER, TS_VMIX, TS_HMIX, TS_BTROP, TS_QFLUX, TS_NSITES };
struct TavgEntry {
  std::string name;
  int stream = 0, site = 0, ndims = 2, method = TAVG_AVG;
  int kmax = 1;              // levels the entry is fed from: km for a 3-D entry, 1 .. 8 for U1_8, km for RHO_VINT
  int nlev = 1;              // levels of the buffer
  int expr = TX_X, a = -1, b = -1;   // source ids (launch_tavg.hpp TavgSid)
  double cst = 0.0, cst2 = 0.0;
  bool cells = false;        // served by k_tavg_cells (else k_tavg_columns)
  bool vint = false;         // columns: fed once per level
  double *buf = nullptr;     // device, (nxb, nyb, nlev, nblocks); null on a host-only context
};
struct TavgSiteTab {
  TavgTable cells{}, cols{}; int sid_cells[TAVG_MAX_SRC] = {}, sid_cols[TAVG_MAX_SRC] = {}; bool vint_psurf = false;
  // a second launch of the 2-D column entries whose sources no longer fit the first (the forcing site with the coupled fields)
  TavgTable cols_more{}; int sid_cols_more[TAVG_MAX_SRC] = {};
};
struct TavgState {
  std::vector<TavgEntry> req;
  bool on[TAVG_MAX_STREAMS + 1] = {};               // ltavg_on
  bool used[TAVG_MAX_STREAMS + 1] = {};             // the stream holds an entry
  bool has_qflux[TAVG_MAX_STREAMS + 1] = {};
  double sum[TAVG_MAX_STREAMS + 1] = {}, sum_qflux[TAVG_MAX_STREAMS + 1] = {};   // tavg_sum, tavg_sum_qflux
  double dtavg = 0.0;                               // weight of the step pop_time_manager last set up
  bool active = false;                              // some entry's stream is on: the one flag the sites of a step test
  bool in_step = false;                             // between pop_time_manager and pop_step_tail
  bool dirty = true;                                // the tables below are out of date (request list or on/off state changed)
  TavgSiteTab site[TS_NSITES];
  double *scratch = nullptr;                        // normalise-into-a-copy: one 3-D field
};

// ---- global and CFL diagnostics (diagnostics.F90; launch_diag.hpp): arming, work buffers, what the sites left for the getters
struct DiagState {
  bool arm_global = false, arm_cfl = false;   // pop_diag_arm: for the next step
  bool run_global = false, run_cfl = false;   // the step in hand is armed (pop_time_manager took the arming): the flags the sites test
  // device work space, allocated by the first armed site
  double *partial = nullptr; size_t partial_n = 0;                            // workgroup partials of the global sums
  double *vec = nullptr; size_t vec_n = 0;                                    // per-block results of every block of the decomposition
  double *cfl_val = nullptr; int *cfl_idx = nullptr; size_t cfl_n = 0;        // workgroup (value, cell) pairs
  // pinned host copies of vec, one per site
  double *h_pre = nullptr, *h_after = nullptr, *h_cfl = nullptr;
  int step_pre = -1, step_after = -1, step_cfl = -1;                          // nsteps_total of the step each site last ran in
  double c2dtt_pre = 0.0, rms_after = 0.0; int iters_after = 0;
};

// ---- meridional overturning circulation (diags_on_lat_aux_grid.F90; host_lat_aux.cpp, launch_moc.hpp)
struct MocState {
  LatAux aux;                                       // pop_init_transports
  bool requested = false; int stream = 0;           // pop_moc_request
  bool active = false;                              // requested and the stream is on: the one flag the site of a step tests
  std::vector<int> loc_list, loc_blist;             // the lists of aux.lists / aux.blists that belong to this rank's blocks
  // device: the local lists (block = local index), their cells (moc_lists_upload: shared with the tracer transports), the
  // accumulators and the scratch field of k_moc_w
  bool lists_up = false;
  MocList *d_lists = nullptr, *d_blists = nullptr; int *d_cells = nullptr, *d_bcells = nullptr;
  double *ACC = nullptr, *BACC = nullptr, *WE = nullptr, *gather = nullptr;
  std::vector<double> set_sums;                     // pop_moc_sums_set: added last when the sums are read
  std::vector<double> snap; bool have_snap = false; // the normalised result pop_tavg_write took before it reset the stream
};

// ---- northward heat and salt transports (compute_tracer_transports; kernels_transport.hpp, launch_transport.hpp).  The latitude
// grid, the regions and the uploaded cell lists are MocState's
struct TrnState {
  bool requested = false, want[2] = {false, false}; int stream = 0;   // pop_transport_request(stream, heat, salt)
  bool active = false;                              // requested and the stream is on: the one flag the site of a step tests
  int n_comp = 3;                                   // n_transport_comp (diags_on_lat_aux_grid.F90:886-889)
  double *COL[2][TRN_NCOL] = {};                    // the per-column terms of the last accumulated step, (nxb, nyb, nblocks) per tracer
  double *ACC = nullptr, *BACC = nullptr, *gather = nullptr;
  std::vector<double> set_sums;                     // pop_transport_sums_set: added last when the sums are read
  std::vector<double> snap[2]; bool have_snap = false;
};

// ---- coupled surface forcing (forcing_coupled.F90, the tail of set_surface_forcing; kernels_forcing.hpp, launch_forcing.hpp)
struct CplState {
  bool inited = false;                              // pop_init_coupled_forcing: the one flag the head of a step tests
  bool imported = false;                            // a pop_set_coupled_forcing has been made: the interval's fields hold values
  pop_coupled_nml nml{}; CplConsts k{};
  int nsteps = 0;                                   // steps of this coupling interval (pop_time_manager advances, an import resets)
  std::vector<double> qsw;                          // qsw_12hr_factor(1 : nml.nsteps_per_interval)
  bool fwf = false, icefw = false;                  // the fresh-water form (not lfw_as_salt_flx); and ice formation on: FW_FREEZE joins FW / TFW every step
  // device (null on a host-only context)
  double *d_qsw = nullptr, *COSA = nullptr, *SINA = nullptr;
  double *F[CF_NF] = {};                            // the imported fields
  double *SHF_COMP_QSW = nullptr, *SFWF_COMP = nullptr, *TFW_COMP[2] = {nullptr, nullptr};
  double *raw = nullptr, *h_raw = nullptr;          // staging of one import: X_NF planes on the device, the same pinned on the host
  hipEvent_t ev_up = nullptr; bool up_pending = false;   // the upload of the last import (the next one reuses h_raw)
  // marginal-sea balance (lms_balance): per sea the indicator and MASK_FRAC, (n2, nblocks, nseas); the per-cell TRANSPORT term; the reduced sums
  bool ms = false; int nseas = 0;
  double *MS_IND = nullptr, *MS_FRAC = nullptr, *MS_T = nullptr, *ms_sums = nullptr;
  double c_q = 0, c_s = 0, c_a = 0, c_t = 0;
};

struct pop_ctx {
  HostModel h;
  Forms f;                                // the plan: every kernel-form and schedule choice, resolved once at create (forms.hpp)
  bool host_only = true;
  std::string err;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  DevGrid g{};
  std::map<std::string, double *> d2;     // device 2-D fields (local blocks)
  std::map<std::string, int *> di2;
  // what the context owns, recorded where it is made (dev_alloc, new_event, new_stream, pinned_alloc) and released by pop_destroy:
  // device memory, events, streams other than the launch stream, pinned host memory
  std::vector<void *> allocs;
  std::vector<hipEvent_t> events;
  std::vector<hipStream_t> streams;
  std::vector<void *> pinned;
  // prognostic state, physical slots; logical levels via oldt/curt/newt
  double *TR[MAXNT][3] = {}, *U[3] = {}, *V[3] = {}, *RHO[3] = {};
  double *PS[3] = {}, *GX[3] = {}, *GY[3] = {}, *UB[3] = {}, *VB[3] = {};
  double *PGUESS = nullptr, *FW = nullptr, *FW_OLD = nullptr, *SHF_QSW = nullptr, *CHL = nullptr;
  double *STF[MAXNT] = {}, *TFW[MAXNT] = {}, *KPP_SRC[MAXNT] = {}, *VDC[2] = {}, *VVC = nullptr;
  double *DH = nullptr, *DHU = nullptr, *ZX = nullptr, *ZY = nullptr, *UH = nullptr, *VH = nullptr;
  double *W3 = nullptr, *W4 = nullptr, *RHS = nullptr, *centerWgt = nullptr;
  double *E3 = nullptr, *F3 = nullptr, *S3a = nullptr, *S3b = nullptr, *S3c = nullptr, *S3d = nullptr;
  // del4: the first Laplacians on the side stream (Forms::del4_side) write own output buffers d2t / d2u; in line they reuse the shared scratch
  double *d2t[2] = {nullptr, nullptr}, *d2u[2] = {nullptr, nullptr};
  // hmix_momentum = 3: the friction hdiffu_aniso forms (3-D, read by the momentum kernel) and the variable viscosities F_PARA, F_PERP
  double *HDU = nullptr, *HDV = nullptr, *FPARA = nullptr, *FPERP = nullptr;
  // del4: the tracer kernel of a step also forms the first Laplacian of its CURRENT tracers -- the mix-time field of the next
  // (leapfrog) step -- from the tile it has in LDS; d2t_next receives it, d2t_next_slot is the time slot it belongs to
  double *d2t_next[2] = {nullptr, nullptr};
  bool d2t_next_valid = false; int d2t_next_slot = -1;
  // the ghost cells of the tracers in a time slot are copies of their source cells (set-up and every halo update leave them so;
  // a caller's pop_set_field / a restart file may not): only then is the halo update of the field formed ahead the same arithmetic
  // as k_del4_d2t on the ghost ring
  bool tr_ghosts_ok[3] = {true, true, true};
  // the same for the velocity (k_momentum_rhs_lds forms k_del4_d2u's field for the next step)
  double *d2u_next[2] = {nullptr, nullptr};
  bool d2u_next_valid = false; int d2u_next_slot = -1;
  bool uv_ghosts_ok[3] = {true, true, true};
  bool d2t_last_formed = false, d2u_last_formed = false;   // did the last tracer / momentum launch write the next step's field (bench accounting)
  hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr, ev_d2t = nullptr, ev_d2u = nullptr, ev_vmixu = nullptr;
  bool vmixu_pending = false, btrop_added = false, vmixu_deferred = false;   // implicit vertical mixing of U,V in flight on the side stream
  double *HBLT = nullptr, *HMXL = nullptr, *HMXL_DR = nullptr;
  MixDev mix{};
  // KPP look-ahead (Forms::kpp_ahead): the vertical-mixing coefficients of the NEXT step depend only on this step's curtime fields (its
  // mixtime on a leapfrog step), so pop_step computes them on a third stream beside the barotropic solver into a second set of output
  // fields; the next step swaps the sets in.
  bool kpp_src_user = false;   // the caller wrote KPP_SRC (pop_set_field): read it at every level until KPP has run again
  bool src_dirty = true, src_dirty_alt = true;   // KPP_SRC / KPPa may hold non-zeros below the KBL stored with them: the next evaluation into that set clears every level
  double *VDCa[2] = {nullptr, nullptr}, *VVCa = nullptr, *KPPa[MAXNT] = {}, *HBLTa = nullptr, *HMXLa = nullptr, *HMXL_DRa = nullptr;
  int *KBL = nullptr, *KBLa = nullptr;   // KBL that belongs to KPP_SRC / KPPa (the tracer kernel reads KPP_SRC down to it)
  hipStream_t ahead = nullptr; hipEvent_t ev_ahead_fork = nullptr, ev_ahead = nullptr;
  bool ahead_valid = false; int ahead_slot = -1, ahead_swaps = 0;   // ahead_swaps: steps that took their coefficients from the look-ahead
  // solver
  double *R = nullptr, *S0 = nullptr, *S1 = nullptr, *Q = nullptr, *Z = nullptr, *AZ = nullptr;
  double *partial = nullptr, *blocksum = nullptr;
  SolverScalars *sc = nullptr;
  int *gid = nullptr, *srcmap = nullptr, *iota = nullptr, *loc_of_gid = nullptr;
  std::vector<int> opre_host;
  int *red_act = nullptr, *red_cnt = nullptr; int red_nact = 0;                // chunks with an ocean cell (fused solver launches, land elimination)
  SolverScalars *host_sc = nullptr;                       // pinned
  double *host_rr = nullptr;                              // pinned ring of (r,r) check results (k_rr_total)
  hipEvent_t chk_ev[4] = {};                              // one event per check interval in flight
  // fused-solver interval graphs, keyed by the solution array and the solver's variant of the interval (graph_for)
  struct IntervalGraph { const double *key; int variant; hipGraphExec_t exec; };
  std::vector<IntervalGraph> graphs;
  bool grid_from_input = false;
  // land elimination (Forms::land_skip, land_full_steps): the first land_full_steps steps after set-up / a restart / a new state run every workgroup (they write
  // the state-independent values of the land tiles), later steps skip workgroups without an ocean cell (DevGrid::skip)
  int full_left = 4, full_seen = 0; double land_fraction = 0.0;
  // the resident pcg of small grids (kernels_pcg_persist.hpp; Forms::persist): one plan per solver view
  struct PersistPlan {
    const void *key = nullptr; bool ok = false; std::string why;
    int CP = 0, nwg = 0, nwin_max = 0, nslots = 0;
    int *own_q = nullptr, *halo_off = nullptr, *halo_q = nullptr; unsigned short *nbr = nullptr;
    PWord *W = nullptr;                                    // [2][nslots] partial words + [2][ncell] z words
    double *X0 = nullptr;                                  // copy of the first guess (a solve that gave up is repeated by the two-launch form)
  };
  unsigned long long persist_epoch = 0;                    // high half of the tags of the next resident solve (never repeats)
  std::vector<PersistPlan> persist;
  std::vector<int> h_srcmap;                               // host copy of srcmap (local view)
  double *persist_out = nullptr;                           // pinned: iterations, (r,r), status, checks
  int persist_used = 0;                                    // the last pcg solve ran as the resident launch
  int persist_gave_up = 0;                                 // resident solves that gave up a wait (then never used again in this model)
  int red_active_total = 0;                                // fused solver kernels: chunks that have work, summed over the local blocks
  int persist_nwg = 0, persist_cp = 0;                     // shape of the last resident launch
  double *pcsi_raw = nullptr;   // P-CSI, two iterations per launch: the residual of the pair before a check (k_pcsi_step_x2<true> -> k_pcsi_rr_chunks)
  int *pcsi_jfold = nullptr;    // tripole: per local block, the first array row beyond the fold (PcsiArgs::jfold)
  SolveView gv{};                                         // replicated barotropic mode: all blocks
  double *gTAREA = nullptr; int *gKMT = nullptr;
  int nchunk = 0, numIterations = 0;
  double rmsResidual = 0.0;
  // halo plan on device
  int *copy_dst = nullptr, *copy_src = nullptr, *fill_dst = nullptr;
  int ncopy = 0, nfill = 0;
  std::vector<DevPeer> peers;
  // all peers concatenated (one pack / unpack launch per halo update)
  int *sa_src = nullptr, *sa_start = nullptr, *sa_cnt = nullptr, *ra_dst = nullptr, *ra_start = nullptr, *ra_cnt = nullptr;
  int nsend_all = 0, nrecv_all = 0;
  // fused distributed solvers: per-cell send entries / receive slots (FusedArgs::sendmap, rmap), nz = 1 message order
  int *sendmap = nullptr, *send_off = nullptr, *send_slot = nullptr, *rmap = nullptr;
  bool halo_ns_only = false;                               // every ghost cell owned by another rank lies in a ghost ROW (j-band shards)
  pop_exchange_fn xchg_side = nullptr;                     // the same exchange on the communication stream (own communicator), or null
  hipStream_t comm_side = nullptr;                         // stream of those exchanges (not `side`: impvmixu runs there beside the solver)
  hipEvent_t ev_sa = nullptr, ev_sx = nullptr;            // solver: z packed (launch stream) / z received (side stream)
  long long solver_ops = 0, solver_enq = 0;               // stream operations / iterations enqueued by the last distributed solve (incl. look-ahead)
  // tripole northern boundary, per field location (single rank)
  int *tp_dst[5] = {}, *tp_a[5] = {}, *tp_b[5] = {}; int tp_n[5] = {}; double *tp_buf = nullptr;
  // comm hooks
  double *sendbuf = nullptr, *recvbuf = nullptr, *redbuf = nullptr;
  long long comm_doubles = 0, red_doubles = 0;
  pop_exchange_fn xchg = nullptr;
  pop_allreduce_fn allred = nullptr;
  void *comm_user = nullptr;
  EvpDev evp{}; bool use_evp = false;                                                // EVP block preconditioner (preconditioner_choice = 1)
  double *pcsi_omega = nullptr; int *pcsi_base = nullptr; double pcsi_csy = 0;        // P-CSI: omega_k table, interval base
  double rf_S[MAXNT] = {}, rf_S_prev[MAXNT] = {}; bool rf_S_prev_valid[MAXNT] = {};   // Robert filter
  Upw3Dev upw3{};                                          // tadvect = 2
  LwDev lw{};                                              // tadvect = 3 (lw_lim): flux-velocity and work fields
  SubmDev subm{};                                          // lsubmesoscale_mixing: the column fields of submeso_sf, diagnostics
  GmDev gm{};                                              // hmix_tracer = 3 (gm): slopes, tapered diffusivities, GTK
  // passive tracers n = 3 .. nt (0-based 2 .. nt-1).  PW[n]: the horizontal-mixing work field of tracer n -- the Gent-McWilliams (+ submeso)
  // tendency (GM_GTK) or del4's first Laplacian; PWX: the second output of a pair launch for an odd tracer count; PL: L(T) of lw_lim
  // of the pair in hand; PTD / PTDX: submeso_diag's tendency (SUBM_ADV_TEND); KPPX / KPPXa: KppDev::SRCX of the two sets of KPP outputs
  double *PW[MAXNT] = {}, *PWX = nullptr, *PL[2] = {nullptr, nullptr}, *PTD[MAXNT] = {}, *PTDX = nullptr, *KPPX = nullptr, *KPPXa = nullptr;
  RcclTransport *rccl_tr = nullptr;                       // in-library RCCL transport (pop_comm_init_rccl)
  // Jayne tidal mixing (pop_init_tidal_mixing): the resolved namelist and the init-time fields of the local blocks (host copies serve
  // pop_get_field; the device copies and the kernel's arguments live in KppHost::tidal)
  struct Tidal { bool inited = false, on = false; pop_tidal_nml nml{}; TidalFields f; } tidal;
  // latitude-varying KPP background (pop_init_kpp_bckgrnd): host copies; the device copies live in KppHost::bck
  struct Bckgrnd { bool inited = false, on = false; pop_kpp_bckgrnd_nml nml{}; BckgrndFields f; } bck;
  // frazil ice formation (pop_init_ice): the namelist, the derived constants, tlast_ice and the four 2-D device fields (null on a
  // host-only context).  liceform: ice forms inside the library's own step and the corrector's freeze clamp is off
  struct Ice { bool inited = false, liceform = false; pop_ice_nml nml{}; IceConsts k{}; double tlast_ice = 0.0;
               double *QICE = nullptr, *AQICE = nullptr, *QFLUX = nullptr, *FWF = nullptr; } ice;
  std::vector<double> tlon;                                // TLON of the local blocks, formed once by whichever of the two init calls comes first
  bool ran = false;                                        // a step or a phase has run (pop_init_tidal_mixing / pop_init_kpp_bckgrnd are refused afterwards)
  // time stepping
  int oldt = 0, curt = 1, newt = 2, mixt = 1;
  int first_step = 1, leapfrogts = 1, f_euler_ts = 0, avg_ts = 0, nsteps_total = 0, nsteps_this_interval = 0;
  int eod = 0, eod_last = 0;                               // the step ends a day / the previous one did (time_management.F90:1809, 3586-3592; runs that start at midnight)
  double c2dtt = 0, c2dtu = 0, c2dtp = 0, beta = 0;
  std::map<std::string, PhaseTimer> timers;
  // the barotropic solve bracketed by two events on the launch stream, read back one step later (no synchronisation inside the
  // step): totals since the last pop_timers_reset / "solver_ms_reset" for the bench's per-iteration figure
  hipEvent_t ev_solve[2] = {nullptr, nullptr}; bool solve_pending = false; int solve_iters_pending = 0;
  double solver_ms_total = 0.0; long long solver_iters_total = 0, solver_calls_total = 0;
  bool timing = false;
  bool phase_timing = false;   // inside pop_time_phase: kernels only
  double *op_scratch = nullptr;   // pop_operator_host: four block-sized 2-D arrays
  TavgState tavg;
  DiagState diag;
  MocState moc;
  TrnState trn;
  CplState cpl;
  MsBalance msb;                                           // pop_init_ms_balance
  std::vector<int> region_mask;                            // the caller's REGION_MASK (ny_global, nx_global): the one copy pop_init_transports and pop_init_ms_balance share
  std::vector<double> anglet, cos_anglet, sin_anglet;      // ANGLET and its cosine / sine on the local blocks, formed on first use (host_anglet_build)
};

namespace {

template <class T>
int dev_alloc(pop_ctx *c, T **p, size_t n, bool zero = true) {
  void *v = nullptr;
  HIPCHK(c, hipMalloc(&v, std::max<size_t>(n, 1) * sizeof(T)));
  c->allocs.push_back(v);
  if (zero) HIPCHK(c, hipMemset(v, 0, std::max<size_t>(n, 1) * sizeof(T)));
  *p = (T *)v;
  return 0;
}
template <class T>
int dev_upload(pop_ctx *c, T **p, const T *src, size_t n) {
  if (dev_alloc(c, p, n, false)) return 1;
  HIPCHK(c, hipMemcpy(*p, src, n * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}
// an event, a non-blocking stream, pinned host memory: made here, released by pop_destroy (lazily made ones included)
int new_event(pop_ctx *c, hipEvent_t *e, unsigned flags = hipEventDisableTiming) {
  HIPCHK(c, hipEventCreateWithFlags(e, flags));
  c->events.push_back(*e);
  return 0;
}
int new_stream(pop_ctx *c, hipStream_t *s) {
  HIPCHK(c, hipStreamCreateWithFlags(s, hipStreamNonBlocking));
  c->streams.push_back(*s);
  return 0;
}
template <class T>
int pinned_alloc(pop_ctx *c, T **p, size_t n) {
  HIPCHK(c, hipHostMalloc((void **)p, n * sizeof(T)));
  c->pinned.push_back(*p);
  return 0;
}
// column kernels: one wave per workgroup; tile order per kernels_common.hpp col_setup
dim3 grid_cols(const pop_ctx *c) { return dim3(col_grid(c->g, POP_COL_THREADS), c->g.nblocks); }
dim3 block_stencil() { return dim3(POP_COL_THREADS, 1); }
dim3 grid_stencil(const pop_ctx *c) { return grid_cols(c); }
dim3 grid_2d(const pop_ctx *c) { return dim3(red_grid_x(c->g), c->g.nblocks); }
dim3 grid_3d(const pop_ctx *c) { return dim3((c->g.n2 + 255) / 256, c->g.km, c->g.nblocks); }

StepParams step_params(const pop_ctx *c) {
  const pop_config &cf = c->h.c;
  StepParams s{};
  s.c2dtu = c->c2dtu; s.c2dtp = c->c2dtp; s.beta = c->beta; s.gamma = 1.0 - 2.0 * (1.0 / 3.0);
  s.dtp = c->h.dtp; s.grav = GRAV;
  s.am = cf.am; s.ah = cf.ah; s.bottom_drag = cf.bottom_drag;
  s.const_vvc = cf.const_vvc; s.const_vdc = cf.const_vdc; s.convect_diff = cf.convect_diff; s.convect_visc = cf.convect_visc;
  s.aidif = cf.aidif;
  s.rich_bckgrnd_vvc = cf.rich_bckgrnd_vvc; s.rich_bckgrnd_vdc = cf.rich_bckgrnd_vdc; s.rich_mix = cf.rich_mix;
  s.leapfrogts = c->leapfrogts; s.pavg = (cf.lpressure_avg && c->leapfrogts) ? 1 : 0;
  s.impcor = cf.impcor; s.reset_to_freezing = (cf.reset_to_freezing && !c->ice.liceform) ? 1 : 0;   // baroclinic.F90:1418
  s.nvdc = (cf.vmix_choice == 3) ? 2 : 1;
  return s;
}

// time_weight of increment_tlast_ice (ice.F90:340-346) for the step pop_time_manager last set up: 0.5 on an averaging step (there are
// no back_to_back steps here), otherwise 1
double ice_time_weight(const pop_ctx *c) { return c->avg_ts ? 0.5 : 1.0; }
// hflux_factor (pop_constants.F90:336) with the code defaults of rho_sw, cp_sw unless pop_init_ice gave others: the one factor of the
// tavg entries, the global diagnostics and the heat transport
double hflux_factor_of(const pop_ctx *c) { return c->ice.inited ? c->ice.k.hflux_factor : 1000.0 / ((4.1 / 3.996) * 3.996e7); }

struct ScopedPhase {   // optional HIP-event timing of a phase on the launch stream
  pop_ctx *c; const char *name; hipEvent_t e0 = nullptr, e1 = nullptr;
  ScopedPhase(pop_ctx *c_, const char *n) : c(c_), name(n) {
    if (c->timing) { hipEventCreate(&e0); hipEventCreate(&e1); hipEventRecord(e0, c->stream); }
  }
  ~ScopedPhase() {
    if (c->timing) {
      hipEventRecord(e1, c->stream); hipEventSynchronize(e1);
      float ms = 0; hipEventElapsedTime(&ms, e0, e1);
      auto &t = c->timers[name]; t.ms += ms; t.calls += 1;
      hipEventDestroy(e0); hipEventDestroy(e1);
    }
  }
};

}  // namespace
