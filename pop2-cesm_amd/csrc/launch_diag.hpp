// launch_diag.hpp -- global and CFL diagnostics (diagnostics.F90): arming, the three sites of an armed step and what the getters
// make of their results.  Part of the single translation unit pop_amd.hip (included after launch_tavg.hpp).
//
// Sites (DiagState::run_global / run_cfl are the host flags a step tests; nothing else happens in a step that is not armed):
//   diag_global_pre    pop_step_tail after PGUESS, before the time levels rotate   diag_global_preupdate  :1174-1431, step_mod.F90:649
//   diag_global_after  end of pop_step_tail (after the rotation / step_rf)          diag_global_afterupdate :1548-1770, step_mod.F90:860
//   diag_cfl           end of pop_baroclinic_driver                                 cfl_advect :2262-2425, cfl_hdiff :2695-2767, cfl_check :2837-3145
// A site is one launch over the sources (kernels_diag.hpp), one small launch that leaves a result per block of the decomposition
// in DiagState::vec (entries of other ranks' blocks 0), a sum all-reduce of that vector where there are several ranks (exact: one
// rank owns each entry) and an asynchronous copy to pinned host memory.  The getters synchronise and finish on the host:
//   sums:    a level-fed quantity adds its levels in the order k = 1 .. per block (local_sums of the reference), blocks are added in
//            block-id order, then the quotient -- the result does not depend on the distribution over ranks;
//   maxima:  per level the first block in block-id order whose maximum is strictly greater (maxloc over the block maxima), the
//            total the first level that is strictly greater, starting from -1.  Across ranks the reference takes the component-wise
//            global_maxval of i and of j of the ranks that hold the maximum (:2975-2980), which depends on the distribution when
//            the maximum ties; here the first block in global order owns the address (the rule of pop_global_extreme).
// cfl_vdiff is only called without implicit_vertical_mix (vertical_mix.F90:677-678) and the library has only the implicit form: the
// vertical-mixing numbers are the reference's 0 with the address (0, 0, 1).
#pragma once

namespace {

// the reference's global diagnostics that are vertical integrals of tendencies formed inside the tracer and momentum kernels, its
// transport and velocity diagnostics and the tracer budgets of budget_diagnostics.F90
const char *const diag_left_out[] = {
  "diag_ke_adv", "diag_ke_hmix", "diag_ke_vmix", "diag_ke_press", "diag_pe", "diag_tracer_adv", "diag_tracer_hdiff", "diag_tracer_vdiff",
  "diag_tracer_source", "diag_tracer_roff_vsf", "diag_tracer_exchcirc", "diag_transport", "diag_velocity", "tracer_mean_initial",
  "tracer_mean_final", "diag_print"};

int diag_nchunk(const pop_ctx *c) { return (c->g.n2 + POP_RED_THREADS - 1) / POP_RED_THREADS; }
int diag_nlev(const pop_ctx *c) { return c->h.km + 1; }
size_t diag_n_pre(const pop_ctx *c) { return (size_t)c->h.nblocks_tot * diag_nlev(c) * 2 * c->h.nt; }
size_t diag_n_after(const pop_ctx *c) { return (size_t)c->h.nblocks_tot * diag_nlev(c) * (c->h.nt + 1); }
size_t diag_n_cfl(const pop_ctx *c) { return (size_t)c->h.nblocks_tot * c->h.km * DIAG_NQ_CFL * 2; }

int diag_pinned(pop_ctx *c, double **p, size_t n) {
  return *p ? 0 : pinned_alloc(c, p, n);
}
int diag_alloc_vec(pop_ctx *c) {
  DiagState &D = c->diag;
  if (D.vec) return 0;
  D.vec_n = std::max(diag_n_pre(c), diag_n_cfl(c));   // n_after < n_pre
  return dev_alloc(c, &D.vec, D.vec_n, false);
}
int diag_alloc_global(pop_ctx *c) {
  DiagState &D = c->diag;
  if (!D.partial) {
    D.partial_n = (size_t)c->h.nblocks * diag_nlev(c) * 2 * c->h.nt * diag_nchunk(c);
    if (dev_alloc(c, &D.partial, D.partial_n, false)) return 1;
  }
  return diag_alloc_vec(c) || diag_pinned(c, &D.h_pre, diag_n_pre(c)) || diag_pinned(c, &D.h_after, diag_n_after(c));
}
int diag_alloc_cfl(pop_ctx *c) {
  DiagState &D = c->diag;
  if (!D.cfl_val) {
    D.cfl_n = (size_t)c->h.nblocks * c->h.km * DIAG_NQ_CFL * diag_nchunk(c);
    if (dev_alloc(c, &D.cfl_val, D.cfl_n, false) || dev_alloc(c, &D.cfl_idx, D.cfl_n, false)) return 1;
  }
  return diag_alloc_vec(c) || diag_pinned(c, &D.h_cfl, diag_n_cfl(c));
}
// the first n entries of vec: summed over the ranks (through the reduce buffer, in pieces of its size), then to the pinned copy
int diag_publish(pop_ctx *c, size_t n, double *host) {
  DiagState &D = c->diag;
  if (c->h.nranks > 1) {
    if (!c->allred || !c->redbuf || c->red_doubles < 1) { c->err = "diagnostics: multi-rank run without a transport"; return 1; }
    for (size_t off = 0; off < n; off += (size_t)c->red_doubles) {
      const size_t cnt = std::min(n - off, (size_t)c->red_doubles);
      HIPCHK(c, hipMemcpyAsync(c->redbuf, D.vec + off, cnt * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
      if (c->allred(c->comm_user, 0, (long long)cnt)) { c->err = "diagnostics: allreduce failed" + tr_err(c); return 1; }
      HIPCHK(c, hipMemcpyAsync(D.vec + off, c->redbuf, cnt * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    }
  }
  HIPCHK(c, hipMemcpyAsync(host, D.vec, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  return 0;
}
int diag_nt_ok(pop_ctx *c, bool launched) {
  if (launched) return 0;
  c->err = "diagnostics: no kernel for nt = " + std::to_string(c->h.nt);
  return 1;
}
const double *diag_dup(pop_ctx *c) { return c->h.c.ns_boundary == 2 ? c->d2["TRIPOLE_DUP"] : nullptr; }

int diag_global_pre(pop_ctx *c) {
  if (diag_alloc_global(c)) return 1;
  DiagState &D = c->diag;
  const int nt = c->h.nt, nlev = diag_nlev(c), nchunk = diag_nchunk(c), nslots = nlev * 2 * nt;
  DiagPreArgs a{};
  a.U = c->U[c->curt]; a.V = c->V[c->curt]; a.UB = c->UB[c->curt]; a.VB = c->VB[c->curt]; a.GX = c->GX[c->curt]; a.GY = c->GY[c->curt];
  a.DH = c->DH; a.DHU = c->DHU; a.PSC = c->PS[c->curt]; a.PSN = c->PS[c->newt]; a.PSM = c->PS[c->mixt];
  for (int n = 0; n < nt; ++n) { a.TN[n] = c->TR[n][c->newt]; a.TO[n] = c->TR[n][c->oldt]; }
  a.UAREA = c->d2["UAREA"]; a.RCALCU = c->d2["RCALCU"]; a.DUP = diag_dup(c); a.grav = GRAV;
  a.out = DiagSumOut{D.partial, nchunk, nlev};
  const size_t n = diag_n_pre(c);
  HIPCHK(c, hipMemsetAsync(D.vec, 0, n * sizeof(double), c->stream));
  const dim3 G(nchunk, nlev, c->g.nblocks);
  const bool ok = with_value<2, 3, 4, 5, 6, 7, 8>(nt, [&](auto NT) {
    with_flags([&](auto PBC) { hipLaunchKernelGGL((k_diag_pre<decltype(NT)::value, decltype(PBC)::value>), G, dim3(POP_RED_THREADS), 0, c->stream, c->g, a); }, c->g.pbc != 0);
  });
  if (diag_nt_ok(c, ok)) return 1;
  hipLaunchKernelGGL(k_diag_block_sums, dim3(nslots, c->g.nblocks), dim3(POP_RED_THREADS), 0, c->stream, (const double *)D.partial, nchunk, nslots, (const int *)c->gid, D.vec);
  HIPCHK(c, hipGetLastError());
  if (diag_publish(c, n, D.h_pre)) return 1;
  D.step_pre = c->nsteps_total; D.c2dtt_pre = c->c2dtt;
  return 0;
}
int diag_global_after(pop_ctx *c) {
  if (diag_alloc_global(c)) return 1;
  DiagState &D = c->diag;
  const int nt = c->h.nt, nlev = diag_nlev(c), nchunk = diag_nchunk(c), nslots = nlev * (nt + 1);
  DiagAfterArgs a{};
  a.U = c->U[c->curt]; a.V = c->V[c->curt]; a.PS = c->PS[c->curt];
  for (int n = 0; n < nt; ++n) { a.TR[n] = c->TR[n][c->curt]; a.TFW[n] = c->TFW[n]; }
  a.UAREA = c->d2["UAREA"]; a.RCALCU = c->d2["RCALCU"]; a.DUP = diag_dup(c); a.grav = GRAV;
  a.out = DiagSumOut{D.partial, nchunk, nlev};
  const size_t n = diag_n_after(c);
  HIPCHK(c, hipMemsetAsync(D.vec, 0, n * sizeof(double), c->stream));
  const dim3 G(nchunk, nlev, c->g.nblocks);
  const bool ok = with_value<2, 3, 4, 5, 6, 7, 8>(nt, [&](auto NT) {
    with_flags([&](auto PBC) { hipLaunchKernelGGL((k_diag_after<decltype(NT)::value, decltype(PBC)::value>), G, dim3(POP_RED_THREADS), 0, c->stream, c->g, a); }, c->g.pbc != 0);
  });
  if (diag_nt_ok(c, ok)) return 1;
  hipLaunchKernelGGL(k_diag_block_sums, dim3(nslots, c->g.nblocks), dim3(POP_RED_THREADS), 0, c->stream, (const double *)D.partial, nchunk, nslots, (const int *)c->gid, D.vec);
  HIPCHK(c, hipGetLastError());
  if (diag_publish(c, n, D.h_after)) return 1;
  D.step_after = c->nsteps_total; D.iters_after = c->numIterations; D.rms_after = c->rmsResidual;
  return 0;
}
int diag_cfl(pop_ctx *c) {
  if (diag_alloc_cfl(c)) return 1;
  DiagState &D = c->diag;
  const pop_config &cf = c->h.c;
  const int km = c->h.km, nchunk = diag_nchunk(c), nslots = km * DIAG_NQ_CFL;
  DiagCflArgs a{};
  a.U = c->U[c->curt]; a.V = c->V[c->curt]; a.DH = c->DH; a.DXTR = c->d2["DXTR"]; a.DYTR = c->d2["DYTR"];
  a.pow_t = a.pow_u = 1; a.with_u = 1;
  // hmix_del2.F90:1125-1137, hmix_del4.F90:1089-1100, hmix_gm.F90:2162-2172
  if (cf.hmix_tracer == 4) { a.ct = 16.0 * cf.ah; a.pow_t = 2; if (cf.lvariable_hmix) a.HT_COEF = c->d2["D4AHF"]; }
  else if (cf.hmix_tracer == 3) { a.KI0 = c->gm.KI[0]; a.KI1 = c->gm.KI[1]; }
  else { a.ct = 4.0 * cf.ah; if (cf.lvariable_hmix) a.HT_COEF = c->d2["AHF"]; }
  // hmix_del2.F90:944-956, hmix_del4.F90:865-876, hmix_aniso.F90:1043-1055 (not formed with Smagorinsky viscosities)
  if (cf.hmix_momentum == 4) { a.cu = 16.0 * cf.am; a.pow_u = 2; if (cf.lvariable_hmix) a.HU_COEF = c->d2["D4AMF"]; }
  else if (cf.hmix_momentum == 3) {
    if (cf.lsmag_aniso) a.with_u = 0;
    else if (cf.lvariable_hmix_aniso) a.FPARA = c->FPARA;
    else a.cu = 4.0 * cf.visc_para;
  } else { a.cu = 4.0 * cf.am; if (cf.lvariable_hmix) a.HU_COEF = c->d2["AMF"]; }
  a.dt = c->h.dt[1];
  a.val = D.cfl_val; a.idx = D.cfl_idx; a.nchunk = nchunk;
  const size_t n = diag_n_cfl(c);
  HIPCHK(c, hipMemsetAsync(D.vec, 0, n * sizeof(double), c->stream));
  with_flags([&](auto PBC) { hipLaunchKernelGGL(k_cfl_partial<decltype(PBC)::value>, dim3(nchunk, c->g.nblocks), dim3(POP_RED_THREADS), 0, c->stream, c->g, a); }, c->g.pbc != 0);
  hipLaunchKernelGGL(k_cfl_block_max, dim3(nslots, c->g.nblocks), dim3(64), 0, c->stream, (const double *)D.cfl_val, (const int *)D.cfl_idx, nchunk, nslots, (const int *)c->gid, D.vec);
  HIPCHK(c, hipGetLastError());
  if (diag_publish(c, n, D.h_cfl)) return 1;
  D.step_cfl = c->nsteps_total;
  return 0;
}
// pop_run_phase / pop_time_phase: a site on its own runs when the context is armed or inside an armed step
int diag_phase_pre(pop_ctx *c) { return (c->diag.arm_global || c->diag.run_global) ? diag_global_pre(c) : 0; }
int diag_phase_after(pop_ctx *c) { return (c->diag.arm_global || c->diag.run_global) ? diag_global_after(c) : 0; }
int diag_phase_cfl(pop_ctx *c) { return (c->diag.arm_cfl || c->diag.run_cfl) ? diag_cfl(c) : 0; }

// ---- what the getters make of the per-block results (host) ---------------------------------------------------------------
struct DiagGlobalOut { pop_diag_global g; std::vector<double> avg_tracer_k; };
int diag_need_site(pop_ctx *c, const char *who, bool have) {
  if (have) return 0;
  c->err = std::string(who) + ": no armed step has run yet (pop_diag_arm arms the next step)";
  return 1;
}
int diag_finish_global(pop_ctx *c, const char *who, DiagGlobalOut &o) {
  DiagState &D = c->diag;
  if (diag_need_site(c, who, D.step_pre >= 0 || D.step_after >= 0)) return 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const HostModel &h = c->h;
  const int nt = h.nt, km = h.km, nlev = km + 1, NB = h.nblocks_tot;
  pop_diag_global &g = o.g;
  const int bytes = g.struct_bytes;
  g = pop_diag_global{};
  g.struct_bytes = bytes; g.nt = nt; g.km = km; g.nsteps_total_pre = D.step_pre; g.nsteps_total_after = D.step_after;
  const double nan = std::nan("");
  g.rmsResidual = g.diag_sealevel = g.diag_ke = g.diag_ws = g.diag_press_free = g.diag_ke_free = g.diag_ke_psfc = nan;
  for (int n = 0; n < POP_DIAG_MAX_NT; ++n) g.avg_tracer[n] = g.sfc_tracer_flux[n] = g.dtracer_avg[n] = g.dtracer_abs[n] = nan;
  o.avg_tracer_k.assign((size_t)km * nt, nan);
  // pop_constants.F90:336, 364-365 with the code defaults unless pop_init_ice gave others (as launch_tavg.hpp)
  const pop_ctx::Ice &I = c->ice;
  const double hflux_factor = hflux_factor_of(c);
  const double salinity_factor = -(I.inited ? I.nml.ocn_ref_salinity : 34.7) * 1.0e-4;
  const double salt_to_ppt = 1000.0;
  if (D.step_after >= 0) {
    const int NF = nt + 1;
    auto at = [&](int b, int lev, int f) { return D.h_after[((size_t)b * nlev + lev) * NF + f]; };
    auto flat = [&](int f) { double t = 0.0; for (int b = 0; b < NB; ++b) t = t + at(b, 0, f); return t; };          // a 2-D quantity
    auto level = [&](int k, int f) { double t = 0.0; for (int b = 0; b < NB; ++b) t = t + at(b, k, f); return t; };
    auto column = [&](int f) {   // local_sums(iblock) adds the levels in k order; then the blocks
      double t = 0.0;
      for (int b = 0; b < NB; ++b) { double s = 0.0; for (int k = 1; k <= km; ++k) s = s + at(b, k, f); t = t + s; }
      return t;
    };
    g.iterationCount = D.iters_after; g.rmsResidual = D.rms_after;
    g.diag_sealevel = flat(0) / h.area_t;
    g.diag_ke = column(0) / h.volume_u;
    for (int n = 0; n < nt; ++n) {
      g.avg_tracer[n] = column(1 + n) / h.volume_t;
      for (int k = 1; k <= km; ++k) o.avg_tracer_k[(size_t)n * km + k - 1] = level(k, 1 + n) / h.area_t_k[k];
      g.sfc_tracer_flux[n] = flat(1 + n) / h.area_t;
    }
    g.avg_tracer[1] = g.avg_tracer[1] * salt_to_ppt;
    for (int k = 1; k <= km; ++k) o.avg_tracer_k[(size_t)km + k - 1] = o.avg_tracer_k[(size_t)km + k - 1] * salt_to_ppt;
    g.sfc_tracer_flux[0] = g.sfc_tracer_flux[0] / hflux_factor;
    g.sfc_tracer_flux[1] = g.sfc_tracer_flux[1] / salinity_factor;
  }
  if (D.step_pre >= 0) {
    const int NF = 2 * nt;
    auto at = [&](int b, int lev, int f) { return D.h_pre[((size_t)b * nlev + lev) * NF + f]; };
    auto flat = [&](int f) { double t = 0.0; for (int b = 0; b < NB; ++b) t = t + at(b, 0, f); return t; };
    auto column = [&](int f) {   // sum(WORK1) / c2dtt(k), level by level
      double t = 0.0;
      for (int b = 0; b < NB; ++b) { double s = 0.0; for (int k = 1; k <= km; ++k) s = s + at(b, k, f) / D.c2dtt_pre; t = t + s; }
      return t;
    };
    g.diag_ws = flat(0) / h.volume_t; g.diag_press_free = flat(1) / h.volume_t;
    g.diag_ke_free = flat(2) / h.volume_t; g.diag_ke_psfc = flat(3) / h.volume_t;
    for (int n = 0; n < nt; ++n) { g.dtracer_avg[n] = column(2 * n) / h.volume_t; g.dtracer_abs[n] = column(2 * n + 1) / h.volume_t; }
  }
  return 0;
}

struct DiagCflOut { double value = 0.0; int ijk[3] = {0, 0, 0}; std::vector<double> value_k; std::vector<int> ij_k; };
int diag_cfl_index(const char *name) {
  static const char *const names[] = {"advu", "advv", "advw", "advt", "hdifft", "hdiffu", "vdifft", "vdiffu"};
  for (int q = 0; q < 8; ++q) if (!strcmp(name, names[q])) return q;
  return -1;
}
int diag_finish_cfl(pop_ctx *c, int q, DiagCflOut &o) {
  DiagState &D = c->diag;
  if (diag_need_site(c, "pop_diag_cfl", D.step_cfl >= 0)) return 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const HostModel &h = c->h;
  const int km = h.km, NB = h.nblocks_tot;
  o.value_k.assign(km, 0.0); o.ij_k.assign(2 * (size_t)km, 0);
  if (q < DIAG_NQ_CFL)
    for (int k = 1; k <= km; ++k) {
      int win = 0;   // maxloc over the block maxima: the first block that holds the largest
      const double scale = (q == CQ_HDIFFT) ? h.dt[k] : (q == CQ_HDIFFU) ? h.dtu : 1.0;   // cfl_hdiff: the block maximum times dt(k) / dtu
      auto val = [&](int b) { return D.h_cfl[2 * (((size_t)b * km + (k - 1)) * DIAG_NQ_CFL + q)] * scale; };
      for (int b = 1; b < NB; ++b) if (val(b) > val(win)) win = b;
      const long long cell = (long long)D.h_cfl[2 * (((size_t)win * km + (k - 1)) * DIAG_NQ_CFL + q) + 1];
      o.value_k[k - 1] = val(win);
      if (cell >= 0) {
        const BlockInfo &B = h.all_blocks[win];
        o.ij_k[2 * (k - 1)] = B.i_glob[cell % h.nxb]; o.ij_k[2 * (k - 1) + 1] = B.j_glob[cell / h.nxb];
      }
    }
  o.value = -1.0;
  for (int k = 1; k <= km; ++k)
    if (o.value_k[k - 1] > o.value) { o.value = o.value_k[k - 1]; o.ijk[0] = o.ij_k[2 * (k - 1)]; o.ijk[1] = o.ij_k[2 * (k - 1) + 1]; o.ijk[2] = k; }
  return 0;
}

}  // namespace
