// launch_transport.hpp -- northward heat and salt transports (compute_tracer_transports, diags_on_lat_aux_grid.F90:1294-1594): the
// request, the site of a step and what the getters make of the accumulators.  Part of the single translation unit pop_amd.hip
// (included after launch_moc.hpp, whose lists and reduce it shares, and before launch_tavg.hpp, whose stream reset also zeroes these sums).
//
// Site "tavg_transport": in phase_tracer_rhs, right after the (T, S) right-hand side launch.  The advective and diffusive tendencies
// of a step exist only inside the tracer kernels, so the site launches the generic tracer kernel once more in its diagnostic form
// (k_tracer_rhs<., ., false, 2, false, true>) with the arguments the step's kernel got: whichever form the plan selected, the generic
// kernel forms the same L, mixing term and VTN.  Then k_trn_eddy (bolus and submesoscale terms), k_trn_bin and k_trn_bnd
// (kernels_transport.hpp).  TrnState::active is the host flag a step tests.  Nothing is copied, nothing synchronises.  Accumulators
// live per (block, bin) and tracer; the getter reduces them as the MOC's (lat_aux_reduce) and finishes in the reference's order.
// Because the site sits inside phase_tracer_rhs, pop_run_phase("tracer_rhs") with the stream on accumulates as a step does;
// pop_time_phase("tracer_rhs") does not (it times kernels only), and pop_time_phase("tavg_transport") adds the step's sums reps + 1
// times, as timing "tavg_moc" does: reset the stream after timing the site.
#pragma once

namespace {

size_t trn_per_list(const pop_ctx *c) { return (size_t)2 * TRN_NBIN * c->moc.aux.n_reg; }
size_t trn_per_blist(const pop_ctx *) { return (size_t)2 * TRN_NBND; }
size_t trn_n_bins(const pop_ctx *c) { return (size_t)c->moc.aux.n_lat * trn_per_list(c); }
size_t trn_n_sums(const pop_ctx *c) { return trn_n_bins(c) + (c->moc.aux.n_reg > 1 ? trn_per_blist(c) : 0); }
size_t trn_n_out(const pop_ctx *c) { const LatAux &A = c->moc.aux; return (size_t)(A.n_lat + 1) * c->trn.n_comp * A.n_reg; }

// n_transport_comp (:886-889): registry_match('diag_gm_bolus'), registry_match('init_submeso')
int trn_n_comp(const pop_config &cf) {
  int n = 3;
  if (cf.hmix_tracer == 3 && cf.gm_diag_bolus) n = 4;
  if (cf.struct_version >= 7 && cf.lsubmesoscale_mixing) n = 5;
  return n;
}

// the column fields (zero-filled: columns no kernel visits stay 0) and the accumulators
int trn_alloc(pop_ctx *c) {
  TrnState &T = c->trn;
  const MocState &M = c->moc;
  if (moc_lists_upload(c)) return 1;
  const size_t a2 = (size_t)c->h.n2 * c->h.nblocks;
  for (int n = 0; n < 2; ++n) for (int f = 0; f < TRN_NCOL; ++f) {
    if ((f == TRN_C_ADV_I || f == TRN_C_VNF_I) && !c->gm.UISOP) continue;
    if ((f == TRN_C_ADV_SM || f == TRN_C_VNF_SM) && T.n_comp < 5) continue;
    if (dev_alloc(c, &T.COL[n][f], a2)) return 1;
  }
  return dev_alloc(c, &T.ACC, M.loc_list.size() * trn_per_list(c)) || dev_alloc(c, &T.BACC, M.loc_blist.size() * trn_per_blist(c));
}

// the site, once, with the current dtavg, on the launch stream; a: the arguments of the step's (T, S) right-hand side launch
int trn_site(pop_ctx *c, TracerRhsArgs a) {
  TrnState &T = c->trn;
  if (!T.active) return 0;
  const pop_config &cf = c->h.c;
  const MocState &M = c->moc;
  const bool gm = cf.hmix_tracer == 3, up3 = cf.tadvect == 2;
  // the generic kernel's set-up, whichever form ran.  The diagnostic form reads E, F, D2N as its OUTPUTS (kernels_baroclinic.hpp), so
  // every slot the step's launch may have filled for another purpose is set here: HDT, up, E, F, D2N, TNEW, KBL, the source switches
  a.HDT[0] = gm ? c->gm.GTK[0] : nullptr; a.HDT[1] = gm ? c->gm.GTK[1] : nullptr;
  if (up3) a.up = c->upw3;
  a.KBL = nullptr; a.sw_on = 0; a.use_kpp_src = 0;
  for (int n = 0; n < 2; ++n) { a.TNEW[n] = nullptr; a.E[n] = T.COL[n][TRN_C_ADV]; a.F[n] = T.COL[n][TRN_C_HDIF]; a.D2N[n] = T.COL[n][TRN_C_VNF]; }   // the diagnostic form's outputs
  const StepParams sp = step_params(c);
  with_flags([&](auto GM, auto UP3) {
    hipLaunchKernelGGL((k_tracer_rhs<GM.value, UP3.value, false, 2, false, true>), grid_stencil(c), block_stencil(), 0, c->stream, c->g, sp, a);
  }, gm, up3);
  TrnArgs t{};
  for (int n = 0; n < 2; ++n) {
    t.TMIX[n] = c->TR[n][c->mixt];
    for (int f = 0; f < TRN_NCOL; ++f) t.COL[n][f] = T.COL[n][f];
    if (T.want[n]) t.tr[t.ntr++] = n;
  }
  if (T.COL[0][TRN_C_ADV_I]) { t.UI = c->gm.UISOP; t.VI = c->gm.VISOP; }
  if (T.COL[0][TRN_C_ADV_SM]) { t.US = c->subm.US; t.VS = c->subm.VS; if (!t.US || !t.VS) { c->err = "transport: USUBM / VSUBM do not exist"; return 1; } }
  t.lists = M.d_lists; t.blists = M.d_blists; t.cells = M.d_cells; t.bcells = M.d_bcells; t.ACC = T.ACC; t.BACC = T.BACC;
  t.dtavg = c->tavg.dtavg; t.nreg = M.aux.n_reg;
  if (t.UI || t.US) {
    t.HTE = c->d2["HTE"]; t.HTN = c->d2["HTN"];
    hipLaunchKernelGGL(k_trn_eddy, dim3((c->g.n2 + POP_RED_THREADS - 1) / POP_RED_THREADS, c->g.nblocks), dim3(POP_RED_THREADS), 0, c->stream, c->g, t);
  }
  const int nl = (int)M.loc_list.size(), nbl = (int)M.loc_blist.size();
  if (nl) hipLaunchKernelGGL(k_trn_bin, dim3(nl, t.ntr), dim3(POP_RED_THREADS), 0, c->stream, c->g, t);
  if (nbl) hipLaunchKernelGGL(k_trn_bnd, dim3(nbl, t.ntr), dim3(POP_RED_THREADS), 0, c->stream, c->g, t);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// pop_tavg_reset of the transports' stream
int trn_reset(pop_ctx *c) {
  TrnState &T = c->trn;
  const MocState &M = c->moc;
  if (T.ACC) HIPCHK(c, hipMemsetAsync(T.ACC, 0, std::max<size_t>(M.loc_list.size() * trn_per_list(c), 1) * sizeof(double), c->stream));
  if (T.BACC) HIPCHK(c, hipMemsetAsync(T.BACC, 0, std::max<size_t>(M.loc_blist.size() * trn_per_blist(c), 1) * sizeof(double), c->stream));
  T.set_sums.clear();
  return 0;
}

// the reduced unnormalised sums: bins [n][tracer][term][reg], then the boundary row of region 2 [tracer][term]
int trn_reduce(pop_ctx *c, std::vector<double> &sums) {
  TrnState &T = c->trn;
  return lat_aux_reduce(c, "transport", T.ACC, T.BACC, trn_per_list(c), trn_per_blist(c), &T.gather, T.set_sums, sums);
}

// compute_tracer_transports from the sums on (:1441-1581) for tracer tr (0 heat, 1 salt): scale, prefix over the bins, the total,
// the southern boundary of region 2, the heat units, the masks.  out[n][comp][reg]
void trn_finish(const pop_ctx *c, const std::vector<double> &sums, double factor, int tr, double *out) {
  const LatAux &A = c->moc.aux;
  const int N = A.n_lat, km = c->h.km, nc = c->trn.n_comp, nr = A.n_reg;
  auto O = [&](int n, int f, int m) -> double & { return out[((size_t)n * nc + f) * nr + m]; };   // 0-based
  auto B = [&](int n, int f, int m) { return sums[(((size_t)n * 2 + tr) * TRN_NBIN + f) * nr + m]; };
  std::fill(out, out + trn_n_out(c), 0.0);
  for (int n = 1; n <= N; ++n) for (int f = 1; f < nc; ++f) for (int m = 0; m < nr; ++m) O(n, f, m) = O(n - 1, f, m) + B(n - 1, f - 1, m) * factor;
  for (int n = 0; n <= N; ++n) for (int m = 0; m < nr; ++m) O(n, 0, m) = O(n, 1, m) + O(n, 2, m);
  if (nr > 1) {   // trans_s(2 | 4 | 5, 2)
    const double *bs = sums.data() + trn_n_bins(c) + (size_t)tr * TRN_NBND;
    const int comp[TRN_NBND] = {1, 3, 4};
    for (int f = 0; f < TRN_NBND; ++f) if (comp[f] < nc) for (int n = 0; n <= N; ++n) O(n, comp[f], 1) = O(n, comp[f], 1) + bs[f] * factor;
  }
  if (tr == 0) {
    const double conversion = 1.0e-19 / hflux_factor_of(c);
    for (size_t e = 0; e < trn_n_out(c); ++e) out[e] = out[e] * conversion;
  }
  auto masked = [&](int n, int m) { return A.mask[((size_t)n * km + 0) * nr + m] != 0; };   // MASK_LAT_DEPTH(n + 1, 1, m + 1)
  for (int m = 0; m < nr; ++m) {
    for (int n = 0; n + 1 < N; ++n) if (masked(n, m) && masked(n + 1, m)) for (int f = 0; f < nc; ++f) O(n + 1, f, m) = POP_UNDEFINED_NF;
    if (masked(0, m)) for (int f = 0; f < nc; ++f) O(0, f, m) = POP_UNDEFINED_NF;
    if (masked(N - 1, m)) for (int f = 0; f < nc; ++f) O(N, f, m) = POP_UNDEFINED_NF;
  }
  for (int m = 1; m < nr; ++m) for (int n = 0; n <= N; ++n) { O(n, 0, m) = POP_UNDEFINED_NF; O(n, 2, m) = POP_UNDEFINED_NF; }
}

int trn_factor(pop_ctx *c, int normalize, double *factor) {
  *factor = 1.0;
  if (!normalize) return 0;
  const double s = c->tavg.sum[c->trn.stream];
  if (s == 0.0) { c->err = "transport: cannot normalise: tavg_sum of stream " + std::to_string(c->trn.stream) + " is 0"; return 1; }
  *factor = 1.0 / s;
  return 0;
}
// pop_tavg_write(stream, path, 0): the normalised results, taken just before the stream is reset
int trn_snapshot(pop_ctx *c) {
  TrnState &T = c->trn;
  double factor;
  std::vector<double> sums;
  if (trn_factor(c, 1, &factor) || trn_reduce(c, sums)) return 1;
  for (int n = 0; n < 2; ++n) {
    T.snap[n].assign(trn_n_out(c), 0.0);
    trn_finish(c, sums, factor, n, T.snap[n].data());
  }
  T.have_snap = true;
  return 0;
}

}  // namespace
