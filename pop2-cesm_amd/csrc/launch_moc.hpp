// launch_moc.hpp -- meridional overturning circulation (compute_moc, diags_on_lat_aux_grid.F90:942-1288): the request, the site of a
// step and what the getters make of the accumulators.  Part of the single translation unit pop_amd.hip (included before
// launch_tavg.hpp, whose stream reset also zeroes these sums).
//
// Site "tavg_moc": end of pop_baroclinic_driver, beside diag_cfl.  U, V (cur) and DH are the ones advt saw -- the VVEL that tavg_state
// accumulates in the same step and the WTK that advection.F90:1750 accumulates as WVEL; WISOP / VISOP and WSUBM / VSUBM are the stored
// fields tavg_hmix reads.  MocState::active is the host flag a step tests.  Three launches (kernels_moc.hpp), nothing copied, no
// synchronisation.  Accumulators live per (block, bin): the getter copies them to the host, places them in the vector of all lists
// of the decomposition, sums that vector over the ranks (exact: one rank owns each entry), and finishes in the reference's order --
// within a bin the blocks are added in block-id order, so the result does not depend on how blocks are spread over ranks.
#pragma once

namespace {

size_t moc_per_list(const pop_ctx *c) { return (size_t)c->h.km * c->moc.aux.n_comp * c->moc.aux.n_reg; }
size_t moc_per_blist(const pop_ctx *c) { return (size_t)c->h.km * c->moc.aux.n_comp; }
size_t moc_n_bins(const pop_ctx *c) { return (size_t)c->moc.aux.n_lat * moc_per_list(c); }
size_t moc_n_sums(const pop_ctx *c) { return moc_n_bins(c) + (c->moc.aux.n_reg > 1 ? moc_per_blist(c) : 0); }
size_t moc_n_out(const pop_ctx *c) { const LatAux &A = c->moc.aux; return (size_t)(A.n_lat + 1) * (c->h.km + 1) * A.n_comp * A.n_reg; }

int moc_inited(pop_ctx *c, const char *who) {
  if (c->moc.aux.inited) return 0;
  c->err = std::string(who) + ": pop_init_transports has not been called";
  return 1;
}

// the lists of this rank's blocks on the device, once: the MOC and the tracer transports walk the same lists
int moc_lists_upload(pop_ctx *c) {
  MocState &M = c->moc;
  const LatAux &A = M.aux;
  if (M.lists_up) return 0;
  auto local = [&](const std::vector<MocList> &all, const std::vector<int> &cells, std::vector<int> &pick, MocList **d_lists, int **d_cells) {
    std::vector<MocList> loc;
    std::vector<int> lc;
    pick.clear();
    for (size_t l = 0; l < all.size(); ++l) {
      const MocList &L = all[l];
      if (c->h.block_owner[L.block] != c->h.rank) continue;
      pick.push_back((int)l);
      loc.push_back(MocList{c->h.block_local[L.block], L.bin, (int)lc.size(), L.cnt});
      lc.insert(lc.end(), cells.begin() + L.off, cells.begin() + L.off + L.cnt);
    }
    return dev_upload(c, d_lists, loc.data(), loc.size()) || dev_upload(c, d_cells, lc.data(), lc.size());
  };
  if (local(A.lists, A.cells, M.loc_list, &M.d_lists, &M.d_cells) || local(A.blists, A.bcells, M.loc_blist, &M.d_blists, &M.d_bcells)) return 1;
  M.lists_up = true;
  return 0;
}
// the accumulators and the scratch field
int moc_alloc(pop_ctx *c) {
  MocState &M = c->moc;
  const LatAux &A = M.aux;
  if (moc_lists_upload(c)) return 1;
  if (dev_alloc(c, &M.ACC, M.loc_list.size() * moc_per_list(c)) || dev_alloc(c, &M.BACC, M.loc_blist.size() * moc_per_blist(c))) return 1;
  if (dev_alloc(c, &M.WE, (size_t)c->h.n3 * c->h.nblocks, false)) return 1;
  if (A.n_comp > 1 && !c->d2.count("HTN")) {
    std::vector<double> htn = local_part(c->h, c->h.f2.at("HTN"));
    if (dev_upload(c, &c->d2["HTN"], htn.data(), htn.size())) return 1;
  }
  return 0;
}

// the site, once, with the current dtavg, on the launch stream.  Callers inside a step test c->moc.active first
int moc_site(pop_ctx *c) {
  MocState &M = c->moc;
  if (!M.active) return 0;
  const pop_config &cf = c->h.c;
  const LatAux &A = M.aux;
  MocArgs a{};
  a.U = c->U[c->curt]; a.V = c->V[c->curt]; a.DH = c->DH;
  if (A.n_comp > 1) {
    if (cf.hmix_tracer == 3 && cf.gm_diag_bolus) { a.W2 = c->gm.WISOP; a.V2 = c->gm.VISOP; }
    a.HTN = c->d2["HTN"];
  }
  if (A.n_comp > 2) { a.W3 = c->subm.WS; a.V3 = c->subm.VS; if (!a.W3 || !a.V3) { c->err = "moc: WSUBM / VSUBM do not exist"; return 1; } }
  a.WE = M.WE; a.lists = M.d_lists; a.blists = M.d_blists; a.cells = M.d_cells; a.bcells = M.d_bcells; a.ACC = M.ACC; a.BACC = M.BACC;
  a.dtavg = c->tavg.dtavg; a.nreg = A.n_reg;
  const int km = c->g.km, nl = (int)M.loc_list.size(), nbl = (int)M.loc_blist.size();
  hipLaunchKernelGGL(k_moc_w, dim3((c->g.n2 + POP_RED_THREADS - 1) / POP_RED_THREADS, c->g.nblocks), dim3(POP_RED_THREADS), 0, c->stream, c->g, a);
  with_value<1, 2, 3>(A.n_comp, [&](auto NC) {
    if (nl) hipLaunchKernelGGL(k_moc_bin<decltype(NC)::value>, dim3(nl, km), dim3(POP_RED_THREADS), 0, c->stream, c->g, a);
    if (nbl) hipLaunchKernelGGL(k_moc_bnd<decltype(NC)::value>, dim3(nbl, km), dim3(POP_RED_THREADS), 0, c->stream, c->g, a);
  });
  HIPCHK(c, hipGetLastError());
  return 0;
}
// pop_run_phase / pop_time_phase
int moc_phase(pop_ctx *c) {
  if (!c->moc.requested) { c->err = "tavg_moc: pop_moc_request has not been called"; return 1; }
  return moc_site(c);
}

// pop_tavg_reset of the MOC's stream
int moc_reset(pop_ctx *c) {
  MocState &M = c->moc;
  if (M.ACC) HIPCHK(c, hipMemsetAsync(M.ACC, 0, std::max<size_t>(M.loc_list.size() * moc_per_list(c), 1) * sizeof(double), c->stream));
  if (M.BACC) HIPCHK(c, hipMemsetAsync(M.BACC, 0, std::max<size_t>(M.loc_blist.size() * moc_per_blist(c), 1) * sizeof(double), c->stream));
  M.set_sums.clear();
  return 0;
}

// per-(block, bin) accumulators on the lists of pop_init_transports (pl numbers per bin list in ACC, pb per boundary-row list in
// BACC) -> the reduced unnormalised sums: the bins [n][pl], then the boundary row of region 2 [pb].  Shared by the MOC and the
// tracer transports (launch_transport.hpp); gather: the caller's device buffer of a multi-rank reduce
int lat_aux_reduce(pop_ctx *c, const char *who, const double *ACC, const double *BACC, size_t pl, size_t pb, double **gather,
                   const std::vector<double> &set_sums, std::vector<double> &sums) {
  const MocState &M = c->moc;
  const LatAux &A = M.aux;
  const size_t nL = A.lists.size(), boff = nL * pl, nbins = (size_t)A.n_lat * pl;
  std::vector<double> G(nL * pl + A.blists.size() * pb, 0.0), loc(std::max(M.loc_list.size() * pl, M.loc_blist.size() * pb));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!M.loc_list.empty()) HIPCHK(c, hipMemcpy(loc.data(), ACC, M.loc_list.size() * pl * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < M.loc_list.size(); ++i) std::copy(loc.begin() + i * pl, loc.begin() + (i + 1) * pl, G.begin() + (size_t)M.loc_list[i] * pl);
  if (!M.loc_blist.empty()) HIPCHK(c, hipMemcpy(loc.data(), BACC, M.loc_blist.size() * pb * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < M.loc_blist.size(); ++i) std::copy(loc.begin() + i * pb, loc.begin() + (i + 1) * pb, G.begin() + boff + (size_t)M.loc_blist[i] * pb);
  if (c->h.nranks > 1 && !G.empty()) {   // as diag_publish: through the reduce buffer, in pieces of its size
    if (!c->allred || !c->redbuf || c->red_doubles < 1) { c->err = std::string(who) + ": multi-rank run without a transport"; return 1; }
    if (!*gather && dev_alloc(c, gather, G.size(), false)) return 1;
    HIPCHK(c, hipMemcpyAsync(*gather, G.data(), G.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    for (size_t off = 0; off < G.size(); off += (size_t)c->red_doubles) {
      const size_t cnt = std::min(G.size() - off, (size_t)c->red_doubles);
      HIPCHK(c, hipMemcpyAsync(c->redbuf, *gather + off, cnt * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
      if (c->allred(c->comm_user, 0, (long long)cnt)) { c->err = std::string(who) + ": allreduce failed" + tr_err(c); return 1; }
      HIPCHK(c, hipMemcpyAsync(*gather + off, c->redbuf, cnt * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(G.data(), *gather, G.size() * sizeof(double), hipMemcpyDeviceToHost));
  }
  sums.assign(nbins + (A.n_reg > 1 ? pb : 0), 0.0);
  for (size_t l = 0; l < nL; ++l) {   // (block id, bin) order: within a bin the blocks in block-id order
    double *s = sums.data() + (size_t)A.lists[l].bin * pl;
    for (size_t e = 0; e < pl; ++e) s[e] = s[e] + G[l * pl + e];
  }
  if (A.n_reg > 1)
    for (size_t l = 0; l < A.blists.size(); ++l) {
      double *s = sums.data() + nbins;
      for (size_t e = 0; e < pb; ++e) s[e] = s[e] + G[boff + l * pb + e];
    }
  if (!set_sums.empty()) for (size_t e = 0; e < sums.size(); ++e) sums[e] = sums[e] + set_sums[e];
  return 0;
}
// the MOC's: bins [n][k][comp][reg], then the boundary row of region 2 [k][comp]
int moc_reduce(pop_ctx *c, std::vector<double> &sums) {
  MocState &M = c->moc;
  return lat_aux_reduce(c, "moc", M.ACC, M.BACC, moc_per_list(c), moc_per_blist(c), &M.gather, M.set_sums, sums);
}

// compute_moc from the sums on (:1054-1189): scale, prefix over the bins, southern boundary of region 2, Sverdrups
void moc_finish(const pop_ctx *c, const std::vector<double> &sums, double factor, double *out) {
  const LatAux &A = c->moc.aux;
  const int N = A.n_lat, km = c->h.km, nc = A.n_comp, nr = A.n_reg;
  auto O = [&](int n, int k, int f, int m) -> double & { return out[(((size_t)n * (km + 1) + k) * nc + f) * nr + m]; };   // 0-based
  std::fill(out, out + moc_n_out(c), 0.0);
  for (int n = 1; n <= N; ++n) for (int k = 0; k < km; ++k) for (int f = 0; f < nc; ++f) for (int m = 0; m < nr; ++m)
    O(n, k, f, m) = O(n - 1, k, f, m) + sums[(((size_t)(n - 1) * km + k) * nc + f) * nr + m] * factor;
  if (nr > 1) {
    const double *bs = sums.data() + moc_n_bins(c);
    for (int f = 0; f < nc; ++f) {
      std::vector<double> moc_s(km + 1, 0.0);
      moc_s[km - 1] = -c->h.dz[km] * (bs[(size_t)(km - 1) * nc + f] * factor);
      for (int k = km - 1; k >= 1; --k) moc_s[k - 1] = moc_s[k] - c->h.dz[k] * (bs[(size_t)(k - 1) * nc + f] * factor);
      for (int k = 0; k < km; ++k) for (int n = 0; n <= N; ++n) O(n, k, f, 1) = O(n, k, f, 1) + moc_s[k];
    }
  }
  for (size_t e = 0; e < moc_n_out(c); ++e) out[e] = out[e] * 1.0e-12;
}

int moc_factor(pop_ctx *c, int normalize, double *factor) {
  *factor = 1.0;
  if (!normalize) return 0;
  const double s = c->tavg.sum[c->moc.stream];
  if (s == 0.0) { c->err = "moc: cannot normalise: tavg_sum of stream " + std::to_string(c->moc.stream) + " is 0"; return 1; }
  *factor = 1.0 / s;
  return 0;
}
// pop_tavg_write(stream, path, 0): the normalised result, taken just before the stream is reset
int moc_snapshot(pop_ctx *c) {
  MocState &M = c->moc;
  double factor;
  std::vector<double> sums;
  if (moc_factor(c, 1, &factor) || moc_reduce(c, sums)) return 1;
  M.snap.assign(moc_n_out(c), 0.0);
  moc_finish(c, sums, factor, M.snap.data());
  M.have_snap = true;
  return 0;
}

}  // namespace
