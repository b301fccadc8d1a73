// launch_halo.hpp -- host side of the halo updates and of the global sums (part of pop_amd.hip, after pop_ctx.hpp).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// halo update of a device-resident field with nz levels (mpi/POP_HaloMod.F90:1732-2071 2-D,
// :2766-3211 3-D): local ghost copies + fills in one launch, then one packed message per peer
// ---------------------------------------------------------------------------------------------
// what the transport said about a failed exchange / all-reduce
std::string tr_err(const pop_ctx *c) { return c->rccl_tr ? ": " + c->rccl_tr->err : std::string(" in the host callback"); }
// one message per neighbour rank, `words` doubles per cell: the peer list and the offsets / counts an exchange callback takes
struct PeerSpans {
  std::vector<int> peer; std::vector<long long> soff, scnt, roff, rcnt;
  long long send_total = 0, recv_total = 0;
  PeerSpans(const pop_ctx *c, long long words) {
    for (auto &p : c->peers) {
      peer.push_back(p.rank); soff.push_back(send_total); scnt.push_back(p.nsend * words); roff.push_back(recv_total); rcnt.push_back(p.nrecv * words);
      send_total += p.nsend * words; recv_total += p.nrecv * words;
    }
  }
  bool fits(const pop_ctx *c) const { return send_total <= c->comm_doubles && recv_total <= c->comm_doubles; }
  int exchange(pop_ctx *c, pop_exchange_fn fn) { return fn(c->comm_user, (int)peer.size(), peer.data(), soff.data(), scnt.data(), roff.data(), rcnt.data()); }
};
// remote part only: one pack launch, the exchange, one unpack launch
int halo_remote(pop_ctx *c, double *F, int nz) {
  if (c->peers.empty()) return 0;
  const int n2 = c->g.n2;
  if (!c->xchg || !c->sendbuf) { c->err = "halo_update: multi-rank run without pop_set_comm"; return 1; }
  PeerSpans ps(c, nz);
  if (!ps.fits(c)) { c->err = "halo_update: comm buffer too small"; return 1; }
  if (c->nsend_all) hipLaunchKernelGGL(k_halo_pack_all, dim3((c->nsend_all + 255) / 256, nz), dim3(256), 0, c->stream, (const double *)F, c->sa_src, c->sa_start, c->sa_cnt, c->nsend_all, c->sendbuf, nz, n2);
  if (ps.exchange(c, c->xchg)) { c->err = "halo_update: exchange failed" + tr_err(c); return 1; }
  if (c->nrecv_all) hipLaunchKernelGGL(k_halo_unpack_all, dim3((c->nrecv_all + 255) / 256, nz), dim3(256), 0, c->stream, F, c->ra_dst, c->ra_start, c->ra_cnt, c->nrecv_all, (const double *)c->recvbuf, nz, n2);
  return 0;
}
int halo_update(pop_ctx *c, double *F, int nz, double fill = 0.0, int loc = 0, int kind = 0) {
  const int n2 = c->g.n2;
  if (halo_remote(c, F, nz)) return 1;
  const int nloc = c->ncopy + c->nfill;
  if (nloc) hipLaunchKernelGGL(k_halo_local, dim3((nloc + 255) / 256, nz), dim3(256), 0, c->stream, F, c->copy_dst, c->copy_src, c->ncopy, c->fill_dst, c->nfill, fill, nz, n2);
  if (c->h.c.ns_boundary == 2 && c->tp_n[loc]) {   // tripole northern boundary (mpi/POP_HaloMod.F90:1936-2050)
    const int n = c->tp_n[loc];
    if (nz > c->h.km + 2) { c->err = "halo_update: too many levels for the tripole buffer"; return 1; }
    hipLaunchKernelGGL(k_tripole_eval, dim3((n + 255) / 256, nz), dim3(256), 0, c->stream, (const double *)F, c->tp_a[loc], c->tp_b[loc], n, c->tp_buf,
                       kind == 0 ? 1.0 : -1.0, nz, n2);
    hipLaunchKernelGGL(k_tripole_store, dim3((n + 255) / 256, nz), dim3(256), 0, c->stream, F, c->tp_dst[loc], n, (const double *)c->tp_buf, nz, n2);
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}

// Several fields, one halo update: ONE message per neighbour rank carrying all of them (pack, exchange, unpack = three
// stream operations whatever the number of fields) and one launch for the ghost copies / fills inside the rank.
// Field by field the result is the one halo_update gives (same cells, same values).  fill value 0.
// loc / kind: POP_HaloUpdate's fieldLoc / fieldKind (0 centre, 1 NE corner, 2 N face, 3 E face; 0 scalar, 1 vector); they matter on a tripole boundary only
struct HaloItem { double *F; int nz; int loc = 0, kind = 0; };
HaloFields halo_fields(const std::vector<HaloItem> &items) {
  HaloFields H{};
  H.nf = (int)items.size();
  for (int f = 0; f < H.nf; ++f) { H.F[f] = items[f].F; H.nz[f] = items[f].nz; H.lev0[f] = H.nztot; H.nztot += items[f].nz; }
  return H;
}
int halo_update_many(pop_ctx *c, const std::vector<HaloItem> &items) {
  if (items.size() == 1 || items.size() > 8 || c->h.c.ns_boundary == 2 || c->f.halo_separate) {
    for (const HaloItem &it : items) if (halo_update(c, it.F, it.nz, 0.0, it.loc, it.kind)) return 1;
    return 0;
  }
  const HaloFields H = halo_fields(items);
  const int n2 = c->g.n2, tot = H.nztot;
  if (!c->peers.empty()) {
    if (!c->xchg || !c->sendbuf) { c->err = "halo_update: multi-rank run without pop_set_comm"; return 1; }
    PeerSpans ps(c, tot);
    if (!ps.fits(c)) {   // buffers of an older host framework: field by field
      for (const HaloItem &it : items) if (halo_update(c, it.F, it.nz)) return 1;
      return 0;
    }
    if (c->nsend_all) hipLaunchKernelGGL(k_halo_pack_many, dim3((c->nsend_all + 255) / 256, tot), dim3(256), 0, c->stream, H, c->sa_src, c->sa_start, c->sa_cnt, c->nsend_all, c->sendbuf, n2);
    if (ps.exchange(c, c->xchg)) { c->err = "halo_update: exchange failed" + tr_err(c); return 1; }
    if (c->nrecv_all) hipLaunchKernelGGL(k_halo_unpack_many, dim3((c->nrecv_all + 255) / 256, tot), dim3(256), 0, c->stream, H, c->ra_dst, c->ra_start, c->ra_cnt, c->nrecv_all, (const double *)c->recvbuf, n2);
  }
  const int nloc = c->ncopy + c->nfill;
  if (nloc) hipLaunchKernelGGL(k_halo_local_many, dim3((nloc + 255) / 256, tot), dim3(256), 0, c->stream, H, c->copy_dst, c->copy_src, c->ncopy, c->fill_dst, c->nfill, 0.0, n2);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// The same update in two halves around work that does not need the ghost cells of other ranks (north_star: "halo updates
// ... overlapped with interior stencil work on a second HIP stream").  begin: ghost copies inside the rank, pack, and the
// exchange on the communication stream (second communicator); end: unpack and the ghost copies again (corner ghosts
// take values that just arrived; the others are rewritten with the same values).  Between the two the launch stream
// may run anything that reads only cells this rank owns or ghosts with a source on this rank.
bool halo_async_ok(const pop_ctx *c) {
  return !c->peers.empty() && c->halo_ns_only && c->xchg_side && c->comm_side && c->h.c.ns_boundary != 2 && c->f.halo_overlap;
}
struct HaloAsync { HaloFields H; int tot; };
int halo_many_begin(pop_ctx *c, const std::vector<HaloItem> &items, HaloAsync &A) {
  const HaloFields &H = A.H = halo_fields(items);
  const int n2 = c->g.n2, nloc = c->ncopy + c->nfill, tot = A.tot = H.nztot;
  PeerSpans ps(c, tot);
  if (!ps.fits(c)) { c->err = "halo_update: comm buffer too small"; return 1; }
  if (nloc) hipLaunchKernelGGL(k_halo_local_many, dim3((nloc + 255) / 256, tot), dim3(256), 0, c->stream, H, c->copy_dst, c->copy_src, c->ncopy, c->fill_dst, c->nfill, 0.0, n2);
  if (c->nsend_all) hipLaunchKernelGGL(k_halo_pack_many, dim3((c->nsend_all + 255) / 256, tot), dim3(256), 0, c->stream, H, c->sa_src, c->sa_start, c->sa_cnt, c->nsend_all, c->sendbuf, n2);
  HIPCHK(c, hipEventRecord(c->ev_sa, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->comm_side, c->ev_sa, 0));
  if (ps.exchange(c, c->xchg_side)) { c->err = "halo_update: exchange failed" + tr_err(c); return 1; }
  HIPCHK(c, hipEventRecord(c->ev_sx, c->comm_side));
  return 0;
}
int halo_many_end(pop_ctx *c, const HaloAsync &A) {
  const int n2 = c->g.n2, nloc = c->ncopy + c->nfill;
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_sx, 0));
  if (c->nrecv_all) hipLaunchKernelGGL(k_halo_unpack_many, dim3((c->nrecv_all + 255) / 256, A.tot), dim3(256), 0, c->stream, A.H, c->ra_dst, c->ra_start, c->ra_cnt, c->nrecv_all, (const double *)c->recvbuf, n2);
  if (nloc) hipLaunchKernelGGL(k_halo_local_many, dim3((nloc + 255) / 256, A.tot), dim3(256), 0, c->stream, A.H, c->copy_dst, c->copy_src, c->ncopy, c->fill_dst, c->nfill, 0.0, n2);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// stage 2+3 of a reduction whose partials are already in c->partial
template <int NF>
int reduce_finish(pop_ctx *c, int mode) {
  double *bs = c->blocksum;
  if (c->h.nranks > 1) {
    if (!c->allred || !c->redbuf) { c->err = "global sum: multi-rank run without pop_set_comm"; return 1; }
    bs = c->redbuf;
    hipLaunchKernelGGL(k_block_sums_global<NF>, dim3(c->h.nblocks_tot), dim3(POP_RED_THREADS), 0, c->stream, c->partial, c->nchunk, c->loc_of_gid, bs);
  } else hipLaunchKernelGGL(k_block_sums<NF>, dim3(c->g.nblocks), dim3(POP_RED_THREADS), 0, c->stream, c->partial, c->nchunk, c->gid, bs);
  if (c->h.nranks > 1 && c->allred(c->comm_user, 0, (long long)NF * c->h.nblocks_tot)) { c->err = "global sum: allreduce callback failed" + tr_err(c); return 1; }
  hipLaunchKernelGGL(k_finalize<NF>, dim3(1), dim3(1), 0, c->stream, bs, c->h.nblocks_tot, c->sc, mode);
  HIPCHK(c, hipGetLastError());
  return 0;
}
int read_scalars(pop_ctx *c, SolverScalars *out) {
  HIPCHK(c, hipMemcpyAsync(out, c->sc, sizeof(SolverScalars), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
// the tail every global sum shares: partials in c->partial -> the total on the host
template <int NF>
int finish_sum(pop_ctx *c, int mode, double *result) {
  if (reduce_finish<NF>(c, mode)) return 1;
  SolverScalars s;
  if (read_scalars(c, &s)) return 1;
  *result = s.sum0;
  return 0;
}
// a tripole grid and an N-face or NE-corner field: the redundant half of the top row counts once (mpi/POP_ReductionsMod.F90:308-341)
bool top_row_once(const pop_ctx *c, int field_loc) { return c->h.c.ns_boundary == 2 && (field_loc == 1 || field_loc == 2); }
// b4b global sum of A [* B] [* M] over the physical domain, result on the host.  once: the tripole rule; that kernel has no B operand
int masked_sum(pop_ctx *c, const double *A, const double *B, const double *M, bool once, double *result) {
  if (once && B) { c->err = "global sum: the product of two fields has no form with the tripole top-row rule"; return 1; }
  if (once) {
    hipLaunchKernelGGL(k_dot_partial_dup, grid_2d(c), dim3(POP_RED_THREADS), 0, c->stream, c->g, A, M, (const double *)c->d2["TRIPOLE_DUP"], c->partial);
    return finish_sum<2>(c, FIN_TRIPOLE, result);
  }
  hipLaunchKernelGGL(k_dot_partial, grid_2d(c), dim3(POP_RED_THREADS), 0, c->stream, c->g, A, B, M, c->partial);
  return finish_sum<1>(c, FIN_PLAIN, result);
}

}  // namespace
