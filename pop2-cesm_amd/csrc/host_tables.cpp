// host_tables.cpp -- the index lists and rewritten tables context creation uploads (create_device.hpp), each a pure function of
// the host model: land-elimination prefix counts, the chunk lists of the fused solvers, the concatenated peer lists and per-cell
// message maps, the EVP tables of the local blocks, the off-centre operator weights with their first row and column, the byte
// mask and the P-CSI omega table.  No HIP.  The order of every list is part of the result: the solver's summation order and the
// placement of workgroups on the XCDs follow it.
#include "pop_internal.hpp"

namespace pop {

// Land elimination (DevGrid::opre): prefix count of the cells that have an ocean T cell within two cells in either direction.
// The margin is what makes the skipped values independent of the state: every field the full kernels write on a cell further
// than one stencil from any ocean cell (tgrid_to_ugrid averages, gradients at land U points, ...) is a constant.  Ghost cells
// count with the KMT their halo update gave them.
std::vector<int> land_prefix(const HostModel &h, double &land_fraction) {
  const std::vector<int> kmt = local_part(h, h.i2.at("KMT"));
  std::vector<int> pre((size_t)(h.n2 + 1) * h.nblocks);
  long long tiles = 0, land = 0;
  for (int b = 0; b < h.nblocks; ++b) {
    const int *K = kmt.data() + (size_t)b * h.n2;
    int *P = pre.data() + (size_t)b * (h.n2 + 1);
    const BlockInfo &B = h.all_blocks[h.local_ids[b] - 1];
    P[0] = 0;
    for (int j = 0; j < h.nyb; ++j)
      for (int i = 0; i < h.nxb; ++i) {
        // ghost cells beyond a closed boundary are rewritten with the fill value by every halo update and recomputed by the
        // whole-block kernels of averaging steps: their values do depend on the step, so they count as cells to compute
        int near = (B.i_glob[i] == 0 || B.j_glob[j] == 0) ? 1 : 0;
        for (int dj = -2; dj <= 2 && !near; ++dj)
          for (int di = -2; di <= 2; ++di) {
            const int ii = i + di, jj = j + dj;
            if (ii >= 0 && ii < h.nxb && jj >= 0 && jj < h.nyb && K[(size_t)jj * h.nxb + ii] > 0) { near = 1; break; }
          }
        P[(size_t)j * h.nxb + i + 1] = P[(size_t)j * h.nxb + i] + near;
      }
    for (int j = 0; j < h.nyb; ++j)
      for (int i0 = 0; i0 < h.nxb; i0 += 64) {
        const int i1 = std::min(i0 + 64, h.nxb);
        ++tiles;
        if (P[(size_t)j * h.nxb + i1] == P[(size_t)j * h.nxb + i0]) ++land;
      }
  }
  land_fraction = tiles ? (double)land / (double)tiles : 0.0;
  return pre;
}

// DevGrid::red_act: the chunks (256 consecutive cells) the fused solver kernels have to visit
ChunkLists solver_chunk_lists(const HostModel &h, const std::vector<int> &pre) {
  ChunkLists out;
  const int nc = (int)((h.n2 + 255) / 256), ib = NGHOST + 1, jb = NGHOST + 1;
  const bool multi = h.nranks > 1;
  std::vector<std::vector<int>> act(h.nblocks), land(h.nblocks);
  size_t longest = 0;
  for (int b = 0; b < h.nblocks; ++b) {
    const int *P = pre.data() + (size_t)b * (h.n2 + 1);
    for (int k = 0; k < nc; ++k) {
      const long long p0 = 256LL * k, p1 = std::min<long long>(p0 + 256, (long long)h.n2);
      bool is_land = P[p1] == P[p0];
      if (is_land && multi) {   // as red_land(g, deep): chunks within NGHOST of the edge of the physical domain work for other ranks
        const int j0 = (int)(p0 / h.nxb), j1 = (int)((p1 - 1) / h.nxb);
        const int i0 = (j0 == j1) ? (int)(p0 % h.nxb) : 0, i1 = (j0 == j1) ? (int)((p1 - 1) % h.nxb) : h.nxb - 1;
        const BlockInfo &Bk = h.all_blocks[h.local_ids[b] - 1];
        is_land = i0 >= ib - 1 + NGHOST && i1 <= Bk.ie - 1 - NGHOST && j0 >= jb - 1 + NGHOST && j1 <= Bk.je - 1 - NGHOST;
      }
      (is_land && !(b == 0 && k == 0) ? land[b] : act[b]).push_back(k);
    }
    longest = std::max(longest, act[b].size());
    out.active_total += (int)act[b].size();
  }
  // launch order: workgroup w runs on XCD w % 8; XCD x takes one contiguous band of the chunks with ocean (as red_band does
  // for the full launch), so the rows j +- 1 of the 9-point matvec are in the L2 that fetched row j.  The publishing workgroup
  // (0,0) stays chunk 0.  Padding (land chunks) fills each band up to the common length.
  longest = 16 * ((longest + 15) / 16);   // multiple of 16: k_fpcg_a_pair takes entries e and e + 8
  std::vector<int> list((size_t)longest * h.nblocks);
  bool can_pad = true;
  for (int b = 0; b < h.nblocks; ++b) if (act[b].size() + land[b].size() < longest) can_pad = false;
  for (int b = 0; b < h.nblocks && can_pad; ++b) {
    std::vector<int> seq = act[b];
    for (size_t w = act[b].size(); w < longest; ++w) seq.push_back(land[b][w - act[b].size()]);   // shorter list => it has land chunks to pad with
    const size_t per = longest / 8;
    for (size_t w = 0; w < longest; ++w) list[(size_t)b * longest + (w % per) * 8 + w / per] = seq[w];
  }
  if (!can_pad) longest = (size_t)nc;   // no list
  if (longest < (size_t)nc) {
    out.cnt.resize(h.nblocks);
    for (int b = 0; b < h.nblocks; ++b) out.cnt[b] = (int)act[b].size();
    out.list = std::move(list);
    out.nact = (int)longest;
  }
  return out;
}

PeerLists peer_lists(const HaloPlan &p) {
  PeerLists L;
  for (auto &pp : p.peers) {
    const int s0 = (int)L.ss.size(), r0 = (int)L.rd.size();
    for (int v : pp.send_src) { L.ss.push_back(v); L.st.push_back(s0); L.sc.push_back((int)pp.send_src.size()); }
    for (int v : pp.recv_dst) { L.rd.push_back(v); L.rt.push_back(r0); L.rc.push_back((int)pp.recv_dst.size()); }
  }
  return L;
}

// per-cell maps of the same lists for the kernels that pack / read a one-level message themselves
PeerCellMaps peer_cell_maps(const PeerLists &L, size_t ncells) {
  PeerCellMaps M;
  M.smap.assign(ncells, -1); M.rmap.assign(ncells, -1); M.off.assign(1, 0);
  std::map<int, std::vector<int>> by_cell;
  for (size_t t = 0; t < L.ss.size(); ++t) by_cell[L.ss[t]].push_back((int)t);
  for (auto &kv : by_cell) { M.smap[kv.first] = (int)M.off.size() - 1; for (int t : kv.second) M.slot.push_back(t); M.off.push_back((int)M.slot.size()); }
  for (size_t t = 0; t < L.rd.size(); ++t) M.rmap[L.rd[t]] = (int)t;
  return M;
}

// the same answer on every rank (the overlapped update uses the second communicator: all ranks or none): every
// block's east neighbour -- the cyclic one included -- is owned by the block's own rank, i.e. the shards are j-bands
bool halo_ns_only(const HostModel &h) {
  for (const BlockInfo &B : h.all_blocks) {
    int ie = B.iblock + 1;
    if (ie > h.nbx) { if (h.c.ew_boundary != 1) continue; ie = 1; }
    for (const BlockInfo &E : h.all_blocks)
      if (E.jblock == B.jblock && E.iblock == ie && h.block_owner[E.block_id - 1] != h.block_owner[B.block_id - 1]) return false;
  }
  return true;
}

// EVP sub-blocks of the local blocks, coefficient arrays transposed to [cell][sub-block]
EvpTables evp_tables(const HostModel &h) {
  const EvpHost &E = h.evp;
  const size_t nsb = (size_t)E.xnb * E.ynb, S = nsb * h.nblocks;
  constexpr int NC = EVP_LD * EVP_LD, NR = EVP_LE * EVP_LE;
  EvpTables T;
  T.S = S;
  T.meta.resize(4 * S);
  T.cc.resize(S * NC); T.ne.resize(S * NC); T.icc.resize(S * NC); T.ine.resize(S * NC); T.rinv.resize(S * NR);
  const std::vector<int> &KMT = h.i2.at("KMT");
  for (int lb = 0; lb < h.nblocks; ++lb) {
    const size_t gb = (size_t)h.local_ids[lb] - 1;
    for (int j = 1; j <= E.ynb; ++j) for (int i = 1; i <= E.xnb; ++i) {
      const size_t sl = lb * nsb + (size_t)(j - 1) * E.xnb + (i - 1), sg = gb * nsb + (size_t)(j - 1) * E.xnb + (i - 1);
      const int is = E.xidx[i], ie = E.xidx[i + 1] + 1, js = E.yidx[j], je = E.yidx[j + 1] + 1;
      int ocean = 0;   // w: no ocean cell in the interior of the sub-block (cells of no block at all count as land)
      for (int cj = js + 1; cj <= je - 1; ++cj) for (int ci = is + 1; ci <= ie - 1; ++ci)
        if (KMT[gb * h.n2 + (size_t)(cj - 1) * h.nxb + (ci - 1)] > 0) ocean = 1;
      int *m = &T.meta[4 * sl];
      m[0] = (int)(lb * h.n2 + (size_t)(js - 1) * h.nxb + (is - 1)); m[1] = (ie - is + 1) | ((je - js + 1) << 8);
      m[2] = E.land[sg]; m[3] = (E.land[sg] && !ocean) ? 1 : 0;
      for (int q = 0; q < NC; ++q) {
        T.cc[q * S + sl] = E.cc[sg * NC + q]; T.ne[q * S + sl] = E.ne[sg * NC + q];
        T.icc[q * S + sl] = E.icc[sg * NC + q]; T.ine[q * S + sl] = E.ine[sg * NC + q];
      }
      for (int q = 0; q < NR; ++q) T.rinv[q * S + sl] = E.rinv[sg * NR + q];
    }
  }
  return T;
}

// The reference forms the off-centre weights from i = 2, j = 2 of the block array on (POP_SolversMod.F90:795-815); the
// first row and column stay 0 and nothing reads them.  The two-iterations-per-launch P-CSI across ranks forms the operator at the
// first ring of ghost cells, whose west / south weights live in that row and column: the device copy holds them, made of the
// same two U-point terms in the same order.  The host copy keeps the reference's values.
std::vector<double> btrop_wgt_ring(const HostModel &h, int wgt) {
  std::vector<double> all = h.f2.at(wgt == 1 ? "btropWgtNE" : wgt == 2 ? "btropWgtEast" : "btropWgtNorth");
  const std::vector<double> &XW = h.f2.at("btropXW"), &YW = h.f2.at("btropYW");
  const int nxb = h.nxb, nyb = h.nyb;
  const size_t n2 = (size_t)nxb * nyb;
  for (size_t b = 0; b < all.size() / n2; ++b)
    for (int j = 0; j < nyb; ++j) for (int i = 0; i < nxb; ++i) {
      if (i > 0 && j > 0) continue;
      const size_t q = b * n2 + (size_t)j * nxb + i;
      if (wgt == 1) all[q] = XW[q] + YW[q];
      else if (wgt == 2 && j > 0) all[q] = XW[q] + XW[q - nxb] - YW[q] - YW[q - nxb];
      else if (wgt == 3 && i > 0) all[q] = YW[q] + YW[q - 1] - XW[q] - XW[q - 1];
    }
  return all;
}

// byte copy of a mask (RCALCT: exactly 0 or 1, POP_SolversMod.F90:886)
int mask_bytes(const std::vector<double> &m, std::vector<unsigned char> &m8) {
  m8.resize(m.size());
  for (size_t p = 0; p < m.size(); ++p) {
    if (m[p] != 0.0 && m[p] != 1.0) return 1;
    m8[p] = m[p] != 0.0;
  }
  return 0;
}

// omega_k of P-CSI (POP_SolversMod.F90:1617-1620, 1695): a function of the eigenvalue bounds only
std::vector<double> pcsi_omega(const HostModel &h, double &csy) {
  const double csalpha = 2.0 / (h.pcsi_max_eig - h.pcsi_min_eig);
  const double csbeta = (h.pcsi_max_eig + h.pcsi_min_eig) / (h.pcsi_max_eig - h.pcsi_min_eig);
  csy = csbeta / csalpha;
  std::vector<double> om(h.c.max_iterations + 2);
  om[0] = 1.0 / csy;
  double csomga = 2.0 / csy;
  for (int m = 1; m <= h.c.max_iterations; ++m) { csomga = 1.0 / (csy - csomga / (4.0 * csalpha * csalpha)); om[m] = csomga; }
  return om;
}

}  // namespace pop
