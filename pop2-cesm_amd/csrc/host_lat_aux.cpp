// host_lat_aux.cpp -- init-time part of the transport diagnostics (diags_on_lat_aux_grid.F90): the auxiliary latitude grid of
// init_lat_aux_grid (:121-597), the region masks, the southern boundary of region 2, MASK_LAT_DEPTH and n_moc_comp of
// init_moc_ts_transport_arrays (:603-936), and the cell lists the device walks (kernels_moc.hpp).  The reference works on the
// gathered global arrays TLATD_G, ULATD_G, KMT and REGION_MASK; they are assembled here from the host grid fields of all blocks,
// which every rank holds.  No HIP: a host-only context takes pop_init_transports too.
#include <algorithm>
#include "pop_internal.hpp"

namespace pop {

void transports_nml_defaults(pop_transports_nml &n) {   // :222-230
  std::memset(&n, 0, sizeof n);
  n.struct_bytes = (int)sizeof(pop_transports_nml);
  n.lat_aux_grid_type = 0; n.lat_aux_begin = -90.0; n.lat_aux_end = 90.0; n.n_lat_aux_grid = 180; n.n_transport_reg = 2;
}

int host_lat_aux_build(const HostModel &h, const pop_transports_nml &nml, const int *region_mask, LatAux &L, std::string &err) {
  const pop_config &cf = h.c;
  const int nx = cf.nx_global, ny = cf.ny_global, km = h.km, nxb = h.nxb;
  const size_t n2 = h.n2;
  const double pi = 4.0 * std::atan(1.0), radian = 180.0 / pi, eps_grid = 1.0e-7;
  auto fail = [&](const std::string &s) { err = s; return 1; };
  L = LatAux{};
  L.nml = nml;
  const int type = nml.lat_aux_grid_type;
  if (type < 0 || type > 2) return fail("(init_lat_aux_grid) unknown auxilary latitudinal grid choice");
  if (cf.partial_bottom_cells)
    return fail("(init_lat_aux_grid): if (partial_bottom_cells), then 1st modify  subroutines compute_moc and compute_tracer_transports");
  // the gathered global arrays, (ny_global, nx_global) with i fastest
  std::vector<double> TLATD((size_t)nx * ny, 0.0), ULATD((size_t)nx * ny, 0.0);
  std::vector<int> KMT((size_t)nx * ny, 0);
  {
    const std::vector<double> &TLAT = h.f2.at("TLAT"), &ULAT = h.f2.at("ULAT");
    const std::vector<int> &kmt = h.i2.at("KMT");
    for (int b = 0; b < h.nblocks_tot; ++b) {
      const BlockInfo &B = h.all_blocks[b];
      for (int j = B.jb; j <= B.je; ++j) for (int i = B.ib; i <= B.ie; ++i) {
        const int ig = B.i_glob[i - 1], jg = B.j_glob[j - 1];
        if (ig < 1 || jg < 1) continue;   // padding
        const size_t p = (size_t)b * n2 + (size_t)(j - 1) * nxb + (i - 1), q = (size_t)(jg - 1) * nx + (ig - 1);
        TLATD[q] = TLAT[p] * radian; ULATD[q] = ULAT[p] * radian; KMT[q] = kmt[p];
      }
    }
  }
  auto T = [&](int i, int j) { return TLATD[(size_t)(j - 1) * nx + (i - 1)]; };   // 1-based, as the reference
  auto U = [&](int i, int j) { return ULATD[(size_t)(j - 1) * nx + (i - 1)]; };
  const int i_copy = 1;
  double dlat = 0.0, southern_edge = 0.0;
  int N = nml.n_lat_aux_grid, j_dim_sh = 0;
  if (type == 0 || type == 1) {   // :386-404
    dlat = 2.0 * (U(i_copy, 1) - T(i_copy, 1));
    southern_edge = U(i_copy, 1) - dlat;
  }
  if (type == 0) {   // 'southern' :406-474
    for (int j = 1; j <= ny; ++j) if (T(i_copy, j) < 0.0) ++j_dim_sh;
    if (j_dim_sh == 0) return fail("(init_lat_aux_grid) there are no Southern Hemisphere grid points");
    // TLATD_Gcopy(j) is the row's first value that is not the netCDF fill value, which no latitude is: TLATD_G(1, j)
    for (int j = 1; j <= j_dim_sh; ++j) for (int i = 1; i <= nx; ++i)
      if (std::fabs(T(i, j) - T(1, j)) > eps_grid)
        return fail("(init_lat_aux_grid): SH is not a regular at-lon grid. Use a different choice for lat_aux_grid_type.");
    const double np_minus_northern_edge = 90.0 + southern_edge;
    if (np_minus_northern_edge >= 0.5 * dlat) {
      N = (int)std::round(np_minus_northern_edge / dlat);   // nint: halves away from zero
      if (N == 0) return fail("(init_lat_aux_grid) n_lat_aux_grid is zero");
      dlat = np_minus_northern_edge / (double)N;
      N = 2 * j_dim_sh + N;
    } else N = 2 * j_dim_sh;
  }
  if (type == 1) {   // 'full' :476-495
    N = ny;
    for (int j = 1; j <= N; ++j) for (int i = 1; i <= nx; ++i)
      if (T(i, j) != T(i_copy, j))
        return fail("(init_lat_aux_grid): The model grid is not a regular lat-lon grid. Use a different choice for lat_aux_grid_type.");
  }
  if (type == 2) {   // 'user-specified' :497-504
    if (nml.lat_aux_end <= nml.lat_aux_begin) return fail("(init_lat_aux_grid) lat_aux_end should be > lat_aux_begin");
    if (N < 1) return fail("(init_lat_aux_grid) n_lat_aux_grid must be > 0 with the user-specified grid");
  }
  L.n_lat = N;
  L.edge.assign(N + 1, 0.0); L.center.assign(N, 0.0);
  std::vector<double> &E = L.edge, &C = L.center;   // E[j - 1] = lat_aux_edge(j)
  if (type == 0) {   // :520-551
    E[0] = southern_edge;
    for (int j = 1; j <= j_dim_sh; ++j) E[j] = U(i_copy, j);
    for (int j = j_dim_sh + 2, jj = j_dim_sh; j <= 2 * j_dim_sh + 1; ++j, --jj) E[j - 1] = -E[jj - 1];
    for (int j = 1; j <= j_dim_sh; ++j) C[j - 1] = T(i_copy, j);
    for (int j = j_dim_sh + 1, jj = j_dim_sh; j <= 2 * j_dim_sh; ++j, --jj) C[j - 1] = -C[jj - 1];
    if (N == 2 * j_dim_sh) E[N] = 90.0;
    else {
      const double e0 = E[2 * j_dim_sh];
      for (int j = 2 * j_dim_sh + 2; j <= N + 1; ++j) E[j - 1] = e0 + (j - 2 * j_dim_sh - 1) * dlat;
      for (int j = 2 * j_dim_sh + 1; j <= N; ++j) C[j - 1] = e0 + (j - 2 * j_dim_sh - 0.5) * dlat;
    }
  } else if (type == 1) {   // :553-558
    E[0] = southern_edge;
    for (int j = 1; j <= N; ++j) { E[j] = U(i_copy, j); C[j - 1] = T(i_copy, j); }
  } else {   // :560-570
    dlat = (nml.lat_aux_end - nml.lat_aux_begin) / (double)N;
    for (int j = 1; j <= N + 1; ++j) E[j - 1] = nml.lat_aux_begin + (double)(j - 1) * dlat;
    for (int j = 1; j <= N; ++j) C[j - 1] = nml.lat_aux_begin + 0.5 * dlat + (double)(j - 1) * dlat;
  }

  // ---- init_moc_ts_transport_arrays (:603-936)
  const int nreg = nml.n_transport_reg;
  if (nreg < 1) return fail("(init_moc_ts_transport_arrays)  n_transport_reg must be > 0  --  check namelist transports_nml");
  if (nreg > 2) return fail("(init_moc_ts_transport_arrays)  n_transport_reg must be < 3  --  check namelist transports_nml");
  if (nreg > 1 && (nml.nreg2 <= 0 || nml.nreg2 > POP_MAX_TRANSPORT_REG2))
    return fail(nml.nreg2 <= 0 ? "(init_moc_ts_transport_arrays)  no transport regions have been detected --  check namelist transports_nml"
                               : "(init_moc_ts_transport_arrays)  more than POP_MAX_TRANSPORT_REG2 region numbers");
  if (nreg > 1 && !region_mask) return fail("pop_init_transports: n_transport_reg = 2 needs REGION_MASK (region_mask_global is NULL)");
  L.n_reg = nreg;
  L.region_start.assign(nreg, 0);
  std::vector<unsigned char> flag((size_t)nx * ny, 0);   // bit m - 1: REGION_MASK_LAT_AUX(i, j, m) == 1
  for (size_t q = 0; q < flag.size(); ++q) {
    const int r = region_mask ? region_mask[q] : (KMT[q] > 0 ? 1 : 0);
    if (r > 0) flag[q] |= 1;
    if (nreg > 1) for (int n = 0; n < nml.nreg2; ++n) if (std::abs(r) == nml.reg2_numbers[n]) { flag[q] |= 2; break; }
  }
  if (nreg > 1) {   // :755-787
    int j_southern = ny;
    for (int j = 1; j <= ny && j_southern == ny; ++j) for (int i = 1; i <= nx; ++i)
      if (flag[(size_t)(j - 1) * nx + (i - 1)] & 2) { j_southern = j; break; }
    for (int i = 1; i <= nx; ++i) for (int i2 = 1; i2 <= nx; ++i2)
      if (std::fabs(T(i2, j_southern) - T(i, j_southern)) > eps_grid)
        return fail("(init_moc_ts_transport_arrays) SH is not a regular lat-lon grid. The southern boundary for region 2 (\"Atlantic\") cannot be specified.");
    if (j_southern == 1)
      return fail("pop_init_transports: region 2 starts in row j = 1, so lat_aux_region_start(2) = 0: the reference reads row 0 of its global arrays there");
    L.j_southern = j_southern;
    L.region_start[1] = j_southern - 1;
  }
  // n_moc_comp (:842-844)
  L.n_comp = 1;
  if (cf.hmix_tracer == 3 && cf.gm_diag_bolus) L.n_comp = 2;
  if (cf.struct_version >= 7 && cf.lsubmesoscale_mixing) {
    if (!cf.submeso_diag) return fail("pop_init_transports: the submesoscale component of the MOC (lsubmesoscale_mixing) needs submeso_diag = 1: WSUBM and VSUBM are not formed without it");
    L.n_comp = 3;
  }

  // ---- the bin of every cell (:811-812, :1061-1062): lat_aux_edge(n-1) <= TLATD_G < lat_aux_edge(n), n = 2 .. N + 1
  bool increasing = true;
  for (int n = 1; n <= N; ++n) if (!(E[n] > E[n - 1])) increasing = false;
  auto bins_of = [&](double t, std::vector<int> &out) {   // 0-based bins
    out.clear();
    if (increasing) {
      const int n = (int)(std::upper_bound(E.begin(), E.end(), t) - E.begin());   // E[n-1] <= t < E[n]
      if (n >= 1 && n <= N) out.push_back(n - 1);
    } else for (int n = 1; n <= N; ++n) if (t >= E[n - 1] && t < E[n]) out.push_back(n - 1);
  };
  L.bin_map.assign((size_t)nx * ny, 0);
  L.mask.assign((size_t)N * km * nreg, 1);
  std::vector<int> bb;
  for (size_t q = 0; q < (size_t)nx * ny; ++q) {
    bins_of(TLATD[q], bb);
    if (bb.empty()) continue;
    L.bin_map[q] = bb[0] + 1;
    for (int n : bb) for (int m = 0; m < nreg; ++m) if (flag[q] >> m & 1)
      for (int k = 1; k <= KMT[q] && k <= km; ++k) L.mask[((size_t)n * km + (k - 1)) * nreg + m] = 0;
  }
  // ---- cell lists: per block and bin the physical ocean cells that lie in some region, in (j, i) order
  if (n2 >= ((size_t)1 << MOC_FLAG_SHIFT)) return fail("pop_init_transports: a block has 2^29 cells or more");
  for (int b = 0; b < h.nblocks_tot; ++b) {
    const BlockInfo &B = h.all_blocks[b];
    std::map<int, std::vector<int>> per_bin;
    std::vector<int> row;
    for (int j = B.jb; j <= B.je; ++j) for (int i = B.ib; i <= B.ie; ++i) {
      const int ig = B.i_glob[i - 1], jg = B.j_glob[j - 1];
      if (ig < 1 || jg < 1) continue;
      const size_t q = (size_t)(jg - 1) * nx + (ig - 1);
      const int p2 = (j - 1) * nxb + (i - 1);
      // the boundary row of region 2 (:1134-1136): row j = lat_aux_region_start(2), cells whose mask at (i, j + 1) is 1
      if (nreg > 1 && jg == L.region_start[1] && (flag[q + nx] & 2)) row.push_back(p2);
      if (!flag[q] || KMT[q] < 1) continue;
      bins_of(TLATD[q], bb);
      for (int n : bb) per_bin[n].push_back(p2 | (int)flag[q] << MOC_FLAG_SHIFT);
    }
    for (auto &kv : per_bin) {
      L.lists.push_back(MocList{b, kv.first, (int)L.cells.size(), (int)kv.second.size()});
      L.cells.insert(L.cells.end(), kv.second.begin(), kv.second.end());
    }
    if (!row.empty()) {
      L.blists.push_back(MocList{b, 0, (int)L.bcells.size(), (int)row.size()});
      L.bcells.insert(L.bcells.end(), row.begin(), row.end());
    }
  }
  L.inited = true;
  return 0;
}

}  // namespace pop
