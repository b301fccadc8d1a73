// host_tidal.cpp -- init-time part of Jayne tidal mixing (tidal_mixing.F90 init_tidal_mixing1 / 2 for tidal_mixing_method 'jayne'):
// the energy flux in g/s^3 (tidal_read_energy_jayne :2246-2295), the vertical decay function and TIDAL_COEF_3D (:1266-1309,
// tidal_form_qE_2D :2631-2661, tidal_form_coef_jayne :2512-2548), TLON (calc_tpoints, grid.F90:2985-3100) and the region boxes of ltidal_min_regions
// (:880-1003).  Every cell of every local block, ghost cells included: the KPP kernels run on them.
#include <algorithm>
#include "pop_internal.hpp"

namespace pop {

void tidal_nml_defaults(pop_tidal_nml &n) {   // tidal_mixing.F90:670-760
  std::memset(&n, 0, sizeof n);
  n.struct_bytes = (int)sizeof(pop_tidal_nml);
  n.ltidal_max = 1; n.ltidal_stabc = 1;
  n.tidal_local_mixing_fraction = 0.33; n.tidal_mixing_efficiency = 0.20; n.vertical_decay_scale = 500.0e02; n.tidal_mix_max = 100.0;
  for (int r = 0; r < POP_MAX_TIDAL_MIN_REGIONS; ++r) { n.tidal_min_values[r] = 20.0; n.tidal_min_regions_klevels[r] = 6; }
}

// checks that need no model; a 0 in a double member becomes the code default
int tidal_nml_resolve(pop_tidal_nml &n, std::string &err) {
  if (n.tidal_mixing_method != 0) { err = "tidal mixing: tidal_mixing_method 0 'jayne' only (1 'schmittner' and 2 'polzin' are not built)"; return 1; }
  if (n.tidal_local_mixing_fraction < 0.0 || n.tidal_mixing_efficiency < 0.0 || n.vertical_decay_scale < 0.0 || n.tidal_mix_max < 0.0) {
    err = "tidal mixing: negative parameter (tidal_local_mixing_fraction, tidal_mixing_efficiency, vertical_decay_scale, tidal_mix_max)"; return 1;
  }
  if (n.num_tidal_min_regions < 0 || n.num_tidal_min_regions > POP_MAX_TIDAL_MIN_REGIONS) {
    err = "tidal mixing: num_tidal_min_regions out of range 0 .. " + std::to_string(POP_MAX_TIDAL_MIN_REGIONS); return 1;
  }
  for (int r = 0; r < n.num_tidal_min_regions; ++r)
    if (n.tidal_min_values[r] < 0.0) { err = "tidal mixing: negative parameter (tidal_min_values)"; return 1; }
  if (n.tidal_local_mixing_fraction == 0.0) n.tidal_local_mixing_fraction = 0.33;
  if (n.tidal_mixing_efficiency == 0.0) n.tidal_mixing_efficiency = 0.20;
  if (n.vertical_decay_scale == 0.0) n.vertical_decay_scale = 500.0e02;
  if (n.tidal_mix_max == 0.0) n.tidal_mix_max = 100.0;
  return 0;
}

// TLON of the local blocks (calc_tpoints, grid.F90:2985-3100): Cartesian average of the four surrounding U points, the southernmost
// row copied from the row north of it, 0 <= TLON < 2 pi, then the halo update.  Shared by pop_init_tidal_mixing (region boxes) and
// pop_init_kpp_bckgrnd (Banda Sea boxes); nothing else needs it.
void host_tlon_build(const HostModel &h, std::vector<double> &tlon) {
  const size_t n2 = h.n2;
  std::vector<double> TLON;
  host_tlon_all(h, TLON);
  tlon.assign(n2 * h.nblocks, 0.0);
  for (int lb = 0; lb < h.nblocks; ++lb) {
    const size_t g0 = (size_t)(h.local_ids[lb] - 1) * n2;
    std::copy(TLON.begin() + g0, TLON.begin() + g0 + n2, tlon.begin() + (size_t)lb * n2);
  }
}
// the same on ALL blocks of the decomposition
void host_tlon_all(const HostModel &h, std::vector<double> &TLON) {
  const int nxb = h.nxb, nyb = h.nyb, NB = h.nblocks_tot;
  const size_t n2 = h.n2;
  const double pi = 4.0 * std::atan(1.0), pi2 = 2.0 * pi;
  const std::vector<double> &ULAT = h.f2.at("ULAT"), &ULON = h.f2.at("ULON");
  auto idx = [&](int b, int i, int j) { return (size_t)b * n2 + (size_t)j * nxb + i; };
  TLON.assign(n2 * NB, 0.0);
  for (int b = 0; b < NB; ++b) {
    const BlockInfo &B = h.all_blocks[b];
    for (int j = 1; j < nyb; ++j) for (int i = 1; i < nxb; ++i) {
      double x[4], y[4];
      const int di[4] = {0, 0, -1, -1}, dj[4] = {0, -1, 0, -1};   // c, s, w, sw
      for (int q = 0; q < 4; ++q) {
        const size_t p = idx(b, i + di[q], j + dj[q]);
        const double cz = std::cos(ULAT[p]);
        x[q] = std::cos(ULON[p]) * cz; y[q] = std::sin(ULON[p]) * cz;
      }
      const double tx = 0.25 * (x[0] + x[1] + x[2] + x[3]), ty = 0.25 * (y[0] + y[1] + y[2] + y[3]);
      TLON[idx(b, i, j)] = (tx != 0.0 || ty != 0.0) ? std::atan2(ty, tx) : 0.0;
    }
    if (B.j_glob[B.jb - 1] == 1)
      for (int i = B.ib - 1; i < B.ie; ++i) TLON[idx(b, i, B.jb - 1)] = TLON[idx(b, i, B.jb)];
    for (size_t p = (size_t)b * n2; p < (size_t)(b + 1) * n2; ++p) {
      if (TLON[p] > pi2) TLON[p] = TLON[p] - pi2;
      if (TLON[p] < 0.0) TLON[p] = TLON[p] + pi2;
    }
  }
  host_halo_r8_loc(h, TLON.data(), 1, 0.0, 0, 0);
}

// flux: W/m^2 on the local blocks, ghost cells already updated; tlon: host_tlon_build
void host_tidal_build(const HostModel &h, const pop_tidal_nml &n, const double *flux, const std::vector<double> &tlon, TidalFields &out) {
  const int nxb = h.nxb, nyb = h.nyb, km = h.km;
  const size_t n2 = h.n2, n3 = h.n3, a2 = n2 * h.nblocks;
  const double pi = 4.0 * std::atan(1.0), radian = 180.0 / pi;
  const std::vector<double> &TLATg = h.f2.at("TLAT"), &HTg = h.f2.at("HT"), &RCg = h.f2.at("RCALCT");
  const std::vector<int> &KMTg = h.i2.at("KMT");
  auto idx = [&](int b, int i, int j) { return (size_t)b * n2 + (size_t)j * nxb + i; };
  out.flux.assign(a2, 0.0); out.coef.assign(n3 * h.nblocks, 0.0); out.box.assign(a2, 0);
  const double gamma_rhor = n.tidal_mixing_efficiency / 1.0;   // tidal_gamma_rhor = tidal_mixing_efficiency / rho_fw, rho_fw = 1 g/cm^3 (:1181)
  const double decay = n.vertical_decay_scale;
  for (int lb = 0; lb < h.nblocks; ++lb) {
    const int b = h.local_ids[lb] - 1;
    const BlockInfo &B = h.all_blocks[b];
    for (int j = 0; j < nyb; ++j) for (int i = 0; i < nxb; ++i) {
      const size_t pg = idx(b, i, j), pl = idx(lb, i, j);
      const int kmt = KMTg[pg];
      const double ht = HTg[pg];
      const double ef = 1000.0 * flux[pl];                       // W/m^2 -> g/s^3
      out.flux[pl] = ef;
      const double qe = n.tidal_local_mixing_fraction * ef;      // TIDAL_QE_2D
      const double coef2 = gamma_rhor * RCg[pg] * qe;            // TIDAL_COEF_2D
      // WORK = 0 where KMT <= 1: the reference divides by it there (1 / 0 at k = KMT = 1, nothing at KMT = 0), and TIDAL_COEF_3D(KMT)
      // is then infinite or not a number; no statement reads it, because TIDAL_DIFF is formed where N2 > 0 and DBLOC(k >= KMT) = 0.
      // Stored as 0 here.
      double work = 0.0;
      for (int k = 1; k <= km; ++k) if (k < kmt) work = work + std::exp(-(ht - h.zw[k]) / decay) * h.dzw[k];
      if (kmt > 1)
        for (int k = 1; k <= km && k <= kmt; ++k) {
          const double vf = (k < kmt) ? std::exp(-(ht - h.zw[k]) / decay) / work : 1.0 / work;   // VERTICAL_FUNC
          out.coef[(size_t)lb * n3 + (size_t)(k - 1) * n2 + (size_t)j * nxb + i] = coef2 * vf;
        }
      if (n.ltidal_min_regions && B.i_glob[i] != 0 && B.j_glob[j] != 0) {
        // the box is formed on the global arrays and scattered (:910-962): a ghost cell carries the value of its source cell (its
        // TLAT / TLON are that cell's after the halo update), a cell without a global address 0
        const double latd = TLATg[pg] * radian, lond = tlon[pl] * radian;
        int box = 0;
        for (int r = 0; r < n.num_tidal_min_regions; ++r) {
          if (!(latd >= n.tidal_TLATmin_regions[r] && latd <= n.tidal_TLATmax_regions[r])) continue;
          const bool wrap = !(n.tidal_TLONmin_regions[r] <= n.tidal_TLONmax_regions[r]);
          const bool in = !wrap ? (lond >= n.tidal_TLONmin_regions[r] && lond <= n.tidal_TLONmax_regions[r])
                                : ((lond >= n.tidal_TLONmin_regions[r] && lond <= 360.0) || lond <= n.tidal_TLONmax_regions[r]);
          if (in) box = r + 1;   // later regions overwrite earlier ones
        }
        out.box[pl] = box;
      }
    }
  }
}

}  // namespace pop
