// host_forcing.cpp -- the coupled surface forcing, host logic: ANGLET from ANGLE (grid.F90:660-735) with its cosine and sine, the
// short-wave factor of qsw_distrb_opt '12hr' (forcing_coupled.F90:358-408), the defaults, refusals and derived constants of
// pop_init_coupled_forcing.  The kernels are in kernels_forcing.hpp.
#include "pop_internal.hpp"

namespace pop {

void coupled_nml_defaults(pop_coupled_nml &n) {
  std::memset(&n, 0, sizeof n);
  n.struct_bytes = (int)sizeof(pop_coupled_nml);
}

int coupled_nml_resolve(const HostModel &h, pop_coupled_nml &n, std::string &err) {
  auto bad = [&](const std::string &m) { err = "pop_init_coupled_forcing: " + m; return 1; };
  if (n.qsw_distrb_opt == 2)
    return bad("qsw_distrb_opt 'cosz' is not built: compute_cosz (forcing_coupled.F90:1540-1600) needs shr_orb_mod of CIME, which is not part of POP; 0 'const' or 1 '12hr'");
  if (n.qsw_distrb_opt != 0 && n.qsw_distrb_opt != 1) return bad("qsw_distrb_opt: 0 'const', 1 '12hr'");
  if (n.shf_formulation != 0 || n.sfwf_formulation != 0)
    return bad("the 'partially-coupled' shf / sfwf formulations are not built: set_combined_forcing and the restoring components (forcing_shf.F90, forcing_sfwf.F90) are the caller's");
  if (n.lestuary_on || n.lvsf_river || n.lebm_on)
    return bad("lestuary_on / lvsf_river / lebm_on are not built: the estuary box model (estuary_vsf_mod.F90) is not part of this library, MASK_ESTUARY is 0");
  if (n.luse_cpl_ifrac) return bad("luse_cpl_ifrac is not built: OCN_WGT feeds the partially-coupled formulations only");
  if (n.lms_balance != 0 && n.lms_balance != 1) return bad("lms_balance: 0 or 1");
  if (n.nsteps_per_interval < 0) return bad("nsteps_per_interval: >= 0 (0 = the time manager's " + std::to_string(h.nsteps_per_interval) + ")");
  if (n.latent_heat_vapor_mks < 0.0 || n.latent_heat_fusion_mks < 0.0 || n.sea_ice_salinity < 0.0 || n.rho_fw < 0.0)
    return bad("negative constant (latent_heat_vapor_mks, latent_heat_fusion_mks, sea_ice_salinity, rho_fw)");
  if (n.nsteps_per_interval == 0) n.nsteps_per_interval = h.nsteps_per_interval;
  return 0;
}

CplConsts coupled_consts(const pop_coupled_nml &n, double hflux_factor, double ocn_ref_salinity) {
  CplConsts k;
  k.lhv = n.latent_heat_vapor_mks != 0.0 ? n.latent_heat_vapor_mks : 2.501e6;     // SHR_CONST_LATVAP (pop_constants.F90:286)
  k.lhf = n.latent_heat_fusion_mks != 0.0 ? n.latent_heat_fusion_mks : 3.337e5;   // SHR_CONST_LATICE (:288)
  k.hflux_factor = hflux_factor;
  k.salinity_factor = -ocn_ref_salinity * 1.0e-4;   // -ocn_ref_salinity * fwflux_factor (:364-365)
  k.sflux_factor = 0.1;                             // :385
  k.fwmass_to_fwflux = 0.1;                         // :405
  k.momentum_factor = 10.0;                         // :314
  return k;
}

// grid.F90:686-732: the four-corner average (AT0 = ATW = ATS = ATSW = p25, grid.F90:2908-2911) with the +-pi unwrapping on the physical
// cells of every block, the row j_glob = 1 zeroed, then the halo update as a centre-located angle.  Formed on ALL blocks (the host
// halo update works there), the local ones returned.
void host_anglet_build(const HostModel &h, std::vector<double> &anglet, std::vector<double> &cosa, std::vector<double> &sina) {
  const int nxb = h.nxb, NB = h.nblocks_tot;
  const size_t n2 = h.n2;
  const double pi = 4.0 * std::atan(1.0), pi2 = 2.0 * pi;
  std::vector<double> T(n2 * NB, 0.0);
  if (!h.angle.empty()) {
    const std::vector<double> &A = h.angle;
    for (int b = 0; b < NB; ++b) {
      const BlockInfo &B = h.all_blocks[b];
      for (int j = B.jb - 1; j < B.je; ++j) {
        for (int i = B.ib - 1; i < B.ie; ++i) {
          const size_t p = b * n2 + (size_t)j * nxb + i;
          const double a0 = A[p];
          double aw = A[p - 1], as = A[p - nxb], asw = A[p - nxb - 1];
          if (a0 < 0.0) {
            if (std::fabs(aw - a0) > pi) aw = aw - pi2;
            if (std::fabs(as - a0) > pi) as = as - pi2;
            if (std::fabs(asw - a0) > pi) asw = asw - pi2;
          }
          T[p] = a0 * 0.25 + aw * 0.25 + as * 0.25 + asw * 0.25;
        }
        if (B.j_glob[j] == 1) for (int i = 0; i < nxb; ++i) T[b * n2 + (size_t)j * nxb + i] = 0.0;
      }
    }
    host_halo_r8_loc(h, T.data(), 1, 0.0, 0, 2);   // centre, angle (grid.F90:730-732)
  }
  anglet.resize(n2 * h.nblocks); cosa.resize(anglet.size()); sina.resize(anglet.size());
  for (int lb = 0; lb < h.nblocks; ++lb)
    std::copy(T.begin() + (size_t)(h.local_ids[lb] - 1) * n2, T.begin() + (size_t)h.local_ids[lb] * n2, anglet.begin() + (size_t)lb * n2);
  for (size_t p = 0; p < anglet.size(); ++p) { cosa[p] = std::cos(anglet[p]); sina[p] = std::sin(anglet[p]); }
}

// forcing_coupled.F90:358-408.  The weights of the loop are the half steps of the stepping in hand: for avgfit and the Robert filter
// the reference's own test (count == 2 or mod(count, time_mix_freq) == 0); the reference refuses '12hr' with any other stepping
// (:337-343), where this library takes the averaging steps the context really makes -- every time_mix_freq-th step with 'avg', none
// without time mixing -- so that the normalised factor integrates to a day over the steps taken.
int host_qsw_12hr_factor(const HostModel &h, int qsw_distrb_opt, int nspi, std::vector<double> &factor, std::string &err) {
  factor.assign((size_t)std::max(nspi, 0), 1.0);
  if (qsw_distrb_opt != 1) return 0;
  const double pi = 4.0 * std::atan(1.0), seconds_in_day = 86400.0, dt1 = h.dt[1];
  const int tmix = h.c.tmix_opt, freq = h.c.time_mix_freq;
  auto weight = [&](int count) {
    if (tmix == 2 || tmix == 3) return (count == 2 || (freq > 0 && count % freq == 0)) ? 0.5 : 1.0;
    if (tmix == 1) return (freq > 0 && count % freq == 0) ? 0.5 : 1.0;
    return 1.0;
  };
  double time_for_forcing = 0.0, sum_forcing = 0.0;
  int count_forcing = 1;
  for (int n = 0; n < nspi; ++n) {
    const double frac_day_forcing = time_for_forcing / seconds_in_day;
    const double cycle_function = std::cos(pi * (2.0 * frac_day_forcing - 1.0));
    factor[n] = 2.0 * (cycle_function + std::fabs(cycle_function)) * cycle_function;
    const double weight_forcing = weight(count_forcing);
    time_for_forcing = time_for_forcing + weight_forcing * dt1;
    sum_forcing = sum_forcing + weight_forcing * dt1 * factor[n];
    count_forcing = count_forcing + 1;
  }
  if (!(sum_forcing > 0.0)) { err = "pop_init_coupled_forcing: qsw '12hr': the interval of " + std::to_string(nspi) + " steps never sees the sun (the factor sums to 0)"; return 1; }
  for (int n = 0; n < nspi; ++n) factor[n] = factor[n] * seconds_in_day / sum_forcing;
  count_forcing = 1; sum_forcing = 0.0;   // check the final integral (:390-406)
  for (int n = 0; n < nspi; ++n) {
    sum_forcing = sum_forcing + weight(count_forcing) * dt1 * factor[n];
    count_forcing = count_forcing + 1;
  }
  if (sum_forcing < seconds_in_day - 1.0e-5 || sum_forcing > seconds_in_day + 1.0e-5) { err = "pop_init_coupled_forcing: qsw 12hr temporal integral is incorrect"; return 1; }
  return 0;
}

// init_ms_balance (ms_balance.F90:61-453).  The global arrays the reference gathers (TLOND, TLATD, DXT * DYT, REGION_MASK) are formed
// from the host's copy of every block; the search is the reference's loop nest, unchanged: an expanding box, j outer, i inner, the
// whole box searched again after every growth (hence the duplicate test).
int host_ms_balance_build(const HostModel &h, const pop_ms_balance_nml &nml, const int *region_mask_global, MsBalance &out, std::string &err) {
  auto bad = [&](const std::string &m) { err = "pop_init_ms_balance: " + m; return 1; };
  const int nxg = h.c.nx_global, nyg = h.c.ny_global, nxb = h.nxb, nyb = h.nyb, max_iter = 16;
  const size_t n2 = h.n2, NG = (size_t)nxg * nyg;
  if (nml.num_regions < 1 || !nml.regions) return bad("num_regions >= 1 records of the region table are needed");
  if (nml.max_points < 0) return bad("max_points: >= 0 (0 = 5000)");
  if (!region_mask_global) return bad("REGION_MASK is needed (region_mask_global)");
  const int max_points = nml.max_points ? nml.max_points : 5000;
  int num_ms = 0;
  for (int n = 0; n < nml.num_regions; ++n) num_ms += nml.regions[n].number < 0 ? 1 : 0;
  if (num_ms > POP_MAX_MS) return bad("maximum number of marginal seas exceeded: " + std::to_string(num_ms) + " > max_ms = " + std::to_string(POP_MAX_MS) + " (grid.F90:2751-2757)");
  const double pi = 4.0 * std::atan(1.0), radian = 180.0 / pi;
  std::vector<double> TLON, TLON_G(NG, 0.0), TLAT_G(NG, 0.0), AREAT_G(NG, 0.0);
  host_tlon_all(h, TLON);
  const std::vector<double> &TLAT = h.f2.at("TLAT"), &DXT = h.f2.at("DXT"), &DYT = h.f2.at("DYT");
  for (int b = 0; b < h.nblocks_tot; ++b) {   // gather_global: the physical cells of every block
    const BlockInfo &B = h.all_blocks[b];
    for (int j = B.jb - 1; j < B.je; ++j) for (int i = B.ib - 1; i < B.ie; ++i) {
      const int ig = B.i_glob[i], jg = B.j_glob[j];
      if (ig < 1 || jg < 1) continue;
      const size_t p = b * n2 + (size_t)j * nxb + i, g = (size_t)(jg - 1) * nxg + (ig - 1);
      TLON_G[g] = TLON[p] * radian; TLAT_G[g] = TLAT[p] * radian; AREAT_G[g] = DXT[p] * DYT[p];
    }
  }
  MsBalance M;
  M.region_mask.assign(region_mask_global, region_mask_global + NG);
  const std::vector<int> &R = M.region_mask;
  std::vector<std::vector<double>> MASK_G;
  for (int n = 0; n < nml.num_regions; ++n) {
    const pop_ms_region &reg = nml.regions[n];
    if (reg.number >= 0) continue;
    MsSea S;
    S.number = reg.number; S.name = std::string(reg.name, strnlen(reg.name, sizeof reg.name));
    std::vector<double> areas;
    double area = 0.0, lat_reach = 1.0, lon_reach = 1.0;
    bool done = false;
    for (int iter = 1; iter <= max_iter && !done; ++iter) {
      for (int j = 1; j <= nyg && !done; ++j) for (int i = 1; i <= nxg && !done; ++i) {
        const size_t g = (size_t)(j - 1) * nxg + (i - 1);
        if (!(reg.lat - lat_reach <= TLAT_G[g] && reg.lat + lat_reach >= TLAT_G[g] && reg.lon - lon_reach <= TLON_G[g] && reg.lon + lon_reach >= TLON_G[g])) continue;
        bool duplicate = false;
        for (size_t nn = 0; nn < S.ipts.size() && !duplicate; ++nn) duplicate = S.ipts[nn] == i && S.jpts[nn] == j;
        if (duplicate || R[g] < 0 || R[g] == 0) continue;   // duplicate, marginal-sea and land points are rejected
        if ((int)S.ipts.size() == max_points) { done = true; break; }
        S.ipts.push_back(i); S.jpts.push_back(j); areas.push_back(AREAT_G[g]);
        area = area + AREAT_G[g];
        if (area >= reg.area) done = true;
      }
      lat_reach = lat_reach + 1.0; lon_reach = lon_reach + 1.0;
    }
    const int npts = (int)S.ipts.size();
    if (npts <= 0) return bad("marginal sea " + S.name + ": no points selected for distribution area (must select at least one set of active points)");
    if (npts == max_points) S.warn |= POP_MS_WARN_MAX_POINTS;
    const int region_number = R[(size_t)(S.jpts[0] - 1) * nxg + (S.ipts[0] - 1)];
    for (int pt = 0; pt < npts; ++pt) if (R[(size_t)(S.jpts[pt] - 1) * nxg + (S.ipts[pt] - 1)] != region_number) S.warn |= POP_MS_WARN_TWO_REGIONS;
    double sum_frac = 0.0;
    S.fracs.resize(npts);
    for (int pt = 0; pt < npts; ++pt) { S.fracs[pt] = areas[pt] / area; sum_frac = sum_frac + S.fracs[pt]; }
    S.fracs[npts - 1] = S.fracs[npts - 1] + (1.0 - sum_frac);
    S.area = area;
    std::vector<double> G(NG, 0.0);
    for (int pt = 0; pt < npts; ++pt) G[(size_t)(S.jpts[pt] - 1) * nxg + (S.ipts[pt] - 1)] = S.fracs[pt];
    MASK_G.push_back(G);
    M.seas.push_back(S);
  }
  // scatter_global as a centre scalar onto the local blocks (ghost cells take their source cell's value, mirrored beyond a tripole
  // fold; cells without a global index 0): MASK_FRAC, and the indicator of REGION_MASK == number the balancing tests
  const size_t a2 = n2 * h.nblocks, ns = M.seas.size();
  M.mask_frac.assign(a2 * ns, 0.0); M.ind.assign(a2 * ns, 0.0);
  for (int lb = 0; lb < h.nblocks; ++lb) {
    const BlockInfo &B = h.all_blocks[h.local_ids[lb] - 1];
    for (int j = 0; j < nyb; ++j) for (int i = 0; i < nxb; ++i) {
      const int ig = B.i_glob[i], jg = B.j_glob[j];
      if (ig == 0 || jg == 0) continue;
      int is = ig, js = jg;
      if (jg < 0) { js = nyg + 1 + (jg + nyg); is = nxg + 1 - ig; if (is < 1) is += nxg; if (is > nxg) is -= nxg; }
      const size_t g = (size_t)(js - 1) * nxg + (is - 1), p = (size_t)lb * n2 + (size_t)j * nxb + i;
      for (size_t s = 0; s < ns; ++s) { M.mask_frac[s * a2 + p] = MASK_G[s][g]; M.ind[s * a2 + p] = (R[g] == M.seas[s].number) ? 1.0 : 0.0; }
    }
  }
  M.inited = true;
  out = M;
  return 0;
}

}  // namespace pop
