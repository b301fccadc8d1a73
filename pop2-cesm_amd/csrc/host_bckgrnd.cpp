// host_bckgrnd.cpp -- the lhoriz_varying_bckgrnd branch of init_vmix_kpp (vmix_kpp.F90:544-611): the latitude-varying KPP background
// diffusivity from TLAT and TLON in degrees.  Every cell of every local block, ghost cells included: the KPP kernels run on them, and
// a ghost cell carries its source cell's latitude and longitude after the halo updates of TLAT and TLON.  One level is kept: the
// reference copies level 1 to every level (:606-609).
#include "pop_internal.hpp"

namespace pop {

void kpp_bckgrnd_nml_defaults(pop_kpp_bckgrnd_nml &n) {   // vmix_kpp.F90:337-349
  std::memset(&n, 0, sizeof n);
  n.struct_bytes = (int)sizeof(pop_kpp_bckgrnd_nml);
  n.bckgrnd_vdc_eq = 0.01; n.bckgrnd_vdc_psim = 0.13; n.bckgrnd_vdc_ban = 1.0;
}

// tlon: host_tlon_build
void host_bckgrnd_build(const HostModel &h, const pop_kpp_bckgrnd_nml &n, const std::vector<double> &tlon, BckgrndFields &out) {
  const size_t n2 = h.n2, a2 = n2 * h.nblocks;
  const double pi = 4.0 * std::atan(1.0), radian = 180.0 / pi;
  const std::vector<double> &TLATg = h.f2.at("TLAT");
  const double vdc1 = h.c.bckgrnd_vdc1, eq = n.bckgrnd_vdc_eq, psim = n.bckgrnd_vdc_psim, ban = n.bckgrnd_vdc_ban, Pr = h.c.Prandtl;
  out.vdc.assign(a2, 0.0); out.vvc.assign(a2, 0.0); out.vvc_pr.assign(a2, 0.0);
  for (int lb = 0; lb < h.nblocks; ++lb) {
    const size_t g0 = (size_t)(h.local_ids[lb] - 1) * n2, l0 = (size_t)lb * n2;
    for (size_t p = 0; p < n2; ++p) {
      const double lat = TLATg[g0 + p] * radian, lon = tlon[l0 + p] * radian;   // TLATD, TLOND
      const double ts = 0.4 * (lat + 28.9), tn = 0.4 * (lat - 28.9);
      const double psis = psim * std::exp(-(ts * ts)), psin = psim * std::exp(-(tn * tn));
      double b = eq + psin + psis;
      if (lat < -10.0) b = b + vdc1;
      else if (lat <= 10.0) { const double r = lat / 10.0; b = b + vdc1 * (r * r); }
      else b = b + vdc1;
      if (lat < -1.0 && lat > -4.0 && lon > 103.0 && lon < 134.0) b = ban;    // North Banda Sea
      if (lat <= -4.0 && lat > -7.0 && lon > 106.0 && lon < 140.0) b = ban;   // Middle Banda Sea
      if (lat <= -7.0 && lat > -8.3 && lon > 111.0 && lon < 142.0) b = ban;   // South Banda Sea
      if (n.larctic_bckgrnd_vdc && lat >= 70.0) b = eq;
      out.vdc[l0 + p] = b;
      out.vvc[l0 + p] = Pr * b;
      out.vvc_pr[l0 + p] = (Pr * b) / Pr;   // bckgrnd_vvc / Prandtl as the tidal branch forms it (vmix_kpp.F90:1826)
    }
  }
}

}  // namespace pop
