// host_ice.cpp -- init_ice (ice.F90:98-317), host logic: the code defaults of ice_nml and of the constants ice formation reads, what
// pop_init_ice refuses, and the derived constants.  The kernels are in kernels_ice.hpp.
#include "pop_internal.hpp"

namespace pop {

void ice_nml_defaults(pop_ice_nml &n) {   // ice.F90:158-162, forcing_sfwf.F90:268, pop_constants.F90:239-250
  std::memset(&n, 0, sizeof n);
  n.struct_bytes = (int)sizeof(pop_ice_nml);
  n.ice_freq_opt = 0; n.licecesm2 = 0; n.kmxice = 1; n.lactive_ice = 0; n.lfw_as_salt_flx = 0; n.tfreeze_option = 0;
  n.sea_ice_salinity = 4.0; n.ocn_ref_salinity = 34.7; n.latent_heat_fusion = 3.34e9;
  n.cp_sw = 3.996e7; n.rho_sw = 4.1 / 3.996; n.rho_fw = 1.0;
}

// everything pop_init_ice refuses that depends on the namelist and the configuration only
int ice_nml_check(const HostModel &h, const pop_ice_nml &n, std::string &err) {
  auto bad = [&](const std::string &m) { err = "pop_init_ice: " + m; return 1; };
  if (n.ice_freq_opt >= 2 && n.ice_freq_opt <= 7)
    return bad("ice_freq_opt 'nyear' .. 'nstep' (2 .. 7) is not built: ice.F90:211-234 sets a time flag that ice_formation never reads (:424-428); 0 'never' or 1 'coupled'");
  if (n.ice_freq_opt != 0 && n.ice_freq_opt != 1) return bad("ice_freq_opt: 0 'never', 1 'coupled'");
  if (n.kmxice < 1 || n.kmxice > h.km) return bad("kmxice = " + std::to_string(n.kmxice) + " is outside 1 .. km = " + std::to_string(h.km));
  if (n.tfreeze_option < 0 || n.tfreeze_option > 2) return bad("tfreeze_option: 0 'minus1p8', 1 'linear_salt', 2 'mushy'");
  if (n.sea_ice_salinity < 0.0 || n.ocn_ref_salinity < 0.0 || n.latent_heat_fusion < 0.0 || n.cp_sw < 0.0 || n.rho_sw < 0.0 || n.rho_fw < 0.0)
    return bad("negative constant (sea_ice_salinity, ocn_ref_salinity, latent_heat_fusion, cp_sw, rho_sw, rho_fw)");
  if (n.ice_freq_opt == 1 && !n.licecesm2 && h.c.tmix_opt != 3 && h.c.tmix_opt != 2)
    return bad("ice_freq_opt 'coupled' with licecesm2 = 0 needs tmix_opt robert or avgfit: the pre-CESM2 rule follows the coupler's calendar (time_management.F90:1959-1991)");
  return 0;
}

IceConsts ice_consts(const pop_ice_nml &n) {
  IceConsts k;
  k.cp_over_lhfusion = n.rho_sw * n.cp_sw / (n.latent_heat_fusion * n.rho_fw);   // ice.F90:156
  k.salice = n.sea_ice_salinity * 1.0e-3;                                         // ppt_to_salt (:197-198)
  k.salref = n.ocn_ref_salinity * 1.0e-3;
  k.hflux_factor = 1000.0 / (n.rho_sw * n.cp_sw);                                 // pop_constants.F90:336
  return k;
}

}  // namespace pop
