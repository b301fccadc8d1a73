// launch_forcing.hpp -- host side of the coupled surface forcing (part of pop_amd.hip, after launch_halo.hpp): the device fields of
// pop_init_coupled_forcing, the staged upload and the three launches of pop_set_coupled_forcing, the launch of
// pop_set_surface_forcing.  Nothing here waits for the stream or copies device-to-host.
#pragma once

namespace {

const char *const CPL_FIELD_NAMES[CF_NF] = {"SNOW_F", "PREC_F", "EVAP_F", "MELT_F", "ROFF_F", "IOFF_F", "SALT_F", "SENH_F", "LWUP_F", "LWDN_F", "MELTH_F", "IFRAC", "ATM_PRESS", "U10_SQR"};

// ANGLET, COS_ANGLET, SIN_ANGLET of the local blocks, formed on first use
void cpl_anglet(pop_ctx *c) {
  if (c->anglet.empty()) host_anglet_build(c->h, c->anglet, c->cos_anglet, c->sin_anglet);
}

// a named field of the coupled forcing; null: not one of them (or not allocated)
double *cpl_field(pop_ctx *c, const std::string &name, int n) {
  const CplState &s = c->cpl;
  if (!s.inited) return nullptr;
  for (int f = 0; f < CF_NF; ++f) if (name == CPL_FIELD_NAMES[f]) return s.F[f];
  if (name == "SHF_QSW_RAW" || name == "SHF_COMP_QSW") return s.SHF_COMP_QSW;   // forcing_coupled.F90:856, :867: two copies of one field
  if (name == "SFWF_COMP_CPL") return s.SFWF_COMP;
  if (name == "TFW_COMP_CPL") return (n == 0 || n == 1) ? s.TFW_COMP[n] : nullptr;
  if (name == "MASK_FRAC") return (s.ms && n >= 0 && n < s.nseas) ? s.MS_FRAC + (size_t)n * c->g.n2 * c->g.nblocks : nullptr;   // by sea
  if (name == "MS_TRANSPORT_TERM") return s.ms ? s.MS_T : nullptr;   // the per-cell TRANSPORT of the last import, every sea in one field
  return nullptr;
}

int cpl_init_device(pop_ctx *c, CplState &s) {
  const size_t a2 = (size_t)c->g.n2 * c->g.nblocks;
  for (int f = 0; f < CF_NF; ++f) if (dev_alloc(c, &s.F[f], a2)) return 1;
  if (dev_alloc(c, &s.SHF_COMP_QSW, a2)) return 1;
  if (s.icefw && (dev_alloc(c, &s.SFWF_COMP, a2) || dev_alloc(c, &s.TFW_COMP[0], a2) || dev_alloc(c, &s.TFW_COMP[1], a2))) return 1;
  if (dev_upload(c, &s.COSA, c->cos_anglet.data(), a2) || dev_upload(c, &s.SINA, c->sin_anglet.data(), a2)) return 1;
  if (dev_upload(c, &s.d_qsw, s.qsw.data(), s.qsw.size())) return 1;
  if (dev_alloc(c, &s.raw, a2 * X_NF, false)) return 1;
  if (s.ms) {
    if (dev_upload(c, &s.MS_IND, c->msb.ind.data(), c->msb.ind.size()) || dev_upload(c, &s.MS_FRAC, c->msb.mask_frac.data(), c->msb.mask_frac.size())) return 1;
    if (dev_alloc(c, &s.MS_T, a2) || dev_alloc(c, &s.ms_sums, POP_MAX_MS)) return 1;
  }
  return pinned_alloc(c, &s.h_raw, a2 * X_NF) || new_event(c, &s.ev_up);
}

template <class K, class A>
void cpl_launch(pop_ctx *c, K kv1, K kv2, const A &a) {
  const bool vec = c->g.n2 % 2 == 0;
  const int per = vec ? 512 : 256;
  hipLaunchKernelGGL(vec ? kv2 : kv1, dim3((c->g.n2 + per - 1) / per, c->g.nblocks), dim3(256), 0, c->stream, c->g, a);
}

// ms_balancing (ms_balance.F90:577-642) on STF(2) of the virtual-salt-flux branch: the per-cell terms and the overwrite inside the
// seas, then per sea the library's global sum (workgroup partials, ordered block sums, blocks in block-id order, the all-reduce of
// the block-sum vector across ranks: the result does not depend on the distribution and never leaves the device), then the
// distribution over every sea's points, seas in region order
int cpl_ms_balancing(pop_ctx *c) {
  const CplState &s = c->cpl;
  const size_t a2 = (size_t)c->g.n2 * c->g.nblocks;
  MsArgs a{};
  for (int f = 0; f < CF_NF; ++f) a.F[f] = s.F[f];
  a.QFLUX = c->ice.QFLUX; a.DXT = c->d2["DXT"]; a.DYT = c->d2["DYT"];
  for (int m = 0; m < s.nseas; ++m) { a.IND[m] = s.MS_IND + m * a2; a.MASK_FRAC[m] = s.MS_FRAC + m * a2; }
  a.STF2 = c->STF[1]; a.TRANSPORT = s.MS_T; a.sums = s.ms_sums;
  a.c_q = s.c_q; a.c_s = s.c_s; a.c_a = s.c_a; a.c_t = s.c_t; a.nseas = s.nseas;
  cpl_launch(c, k_ms_transport<1>, k_ms_transport<2>, a);
  for (int m = 0; m < s.nseas; ++m) {
    hipLaunchKernelGGL(k_dot_partial, grid_2d(c), dim3(POP_RED_THREADS), 0, c->stream, c->g, (const double *)s.MS_T, (const double *)nullptr, a.IND[m], c->partial);
    if (reduce_finish<1>(c, FIN_PLAIN)) return 1;
    hipLaunchKernelGGL(k_ms_keep, dim3(1), dim3(1), 0, c->stream, (const SolverScalars *)c->sc, s.ms_sums, m);
  }
  cpl_launch(c, k_ms_distribute<1>, k_ms_distribute<2>, a);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// ocn_import, rotate_wind_stress, update_ghost_cells_coupler_fluxes, pop_set_coupled_forcing
int cpl_import(pop_ctx *c, const pop_x2o *x) {
  CplState &s = c->cpl;
  const size_t a2 = (size_t)c->g.n2 * c->g.nblocks;
  const double *src[X_NF] = {x->taux, x->tauy, x->snow, x->rain, x->evap, x->meltw, x->rofl, x->rofi, x->salt, x->swnet, x->sen, x->lwup, x->lwdn, x->melth, x->ifrac, x->pslv, x->duu10n};
  // the pinned buffer is free once the previous import's upload has run (an interval ago: no wait in practice)
  if (s.up_pending) { HIPCHK(c, hipEventSynchronize(s.ev_up)); s.up_pending = false; }
  CplImportArgs ia{};
  size_t given = 0;
  for (int f = 0; f < X_NF; ++f) {
    if (!src[f]) continue;
    std::memcpy(s.h_raw + given * a2, src[f], a2 * sizeof(double));
    ia.raw[f] = s.raw + given * a2;
    ++given;
  }
  if (given) {   // one staged upload of all given fields
    HIPCHK(c, hipMemcpyAsync(s.raw, s.h_raw, given * a2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(s.ev_up, c->stream));
    s.up_pending = true;
  }
  for (int f = 0; f < CF_NF; ++f) ia.F[f] = s.F[f];
  ia.SHF_QSW = c->SHF_QSW; ia.SMFT1 = c->d2["SMFT1"]; ia.SMFT2 = c->d2["SMFT2"];
  ia.COSA = s.COSA; ia.SINA = s.SINA; ia.hflux_factor = s.k.hflux_factor; ia.momentum_factor = s.k.momentum_factor;
  cpl_launch(c, k_cpl_import<1>, k_cpl_import<2>, ia);
  {   // SMFT as a centre-located vector (forcing_coupled.F90:1508-1516), then the scalars of update_ghost_cells_coupler_fluxes (:1165-1328)
    std::vector<HaloItem> items = {{ia.SMFT1, 1, 0, 1}, {ia.SMFT2, 1, 0, 1}};
    for (int f : {CF_SNOW, CF_PREC, CF_EVAP, CF_MELT, CF_ROFF, CF_IOFF, CF_SALT, CF_SENH, CF_LWUP, CF_LWDN, CF_MELTH}) items.push_back({s.F[f], 1});
    items.push_back({c->SHF_QSW, 1});
    for (int f : {CF_IFRAC, CF_PRESS, CF_U10}) items.push_back({s.F[f], 1});
    // halo_update_many fuses at most eight fields into one message per neighbour: three batches instead of seventeen updates
    for (size_t i0 = 0; i0 < items.size(); i0 += 8)
      if (halo_update_many(c, std::vector<HaloItem>(items.begin() + i0, items.begin() + std::min(items.size(), i0 + 8)))) return 1;
  }
  CplCombineArgs ca{};
  for (int f = 0; f < CF_NF; ++f) ca.F[f] = s.F[f];
  ca.SMFT1 = ia.SMFT1; ca.SMFT2 = ia.SMFT2; ca.T = c->TR[0][c->curt]; ca.S = c->TR[1][c->curt]; ca.SHF_QSW = c->SHF_QSW;
  ca.SMF1 = c->d2["SMF1"]; ca.SMF2 = c->d2["SMF2"]; ca.STF1 = c->STF[0]; ca.STF2 = c->STF[1]; ca.FW = c->FW; ca.TFW1 = c->TFW[0]; ca.TFW2 = c->TFW[1];
  ca.SHF_COMP_QSW = s.SHF_COMP_QSW; ca.SFWF_COMP = s.SFWF_COMP; ca.TFW_COMP1 = s.TFW_COMP[0]; ca.TFW_COMP2 = s.TFW_COMP[1];
  ca.lhv = s.k.lhv; ca.lhf = s.k.lhf; ca.hflux_factor = s.k.hflux_factor; ca.salinity_factor = s.k.salinity_factor;
  ca.sflux_factor = s.k.sflux_factor; ca.fwmass_to_fwflux = s.k.fwmass_to_fwflux;
  const pop_ice_nml &in = c->ice.nml;   // pop_init_ice's; without that call the zero-initialised struct, whose tfreeze_option 0 'minus1p8' and lactive_ice 0 are the code defaults
  ca.tfz = in.tfreeze_option; ca.lactive_ice = in.lactive_ice;
  if (s.fwf) {
    cpl_launch(c, k_cpl_combine<1, true>, k_cpl_combine<2, true>, ca);
    for (int n = 2; n < c->h.nt; ++n) HIPCHK(c, hipMemsetAsync(c->TFW[n], 0, a2 * sizeof(double), c->stream));   // :793-795
  } else {
    cpl_launch(c, k_cpl_combine<1, false>, k_cpl_combine<2, false>, ca);
    if (s.ms && cpl_ms_balancing(c)) return 1;   // forcing_coupled.F90:845-848
  }
  HIPCHK(c, hipGetLastError());
  s.imported = true; s.nsteps = 0;
  return 0;
}

// does the per-step phase change a field?  With 'const' the factor is 1 and SHF_QSW already holds SHF_COMP_QSW: nothing to launch
bool cpl_step_active(const pop_ctx *c) { return c->cpl.inited && c->cpl.imported && (c->cpl.nml.qsw_distrb_opt == 1 || c->cpl.icefw); }

int cpl_step(pop_ctx *c) {
  const CplState &s = c->cpl;
  SfcStepArgs a{};
  a.qsw_factor = s.d_qsw; a.index_qsw = s.nsteps % s.nml.nsteps_per_interval;   // index_qsw - 1 (forcing.F90:379)
  a.SHF_COMP_QSW = s.SHF_COMP_QSW; a.SFWF_COMP = s.SFWF_COMP; a.TFW_COMP1 = s.TFW_COMP[0]; a.TFW_COMP2 = s.TFW_COMP[1];
  a.FW_FREEZE = c->ice.FWF; a.S = c->TR[1][c->curt];
  a.SHF_QSW = c->SHF_QSW; a.FW = c->FW; a.TFW1 = c->TFW[0]; a.TFW2 = c->TFW[1];
  a.salice = c->ice.k.salice; a.tfz = c->ice.nml.tfreeze_option;
  if (s.icefw) cpl_launch(c, k_sfc_forcing_step<1, true>, k_sfc_forcing_step<2, true>, a);
  else cpl_launch(c, k_sfc_forcing_step<1, false>, k_sfc_forcing_step<2, false>, a);
  HIPCHK(c, hipGetLastError());
  return 0;
}

}  // namespace
