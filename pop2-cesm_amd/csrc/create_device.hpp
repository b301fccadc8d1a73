// create_device.hpp -- the device half of pop_create_tuned: the steps that fill a context from the host model, called in the
// order they stand here.  Each returns 1 with c->err set.  A step uploads; the lists it uploads are built by the pure functions
// of host_tables.cpp (and lds_tile_list below, which needs the tile numbering of kernels_common.hpp).
// Part of the single translation unit pop_amd.hip (included after the launch files).
//
// What the order rests on:
//   create_grid_device fills c->d2 / c->di2, which every later step reads by name (the G2 / GI wiring included);
//   create_land_lists leaves c->opre_host, which create_solver_lists reads;
//   create_gm sets c->gm before create_submeso borrows its pointers;
//   create_state_fields allocates VDC, VVC and CHL, which create_mix_and_ahead fills and mix_create needs; it also makes the
//     side stream's events before create_halo_device and create_solver_device add theirs;
//   create_solver_lists sets c->nchunk, which the replicated view of create_solver_device sizes its partials by, and
//     create_solver_device copies c->g into that view, so every step that writes c->g comes before it;
//   create_initial_state runs kernels on the finished grid and drops the host copy of the initial state.
#pragma once

namespace {

int create_grid_device(pop_ctx *c) {
  const Forms &f = c->f;
  HostModel &h = c->h;
  DevGrid &g = c->g;
  g.nxb = h.nxb; g.nyb = h.nyb; g.km = h.km; g.nt = h.nt; g.nblocks = h.nblocks;
  g.n2 = (int)h.n2; g.n3 = (long long)h.n3;
  g.xcd_remap = f.xcd_remap; g.lds_order = f.lds_order; g.red_band = f.red_band;   // workgroup orders (kernels_common.hpp)
  g.ib = NGHOST + 1; g.ie = h.nxb - NGHOST; g.jb = NGHOST + 1; g.je = h.nyb - NGHOST;
  {   // padded blocks (blocks.F90:174-265): per-block last physical column / row, only when some local block ends early
    std::vector<int> ieb(h.nblocks), jeb(h.nblocks);
    bool short_block = false;
    for (int lb = 0; lb < h.nblocks; ++lb) {
      const BlockInfo &B = h.all_blocks[h.local_ids[lb] - 1];
      ieb[lb] = B.ie; jeb[lb] = B.je;
      if (B.ie != g.ie || B.je != g.je) short_block = true;
    }
    g.ieb = nullptr; g.jeb = nullptr;
    if (short_block) {
      int *d0, *d1;
      if (dev_upload(c, &d0, ieb.data(), ieb.size()) || dev_upload(c, &d1, jeb.data(), jeb.size())) return 1;
      g.ieb = d0; g.jeb = d1;
    }
  }
  // vertical arrays
  struct { CArr *dst; std::vector<double> *src; } V[] = {
    {&g.dz, &h.dz}, {&g.dzw, &h.dzw}, {&g.zt, &h.zt}, {&g.zw, &h.zw}, {&g.c2dz, &h.c2dz}, {&g.dzr, &h.dzr}, {&g.dz2r, &h.dz2r},
    {&g.dzwr, &h.dzwr}, {&g.pressz, &h.pressz}, {&g.bouss, &h.bouss}, {&g.afac_t, &h.afac_t}, {&g.afac_u, &h.afac_u}};
  for (auto &v : V) { double *p; if (dev_upload(c, &p, v.src->data(), v.src->size())) return 1; *v.dst = p; }
  // per-level MWJF coefficients (k_state3d_lv): formed on the device
  if (g.km + 1 <= 1024) {
    double *p = nullptr;
    std::vector<double> z((size_t)6 * (g.km + 2), 0.0);
    if (dev_upload(c, &p, z.data(), z.size())) return 1;
    hipLaunchKernelGGL(k_eos_level_table, dim3(1), dim3(g.km + 1), 0, 0, g, p);
    HIPCHK(c, hipDeviceSynchronize());
    g.eosP = p;
  }
  g.state_lv = f.state3d_levels;
  // 2-D fields: upload the local blocks of every host field
  for (auto &kv : h.f2) {
    std::vector<double> all;
    const std::vector<double> *src = &kv.second;
    if (h.c.ns_boundary == 2 && kv.first == "centerWgtIndep") {
      // Beyond a tripole fold the reference forms z = r / centerWgt in the ghost rows with the ghost cells' OWN centerWgt, whose four
      // terms were added in the mirrored order: equal to the owner's value up to rounding only.  The fused solver kernels (and
      // the exchange of z between ranks) give a ghost cell its owner's z instead; so that every solver path of this library
      // agrees bit for bit, the device copy of the state-independent part of centerWgt takes the owners' values in those rows
      // (the area and the mask in the other part are mirrored copies already).  The host copy keeps the reference's values.
      all = kv.second;
      host_halo_r8_loc(h, all.data(), 1, 0.0, 0, 0);
      src = &all;
    }
    // the device copies of the off-centre weights hold the first row and column too (host_tables.cpp btrop_wgt_ring)
    const int wgt = kv.first == "btropWgtNE" ? 1 : kv.first == "btropWgtEast" ? 2 : kv.first == "btropWgtNorth" ? 3 : 0;
    if (wgt) { all = btrop_wgt_ring(h, wgt); src = &all; }
    auto loc = local_part(h, *src); double *p; if (dev_upload(c, &p, loc.data(), loc.size())) return 1; c->d2[kv.first] = p;
  }
  for (auto &kv : h.i2) { auto loc = local_part(h, kv.second); int *p; if (dev_upload(c, &p, loc.data(), loc.size())) return 1; c->di2[kv.first] = p; }
#define G2(f) g.f = c->d2[#f]
  G2(DXU); G2(DYU); G2(DXUR); G2(DYUR); G2(UAREA_R); G2(TAREA_R); G2(TAREA); G2(FCOR); G2(FCORT); G2(HU); G2(HUR);
  G2(AU0); G2(AUN); G2(AUE); G2(AUNE); G2(RCALCT); G2(DTN); G2(DTS); G2(DTE); G2(DTW);
  G2(DUC); G2(DUN); G2(DUS); G2(DUE); G2(DUW); G2(DMC); G2(DMN); G2(DMS); G2(DME); G2(DMW); G2(DUM); G2(KXU); G2(KYU);
  {   // byte copy of the solver mask
    std::vector<unsigned char> m8;
    if (mask_bytes(local_part(h, h.f2["mMask"]), m8)) { c->err = "solver mask is not 0/1"; return 1; }
    unsigned char *d8;
    if (dev_upload(c, &d8, m8.data(), m8.size())) return 1;
    g.mMask8 = d8;
  }
  G2(mMask); G2(CHECKER); G2(CONSTNT); G2(SMF1); G2(SMF2); G2(SMFT1); G2(SMFT2);
  g.pbc = h.c.partial_bottom_cells ? 1 : 0;
  if (g.pbc) { G2(DZBC); G2(DZUB); }
#undef G2
#define GI(f) g.f = c->di2[#f]
  GI(KMT); GI(KMU); GI(KMTN); GI(KMTS); GI(KMTE); GI(KMTW); GI(KMTEE); GI(KMTNN);
#undef GI
  g.WNE = c->d2["btropWgtNE"]; g.WEa = c->d2["btropWgtEast"]; g.WNo = c->d2["btropWgtNorth"]; g.WC0 = c->d2["centerWgtIndep"];
  g.XW = c->d2["btropXW"]; g.YW = c->d2["btropYW"];
  if (dev_alloc(c, &g.dump, 8192)) return 1;
  { double *z; if (dev_alloc(c, &z, 64)) return 1; g.zero = z; }
  return 0;
}

// DevGrid::lds_act4 / lds_act8: per block the R-row tiles of the LDS kernels that hold a cell to compute, packed (tj << 16 | ti,
// -1 = padding); `longest` entries per block.  Empty when every tile or no tile has work, or the tile counts do not fit the packing.
std::vector<int> lds_tile_list(const HostModel &h, const std::vector<int> &pre, int R, int lds_order, int &longest_out) {
  longest_out = 0;
  const int ntx = (h.nxb - 2 * NGHOST + POP_COL_THREADS - 1) / POP_COL_THREADS, nty = (h.nyb - 2 * NGHOST + R - 1) / R;
  if (ntx > 0xffff || nty > 0x7fff) return {};
  // tiles in the numbering the launch order is built on (patch by patch for lds_order 1, row-major otherwise)
  std::vector<std::vector<int>> act(h.nblocks);
  size_t longest = 0;
  for (int b = 0; b < h.nblocks; ++b) {
    const int *P = pre.data() + (size_t)b * (h.n2 + 1);
    for (int gi = 0; gi < ntx * nty; ++gi) {
      int ti, tj;
      if (lds_order) { if (!lds_tile_from_gi(gi, ntx, nty, ti, tj)) continue; }
      else { ti = gi % ntx; tj = gi / ntx; }
      const int i0 = NGHOST + ti * POP_COL_THREADS, i1 = std::min(i0 + POP_COL_THREADS, h.nxb);
      int n = 0;
      for (int j = NGHOST + tj * R; j < std::min(NGHOST + tj * R + R, h.nyb); ++j) n += P[(size_t)j * h.nxb + i1] - P[(size_t)j * h.nxb + i0];
      if (n) act[b].push_back(tj << 16 | ti);
    }
    longest = std::max(longest, act[b].size());
  }
  if (longest == 0 || longest == (size_t)ntx * nty) return {};
  // lds_order 1: the a-th tile WITH OCEAN goes where the a-th tile of the full numbering would: runs of 32 such tiles -- a
  // compact patch -- to one XCD, so the halo rows neighbouring tiles share are still fetched into one L2 (a plain packed list
  // would deal consecutive tiles to eight different XCDs: measured 1.34 x the algorithmic traffic for the momentum kernel
  // against 1.15 x)
  if (lds_order) longest = 256 * ((longest + 255) / 256);
  std::vector<int> list((size_t)longest * h.nblocks, -1);
  for (int b = 0; b < h.nblocks; ++b)
    for (size_t a = 0; a < act[b].size(); ++a) list[(size_t)b * longest + (lds_order ? (size_t)lds_slot_of((int)a) : a)] = act[b][a];
  longest_out = (int)longest;
  return list;
}

int create_land_lists(pop_ctx *c) {   // land elimination: DevGrid::opre, lds_act4 / lds_act8
  DevGrid &g = c->g;
  c->opre_host = land_prefix(c->h, c->land_fraction);
  int *d;
  if (dev_upload(c, &d, c->opre_host.data(), c->opre_host.size())) return 1;
  g.opre = d;
  g.skip = 0;
  for (int R : {4, 8}) {
    int longest = 0, *dl;
    const std::vector<int> list = lds_tile_list(c->h, c->opre_host, R, g.lds_order, longest);
    if (list.empty()) continue;
    if (dev_upload(c, &dl, list.data(), list.size())) return 1;
    if (R == 4) { g.lds_act4 = dl; g.lds_n4 = longest; } else { g.lds_act8 = dl; g.lds_n8 = longest; }
  }
  c->full_left = c->f.land_full_steps;
  return 0;
}

int create_hmix_advect(pop_ctx *c) {   // del4 and anis, upwind3, lw_lim
  const pop_config *cfg = &c->h.c;
  HostModel &h = c->h;
  DevGrid &g = c->g;
  if (cfg->hmix_tracer == 4) { g.DTN = c->d2["d4DTN"]; g.DTS = c->d2["d4DTS"]; g.DTE = c->d2["d4DTE"]; g.DTW = c->d2["d4DTW"]; }
  if (cfg->hmix_momentum == 4) {
    g.DUC = c->d2["d4DUC"]; g.DUN = c->d2["d4DUN"]; g.DUS = c->d2["d4DUS"]; g.DUE = c->d2["d4DUE"]; g.DUW = c->d2["d4DUW"];
    g.DMC = c->d2["d4DMC"]; g.DMN = c->d2["d4DMN"]; g.DMS = c->d2["d4DMS"]; g.DME = c->d2["d4DME"]; g.DMW = c->d2["d4DMW"]; g.DUM = c->d2["d4DUM"];
  }
  if (cfg->hmix_tracer == 4 || cfg->hmix_momentum == 4) { c->mix.D4AMF = c->d2["D4AMF"]; c->mix.D4AHF = c->d2["D4AHF"]; }
  if (cfg->hmix_momentum == 3) {   // anisotropic viscosity: the friction fields and the variable viscosities (local blocks)
    const size_t a3h = h.n3 * h.nblocks;
    if (dev_alloc(c, &c->HDU, a3h) || dev_alloc(c, &c->HDV, a3h)) return 1;
    if (cfg->lvariable_hmix_aniso) {
      const std::vector<double> fpa = local_part3(h, h.aniso_f[0]), fpe = local_part3(h, h.aniso_f[1]);
      if (dev_upload(c, &c->FPARA, fpa.data(), fpa.size()) || dev_upload(c, &c->FPERP, fpe.data(), fpe.size())) return 1;
    }
  }
  if (cfg->tadvect == 2) {
    const char *nx[6] = {"TALFXP", "TBETXP", "TGAMXP", "TALFXM", "TBETXM", "TDELXM"};
    const char *ny[6] = {"TALFYP", "TBETYP", "TGAMYP", "TALFYM", "TBETYM", "TDELYM"};
    for (int t = 0; t < 6; ++t) {
      c->upw3.cx[t] = c->d2[nx[t]]; c->upw3.cy[t] = c->d2[ny[t]];
      double *p; if (dev_upload(c, &p, h.upw_z[t].data(), h.upw_z[t].size())) return 1;
      c->upw3.cz[t] = p;
    }
  }
  if (cfg->tadvect == 3) {   // lw_lim: three flux-velocity fields, three work fields per tracer
    const size_t a3l = h.n3 * h.nblocks;
    if (dev_alloc(c, &c->lw.UTE, a3l) || dev_alloc(c, &c->lw.VTN, a3l) || dev_alloc(c, &c->lw.WTKB, a3l)) return 1;
    for (int n = 0; n < 2; ++n) if (dev_alloc(c, &c->lw.XOUT[n], a3l) || dev_alloc(c, &c->lw.XSTAR[n], a3l) || dev_alloc(c, &c->lw.XSTAR2[n], a3l)) return 1;
    c->lw.HTE = c->d2["HTE"]; c->lw.HTN = c->d2["HTN"]; c->lw.DXT = c->d2["DXT"]; c->lw.DYT = c->d2["DYT"];
    if (!c->lw.HTE || !c->lw.HTN || !c->lw.DXT || !c->lw.DYT) { c->err = "lw_lim: grid fields HTE / HTN / DXT / DYT missing"; return 1; }
  }
  return 0;
}

int create_gm(pop_ctx *c) {   // Gent-McWilliams: 14 coefficient fields + the tendency of each tracer
  const pop_config *cfg = &c->h.c;
  HostModel &h = c->h;
  if (cfg->hmix_tracer != 3) return 0;
  const size_t a3g = h.n3 * h.nblocks;
  GmDev &G = c->gm;
  for (int t = 0; t < 4; ++t) if (dev_alloc(c, &G.SLX[t], a3g) || dev_alloc(c, &G.SLY[t], a3g)) return 1;
  for (int t = 0; t < 2; ++t) if (dev_alloc(c, &G.KI[t], a3g) || dev_alloc(c, &G.KT[t], a3g) || dev_alloc(c, &G.HD[t], a3g) || dev_alloc(c, &G.GTK[t], a3g)) return 1;
  if (cfg->gm_kappa_type == 1) {   // KAPPA_VERTICAL: module state, 1 until the profile is computed (hmix_gm.F90:860)
    if (dev_alloc(c, &G.KV, a3g, false)) return 1;
    std::vector<double> ones(a3g, 1.0);
    HIPCHK(c, hipMemcpy(G.KV, ones.data(), a3g * sizeof(double), hipMemcpyHostToDevice));
  }
  G.tlt = cfg->gm_transition_layer == 1;
  if (G.tlt) {   // transition layer: SLA_SAVE of both halves, the layer's 2-D fields, the column terms of the merged stream function
    const size_t a2g = h.n2 * h.nblocks;
    for (int t = 0; t < 2; ++t) if (dev_alloc(c, &G.SLA[t], a3g)) return 1;
    if (dev_alloc(c, &G.DD, a2g) || dev_alloc(c, &G.TH, a2g) || dev_alloc(c, &G.ID, a2g) || dev_alloc(c, &G.KL, a2g) || dev_alloc(c, &G.ZTW, a2g)) return 1;
    for (int t = 0; t < 8; ++t) if (dev_alloc(c, &G.MW[t], a2g)) return 1;
  }
  if (cfg->gm_diag_bolus) {
    if (dev_alloc(c, &G.UISOP, a3g) || dev_alloc(c, &G.VISOP, a3g) || dev_alloc(c, &G.WISOP, a3g)) return 1;
    G.HTE = c->d2["HTE"]; G.HTN = c->d2["HTN"];
    if (!G.HTE || !G.HTN) { c->err = "gm: HTE / HTN missing"; return 1; }
  }
  G.HYX = c->d2["gmHYX"]; G.HXY = c->d2["gmHXY"]; G.RBR = c->d2["gmRBR"]; G.DXT = c->d2["DXT"]; G.DYT = c->d2["DYT"];
  if (!G.HYX || !G.HXY || !G.RBR || !G.DXT || !G.DYT) { c->err = "gm: grid fields missing"; return 1; }
  // hmix_gm_nml (hmix_gm.F90:364-428); 0 = the value of the default set-up
  G.ah = cfg->ah;
  G.ah_bolus = (cfg->ah_bolus != 0.0) ? cfg->ah_bolus : cfg->ah;
  G.ah_bkg_srfbl = (cfg->ah_bkg_srfbl != 0.0) ? cfg->ah_bkg_srfbl : cfg->ah;
  G.slm_r = (cfg->slm_r != 0.0) ? cfg->slm_r : 0.3;
  G.slm_b = (cfg->slm_b != 0.0) ? cfg->slm_b : 0.3;
  G.slope_tanh = cfg->gm_slope_control == 1; G.slope_ctl = cfg->gm_slope_control;
  G.HUS = c->d2["HUS"]; G.HUW = c->d2["HUW"];
  if (cfg->gm_kappa_type == 2) {   // KAPPA_VERTICAL(k) = kappa_depth(k) (:850-874): a 1-D profile, uploaded as the level table the coefficient kernel reads
    std::vector<double> kd(h.km + 2, 1.0);
    const double sc = (cfg->kappa_depth_scale != 0.0) ? cfg->kappa_depth_scale : 150000.0;
    for (int k = 1; k <= h.km; ++k) kd[k] = cfg->kappa_depth_1 + cfg->kappa_depth_2 * std::exp(-h.zt[k] / sc);
    double *p = nullptr;
    if (dev_upload(c, &p, kd.data(), kd.size())) return 1;
    G.kdepth = p;
  }
  G.kappa_bkg = cfg->gm_kappa_bkg_srfbl == 1; G.ah_bkg_bottom = cfg->ah_bkg_bottom;
  G.diff_tapering = G.slm_r != G.slm_b;                              // :964-968
  G.cancellation = !(G.diff_tapering || G.ah != G.ah_bolus) && !G.tlt;   // :970-987 (both kappa types equal)
  if (!G.cancellation && c->f.gm_sf_stored) for (int t = 0; t < 8; ++t) if (dev_alloc(c, &G.SF[t], a3g)) return 1;
  return 0;
}

int create_submeso(pop_ctx *c) {   // submesoscale scheme: six 2-D fields; with submeso_diag the tendency alone and the velocities
  const pop_config *cfg = &c->h.c;
  if (!cfg->lsubmesoscale_mixing) return 0;
  const size_t a2s = c->h.n2 * c->h.nblocks, a3s = c->h.n3 * c->h.nblocks;
  SubmDev &W = c->subm;
  if (dev_alloc(c, &W.ML, a2s) || dev_alloc(c, &W.HLS, a2s)) return 1;
  for (int t = 0; t < 4; ++t) if (dev_alloc(c, &W.B[t], a2s)) return 1;
  if (cfg->submeso_diag) {
    if (dev_alloc(c, &W.TD[0], a3s) || dev_alloc(c, &W.TD[1], a3s) || dev_alloc(c, &W.US, a3s) || dev_alloc(c, &W.VS, a3s) || dev_alloc(c, &W.WS, a3s)) return 1;
  }
  W.GTK[0] = c->gm.GTK[0]; W.GTK[1] = c->gm.GTK[1];
  W.TS = c->d2["SUBM_TIME_SCALE"]; W.HYX = c->gm.HYX; W.HXY = c->gm.HXY; W.DXT = c->gm.DXT; W.DYT = c->gm.DYT; W.HTE = c->d2["HTE"]; W.HTN = c->d2["HTN"];
  if (!W.TS || !W.HTE || !W.HTN) { c->err = "submeso: TIME_SCALE / HTE / HTN missing"; return 1; }
  // mix_submeso_nml (mix_submeso.F90:183-188); 0 = the code default
  W.eff = (cfg->efficiency_factor != 0.0) ? cfg->efficiency_factor : 0.07;
  W.hls0 = (cfg->hor_length_scale != 0.0) ? cfg->hor_length_scale : 5.0e5;
  W.max_hgs = 111.0e5;
  W.const_hls = cfg->luse_const_horiz_len_scale;
  W.all_levels = c->f.submeso_all_levels ? 1 : 0;
  return 0;
}

int create_state_fields(pop_ctx *c) {   // the prognostic state and the work fields
  const pop_config *cfg = &c->h.c;
  const Forms &f = c->f;
  HostModel &h = c->h;
  const size_t a2 = h.n2 * h.nblocks, a3 = h.n3 * h.nblocks;
  for (int t = 0; t < 3; ++t) {
    for (int n = 0; n < h.nt; ++n) if (dev_alloc(c, &c->TR[n][t], a3)) return 1;
    if (dev_alloc(c, &c->U[t], a3) || dev_alloc(c, &c->V[t], a3) || dev_alloc(c, &c->RHO[t], a3)) return 1;
    if (dev_alloc(c, &c->PS[t], a2) || dev_alloc(c, &c->GX[t], a2) || dev_alloc(c, &c->GY[t], a2) || dev_alloc(c, &c->UB[t], a2) || dev_alloc(c, &c->VB[t], a2)) return 1;
  }
  for (int n = 0; n < h.nt; ++n)
    if (dev_alloc(c, &c->STF[n], a2) || dev_alloc(c, &c->TFW[n], a2) || dev_alloc(c, &c->KPP_SRC[n], a3)) return 1;
  if (h.nt > 2) {   // work fields of the passive tracers (pop_ctx.hpp)
    if (cfg->hmix_tracer == 3 || cfg->hmix_tracer == 4) {
      for (int n = 2; n < h.nt; ++n) if (dev_alloc(c, &c->PW[n], a3)) return 1;
      if ((h.nt & 1) && dev_alloc(c, &c->PWX, a3)) return 1;
    }
    if (cfg->tadvect == 3 && (dev_alloc(c, &c->PL[0], a3) || dev_alloc(c, &c->PL[1], a3))) return 1;
    if (cfg->lsubmesoscale_mixing && cfg->submeso_diag) {
      for (int n = 2; n < h.nt; ++n) if (dev_alloc(c, &c->PTD[n], a3)) return 1;
      if ((h.nt & 1) && dev_alloc(c, &c->PTDX, a3)) return 1;
    }
    if (cfg->vmix_choice == 3 && dev_alloc(c, &c->KPPX, a3)) return 1;
  }
  // Forms::vdc_shared: one array serves both tracer classes; pop_get_field("VDC", n) returns it for n = 0 and 1
  if (dev_alloc(c, &c->VDC[0], (size_t)(h.km + 2) * a2)) return 1;
  if (f.vdc_shared) c->VDC[1] = c->VDC[0];
  else if (dev_alloc(c, &c->VDC[1], (size_t)(h.km + 2) * a2)) return 1;
  double **two[] = {&c->PGUESS, &c->FW, &c->FW_OLD, &c->SHF_QSW, &c->CHL, &c->DH, &c->DHU, &c->ZX, &c->ZY, &c->UH, &c->VH, &c->W3, &c->W4, &c->RHS,
                    &c->R, &c->S0, &c->S1, &c->Q, &c->Z, &c->AZ, &c->HBLT, &c->HMXL, &c->HMXL_DR};
  for (auto p : two) if (dev_alloc(c, p, a2)) return 1;
  c->centerWgt = c->d2["centerWgt"];
  double **three[] = {&c->VVC, &c->E3, &c->F3, &c->S3a, &c->S3b, &c->S3c, &c->S3d};
  for (auto p : three) if (dev_alloc(c, p, a3)) return 1;
  c->d2t[0] = c->S3a; c->d2t[1] = c->S3b; c->d2u[0] = c->S3a; c->d2u[1] = c->S3b;
  if (f.side_stream && (new_stream(c, &c->side) || new_event(c, &c->ev_fork) || new_event(c, &c->ev_d2t) || new_event(c, &c->ev_d2u) || new_event(c, &c->ev_vmixu))) return 1;
  if (f.del4_side && (dev_alloc(c, &c->d2t[0], a3) || dev_alloc(c, &c->d2t[1], a3) || dev_alloc(c, &c->d2u[0], a3) || dev_alloc(c, &c->d2u[1], a3))) return 1;
  if (f.d2t_fuse && (dev_alloc(c, &c->d2t_next[0], a3) || dev_alloc(c, &c->d2t_next[1], a3))) return 1;
  if (f.d2u_fuse && (dev_alloc(c, &c->d2u_next[0], a3) || dev_alloc(c, &c->d2u_next[1], a3))) return 1;
  return 0;
}

int create_solver_lists(pop_ctx *c) {   // the chunk lists of the fused solvers, their partials, the block numbering
  HostModel &h = c->h;
  c->nchunk = red_grid_x(c->g);
  const ChunkLists L = solver_chunk_lists(h, c->opre_host);
  c->red_active_total += L.active_total;
  if (L.nact) {
    if (dev_upload(c, &c->red_act, L.list.data(), L.list.size()) || dev_upload(c, &c->red_cnt, L.cnt.data(), L.cnt.size())) return 1;
    c->red_nact = L.nact;
  }
  if (dev_alloc(c, &c->partial, (size_t)c->nchunk * h.nblocks * 2 + POP_RELAY_SLACK) || dev_alloc(c, &c->blocksum, (size_t)h.nblocks_tot * 4)) return 1;
  { std::vector<int> io(h.nblocks_tot); for (int b = 0; b < h.nblocks_tot; ++b) io[b] = b; if (dev_upload(c, &c->iota, io.data(), io.size())) return 1; }
  if (dev_alloc(c, &c->sc, 1)) return 1;
  { std::vector<int> gid(h.nblocks); for (int lb = 0; lb < h.nblocks; ++lb) gid[lb] = h.local_ids[lb] - 1; if (dev_upload(c, &c->gid, gid.data(), gid.size())) return 1; }
  { std::vector<int> log(h.nblocks_tot, -1); for (int lb = 0; lb < h.nblocks; ++lb) log[h.local_ids[lb] - 1] = lb; if (dev_upload(c, &c->loc_of_gid, log.data(), log.size())) return 1; }
  return 0;
}

int create_halo_device(pop_ctx *c) {   // the halo plan: copies and fills, peers, the tripole plan, the concatenated lists and per-cell maps
  HostModel &h = c->h;
  c->ncopy = (int)h.halo.copy_dst.size(); c->nfill = (int)h.halo.fill_dst.size();
  if (c->ncopy && (dev_upload(c, &c->copy_dst, h.halo.copy_dst.data(), c->ncopy) || dev_upload(c, &c->copy_src, h.halo.copy_src.data(), c->ncopy))) return 1;
  if (c->nfill && dev_upload(c, &c->fill_dst, h.halo.fill_dst.data(), c->nfill)) return 1;
  for (auto &pp : h.halo.peers) {
    DevPeer d; d.rank = pp.rank; d.nsend = (int)pp.send_src.size(); d.nrecv = (int)pp.recv_dst.size();
    if (d.nsend && dev_upload(c, &d.send_src, pp.send_src.data(), d.nsend)) return 1;
    if (d.nrecv && dev_upload(c, &d.recv_dst, pp.recv_dst.data(), d.nrecv)) return 1;
    c->peers.push_back(d);
  }
  if (h.c.ns_boundary == 2) {   // tripole plan (non-empty on the rank that owns the top row of blocks) + evaluation buffer
    size_t nmax = 1;
    for (int loc = 0; loc < 5; ++loc) {
      const TripolePlan &T = h.halo.tripole[loc];
      c->tp_n[loc] = (int)T.dst.size();
      nmax = std::max(nmax, T.dst.size());
      if (c->tp_n[loc] && (dev_upload(c, &c->tp_dst[loc], T.dst.data(), T.dst.size()) || dev_upload(c, &c->tp_a[loc], T.a.data(), T.a.size()) ||
                           dev_upload(c, &c->tp_b[loc], T.b.data(), T.b.size()))) return 1;
    }
    if (dev_alloc(c, &c->tp_buf, nmax * (size_t)(h.km + 2))) return 1;
  }
  const PeerLists L = peer_lists(h.halo);
  c->nsend_all = (int)L.ss.size(); c->nrecv_all = (int)L.rd.size();
  if (!h.halo.peers.empty()) {   // the kernels that pack / read a one-level message themselves
    const PeerCellMaps M = peer_cell_maps(L, h.n2 * h.nblocks);
    c->halo_ns_only = halo_ns_only(h);
    if (dev_upload(c, &c->sendmap, M.smap.data(), M.smap.size()) || dev_upload(c, &c->send_off, M.off.data(), M.off.size()) ||
        dev_upload(c, &c->send_slot, M.slot.data(), std::max<size_t>(M.slot.size(), 1)) || dev_upload(c, &c->rmap, M.rmap.data(), M.rmap.size())) return 1;
    if (new_event(c, &c->ev_sa) || new_event(c, &c->ev_sx)) return 1;
  }
  if (c->nsend_all && (dev_upload(c, &c->sa_src, L.ss.data(), L.ss.size()) || dev_upload(c, &c->sa_start, L.st.data(), L.st.size()) || dev_upload(c, &c->sa_cnt, L.sc.data(), L.sc.size()))) return 1;
  if (c->nrecv_all && (dev_upload(c, &c->ra_dst, L.rd.data(), L.rd.size()) || dev_upload(c, &c->ra_start, L.rt.data(), L.rt.size()) || dev_upload(c, &c->ra_cnt, L.rc.data(), L.rc.size()))) return 1;
  return 0;
}

int create_solver_device(pop_ctx *c) {   // the source map, pinned results, P-CSI and EVP tables, the replicated view
  const pop_config *cfg = &c->h.c;
  const Forms &f = c->f;
  HostModel &h = c->h;
  // source map for the fused solver path: ghost cell -> local source cell, -1 = fill value
  c->h_srcmap = local_srcmap(h);
  if (dev_upload(c, &c->srcmap, c->h_srcmap.data(), c->h_srcmap.size())) return 1;
  if (pinned_alloc(c, &c->persist_out, 4) || pinned_alloc(c, &c->host_sc, 1) || pinned_alloc(c, &c->host_rr, 8)) return 1;
  for (auto &e : c->chk_ev) if (new_event(c, &e)) return 1;
  if (cfg->solver_choice == 3) {
    const std::vector<double> om = pcsi_omega(h, c->pcsi_csy);
    if (dev_upload(c, &c->pcsi_omega, om.data(), om.size()) || dev_alloc(c, &c->pcsi_base, 1)) return 1;
  }
  if (use_evp(*cfg)) {
    const EvpTables T = evp_tables(h);
    int *dm; double *d0, *d1, *d2, *d3, *d4;
    if (dev_upload(c, &dm, T.meta.data(), T.meta.size()) || dev_upload(c, &d0, T.cc.data(), T.cc.size()) || dev_upload(c, &d1, T.ne.data(), T.ne.size()) ||
        dev_upload(c, &d2, T.icc.data(), T.icc.size()) || dev_upload(c, &d3, T.ine.data(), T.ine.size()) || dev_upload(c, &d4, T.rinv.data(), T.rinv.size())) return 1;
    c->evp = EvpDev{(long long)T.S, (const int4 *)dm, d0, d1, d2, d3, d4, c->d2["evpC0"], c->d2["btropWgtNE"]};
    c->use_evp = true;
  }
  if (f.pcsi_two_step || f.pcsi_two_step_dist) {   // two P-CSI iterations per launch: the raw residual of a pair, the fold rows of a tripole
    if (dev_alloc(c, &c->pcsi_raw, h.n2 * h.nblocks)) return 1;
    std::vector<int> jfold;
    pcsi_fold_local(h, c->h_srcmap, jfold);
    if (cfg->ns_boundary == 2 && dev_upload(c, &c->pcsi_jfold, jfold.data(), jfold.size())) return 1;
  }
  if (f.replicated) {   // every block of the decomposition on every rank
    const size_t NG = h.n2 * h.nblocks_tot;
    SolveView &v = c->gv;
    v.g = c->g; v.g.nblocks = h.nblocks_tot;
    double *p;
    if (dev_upload(c, &p, h.f2["btropWgtNE"].data(), NG)) return 1; v.g.WNE = p;
    if (dev_upload(c, &p, h.f2["btropWgtEast"].data(), NG)) return 1; v.g.WEa = p;
    if (dev_upload(c, &p, h.f2["btropWgtNorth"].data(), NG)) return 1; v.g.WNo = p;
    if (dev_upload(c, &p, h.f2["btropXW"].data(), NG)) return 1; v.g.XW = p;
    if (dev_upload(c, &p, h.f2["btropYW"].data(), NG)) return 1; v.g.YW = p;
    if (dev_upload(c, &p, h.f2["centerWgtIndep"].data(), NG)) return 1; v.g.WC0 = p;
    if (dev_upload(c, &p, h.f2["mMask"].data(), NG)) return 1; v.g.mMask = p;
    std::vector<unsigned char> m8;
    unsigned char *d8;
    if (mask_bytes(h.f2["mMask"], m8)) { c->err = "solver mask is not 0/1"; return 1; }
    if (dev_upload(c, &d8, m8.data(), NG)) return 1;
    v.g.mMask8 = d8;
    if (dev_upload(c, &c->gTAREA, h.f2["TAREA"].data(), NG)) return 1;
    if (dev_upload(c, &c->gKMT, h.i2["KMT"].data(), NG)) return 1;
    double **vecs[] = {&v.X, &v.R, &v.Z, &v.S0, &v.S1, &v.Q, &v.RHS, &v.C};
    for (auto q : vecs) if (dev_alloc(c, q, NG)) return 1;
    if (dev_alloc(c, &v.partial, (size_t)c->nchunk * h.nblocks_tot * 2 + POP_RELAY_SLACK) || dev_alloc(c, &v.blocksum, (size_t)h.nblocks_tot * 4)) return 1;
    std::vector<int> gsm = global_srcmap(h), gid(h.nblocks_tot);
    for (int b = 0; b < h.nblocks_tot; ++b) gid[b] = b;
    if (dev_upload(c, &v.srcmap, gsm.data(), gsm.size()) || dev_upload(c, &v.gid, gid.data(), gid.size())) return 1;
    v.nchunk = c->nchunk; v.nblocks_tot = h.nblocks_tot;
  }
  return 0;
}

int create_mix_and_ahead(pop_ctx *c) {   // vertical mixing, the short-wave tables, the second set of KPP outputs
  const pop_config *cfg = &c->h.c;
  const Forms &f = c->f;
  HostModel &h = c->h;
  const size_t a2 = h.n2 * h.nblocks, a3 = h.n3 * h.nblocks;
  // vmix_const: constant coefficients for all time (vmix_const.F90:121-122)
  if (cfg->vmix_choice == 1) {
    std::vector<double> v((size_t)(h.km + 2) * a2, cfg->const_vdc), w(a3, cfg->const_vvc);
    HIPCHK(c, hipMemcpy(c->VDC[0], v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->VVC, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (mix_create(c->h, f, c->g, c->mix, c->allocs, c->err)) return 1;
  c->KBL = const_cast<int *>(mix_kpp_kbl(c->mix));
  if (cfg->lsw_absorb != 0 && sw_tables_create(c->h, c->allocs, c->err)) return 1;   // lsw_absorb without KPP's lshort_wave
  if (c->h.sw.CHLI) {   // the default chlorophyll amount the table index was built for
    std::vector<double> chl((size_t)c->g.n2 * c->g.nblocks, 0.25);
    HIPCHK(c, hipMemcpy(c->CHL, chl.data(), chl.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  // KPP look-ahead (Forms::kpp_ahead): second set of KPP outputs, own stream
  // (Gent-McWilliams adds its isopycnal part to VDC after vmix_coeffs -- to the arrays swapped in, at the step they belong to; with the
  // mixed-layer-depth diagnostics the look-ahead writes a second pair HMXL / HMXL_DR that is swapped in with the rest)
  if (f.kpp_ahead) {
    for (int n = 0; n < 2; ++n) if (dev_alloc(c, &c->KPPa[n], a3)) return 1;
    if (h.nt > 2 && dev_alloc(c, &c->KPPXa, a3)) return 1;
    if (dev_alloc(c, &c->VDCa[0], (size_t)(h.km + 2) * a2)) return 1;
    if (f.vdc_shared) c->VDCa[1] = c->VDCa[0];
    else if (dev_alloc(c, &c->VDCa[1], (size_t)(h.km + 2) * a2)) return 1;
    if (dev_alloc(c, &c->VVCa, a3) || dev_alloc(c, &c->HBLTa, a2) || dev_alloc(c, &c->KBLa, a2)) return 1;
    if (c->h.c.kpp_ml_diagnostics == 1 && (dev_alloc(c, &c->HMXLa, a2) || dev_alloc(c, &c->HMXL_DRa, a2))) return 1;
    if (new_stream(c, &c->ahead) || new_event(c, &c->ev_ahead_fork) || new_event(c, &c->ev_ahead)) return 1;
  }
  return 0;
}

int create_initial_state(pop_ctx *c) {   // initial.F90:1389-1427, 1660-1676: T,S on all three levels, RHO(cur), RHO(old)
  HostModel &h = c->h;
  const size_t a3 = h.n3 * h.nblocks;
  c->oldt = 0; c->curt = 1; c->newt = 2; c->mixt = 1;
  for (int t = 0; t < 3; ++t) {
    HIPCHK(c, hipMemcpy(c->TR[0][t], h.f3["TEMP0"].data(), a3 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->TR[1][t], h.f3["SALT0"].data(), a3 * sizeof(double), hipMemcpyHostToDevice));
  }
  launch_state3d(c->g, c->TR[0][c->curt], c->TR[1][c->curt], c->RHO[c->curt], c->stream);
  launch_state3d(c->g, c->TR[0][c->oldt], c->TR[1][c->oldt], c->RHO[c->oldt], c->stream);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  h.f3.clear();
  return 0;
}

}  // namespace
