// launch_tavg.hpp -- time-averaged output (tavg.F90): the table of entries the library knows, the launch tables of the call
// sites and their launches.  Part of the single translation unit pop_amd.hip (included after pop_ctx.hpp).
//
// An entry is one tavg field of the reference (define_tavg_field): a name, a method, a rank and the call site of
// accumulate_tavg_field that feeds it.  The sites are places in the phase sequence of a step (TavgSite, pop_ctx.hpp):
//   FORCING  pop_dhdt                      tavg_forcing (forcing.F90:502-577), surface_hgt.F90:294-313
//   STATE    head of pop_baroclinic_driver baroclinic.F90:772-806
//   TRACER   the same place; with the Robert filter inside step_rf (baroclinic.F90:810, step_mod.F90:1290-1298)
//   VMIX     after the vertical-mixing coefficients of the step are in place, before Gent-McWilliams adds K33
//   HMIX     after the horizontal mixing of the tracers (bolus and submesoscale velocities)
//   BTROP    end of the barotropic driver  barotropic.F90:687-693
//   QFLUX    pop_ice_flx_to_coupler        step_mod.F90:844-849
#pragma once

namespace {

// sources of the entries; tavg_src resolves one to the array it names at the moment of the launch (time levels rotate, the KPP
// look-ahead swaps the sets of coefficients)
enum TavgSid {
  SID_U = 0, SID_V, SID_T, SID_S, SID_TOLD, SID_RHO,
  SID_TR0,                                  // + n: passive tracer n (0-based, 2 .. MAXNT-1) at cur
  SID_SMF1 = SID_TR0 + MAXNT, SID_SMF2, SID_FW, SID_STF1, SID_STF2, SID_QSW, SID_PS, SID_GX, SID_GY,
  SID_HU, SID_UB, SID_VB,
  SID_HBLT, SID_HMXL, SID_HMXL_DR, SID_VDC_T, SID_VDC_S, SID_VVC, SID_KPPS_T, SID_KPPS_S, SID_KVMIX, SID_KVMIX_M,
  SID_UISOP, SID_VISOP, SID_WISOP, SID_USUBM, SID_VSUBM, SID_WSUBM,
  SID_QFLUX,
  SID_TFW1, SID_TFW2,
  SID_CPL0                                  // + f: imported field f of the coupled forcing (kernels_forcing.hpp CplField)
};
enum TavgNeed { TN_NONE = 0, TN_KPP, TN_MLD, TN_TIDAL, TN_GM_BOLUS, TN_SUBM_DIAG, TN_ICE, TN_CPL };

struct TavgAvail {
  std::string name;
  int site, ndims, method, kmax;            // kmax = 0: km
  int expr, a, b;
  double cst, cst2;
  bool cells, vint;
  int need;
};

// names the reference defines whose call sites are not built
const char *const tavg_left_out[] = {
  "UET", "VNT", "WTT", "UES", "VNS", "WTS", "ADVT", "ADVS", "WVEL", "WVEL2", "PD", "PV", "Q", "RHOU", "RHOV", "URHO", "VRHO", "WRHO", "PVWM", "PVWP",
  "UPV", "VPV", "UQ", "VQ", "UTE_POS", "UTE_NEG", "VTN_POS", "VTN_NEG", "WTK_POS", "WTK_NEG", "UEU", "VNU", "UEV", "VNV", "WTU", "WTV",
  "ADVU", "ADVV", "GRADX", "GRADY", "HDIFFU", "HDIFFV", "VDIFFU", "VDIFFV", "UDP",
  "HDIFT", "HDIFS", "DIA_IMPVF_TEMP", "DIA_IMPVF_SALT", "RF_TEND_TEMP", "RF_TEND_SALT", "RESID_T", "RESID_S",
  "TEMP_27", "TEMP_43", "BSF", "N_HEAT", "N_SALT", "U2_2", "V2_2", "VDC_BCK", "VVC_BCK", "SFWF_WRST",
  "TEMP_z_t_150m", "SALT_z_t_150m", "UVEL_z_t_150m", "VVEL_z_t_150m"};

// every entry this configuration knows.  Host logic only: a host-only context answers pop_tavg_info from it too
std::vector<TavgAvail> tavg_avail(const pop_ctx *c) {
  std::vector<TavgAvail> v;
  auto add = [&](const std::string &name, int site, int ndims, int method, int kmax, int expr, int a, int b, bool cells, bool vint, int need = TN_NONE,
                 double cst = 0.0, double cst2 = 0.0) { v.push_back(TavgAvail{name, site, ndims, method, kmax, expr, a, b, cst, cst2, cells, vint, need}); };
  auto f3 = [&](const std::string &name, int site, int expr, int a, int b = -1, int method = TAVG_AVG, int need = TN_NONE) {
    add(name, site, 3, method, 0, expr, a, b, true, false, need);
  };
  auto lev1 = [&](const std::string &name, int site, int expr, int a) { add(name, site, 2, TAVG_AVG, 1, expr, a, -1, true, false); };   // 2-D, level 1
  auto f2 = [&](const std::string &name, int site, int expr, int a, int b = -1, int method = TAVG_AVG, int need = TN_NONE, double cst = 0.0, double cst2 = 0.0) {
    add(name, site, 2, method, 1, expr, a, b, false, false, need, cst, cst2);
  };
  auto vint = [&](const std::string &name, int site, int kmax, int expr, int a, int b = -1) { add(name, site, 2, TAVG_AVG, kmax, expr, a, b, false, true); };
  const pop_ctx::Ice &I = c->ice;
  // pop_constants.F90:336, 364-365 with the code defaults of rho_sw, cp_sw, ocn_ref_salinity unless pop_init_ice gave others
  const double hflux_factor = hflux_factor_of(c);
  const double salinity_factor = -(I.inited ? I.nml.ocn_ref_salinity : 34.7) * 1.0e-4;
  const bool fw_as_salt = I.inited && I.nml.lfw_as_salt_flx;
  // FORCING
  f2("SHF", TS_FORCING, TX_M_SUMDIVC, SID_STF1, SID_QSW, TAVG_AVG, TN_NONE, hflux_factor);
  f2("SHF_QSW", TS_FORCING, TX_M_DIVC, SID_QSW, -1, TAVG_AVG, TN_NONE, hflux_factor);
  f2("SHF_QSW_2", TS_FORCING, TX_M_DIVC, SID_QSW, -1, TAVG_AVG, TN_NONE, hflux_factor);
  // the variable-thickness surface layer with fresh-water fluxes (forcing.F90:531-537): m/yr; with lfw_as_salt_flx the virtual salt flux
  if (fw_as_salt) f2("SFWF", TS_FORCING, TX_M_DIVC, SID_STF2, -1, TAVG_AVG, TN_NONE, salinity_factor);
  else f2("SFWF", TS_FORCING, TX_M_MULCC, SID_FW, -1, TAVG_AVG, TN_NONE, 86400.0 * 365.0, 0.01);
  f2("TAUX", TS_FORCING, TX_X, SID_SMF1); f2("TAUX2", TS_FORCING, TX_SQR, SID_SMF1);
  f2("TAUY", TS_FORCING, TX_X, SID_SMF2); f2("TAUY2", TS_FORCING, TX_SQR, SID_SMF2);
  f2("FW", TS_FORCING, TX_X, SID_FW);
  f2("SSH", TS_FORCING, TX_DIVC, SID_PS, -1, TAVG_AVG, TN_NONE, GRAV); f2("SSH_2", TS_FORCING, TX_DIVC, SID_PS, -1, TAVG_AVG, TN_NONE, GRAV);
  f2("SSH2", TS_FORCING, TX_DIVC_SQR, SID_PS, -1, TAVG_AVG, TN_NONE, GRAV);
  f2("H3", TS_FORCING, TX_DIVC_SQSUM, SID_GX, SID_GY, TAVG_AVG, TN_NONE, GRAV);
  // forcing.F90:578-580 and tavg_coupled_forcing (forcing_coupled.F90:1111-1122): after pop_init_coupled_forcing
  f2("TFW_T", TS_FORCING, TX_DIVC, SID_TFW1, -1, TAVG_AVG, TN_CPL, hflux_factor);
  f2("TFW_S", TS_FORCING, TX_MULCC, SID_TFW2, -1, TAVG_AVG, TN_CPL, I.inited ? I.nml.rho_sw : 4.1 / 3.996, 10.0);
  f2("U10_SQR", TS_FORCING, TX_X, SID_CPL0 + CF_U10, -1, TAVG_AVG, TN_CPL);
  {
    const std::pair<const char *, int> cpl[] = {{"EVAP_F", CF_EVAP}, {"PREC_F", CF_PREC}, {"SNOW_F", CF_SNOW}, {"MELT_F", CF_MELT}, {"ROFF_F", CF_ROFF}, {"IOFF_F", CF_IOFF},
                                                {"SALT_F", CF_SALT}, {"SENH_F", CF_SENH}, {"LWUP_F", CF_LWUP}, {"LWDN_F", CF_LWDN}, {"MELTH_F", CF_MELTH}, {"IFRAC", CF_IFRAC}};
    for (const auto &e : cpl) f2(e.first, TS_FORCING, TX_X, SID_CPL0 + e.second, -1, TAVG_AVG, TN_CPL);
  }
  // STATE
  f3("UVEL", TS_STATE, TX_X, SID_U); f3("UVEL_2", TS_STATE, TX_X, SID_U); f3("VVEL", TS_STATE, TX_X, SID_V); f3("VVEL_2", TS_STATE, TX_X, SID_V);
  f3("UVEL2", TS_STATE, TX_SQR, SID_U); f3("VVEL2", TS_STATE, TX_SQR, SID_V);
  f3("KE", TS_STATE, TX_KE, SID_U, SID_V); f3("UV", TS_STATE, TX_XY, SID_U, SID_V);
  // 2-D entries the reference feeds at every level k <= 8 (baroclinic.F90:280-292, 784-800): the sum over those levels, in k order
  vint("U1_8", TS_STATE, 8, TX_X, SID_U); vint("V1_8", TS_STATE, 8, TX_X, SID_V);
  lev1("U1_1", TS_STATE, TX_X, SID_U); lev1("V1_1", TS_STATE, TX_X, SID_V);
  // TRACER
  f3("TEMP", TS_TRACER, TX_X, SID_T); f3("TEMP_2", TS_TRACER, TX_X, SID_T); f3("SALT", TS_TRACER, TX_X, SID_S); f3("SALT_2", TS_TRACER, TX_X, SID_S);
  f3("TEMP_MAX", TS_TRACER, TX_X, SID_T, -1, TAVG_MAX); f3("TEMP_MIN", TS_TRACER, TX_X, SID_T, -1, TAVG_MIN);
  f3("SALT_MAX", TS_TRACER, TX_X, SID_S, -1, TAVG_MAX); f3("SALT_MIN", TS_TRACER, TX_X, SID_S, -1, TAVG_MIN);
  f3("TEMP2", TS_TRACER, TX_SQR, SID_T); f3("SALT2", TS_TRACER, TX_SQR, SID_S); f3("ST", TS_TRACER, TX_XY, SID_T, SID_S);
  f3("RHO", TS_TRACER, TX_X, SID_RHO);
  vint("T1_8", TS_TRACER, 8, TX_X, SID_T); vint("S1_8", TS_TRACER, 8, TX_X, SID_S);
  lev1("SST", TS_TRACER, TX_X, SID_T); lev1("SST2", TS_TRACER, TX_SQR, SID_T); lev1("SSS", TS_TRACER, TX_X, SID_S); lev1("SSS2", TS_TRACER, TX_SQR, SID_S);
  f3("dTEMP_POS_3D", TS_TRACER, TX_DPOS, SID_T, SID_TOLD); f3("dTEMP_NEG_3D", TS_TRACER, TX_DNEG, SID_T, SID_TOLD);
  vint("dTEMP_POS_2D", TS_TRACER, 0, TX_DPOS, SID_T, SID_TOLD); vint("dTEMP_NEG_2D", TS_TRACER, 0, TX_DNEG, SID_T, SID_TOLD);
  vint("RHO_VINT", TS_TRACER, 0, TX_RHO_VINT, SID_RHO);
  for (int n = 2; n < c->h.nt; ++n) {   // passive_tracers.F90:1336-1353
    const std::string nm = restart_tracer_name(c->h, n);
    f3(nm, TS_TRACER, TX_X, SID_TR0 + n); f3(nm + "_2", TS_TRACER, TX_X, SID_TR0 + n); f3(nm + "_SQR", TS_TRACER, TX_SQR, SID_TR0 + n);
    lev1(nm + "_SURF", TS_TRACER, TX_X, SID_TR0 + n);
  }
  // VMIX
  f3("VDC_T", TS_VMIX, TX_X, SID_VDC_T); f3("VDC_S", TS_VMIX, TX_X, SID_VDC_S); f3("VVC", TS_VMIX, TX_X, SID_VVC);
  f3("KPP_SRC_TEMP", TS_VMIX, TX_X, SID_KPPS_T, -1, TAVG_AVG, TN_KPP); f3("KPP_SRC_SALT", TS_VMIX, TX_X, SID_KPPS_S, -1, TAVG_AVG, TN_KPP);
  f2("HBLT", TS_VMIX, TX_X, SID_HBLT, -1, TAVG_AVG, TN_KPP); f2("XBLT", TS_VMIX, TX_X, SID_HBLT, -1, TAVG_MAX, TN_KPP); f2("TBLT", TS_VMIX, TX_X, SID_HBLT, -1, TAVG_MIN, TN_KPP);
  f2("HMXL", TS_VMIX, TX_X, SID_HMXL, -1, TAVG_AVG, TN_MLD); f2("HMXL_2", TS_VMIX, TX_X, SID_HMXL, -1, TAVG_AVG, TN_MLD);
  f2("XMXL", TS_VMIX, TX_X, SID_HMXL, -1, TAVG_MAX, TN_MLD); f2("XMXL_2", TS_VMIX, TX_X, SID_HMXL, -1, TAVG_MAX, TN_MLD); f2("TMXL", TS_VMIX, TX_X, SID_HMXL, -1, TAVG_MIN, TN_MLD);
  f2("HMXL_DR", TS_VMIX, TX_X, SID_HMXL_DR, -1, TAVG_AVG, TN_MLD); f2("HMXL_DR_2", TS_VMIX, TX_X, SID_HMXL_DR, -1, TAVG_AVG, TN_MLD);
  f2("HMXL_DR2", TS_VMIX, TX_SQR, SID_HMXL_DR, -1, TAVG_AVG, TN_MLD);
  f2("XMXL_DR", TS_VMIX, TX_X, SID_HMXL_DR, -1, TAVG_MAX, TN_MLD); f2("TMXL_DR", TS_VMIX, TX_X, SID_HMXL_DR, -1, TAVG_MIN, TN_MLD);
  f3("KVMIX", TS_VMIX, TX_X, SID_KVMIX, -1, TAVG_AVG, TN_TIDAL); f3("KVMIX_M", TS_VMIX, TX_X, SID_KVMIX_M, -1, TAVG_AVG, TN_TIDAL);
  // HMIX
  f3("UISOP", TS_HMIX, TX_X, SID_UISOP, -1, TAVG_AVG, TN_GM_BOLUS); f3("VISOP", TS_HMIX, TX_X, SID_VISOP, -1, TAVG_AVG, TN_GM_BOLUS);
  f3("WISOP", TS_HMIX, TX_X, SID_WISOP, -1, TAVG_AVG, TN_GM_BOLUS);
  f3("USUBM", TS_HMIX, TX_X, SID_USUBM, -1, TAVG_AVG, TN_SUBM_DIAG); f3("VSUBM", TS_HMIX, TX_X, SID_VSUBM, -1, TAVG_AVG, TN_SUBM_DIAG);
  f3("WSUBM", TS_HMIX, TX_X, SID_WSUBM, -1, TAVG_AVG, TN_SUBM_DIAG);
  // BTROP
  f2("SU", TS_BTROP, TX_XY, SID_HU, SID_UB); f2("SV", TS_BTROP, TX_XY, SID_HU, SID_VB);
  // QFLUX: const = tlast_ice, set at the launch
  f2("QFLUX", TS_QFLUX, TX_X, SID_QFLUX, -1, TAVG_QFLUX, TN_ICE);
  for (TavgAvail &a : v) if (a.kmax == 0) a.kmax = c->h.km;
  return v;
}

// "" when the configuration produces the source of an entry, else the missing switch
std::string tavg_missing(const pop_ctx *c, int need) {
  const pop_config &cf = c->h.c;
  switch (need) {
    case TN_KPP: return cf.vmix_choice == 3 ? "" : "vmix_choice = 3 (kpp)";
    case TN_MLD: return (cf.vmix_choice == 3 && cf.kpp_ml_diagnostics == 1) ? "" : "vmix_choice = 3 (kpp) with kpp_ml_diagnostics = 1";
    case TN_TIDAL: return (c->tidal.on && c->tidal.nml.tidal_diag) ? "" : "pop_init_tidal_mixing with ltidal_mixing and tidal_diag";
    case TN_GM_BOLUS: return (cf.hmix_tracer == 3 && cf.gm_diag_bolus) ? "" : "hmix_tracer = 3 (gm) with gm_diag_bolus = 1";
    case TN_SUBM_DIAG: return (cf.struct_version >= 7 && cf.lsubmesoscale_mixing && cf.submeso_diag) ? "" : "lsubmesoscale_mixing with submeso_diag = 1";
    case TN_ICE: return c->ice.inited ? "" : "pop_init_ice";
    case TN_CPL: return c->cpl.inited ? "" : "pop_init_coupled_forcing";
    default: return "";
  }
}

TavgSrc tavg_src(pop_ctx *c, int sid) {
  const int km = c->g.km, cu = c->curt, o = c->oldt;
  auto s3 = [&](const double *p) { return TavgSrc{p, km, 0}; };
  auto s2 = [&](const double *p) { return TavgSrc{p, 1, 0}; };
  auto vd = [&](const double *p) { return TavgSrc{p, km + 2, 1}; };   // VDC is stored (0:km+1): reference level kk at slot kk
  if (sid >= SID_TR0 && sid < SID_TR0 + MAXNT) return s3(c->TR[sid - SID_TR0][cu]);
  if (sid >= SID_CPL0 && sid < SID_CPL0 + CF_NF) return s2(c->cpl.F[sid - SID_CPL0]);
  switch (sid) {
    case SID_U: return s3(c->U[cu]);
    case SID_V: return s3(c->V[cu]);
    case SID_T: return s3(c->TR[0][cu]);
    case SID_S: return s3(c->TR[1][cu]);
    case SID_TOLD: return s3(c->TR[0][o]);
    case SID_RHO: return s3(c->RHO[cu]);
    case SID_SMF1: return s2(c->d2["SMF1"]);
    case SID_SMF2: return s2(c->d2["SMF2"]);
    case SID_FW: return s2(c->FW);
    case SID_STF1: return s2(c->STF[0]);
    case SID_STF2: return s2(c->STF[1]);
    case SID_QSW: return s2(c->SHF_QSW);
    case SID_PS: return s2(c->PS[cu]);
    case SID_GX: return s2(c->GX[cu]);
    case SID_GY: return s2(c->GY[cu]);
    case SID_HU: return s2(c->g.HU);
    case SID_UB: return s2(c->UB[cu]);
    case SID_VB: return s2(c->VB[cu]);
    case SID_HBLT: return s2(c->HBLT);
    case SID_HMXL: return s2(c->HMXL);
    case SID_HMXL_DR: return s2(c->HMXL_DR);
    case SID_VDC_T: return vd(c->VDC[0]);
    case SID_VDC_S: return vd(c->VDC[c->h.c.vmix_choice == 3 ? 1 : 0]);
    case SID_VVC: return s3(c->VVC);
    case SID_KPPS_T: return s3(c->KPP_SRC[0]);
    case SID_KPPS_S: return s3(c->KPP_SRC[1]);
    case SID_KVMIX: return s3(c->mix.kpp ? ((const KppHost *)c->mix.kpp)->tidal.KV : nullptr);
    case SID_KVMIX_M: return s3(c->mix.kpp ? ((const KppHost *)c->mix.kpp)->tidal.KVM : nullptr);
    case SID_UISOP: return s3(c->gm.UISOP);
    case SID_VISOP: return s3(c->gm.VISOP);
    case SID_WISOP: return s3(c->gm.WISOP);
    case SID_USUBM: return s3(c->subm.US);
    case SID_VSUBM: return s3(c->subm.VS);
    case SID_WSUBM: return s3(c->subm.WS);
    case SID_QFLUX: return s2(c->ice.QFLUX);
    case SID_TFW1: return s2(c->TFW[0]);
    case SID_TFW2: return s2(c->TFW[1]);
  }
  return TavgSrc{nullptr, 1, 0};
}

// the launch tables of every site from the request list and the on/off state of the streams: only entries whose stream is on
int tavg_build(pop_ctx *c) {
  TavgState &T = c->tavg;
  const std::vector<TavgAvail> avail = tavg_avail(c);
  for (TavgEntry &e : T.req)   // constants that pop_init_ice may have changed since the request
    for (const TavgAvail &a : avail) if (a.name == e.name) { e.expr = a.expr; e.a = a.a; e.b = a.b; e.cst = a.cst; e.cst2 = a.cst2; }
  for (int s = 0; s < TS_NSITES; ++s) {
    TavgSiteTab &S = T.site[s];
    S = TavgSiteTab{};
    auto slot = [&](TavgTable &t, int *sids, int sid) -> int {
      if (sid < 0) return 0;
      for (int i = 0; i < t.nsrc; ++i) if (sids[i] == sid) return i;
      if (t.nsrc == TAVG_MAX_SRC) return -1;
      sids[t.nsrc] = sid;
      return t.nsrc++;
    };
    auto fits = [&](const TavgTable &t, const int *sids, const TavgEntry &e) {   // would the entry's sources find a slot?
      int fresh = 0;
      for (int sid : {e.a, e.b}) {
        bool have = sid < 0;
        for (int i = 0; i < t.nsrc && !have; ++i) have = sids[i] == sid;
        fresh += have ? 0 : 1;
      }
      return t.nsrc + fresh <= TAVG_MAX_SRC && t.n < TAVG_MAX_FIELDS;
    };
    auto put = [&](TavgTable &t, int *sids, const TavgEntry &e) -> int {
      const int a = slot(t, sids, e.a), b = slot(t, sids, e.b);
      if (a < 0 || b < 0 || t.n == TAVG_MAX_FIELDS) { c->err = "tavg: too many sources or entries at one site (" + e.name + ")"; return 1; }
      TavgDesc &d = t.d[t.n++];
      d.buf = e.buf; d.cst = e.cst; d.cst2 = e.cst2; d.kmax = (short)e.kmax; d.a = (unsigned char)a; d.b = (unsigned char)b;
      d.expr = (unsigned char)e.expr; d.method = (unsigned char)e.method;
      t.kmax = std::max(t.kmax, e.kmax);
      return 0;
    };
    for (int pass = 0; pass < 3; ++pass)   // cells; columns: the entries of 2-D sources, then the ones fed once per level
      for (const TavgEntry &e : T.req) {
        if (e.site != s || !T.on[e.stream]) continue;
        const int kind = e.cells ? 0 : (e.vint ? 2 : 1);
        if (kind != pass) continue;
        if (pass == 1 && !fits(S.cols, S.sid_cols, e)) {   // the second launch of the site
          if (put(S.cols_more, S.sid_cols_more, e)) return 1;
          S.cols_more.n2d = S.cols_more.n; S.cols_more.kmax = 0;
          continue;
        }
        if (pass == 0 ? put(S.cells, S.sid_cells, e) : put(S.cols, S.sid_cols, e)) return 1;
        if (pass == 1) { S.cols.n2d = S.cols.n; S.cols.kmax = 0; }
        if (e.expr == TX_RHO_VINT) S.vint_psurf = true;
      }
    if (S.cols.n - S.cols.n2d > TAVG_MAX_VINT) { c->err = "tavg: too many level-fed 2-D entries at one site"; return 1; }
  }
  T.dirty = false;
  return 0;
}

// tavg_set_flag (tavg.F90:1549-1557), called by pop_time_manager: the weight of this step, added to tavg_sum of every stream that is on
void tavg_set_flag(pop_ctx *c) {
  TavgState &T = c->tavg;
  T.dtavg = c->avg_ts ? 0.5 * c->h.dtt : c->h.dtt;
  for (int ns = 1; ns <= TAVG_MAX_STREAMS; ++ns) if (T.on[ns]) T.sum[ns] = T.sum[ns] + T.dtavg;
}

// one site, once, with the current dtavg, on the launch stream.  Callers inside a step test c->tavg.active first
int tavg_site(pop_ctx *c, int site) {
  TavgState &T = c->tavg;
  if (!T.active) return 0;
  if (T.dirty && tavg_build(c)) return 1;
  TavgSiteTab &S = T.site[site];
  if (S.cells.n) {
    TavgTable &t = S.cells;
    for (int i = 0; i < t.nsrc; ++i) { t.src[i] = tavg_src(c, S.sid_cells[i]); if (!t.src[i].p) { c->err = "tavg: a source of the site does not exist"; return 1; } }
    t.dtavg = T.dtavg;
    const int n2 = c->g.n2;
    if (n2 % 2 == 0) hipLaunchKernelGGL(k_tavg_cells<2>, dim3((n2 / 2 + 255) / 256, t.kmax, c->g.nblocks), dim3(256), 0, c->stream, n2, t);
    else hipLaunchKernelGGL(k_tavg_cells<1>, dim3((n2 + 255) / 256, t.kmax, c->g.nblocks), dim3(256), 0, c->stream, n2, t);
  }
  if (S.cols.n) {
    TavgTable &t = S.cols;
    for (int i = 0; i < t.nsrc; ++i) { t.src[i] = tavg_src(c, S.sid_cols[i]); if (!t.src[i].p) { c->err = "tavg: a source of the site does not exist"; return 1; } }
    t.dtavg = T.dtavg;
    if (site == TS_QFLUX) for (int e = 0; e < t.n; ++e) t.d[e].cst = c->ice.tlast_ice;   // const = tlast_ice (step_mod.F90:848-849)
    const TavgVint w{S.vint_psurf ? c->PS[c->curt] : nullptr, GRAV};
    with_flags([&](auto PBC) {
      hipLaunchKernelGGL(k_tavg_columns<PBC.value>, dim3((c->g.n2 + 255) / 256, c->g.nblocks), dim3(256), 0, c->stream, c->g, t, w);
    }, c->g.pbc != 0);
  }
  if (S.cols_more.n) {
    TavgTable &t = S.cols_more;
    for (int i = 0; i < t.nsrc; ++i) { t.src[i] = tavg_src(c, S.sid_cols_more[i]); if (!t.src[i].p) { c->err = "tavg: a source of the site does not exist"; return 1; } }
    t.dtavg = T.dtavg;
    const TavgVint w{nullptr, GRAV};
    with_flags([&](auto PBC) {
      hipLaunchKernelGGL(k_tavg_columns<PBC.value>, dim3((c->g.n2 + 255) / 256, c->g.nblocks), dim3(256), 0, c->stream, c->g, t, w);
    }, c->g.pbc != 0);
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}

double tavg_reset_value(int method) { return method == TAVG_MIN ? TAVG_BIGNUM : method == TAVG_MAX ? -TAVG_BIGNUM : 0.0; }
size_t tavg_count(const pop_ctx *c, const TavgEntry &e) { return (size_t)c->h.n2 * e.nlev * c->h.nblocks; }
int tavg_fill(pop_ctx *c, const TavgEntry &e) {
  if (!e.buf) return 0;
  const long long n = (long long)tavg_count(c, e);
  hipLaunchKernelGGL(k_tavg_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, e.buf, n, tavg_reset_value(e.method));
  HIPCHK(c, hipGetLastError());
  return 0;
}
// tavg_reset_field_stream (tavg.F90:3746-3840)
int tavg_reset_stream(pop_ctx *c, int ns) {
  TavgState &T = c->tavg;
  for (const TavgEntry &e : T.req) if (e.stream == ns && tavg_fill(c, e)) return 1;
  T.sum[ns] = 0.0;
  if (T.has_qflux[ns]) T.sum_qflux[ns] = 0.0;
  if (c->moc.requested && c->moc.stream == ns && moc_reset(c)) return 1;
  if (c->trn.requested && c->trn.stream == ns && trn_reset(c)) return 1;
  return 0;
}
void tavg_refresh_flags(pop_ctx *c) {
  TavgState &T = c->tavg;
  T.active = false;
  for (int ns = 1; ns <= TAVG_MAX_STREAMS; ++ns) { T.used[ns] = false; T.has_qflux[ns] = false; }
  for (const TavgEntry &e : T.req) { T.used[e.stream] = true; if (e.method == TAVG_QFLUX) T.has_qflux[e.stream] = true; if (T.on[e.stream]) T.active = true; }
  T.dirty = true;
  if (c->moc.requested) T.used[c->moc.stream] = true;   // the stream of pop_moc_request holds the MOC
  c->moc.active = c->moc.requested && T.on[c->moc.stream];
  if (c->trn.requested) T.used[c->trn.stream] = true;   // ... and the stream of pop_transport_request the tracer transports
  c->trn.active = c->trn.requested && T.on[c->trn.stream];
}
TavgEntry *tavg_find(pop_ctx *c, const char *name) {
  for (TavgEntry &e : c->tavg.req) if (e.name == name) return &e;
  return nullptr;
}
int tavg_stream_ok(pop_ctx *c, int ns, const char *who) {
  if (ns >= 1 && ns <= TAVG_MAX_STREAMS) return 0;
  c->err = std::string(who) + ": stream " + std::to_string(ns) + " is outside 1 .. " + std::to_string(TAVG_MAX_STREAMS);
  return 1;
}
int tavg_between_steps(pop_ctx *c, const char *who) {
  if (!c->tavg.in_step) return 0;
  c->err = std::string(who) + ": refused between pop_time_manager and pop_step_tail of a step (requests, on/off and resets happen between steps)";
  return 1;
}
// the normalisation factor of an entry (tavg_norm_field_all, tavg.F90:3888-3969): 1 for min / max / constant; an error, never an abort, when the sum is 0
int tavg_factor(pop_ctx *c, const TavgEntry &e, double *factor) {
  const TavgState &T = c->tavg;
  *factor = 1.0;
  if (e.method == TAVG_AVG) {
    if (T.sum[e.stream] == 0.0) { c->err = "tavg: cannot normalise " + e.name + ": tavg_sum of stream " + std::to_string(e.stream) + " is 0"; return 1; }
    *factor = 1.0 / T.sum[e.stream];
  } else if (e.method == TAVG_QFLUX) {
    if (T.sum_qflux[e.stream] == 0.0) { c->err = "tavg: cannot normalise " + e.name + ": tavg_sum_qflux of stream " + std::to_string(e.stream) + " is 0"; return 1; }
    *factor = 1.0 / T.sum_qflux[e.stream];
  }
  return 0;
}
// the buffer of an entry (normalised into a copy, or as it is) on the host
int tavg_to_host(pop_ctx *c, const TavgEntry &e, bool normalize, double *host) {
  const size_t n = tavg_count(c, e);
  double factor = 1.0;
  if (normalize && tavg_factor(c, e, &factor)) return 1;
  const double *src = e.buf;
  if (normalize && (e.method == TAVG_AVG || e.method == TAVG_QFLUX)) {
    if (!c->tavg.scratch && dev_alloc(c, &c->tavg.scratch, (size_t)c->h.n3 * c->h.nblocks, false)) return 1;
    hipLaunchKernelGGL(k_tavg_scale, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const double *)e.buf, c->tavg.scratch, (long long)n, factor);
    HIPCHK(c, hipGetLastError());
    src = c->tavg.scratch;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(host, src, n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace
