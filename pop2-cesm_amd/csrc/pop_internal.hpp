// pop_internal.hpp -- internal types of libpop_amd (MI355X-native POP2 dynamics core).
//
// Data layout on the device (DESIGN.md "Layout"): every field is stored per rank as
// (i, j, k, local_block) with i fastest -- the reference's own block layout
// (source/prognostic.F90:47-66) -- so one wavefront reads 64 consecutive i of one level
// (512 B, fully coalesced) and a thread owns a water column and marches k in registers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>
#include "../../include/pop_amd.h"

namespace pop {

constexpr int NGHOST = 2;          // blocks.F90:51-56
constexpr double GRAV = 980.6;     // pop_constants.F90:235 (non-CCSMCOUPLED)
constexpr double OMEGA = 7.292123625e-5;
constexpr double RADIUS = 6370.0e5;
constexpr int MAXNT = 8;

struct BlockInfo {                 // blocks.F90:30-39 type(block)
  int block_id, local_id, ib, ie, jb, je, iblock, jblock;
  std::vector<int> i_glob, j_glob;
};

// ---- halo plan (mpi/POP_HaloMod.F90:142-1640 POP_HaloCreate, restated as flat index lists)
struct PeerPlan {
  int rank;
  std::vector<int> send_src;   // local 2-D cell index (block*n2 + j*nxb + i) to pack, in message order
  std::vector<int> recv_dst;   // local 2-D cell index to unpack into, in message order
};
// Tripole northern boundary (mpi/POP_HaloMod.F90:1936-2050), per field location: every cell of rows je..je+nghost
// of the northern blocks is a function of one or two physical cells of the global top rows.
//   b < 0 : dst = isign * F[a]                                   (mirrored copy; isign = -1 for vector / angle kinds)
//   b >= 0: dst = sign(0.5*(|F[a]| + |F[b]|), F[a])              (symmetrised degenerate top row, NE-corner / N-face fields)
// a, b are cells of this rank (single-rank decompositions only).
struct TripolePlan { std::vector<int> dst, a, b; };
struct HaloPlan {
  std::vector<int> copy_dst, copy_src;  // ghost <- interior copies between blocks of this rank
  std::vector<int> fill_dst;            // ghosts outside closed boundaries / padding: fill value
  std::vector<PeerPlan> peers;
  long long max_msg_cells = 0;          // sum over peers of max(send, recv) cells
  TripolePlan tripole[5];               // by location: 0 centre, 1 NE corner, 2 N face, 3 E face (ns_boundary = 2); cells numbered over the rank's blocks.
                                        // [4]: N face, ghost rows only (no symmetrised top row): fields the reference forms locally in the ghost rows
  TripolePlan tripole_g[5];             // the same with cells numbered over ALL blocks (host set-up arrays)
  bool tripole_split = false;           // the top row of blocks has more than one owner: no plan
};

// ---- EVP block preconditioner (preconditioner_choice = 1; POP_SolversMod.F90:252-290, 2434-2696): sub-blocks of at most
//      EVP_BS x EVP_BS cells with a one-cell rim, for every block of the decomposition
constexpr int EVP_BS = 8, EVP_LD = EVP_BS + 2, EVP_LE = 2 * EVP_BS - 1;
struct EvpHost {
  int xnb = 0, ynb = 0;                     // sub-blocks per block in x, y
  std::vector<int> xidx, yidx;              // 1-based start indices xidx[1..xnb+1] (EvpBlockPartition)
  // sub-block s = (block*ynb + j-1)*xnb + i-1; (a,c) of the sub-block with rim at (a-1) + EVP_LD*(c-1)
  std::vector<double> cc, ne, icc, ine;     // centre / NE weight and their inverses
  std::vector<double> rinv;                 // inverse influence matrix, (k,j) at (k-1) + EVP_LE*(j-1)
  std::vector<int> land;                    // 1: diagonal scaling instead of the EVP solve
};

// ---- host-side model: everything init-time (restates grid.F90, hmix_del*.F90 init,
//      POP_SolversInit, init_barotropic, init_ts) on the local blocks of this rank
// short-wave absorption tables on the device (sw_absorption.F90): sw_absorb(0:km) of 'top-layer' / 'jerlov' (:355-370); for
// 'chlorophyll' the transmission table Tr over the levels ztr and 401 chlorophyll amounts (:525-728) and the table column of
// every cell (set_chl :500-512).  Shared by KPP (lshort_wave) and the temperature source add_sw_absorb.
struct SwTab {
  double *swabs = nullptr, *Tr = nullptr, *ztr = nullptr;
  int *CHLI = nullptr;
  int ksol = 0;
  double chlmin = 0, chlmax = 0, dlogchl = 0;
};
// tuning switches (include/pop_amd.h pop_tuning): resolved once at pop_create -- size rule < caller's struct < POP_* environment
inline bool tun_set(int v) { return v != POP_TUNING_UNSET; }
inline bool tun_on(int v) { return v != POP_TUNING_UNSET && v != 0; }
inline bool tun_off(int v) { return v == 0; }
inline int tun_or(int v, int dflt) { return v != POP_TUNING_UNSET ? v : dflt; }
struct HostModel {
  SwTab sw;
  pop_config c{};
  pop_tuning tun{};
  const pop_grid_input *gin = nullptr;     // caller's grid (pop_create_with_grid); read during host_build only
  int rank = 0, nranks = 1;
  bool plan_only = false;                  // POP_CREATE_PLAN_ONLY: blocks, distribution and halo plan, no fields
  long long ocean_cols_local = -1, ocean_cols_total = -1;   // ocean columns of the physical domain (global KMT rule / record), make_blocks
  int nxb = 0, nyb = 0, km = 0, nt = 2;
  bool iage[MAXNT] = {};                   // tracer n (0-based) is ideal age (pop_init_iage): interior source, surface reset, restart name
  bool ice = false;                        // pop_init_ice was called: restart files carry AQICE, the real FW_FREEZE and tlast_ice
  int nbx = 0, nby = 0, nblocks_tot = 0, nblocks = 0;   // nblocks = local
  size_t n2 = 0, n3 = 0;
  std::vector<BlockInfo> all_blocks;      // every block of the decomposition (1-based id = index+1)
  std::vector<int> local_ids;             // global ids (1-based) of this rank's blocks
  std::vector<int> block_owner;           // rank owning block id-1
  std::vector<int> block_local;           // local index of block id-1 on its owner
  // vertical grid, 1-based with slot 0 (dzw(0), dzwr(0))
  std::vector<double> dz, dzw, zt, zw, c2dz, dzr, dz2r, dzwr, pressz, bouss, dt, afac_t, afac_u;
  std::vector<double> upw_z[6];           // upwind3 vertical weights talfzp,tbetzp,tgamzp,talfzm,tbetzm,tdelzm (1..km)
  // named 2-D / 3-D fields on local blocks
  std::map<std::string, std::vector<double>> f2;   // (nxb,nyb,nblocks)
  std::map<std::string, std::vector<int>> i2;
  std::map<std::string, std::vector<double>> f3;   // (nxb,nyb,km,nblocks), initial state only
  std::vector<double> aniso_f[2];                  // hmix_momentum = 3 with lvariable_hmix_aniso: F_PARA, F_PERP of ALL blocks (nxb,nyb,km,nblocks_tot)
  std::vector<double> angle;                       // the caller's ANGLE on ALL blocks, kept for ANGLET (host_forcing.cpp); empty: zeros
  double uarea_equator = 0, residualNorm = 0, convergenceCriterion = 0, rcheck = 0, rconst = 0;
  double dtt = 0, dtu = 0, dtp = 0;
  int nsteps_per_interval = 0;
  // Robert filter (tmix_opt = 3): time_management.F90:897-945, step_mod.F90:1577-1615
  double robert_curtime = 0, robert_newtime = 0, bgtarea_t_1 = 0, rf_volume_2_km = 0, open_ocean_volume_2_km = 0;
  int rf_nonzero_newtime = 0;
  // areas and volumes of the global diagnostics (grid.F90:1059-1072); the _k arrays are 1-based with slot 0
  double area_t = 0, volume_t = 0, volume_u = 0;
  std::vector<double> area_t_k, volume_t_k;
  // P-CSI (solver_choice = 3): Lanczos eigenvalue bounds from host_pcsi_prep (POP_SolversMod.F90:181-320)
  double pcsi_max_eig = 0, pcsi_min_eig = 0;
  int pcsi_lanczos_steps = 0;
  EvpHost evp;
  HaloPlan halo;
  std::string err;

  std::vector<double> &F(const std::string &n) { return f2[n]; }
  std::vector<int> &I(const std::string &n) { return i2[n]; }
};

int host_build(HostModel &h);            // host_setup.cpp
// the caller's pop_config read in the layout of its struct_version into `out`, and every refusal rule of pop_create (host_setup.cpp)
int config_read_check(const pop_config *in, const pop_grid_input *grid, pop_config &out, std::string &err);
// the local blocks of an all-blocks host field: 2-D, and 3-D (nxb, nyb, km, nblocks_tot)
template <class T>
std::vector<T> local_part(const HostModel &h, const std::vector<T> &all) {
  std::vector<T> out(h.n2 * h.nblocks);
  for (int lb = 0; lb < h.nblocks; ++lb)
    std::copy(all.begin() + (size_t)(h.local_ids[lb] - 1) * h.n2, all.begin() + (size_t)h.local_ids[lb] * h.n2, out.begin() + (size_t)lb * h.n2);
  return out;
}
inline std::vector<double> local_part3(const HostModel &h, const std::vector<double> &all) {
  std::vector<double> out(h.n3 * h.nblocks);
  for (int lb = 0; lb < h.nblocks; ++lb)
    std::copy(all.begin() + (size_t)(h.local_ids[lb] - 1) * h.n3, all.begin() + (size_t)h.local_ids[lb] * h.n3, out.begin() + (size_t)lb * h.n3);
  return out;
}
// ---- the lists and rewritten tables context creation uploads, as pure functions of the host model (host_tables.cpp).  The
// solver's summation order and the XCD placement follow the order of these lists
std::vector<int> land_prefix(const HostModel &h, double &land_fraction);   // DevGrid::opre, (n2 + 1) per local block; the share of 64-cell row tiles without work
struct ChunkLists { std::vector<int> list, cnt; int nact = 0, active_total = 0; };   // nact = 0: no list, every chunk is visited
ChunkLists solver_chunk_lists(const HostModel &h, const std::vector<int> &pre);      // red_act / red_cnt of the fused solver kernels
struct PeerLists { std::vector<int> ss, st, sc, rd, rt, rc; };     // all peers concatenated: cell, start and length of its message (send, receive)
PeerLists peer_lists(const HaloPlan &p);
struct PeerCellMaps { std::vector<int> smap, off, slot, rmap; };   // per cell: its send entries (smap -> off -> slot) and its receive slot
PeerCellMaps peer_cell_maps(const PeerLists &L, size_t ncells);
bool halo_ns_only(const HostModel &h);                             // every block's east neighbour is on the block's own rank (j-band shards)
struct EvpTables {                                                 // local sub-blocks, coefficient arrays transposed to [cell][sub-block]
  size_t S = 0;
  std::vector<int> meta;                                           // four words per sub-block: first cell, nx | ny << 8, land, land without interior ocean
  std::vector<double> cc, ne, icc, ine, rinv;
};
EvpTables evp_tables(const HostModel &h);
std::vector<double> btrop_wgt_ring(const HostModel &h, int wgt);   // btropWgtNE (1) / East (2) / North (3) of all blocks with the first row and column filled
int mask_bytes(const std::vector<double> &m, std::vector<unsigned char> &m8);   // a 0/1 field as bytes; 1 when a value is neither
std::vector<double> pcsi_omega(const HostModel &h, double &csy);   // omega_k of P-CSI, k = 0 .. max_iterations
// ---- Jayne tidal mixing, init-time fields on the local blocks (host_tidal.cpp; tidal_mixing.F90)
struct TidalFields {
  std::vector<double> flux, coef;          // TIDAL_ENERGY_FLUX_2D [g/s^3], TIDAL_COEF_3D (nxb,nyb,km,nblocks)
  std::vector<int> box;                    // REGION_BOX2D: 1-based region of ltidal_min_regions, 0 = none
};
void tidal_nml_defaults(pop_tidal_nml &n);
int tidal_nml_resolve(pop_tidal_nml &n, std::string &err);
void host_tlon_build(const HostModel &h, std::vector<double> &tlon);   // TLON [radians] of the local blocks (calc_tpoints + halo update)
void host_tidal_build(const HostModel &h, const pop_tidal_nml &n, const double *flux, const std::vector<double> &tlon, TidalFields &out);
// ---- latitude-varying KPP background diffusivity on the local blocks (host_bckgrnd.cpp; vmix_kpp.F90:544-611)
struct BckgrndFields { std::vector<double> vdc, vvc, vvc_pr; };   // bckgrnd_vdc, Prandtl * bckgrnd_vdc, (Prandtl * bckgrnd_vdc) / Prandtl: 2-D
void kpp_bckgrnd_nml_defaults(pop_kpp_bckgrnd_nml &n);
void host_bckgrnd_build(const HostModel &h, const pop_kpp_bckgrnd_nml &n, const std::vector<double> &tlon, BckgrndFields &out);
// ---- frazil ice formation (host_ice.cpp; ice.F90:98-317)
struct IceConsts { double cp_over_lhfusion, salice, salref, hflux_factor; };
void ice_nml_defaults(pop_ice_nml &n);
int ice_nml_check(const HostModel &h, const pop_ice_nml &n, std::string &err);
IceConsts ice_consts(const pop_ice_nml &n);
// ---- coupled surface forcing, host logic (host_forcing.cpp; grid.F90:660-735, forcing_coupled.F90:128-470)
struct CplConsts { double lhv, lhf, hflux_factor, salinity_factor, sflux_factor, fwmass_to_fwflux, momentum_factor; };
void coupled_nml_defaults(pop_coupled_nml &n);
// what pop_init_coupled_forcing refuses from the namelist and the configuration; resolves nsteps_per_interval = 0
int coupled_nml_resolve(const HostModel &h, pop_coupled_nml &n, std::string &err);
CplConsts coupled_consts(const pop_coupled_nml &n, double hflux_factor, double ocn_ref_salinity);
// ANGLET, cos(ANGLET), sin(ANGLET) on the local blocks
void host_anglet_build(const HostModel &h, std::vector<double> &anglet, std::vector<double> &cosa, std::vector<double> &sina);
// qsw_12hr_factor(1 : nspi) (forcing_coupled.F90:358-408); non-zero with the error set when the final integral is off
int host_qsw_12hr_factor(const HostModel &h, int qsw_distrb_opt, int nspi, std::vector<double> &factor, std::string &err);
// ---- marginal-sea balance, init_ms_balance (host_forcing.cpp; ms_balance.F90:61-453)
struct MsSea { int number = 0, warn = 0; std::string name; double area = 0.0; std::vector<int> ipts, jpts; std::vector<double> fracs; };
struct MsBalance {
  bool inited = false;
  std::vector<MsSea> seas;                          // in region order (mask_index - 1)
  std::vector<int> region_mask;                     // (ny_global, nx_global)
  std::vector<double> mask_frac, ind;               // per sea MASK_FRAC and the indicator REGION_MASK == number, local blocks: (n2, nblocks, nseas)
};
void host_tlon_all(const HostModel &h, std::vector<double> &TLON);   // TLON [radians] of ALL blocks (host_tidal.cpp)
int host_ms_balance_build(const HostModel &h, const pop_ms_balance_nml &nml, const int *region_mask_global, MsBalance &out, std::string &err);
// ---- auxiliary latitude grid and transport regions of the MOC (host_lat_aux.cpp; diags_on_lat_aux_grid.F90:121-936)
// A cell list holds the physical ocean cells of one block that lie in one bin and in some region, in (j, i) order, as
// p2 | flag << MOC_FLAG_SHIFT (p2 = j * nxb + i inside the block; flag bit 0: region 1, bit 1: region 2).  Lists are numbered over
// ALL blocks in (block id, bin) order, so every rank knows where another rank's sums belong.
constexpr int MOC_FLAG_SHIFT = 29;
struct MocList { int block, bin, off, cnt; };      // block: 0-based global id; bin: 0-based (the reference's n - 2)
struct LatAux {
  bool inited = false;
  pop_transports_nml nml{};
  int n_lat = 0, n_reg = 1, n_comp = 1, j_southern = 0;
  std::vector<double> edge, center;                // lat_aux_edge (n_lat + 1), lat_aux_center (n_lat)
  std::vector<int> region_start;                   // lat_aux_region_start(m), slot m - 1
  std::vector<int> mask;                           // MASK_LAT_DEPTH as [n][k][m], 1 = .true.
  std::vector<int> bin_map;                        // (ny_global, nx_global): 1-based bin, 0 = none
  std::vector<MocList> lists; std::vector<int> cells;       // the bins
  std::vector<MocList> blists; std::vector<int> bcells;     // row lat_aux_region_start(2) (bin unused): plain p2
};
void transports_nml_defaults(pop_transports_nml &n);
int host_lat_aux_build(const HostModel &h, const pop_transports_nml &nml, const int *region_mask_global, LatAux &out, std::string &err);
// ---- POP binary restart files (host_restart.cpp; restart.F90, io_binary.F90)
// one field of a restart or tavg file: records id .. id + nlev - 1, held on the host as (nxb, nyb, nlev, nblocks)
struct RestartField {
  std::string name; int ndims = 2, nlev = 1, id = 0;   // file name; nfield_dims; levels (km or 1 in a restart, 1 .. km in a tavg file); first record
  // restart files only
  std::string dev; int tl = 1, n = 0, mask = 0;        // device field (empty: none, zeros are written), time level (0 old, 1 cur), tracer;
                                                       // mask: 1 CALCU, 2 CALCT, 3 k > KMU, 4 k > KMT (read_restart :881-935)
  std::string long_name, units, grid_loc;
};
struct RestartAttr { std::string name, type, value; };
std::string fmt_r8(double v);                          // value of an r8 attribute
// a parsed <file>.hdr: typed reads of &GLOBAL and the record of a field
struct RestartHeader {
  std::map<std::string, std::map<std::string, std::string>> sec;   // section -> (attribute -> value)
  std::vector<std::string> order;                                  // section names as they stand in the file
  const std::string *attr(const std::string &a) const;             // of &GLOBAL; null when absent
  bool has(const std::string &a) const { return attr(a) != nullptr; }
  std::string text(const std::string &a) const { return has(a) ? *attr(a) : std::string(); }
  int integer(const std::string &a, int dflt) const { return has(a) ? atoi(attr(a)->c_str()) : dflt; }
  double real(const std::string &a) const { return strtod(text(a).c_str(), nullptr); }
  bool logical(const std::string &a) const;                        // list-directed; false when absent
  enum Rule { PREFIX, EXACT };
  bool find(const std::string &name, Rule rule, int *id, int *ndims) const;
};
typedef std::function<int(size_t, double *)> SlabFieldFn;          // (index into the field list, host buffer) -> 0, or non-zero with the error set
std::string restart_tracer_name(const HostModel &h, int n);
std::vector<RestartField> restart_fields(const HostModel &h);
int restart_parse_header(const std::string &path, RestartHeader &hd, std::string &err);
int slab_file_write(const HostModel &h, const std::string &path, const std::vector<RestartAttr> &attrs, const std::vector<RestartField> &fields, const SlabFieldFn &fetch, const std::string &tag, std::string &err);
int slab_file_read(const HostModel &h, const std::string &path, const std::vector<RestartField> &wanted, bool swap, const SlabFieldFn &store, std::string &err);
void restart_mask(const HostModel &h, const RestartField &f, double *loc, const std::vector<int> &KMT, const std::vector<int> &KMU);
std::vector<double> host_center_init(HostModel &h);                      // centre weight POP_SolversPrep sees (host_pcsi.cpp)
int host_pcsi_prep(HostModel &h, const std::vector<double> &C);         // host_pcsi.cpp
int host_evp_prep(HostModel &h, const std::vector<double> &C);          // host_evp.cpp
void host_evp_apply(const HostModel &h, double *PX, const double *X);   // all blocks
inline bool use_evp(const pop_config &c) { return c.preconditioner_choice == 1; }
void build_halo_plan(HostModel &h);      // halo_plan.cpp
void host_halo_r8(const HostModel &h, double *a, int nz, double fill);   // single-rank host halo
void host_halo_i4(const HostModel &h, int *a, int nz, int fill);
// with field location / kind: the ordinary update, then the tripole pass when ns_boundary = 2
void host_halo_r8_loc(const HostModel &h, double *a, int nz, double fill, int loc, int kind);
void host_halo_i4_loc(const HostModel &h, int *a, int nz, int fill, int loc, int kind);
double host_global_sum(const HostModel &h, const double *a, const double *mask);
double host_global_sum_loc(const HostModel &h, const double *a, const double *mask, int loc);
std::vector<int> global_srcmap(const HostModel &h);   // all blocks: ghost -> source cell, -1 = fill

}  // namespace pop
