// host_restart.cpp -- POP binary restart files (host logic, no HIP): the data format either side of the time step.
//
// Restates the 'bin' path of restart.F90 (write_restart :1095-1715, read_restart :184-1088) and io_binary.F90:
//   <file>       direct-access data, one record = one horizontal slab nx_global x ny_global of r8 in native byte
//                order, no record markers (open_binary :396-399, recl_words = nx_global*ny_global, restart.F90:1262);
//                a 3-D field is km consecutive records (write_real8_3d :2590-2640)
//   <file>.hdr   text: "&GLOBAL" + "name:type:value" lines + "/" (open_binary :414-560), then per field
//                "&SHORT_NAME", long_name / units / grid_loc, "id:int:<first record>", "nfield_dims:int:<2|3>", "/"
//                (define_field_binary :760-880); the separator is ':' (io_binary.F90:59)
// Every rank writes / reads the rows of its own blocks at their place in the global slab (pwrite / pread on the
// shared file), so no gather is needed; rank 0 writes the header.
// The tavg files (tavg.F90 write_tavg / read_tavg, 'bin') have the same layout; slab_file_write and slab_file_read below move
// either kind, and the entry points of pop_amd.hip supply only what a field is on the device.
#include <fcntl.h>
#include <unistd.h>
#include <algorithm>
#include <fstream>
#include <utility>
#include "pop_internal.hpp"

namespace pop {

// fields of the restart file in the order write_restart defines them (restart.F90:1555-1600); varthick surface layer
// tracer_d(n)%short_name of tracer n (0-based): TEMP, SALT; IAGE for an ideal-age tracer (iage_mod.F90:162; IAGE_<n> from the second
// one on, n 1-based), TRACER<nn> for a tracer without a module
std::string restart_tracer_name(const HostModel &h, int n) {
  if (n < 2) return n == 0 ? "TEMP" : "SALT";
  char b[32];
  if (!h.iage[n]) { snprintf(b, sizeof b, "TRACER%02d", n + 1); return b; }
  for (int m = 2; m < n; ++m) if (h.iage[m]) { snprintf(b, sizeof b, "IAGE_%d", n + 1); return b; }
  return "IAGE";
}
std::vector<RestartField> restart_fields(const HostModel &h) {
  std::vector<RestartField> f;
  int rec = 1;
  auto add = [&](const char *name, const char *dev, int tl, int n, int ndims, const char *ln, const char *units, const char *loc, int mask) {
    f.push_back(RestartField{name, ndims, ndims == 3 ? h.km : 1, rec, dev, tl, n, mask, ln, units, loc});
    rec += f.back().nlev;
  };
  add("UBTROP_CUR", "UBTROP", 1, 0, 2, "U barotropic velocity at current time", "cm/s", "2220", 1);
  add("UBTROP_OLD", "UBTROP", 0, 0, 2, "U barotropic velocity at old time", "cm/s", "2220", 1);
  add("VBTROP_CUR", "VBTROP", 1, 0, 2, "V barotropic velocity at current time", "cm/s", "2220", 1);
  add("VBTROP_OLD", "VBTROP", 0, 0, 2, "V barotropic velocity at old time", "cm/s", "2220", 1);
  add("PSURF_CUR", "PSURF", 1, 0, 2, "surface pressure at current time", "dyne/cm2", "2110", 2);
  add("PSURF_OLD", "PSURF", 0, 0, 2, "surface pressure at old time", "dyne/cm2", "2110", 2);
  add("GRADPX_CUR", "GRADPX", 1, 0, 2, "sfc press gradient in x at current time", "dyne/cm3", "2220", 1);
  add("GRADPX_OLD", "GRADPX", 0, 0, 2, "sfc press gradient in x at old time", "dyne/cm3", "2220", 1);
  add("GRADPY_CUR", "GRADPY", 1, 0, 2, "sfc press gradient in y at current time", "dyne/cm3", "2220", 1);
  add("GRADPY_OLD", "GRADPY", 0, 0, 2, "sfc press gradient in y at old time", "dyne/cm3", "2220", 1);
  add("PGUESS", "PGUESS", 1, 0, 2, "guess for sfc pressure at new time", "dyne/cm2", "2110", 2);
  add("FW_OLD", "FW_OLD", 1, 0, 2, "fresh water input at old time", "", "2110", 2);
  // without pop_init_ice there is no ice formation: zeros; with it the field, and the AQICE record after it (restart.F90:1567-1577, the
  // branch that is not a coupled time step)
  add("FW_FREEZE", h.ice ? "FW_FREEZE" : "", 1, 0, 2, "water flux due to frazil ice formation", "", "2110", 2);
  if (h.ice) add("AQICE", "AQICE", 1, 0, 2, "accumulated ice melt/heat", "", "2110", 2);
  add("UVEL_CUR", "UVEL", 1, 0, 3, "U velocity at current time", "cm/s", "3221", 3);
  add("UVEL_OLD", "UVEL", 0, 0, 3, "U velocity at old time", "cm/s", "3221", 3);
  add("VVEL_CUR", "VVEL", 1, 0, 3, "V velocity at current time", "cm/s", "3221", 3);
  add("VVEL_OLD", "VVEL", 0, 0, 3, "V velocity at old time", "cm/s", "3221", 3);
  add("TEMP_CUR", "TRACER", 1, 0, 3, "Potential temperature at current time", "degC", "3111", 4);
  add("SALT_CUR", "TRACER", 1, 1, 3, "Salinity at current time", "msu (g/g)", "3111", 4);
  add("TEMP_OLD", "TRACER", 0, 0, 3, "Potential temperature at old time", "degC", "3111", 4);
  add("SALT_OLD", "TRACER", 0, 1, 3, "Salinity at old time", "msu (g/g)", "3111", 4);
  // passive tracers: <tracer_d(n)%short_name>_CUR for every n, then _OLD (restart.F90:1516-1548), after the records of an nt = 2 file
  for (int tl = 1; tl >= 0; --tl)
    for (int n = 2; n < h.nt; ++n) {
      const std::string sn = restart_tracer_name(h, n);
      add((sn + (tl ? "_CUR" : "_OLD")).c_str(), "TRACER", tl, n, 3, (sn + (tl ? " at current time" : " at old time")).c_str(), h.iage[n] ? "years" : "", "3111", 4);
    }
  return f;
}

static std::string list_directed(const std::string &v) { return " " + v; }   // write(line(n:),*) leaves a leading blank
std::string fmt_r8(double v) { char b[40]; snprintf(b, sizeof b, "%.17g", v); return b; }

static int restart_write_header(const std::string &path, const std::vector<RestartAttr> &attrs, const std::vector<RestartField> &fields, std::string &err) {
  std::ofstream o(path + ".hdr");
  if (!o) { err = "cannot open " + path + ".hdr for writing"; return 1; }
  o << "&GLOBAL\n";
  for (const RestartAttr &a : attrs) o << a.name << ':' << a.type << ':' << list_directed(a.value) << '\n';
  o << "/\n";
  for (const RestartField &f : fields) {
    o << '&' << f.name << '\n';
    if (!f.long_name.empty()) o << "long_name:char:" << f.long_name << '\n';
    if (!f.units.empty()) o << "units:char:" << f.units << '\n';
    if (!f.grid_loc.empty()) o << "grid_loc:char:" << f.grid_loc << '\n';
    o << "id:int:" << list_directed(std::to_string(f.id)) << '\n';
    o << "nfield_dims:int:" << list_directed(std::to_string(f.ndims)) << '\n';
    o << "/\n";
  }
  return o.good() ? 0 : 1;
}

// sections of a header file: name -> (attribute -> value), values trimmed; the type tag is dropped.  `order` lists the section
// names as they stand in the file.  As the reference reads it: each line is its first 80 columns ('(a80)', io_binary.F90:229, 985),
// and of two sections with one name the first counts (define_field_binary searches from the top, :978-989)
int restart_parse_header(const std::string &path, RestartHeader &hd, std::string &err) {
  std::ifstream in(path + ".hdr");
  if (!in) { err = "cannot open " + path + ".hdr"; return 1; }
  auto trim = [](std::string s) {
    const size_t a = s.find_first_not_of(" \t\r"), b = s.find_last_not_of(" \t\r");
    return a == std::string::npos ? std::string() : s.substr(a, b - a + 1);
  };
  std::string line, cur;
  while (std::getline(in, line)) {
    if (line.size() > 80) line.resize(80);
    line = trim(line);
    if (line.empty()) continue;
    if (line[0] == '&') {
      cur = trim(line.substr(1));
      if (hd.sec.count(cur)) cur.clear(); else { hd.sec[cur]; hd.order.push_back(cur); }
      continue;
    }
    if (line[0] == '/') { cur.clear(); continue; }
    if (cur.empty()) continue;
    const size_t p1 = line.find(':');
    if (p1 == std::string::npos) continue;
    const size_t p2 = line.find(':', p1 + 1);
    if (p2 == std::string::npos) continue;
    hd.sec[cur][trim(line.substr(0, p1))] = trim(line.substr(p2 + 1));
  }
  return 0;
}

const std::string *RestartHeader::attr(const std::string &a) const {
  const auto g = sec.find("GLOBAL");
  return g == sec.end() || !g->second.count(a) ? nullptr : &g->second.at(a);
}
bool RestartHeader::logical(const std::string &a) const {   // list-directed logical: T, F, .TRUE., .false., ...
  const std::string v = text(a);
  const size_t k = v.find_first_not_of(" .");
  return k != std::string::npos && (v[k] == 'T' || v[k] == 't');
}
// First record and nfield_dims (0: the section does not say) of a field; false: no section of that name, or one without "id".
//   PREFIX  pop_read_restart.  define_field_binary :979-989 takes the first line of the file that BEGINS with "&<short_name>", so a
//           section whose name merely starts with the one wanted is taken if it comes first; the reference's files are read as it reads them.
//   EXACT   pop_tavg_read.  TEMP and TEMP_2 are both tavg names and a stream lists them in request order: TEMP_2 must not answer for
//           TEMP.  Only this library writes these files, so there is no foreign reader to follow.
bool RestartHeader::find(const std::string &name, Rule rule, int *id, int *ndims) const {
  for (const std::string &s : order) {
    if (rule == EXACT ? s != name : s.compare(0, name.size(), name) != 0) continue;
    const std::map<std::string, std::string> &a = sec.at(s);
    if (!a.count("id")) return false;
    *id = atoi(a.at("id").c_str());
    *ndims = a.count("nfield_dims") ? atoi(a.at("nfield_dims").c_str()) : 0;
    return true;
  }
  return false;
}

static inline double bswap(double v) {
  unsigned char b[8];
  std::memcpy(b, &v, 8);
  for (int i = 0; i < 4; ++i) std::swap(b[i], b[7 - i]);
  std::memcpy(&v, b, 8);
  return v;
}

// one slab (record `rec`, 1-based) <-> the physical cells of the local blocks; `loc` points at the level of local
// block 0 and blocks are `blk_stride` doubles apart.  The texts say "restart" for a tavg file too: they are what callers match.
static int restart_slab_io(const HostModel &h, int fd, long long rec, double *loc, size_t blk_stride, bool write, bool swap, std::string &err) {
  const long long nx = h.c.nx_global, ny = h.c.ny_global, base = (rec - 1) * nx * ny;
  for (int lb = 0; lb < h.nblocks; ++lb) {
    const BlockInfo &B = h.all_blocks[h.local_ids[lb] - 1];
    for (int j = B.jb; j <= B.je; ++j) {
      const int jg = B.j_glob[j - 1];
      if (jg < 1 || jg > ny) continue;
      int i = B.ib;
      while (i <= B.ie) {                      // runs of consecutive global i (a block never wraps inside its physical part)
        const int ig = B.i_glob[i - 1];
        if (ig < 1 || ig > nx) { ++i; continue; }
        int n = 1;
        while (i + n <= B.ie && B.i_glob[i + n - 1] == ig + n) ++n;
        double *p = loc + (size_t)lb * blk_stride + (size_t)(j - 1) * h.nxb + (i - 1);
        const off_t off = (off_t)((base + (long long)(jg - 1) * nx + (ig - 1)) * 8);
        if (write) {
          if (pwrite(fd, p, (size_t)n * 8, off) != (ssize_t)n * 8) { err = "restart: short write"; return 1; }
        } else {
          if (pread(fd, p, (size_t)n * 8, off) != (ssize_t)n * 8) { err = "restart: short read (file smaller than the header says)"; return 1; }
          if (swap) for (int t = 0; t < n; ++t) p[t] = bswap(p[t]);
        }
        i += n;
      }
    }
  }
  return 0;
}

struct Fd { int fd; ~Fd() { if (fd >= 0) ::close(fd); } };   // closed on every return path
// The walk over an open file, either way: for every field zeros in buf, then fn and the records (write) or the records and fn (read).
// buf is (nxb, nyb, nlev, nblocks): blocks are nlev * n2 apart, which for a 3-D restart field (nlev = km) is n3 (host_setup.cpp:
// n3 = n2 * km); no field has more than km levels, so one 3-D field bounds it.  The first failure ends the walk.
static int slab_walk(const HostModel &h, int fd, const std::vector<RestartField> &fields, bool write, bool swap, const SlabFieldFn &fn, std::string &err) {
  std::vector<double> buf((size_t)h.n3 * h.nblocks);
  for (size_t i = 0; i < fields.size(); ++i) {
    const RestartField &f = fields[i];
    std::fill(buf.begin(), buf.begin() + (size_t)f.nlev * h.n2 * h.nblocks, 0.0);
    if (write && fn(i, buf.data())) return 1;
    for (int k = 0; k < f.nlev; ++k)
      if (restart_slab_io(h, fd, f.id + k, buf.data() + (size_t)k * h.n2, (size_t)f.nlev * h.n2, write, swap, err)) return 1;
    if (!write && fn(i, buf.data())) return 1;
  }
  return 0;
}

// Header by rank 0, then every rank puts its part of each field into the one file: fetch(i, buf) fills buf with field i (or leaves the
// zeros it is given), records id .. id + nlev - 1 are written.  The file is never truncated: the other ranks write into it too.
int slab_file_write(const HostModel &h, const std::string &path, const std::vector<RestartAttr> &attrs, const std::vector<RestartField> &fields, const SlabFieldFn &fetch, const std::string &tag, std::string &err) {
  if (h.rank == 0 && restart_write_header(path, attrs, fields, err)) return 1;
  Fd f{open(path.c_str(), O_WRONLY | O_CREAT, 0644)};
  if (f.fd < 0) { err = "cannot open " + path + " for writing"; return 1; }
  if (slab_walk(h, f.fd, fields, true, false, fetch, err)) return 1;
  if (::close(std::exchange(f.fd, -1)) != 0) { err = tag + ": close failed"; return 1; }   // the one close that is checked; f is left with nothing to do
  return 0;
}
// Every field of `wanted` (id: its first record, from the header): its records, then store(i, buf).  What was stored before a failure
// stays stored -- the reference's reader has no rollback either.
int slab_file_read(const HostModel &h, const std::string &path, const std::vector<RestartField> &wanted, bool swap, const SlabFieldFn &store, std::string &err) {
  Fd f{open(path.c_str(), O_RDONLY)};
  if (f.fd < 0) { err = "cannot open " + path; return 1; }
  return slab_walk(h, f.fd, wanted, false, swap, store, err);
}

// read_restart :881-935: values outside the ocean are reset (CALCU / CALCT masks in 2-D, k > KMU / KMT in 3-D)
void restart_mask(const HostModel &h, const RestartField &f, double *loc, const std::vector<int> &KMT, const std::vector<int> &KMU) {
  const size_t n2 = h.n2;
  for (int lb = 0; lb < h.nblocks; ++lb)
    for (size_t p = 0; p < n2; ++p) {
      const size_t q = lb * n2 + p;
      if (f.mask == 1 && !(KMU[q] >= 1)) loc[q] = 0.0;
      if (f.mask == 2 && !(KMT[q] >= 1)) loc[q] = 0.0;
      if (f.mask == 3 || f.mask == 4) {
        const int kb = f.mask == 3 ? KMU[q] : KMT[q];
        for (int k = kb + 1; k <= h.km; ++k) loc[(size_t)lb * h.n3 + (size_t)(k - 1) * n2 + p] = 0.0;
      }
    }
}

}  // namespace pop
