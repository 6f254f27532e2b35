// Deck-driven periodic outputs of the host driver (include/artemis_driver.h: artemis_sim_enable_outputs /
// _outputs_describe): the scheduler of the deck's <parthenon/outputN> blocks and the writer of history files.  Plain C++
// like the rest of the driver; the state is reached through outputs_hooks.hpp, dumps go through artemis_sim_save, field
// dumps (`fld`: a directory of meta.json + one raw part per rank, artemis_sim_write_fields) are written here.
//
// Schedule (parthenon's Outputs::MakeOutputs, upstream): a block is due when time >= next_time; after it has been
// written next_time is the smallest m * dt, m an integer, above time -- by multiplication, so the times do not drift.  A
// fresh run starts with next_time = 0 (every block at cycle 0), a continued one with the first multiple above its clock.
// An output time is never passed to the time step.
#include <algorithm>
#include <cerrno>
#include <dirent.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>
#include <vector>

#include "artemis_driver.h"
#include "checkpoint_hooks.hpp"
#include "outputs_hooks.hpp"
#include "parameter_input.hpp"

namespace artemis_out {

namespace {
enum Kind { HST, RST, FLD, SKIPPED };

struct OutBlock {
  std::string name, file_type; // "parthenon/output0", "hst"
  int index = 0;               // the N of outputN
  Kind kind = SKIPPED;
  double dt = 0.0, next_time = 0.0;
  long written = 0, last_cycle = -1, last_final_cycle = -1;
  long counter = 0;          // rst: number of the next dump
  bool header_done = false;  // hst: this run has written its header section
  std::string path;          // hst: the file; rst, fld: the last dump
  // fld: the names of its `variables` list and their codes, single_precision_output; why the block is skipped, if it is
  std::vector<std::string> variables;
  std::vector<int> codes;
  bool single = false, is_fld = false;
  bool has_level = false; // fld: `level = L`, every block resampled to the zone size of refinement level L (may be negative)
  int level = 0;
  int reduce = 0; // fld: `reduce = x2,x3`, the mask of the directions every block is integrated over (0: none)
  bool has_reduce_level = false; // fld: `reduce_level = L` beside `reduce`: the kept directions brought to the zone size of level L
  int reduce_level = 0;
  std::string skip;
};

// smallest m * dt (m an integer) strictly above t
double next_multiple(double t, double dt, long *m_out = nullptr) {
  long m = static_cast<long>(std::floor(t / dt)) + 1;
  while (m > 1 && static_cast<double>(m - 1) * dt > t) --m;
  while (static_cast<double>(m) * dt <= t) ++m;
  if (m_out) *m_out = m;
  return static_cast<double>(m) * dt;
}

std::string json_str(const std::string &s) {
  std::string o = "\"";
  for (const char ch : s) {
    if (ch == '"' || ch == '\\') o += '\\', o += ch;
    else if (static_cast<unsigned char>(ch) < 0x20) {
      char b[8];
      std::snprintf(b, sizeof b, "\\u%04x", ch);
      o += b;
    } else o += ch;
  }
  return o + "\"";
}
std::string json_num(double v) {
  if (!std::isfinite(v)) return "null";
  char b[40];
  std::snprintf(b, sizeof b, "%.17g", v);
  return b;
}

void make_dirs(const std::string &dir) {
  for (size_t q = 1; q <= dir.size(); ++q)
    if (q == dir.size() || dir[q] == '/') {
      const std::string part = dir.substr(0, q);
      if (::mkdir(part.c_str(), 0777) != 0 && errno != EEXIST)
        throw std::runtime_error("outputs: cannot create directory " + part + ": " + std::strerror(errno));
    }
}
} // namespace

struct State {
  bool on = false;
  std::string dir, problem_id;
  std::vector<OutBlock> blocks;
};

namespace {

// A `fld` block: its comma list of variables against the table of outputs_hooks.hpp and the species of the run
void parse_fld(artemis_host::ParameterInput &pin, const Clock &c, OutBlock &b) {
  b.is_fld = true, b.kind = FLD;
  b.single = pin.GetOrAddBoolean(b.name, "single_precision_output", false);
  std::string list = pin.DoesParameterExist(b.name, "variables") ? pin.GetString(b.name, "variables") : "";
  for (size_t at = 0; at <= list.size();) {
    size_t end = list.find(',', at);
    if (end == std::string::npos) end = list.size();
    std::string name = list.substr(at, end - at);
    const size_t a = name.find_first_not_of(" \t"), z = name.find_last_not_of(" \t");
    if (a != std::string::npos) b.variables.push_back(name.substr(a, z - a + 1));
    at = end + 1;
  }
  if (b.variables.empty()) b.skip = "no variables";
  for (const std::string &name : b.variables) {
    const int code = field_var_code(name);
    if (code < 0 || field_var_components(code, c.ns_gas, c.ns_dust) == 0) {
      if (b.skip.empty()) b.skip = "unknown variable " + name;
    } else b.codes.push_back(code);
  }
  if (b.skip.empty() && pin.GetOrAddBoolean(b.name, "ghost_zones", false)) b.skip = "ghost_zones is not built";
  if (pin.DoesParameterExist(b.name, "level")) {
    b.has_level = true, b.level = pin.GetInteger(b.name, "level");
    // the worst shifts this deck can ever produce: its finest possible level and the root grid
    for (const int lv : {c.finest_level, 0}) {
      const std::string rule = level_rule(lv - b.level, 0, c.mbnx);
      if (b.skip.empty() && !rule.empty()) b.skip = "level " + std::to_string(b.level) + ": a block on level " + std::to_string(lv) + " " + rule;
    }
  }
  if (pin.DoesParameterExist(b.name, "reduce")) {
    std::string rule = reduce_parse(pin.GetString(b.name, "reduce"), b.reduce);
    if (rule.empty()) rule = reduce_rule(b.reduce, c.mbnx);
    if (rule.empty() && b.has_level) rule = "reduce: a block that also sets level is not built";
    if (b.skip.empty() && !rule.empty()) b.skip = rule;
  }
  if (pin.DoesParameterExist(b.name, "reduce_level")) {
    b.has_reduce_level = true, b.reduce_level = pin.GetInteger(b.name, "reduce_level");
    std::string rule;
    if (b.has_level) rule = "reduce_level: a block that also sets level is not built";
    else if (!pin.DoesParameterExist(b.name, "reduce")) rule = "reduce_level: only valid beside reduce";
    // the worst shifts this deck can ever produce: its finest possible level and the root grid
    for (const int lv : {c.finest_level, 0}) {
      if (!rule.empty() || !b.skip.empty()) break;
      const std::string bad = level_rule(lv - b.reduce_level, b.reduce, c.mbnx);
      if (!bad.empty()) rule = "reduce_level " + std::to_string(b.reduce_level) + ": a block on level " + std::to_string(lv) + " " + bad;
    }
    if (b.skip.empty() && !rule.empty()) b.skip = rule;
  }
  if (!b.skip.empty()) b.kind = SKIPPED;
}

// The <parthenon/outputN> blocks of deck + overrides.  A block without a positive dt can never become due: skipped.
std::unique_ptr<State> parse(const artemis_sim_t *sim) {
  artemis_host::ParameterInput pin;
  pin.LoadFromString(deck_of(sim));
  for (const std::string &o : overrides_of(sim)) pin.ApplyOverride(o);
  std::unique_ptr<State> st(new State());
  st->problem_id = pin.DoesParameterExist("parthenon/job", "problem_id") ? pin.GetString("parthenon/job", "problem_id") : "artemis";
  const std::string prefix = "parthenon/output";
  for (const std::string &name : pin.BlocksWithPrefix(prefix)) {
    const std::string tail = name.substr(prefix.size());
    if (tail.empty() || tail.find_first_not_of("0123456789") != std::string::npos) continue;
    OutBlock b;
    b.name = name, b.index = std::atoi(tail.c_str());
    b.file_type = pin.DoesParameterExist(name, "file_type") ? pin.GetString(name, "file_type") : "";
    b.dt = pin.DoesParameterExist(name, "dt") ? pin.GetReal(name, "dt") : 0.0;
    b.kind = (b.file_type == "hst") ? HST : ((b.file_type == "rst") ? RST : SKIPPED);
    if (b.file_type == "fld") parse_fld(pin, clock_of(sim), b);
    st->blocks.push_back(b);
  }
  // (BlocksWithPrefix walks a sorted set: output10 would come before output2)
  for (size_t a = 1; a < st->blocks.size(); ++a)
    for (size_t q = a; q > 0 && st->blocks[q].index < st->blocks[q - 1].index; --q) std::swap(st->blocks[q], st->blocks[q - 1]);
  return st;
}

bool acted_on(const OutBlock &b) { return b.kind != SKIPPED && b.dt > 0.0 && std::isfinite(b.dt); }

std::string status_of(const State &st, const OutBlock &b) {
  if (b.kind == SKIPPED && !b.skip.empty()) return "skipped: " + b.skip;
  if (b.kind == SKIPPED) return "skipped: " + (b.file_type.empty() ? std::string("no file_type") : b.file_type + " is not built");
  if (!acted_on(b)) return "skipped: no positive dt";
  return st.on ? "active" : "inactive: outputs are not enabled";
}

std::vector<std::string> labels(const Clock &c) {
  std::vector<std::string> l = {"time", "dt", "cycle", "nbtotal"};
  const char *gas[6] = {"gas_mass", "gas_momentum_x1", "gas_momentum_x2", "gas_momentum_x3", "gas_energy", "gas_internal_energy"};
  const char *dust[4] = {"dust_mass", "dust_momentum_x1", "dust_momentum_x2", "dust_momentum_x3"};
  for (int q = 0; q < 6; ++q)
    for (int n = 0; n < c.ns_gas; ++n) l.push_back(std::string(gas[q]) + "_" + std::to_string(n));
  for (int q = 0; q < 4; ++q)
    for (int n = 0; n < c.ns_dust; ++n) l.push_back(std::string(dust[q]) + "_" + std::to_string(n));
  return l;
}

// one history row (collective: the sums are reduced over the ranks; rank 0 writes)
void write_history(artemis_sim_t *sim, State &st, OutBlock &b) {
  const Clock c = clock_of(sim);
  std::vector<double> sums(static_cast<size_t>(6 * c.ns_gas + 4 * c.ns_dust) + 1, 0.0);
  history_sums(sim, sums.data());
  b.path = st.dir + "/" + st.problem_id + ".out" + std::to_string(b.index) + ".hst";
  if (c.rank == 0) {
    std::FILE *f = std::fopen(b.path.c_str(), "a");
    if (!f) throw std::runtime_error("outputs: cannot open " + b.path + ": " + std::strerror(errno));
    if (!b.header_done) {
      std::fprintf(f, "#  History data\n#");
      const std::vector<std::string> l = labels(c);
      for (size_t q = 0; q < l.size(); ++q) std::fprintf(f, " [%zu]=%s", q + 1, l[q].c_str());
      std::fprintf(f, "\n");
    }
    std::fprintf(f, "%.16e %.16e %ld %ld", c.time, c.dt, c.ncycle, c.nblocks_global);
    for (int q = 0; q < 6; ++q)
      for (int n = 0; n < c.ns_gas; ++n) std::fprintf(f, " %.16e", sums[6 * n + q]);
    for (int q = 0; q < 4; ++q)
      for (int n = 0; n < c.ns_dust; ++n) std::fprintf(f, " %.16e", sums[6 * c.ns_gas + 4 * n + q]);
    std::fprintf(f, "\n");
    const bool bad = std::ferror(f) != 0;
    if (std::fclose(f) != 0 || bad) throw std::runtime_error("outputs: writing " + b.path + " failed");
  }
  b.header_done = true;
}

void write_dump(artemis_sim_t *sim, State &st, OutBlock &b, bool final) {
  char num[16];
  std::snprintf(num, sizeof num, "%05ld", b.counter);
  b.path = st.dir + "/" + st.problem_id + ".out" + std::to_string(b.index) + "." + (final ? std::string("final") : std::string(num)) + ".rst";
  if (artemis_sim_save(sim, b.path.c_str()) != 0)
    throw std::runtime_error(std::string("outputs: ") + b.path + ": " + artemis_sim_last_error());
  if (!final) b.counter++;
}

// `failed` summed over the ranks (barrier and vote in one); true if anybody failed
bool vote(artemis_sim_t *sim, bool failed) {
  const artemis_comm_t *comm = artemis_ckpt::comm_of(sim);
  if (!comm || comm->nranks <= 1) return failed;
  double v = failed ? 1.0 : 0.0;
  if (!comm->allreduce_sum || comm->allreduce_sum(comm->ctx, &v, 1)) return true;
  return v > 0.0;
}

// meta.json, the rank parts and the directory itself; anything else in there is not ours and keeps the directory
void remove_field_dir(const std::string &dir) {
  DIR *d = opendir(dir.c_str());
  if (!d) {
    if (errno == ENOENT) return;
    throw std::runtime_error("cannot open " + dir + ": " + std::strerror(errno));
  }
  std::vector<std::string> names;
  while (struct dirent *e = readdir(d)) {
    const std::string n = e->d_name;
    const bool part = n.size() > 8 && n.compare(0, 4, "rank") == 0 && n.compare(n.size() - 4, 4, ".bin") == 0 &&
                      n.find_first_not_of("0123456789", 4) == n.size() - 4;
    if (n == "meta.json" || part) names.push_back(n);
  }
  closedir(d);
  for (const std::string &n : names) unlink((dir + "/" + n).c_str());
  if (rmdir(dir.c_str()) != 0) throw std::runtime_error("cannot replace " + dir + " (it holds files that are not parts of a field dump): " + std::strerror(errno));
}

void write_file(const std::string &name, const void *data, size_t bytes) {
  std::FILE *f = std::fopen(name.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot open " + name + ": " + std::strerror(errno));
  const bool bad = bytes && std::fwrite(data, 1, bytes, f) != bytes;
  if (std::fclose(f) != 0 || bad) throw std::runtime_error("writing " + name + " failed");
}

// The request of a `fld` block: the one place its parsed keys become one
FieldRequest request_of(const OutBlock &b) {
  FieldRequest req;
  req.codes = b.codes, req.single = b.single, req.axes = b.reduce;
  req.has_level = b.reduce ? b.has_reduce_level : b.has_level, req.level = b.reduce ? b.reduce_level : b.level;
  return req;
}

// The version says which of the two choices a dump made: 1 neither, 2 a level ("level"), 3 axes ("reduce": the names of
// the directions summed over), 4 both ("reduce" and "reduce_level").  With axes the variables end with "volume" (W).
// From version 2 on every block entry carries the nx it was written with and the element offset of its first value in its
// rank's part (the blocks of a rank follow each other in index order).
std::string meta_json(const Clock &c, const FieldsLayout &L, const FieldRequest &req) {
  const std::vector<int> &codes = req.codes;
  const int version = req.axes ? (req.has_level ? 4 : 3) : (req.has_level ? 2 : 1);
  std::string j = "{\"format\": \"artemis_fld\", \"version\": " + std::to_string(version);
  if (req.axes) {
    j += ", \"reduce\": [";
    for (int d = 0, n = 0; d < 3; ++d)
      if ((req.axes >> d) & 1) j += std::string(n++ ? ", " : "") + "\"x" + std::to_string(d + 1) + "\"";
    j += "]";
  }
  if (req.has_level) j += std::string(req.axes ? ", \"reduce_level\": " : ", \"level\": ") + std::to_string(req.level);
  j += ", \"time\": " + json_num(c.time) + ", \"dt\": " + json_num(c.dt) +
       ", \"cycle\": " + std::to_string(c.ncycle) + ", \"coordinates\": " + json_str(L.coordinates) +
       ", \"ndim\": " + std::to_string(L.ndim) + ", \"nghost\": 0, \"dtype\": " + (req.single ? "\"<f4\"" : "\"<f8\"") +
       ", \"gamma\": " + json_num(L.gamma) + ", \"ns_gas\": " + std::to_string(c.ns_gas) + ", \"ns_dust\": " + std::to_string(c.ns_dust) +
       ", \"nranks\": " + std::to_string(L.nranks);
  j += ", \"nx\": [" + std::to_string(L.nx[0]) + ", " + std::to_string(L.nx[1]) + ", " + std::to_string(L.nx[2]) + "],\n \"variables\": [";
  int rows = req.axes ? 1 : 0;
  for (size_t v = 0; v < codes.size(); ++v) {
    const int ns = field_var_is_dust(codes[v]) ? c.ns_dust : c.ns_gas;
    const std::string name = field_var_name(codes[v]);
    j += std::string(v ? ", " : "") + "{\"name\": " + json_str(name) + ", \"ncomp\": " + std::to_string(field_var_components(codes[v], c.ns_gas, c.ns_dust)) +
         ", \"components\": [";
    for (int n = 0; n < ns; ++n)
      for (int d = 0; d < (field_var_is_vector(codes[v]) ? 3 : 1); ++d)
        j += std::string(n || d ? ", " : "") + json_str(name + "_" + std::to_string(n) + (field_var_is_vector(codes[v]) ? "_x" + std::to_string(d + 1) : ""));
    j += "]}";
    rows += field_var_components(codes[v], c.ns_gas, c.ns_dust);
  }
  if (req.axes) j += ", {\"name\": \"volume\", \"ncomp\": 1, \"components\": [\"volume\"]}";
  j += "],\n \"blocks\": [";
  auto extent = [&](size_t g, int d) { return reduce_level_extent(L.nx[d], req.has_level ? L.blocks[g].level - req.level : 0, req.axes, d); };
  std::vector<long> offset(L.blocks.size(), 0);
  std::vector<std::vector<size_t>> of_rank(static_cast<size_t>(L.nranks));
  for (size_t g = 0; g < L.blocks.size(); ++g) of_rank[static_cast<size_t>(L.blocks[g].rank)].push_back(g);
  for (std::vector<size_t> &gs : of_rank) {
    std::sort(gs.begin(), gs.end(), [&](size_t a, size_t b) { return L.blocks[a].index < L.blocks[b].index; });
    long at = 0;
    for (const size_t g : gs) offset[g] = at, at += static_cast<long>(rows) * extent(g, 0) * extent(g, 1) * extent(g, 2);
  }
  for (size_t g = 0; g < L.blocks.size(); ++g) {
    const FieldBlock &B = L.blocks[g];
    j += std::string(g ? ",\n  " : "\n  ") + "{\"gid\": " + std::to_string(B.gid) + ", \"level\": " + std::to_string(B.level) + ", \"bounds\": [";
    for (int q = 0; q < 6; ++q) j += (q ? ", " : "") + json_num(B.bounds[q]);
    j += "], \"nx\": [" + std::to_string(extent(g, 0)) + ", " + std::to_string(extent(g, 1)) + ", " + std::to_string(extent(g, 2)) + "]" +
         (version > 1 ? ", \"offset\": " + std::to_string(offset[g]) : std::string()) + ", \"rank\": " + std::to_string(B.rank) +
         ", \"index\": " + std::to_string(B.index) + "}";
  }
  return j + "]}\n";
}

// One field dump (artemis_driver.h: artemis_sim_write_fields*).  Every rank takes every vote, whatever happened to it
// before: the votes are collective.
void write_fields(artemis_sim_t *sim, const std::string &path_in, const FieldRequest &req) {
  std::string err, dir = path_in, tmp;
  while (dir.size() > 1 && dir.back() == '/') dir.pop_back();
  tmp = dir + ".tmp";
  const Clock c = clock_of(sim);
  FieldsLayout L;
  try {
    const std::string dead = artemis_ckpt::dead_reason(sim);
    if (!dead.empty()) throw std::runtime_error(dead);
    if (req.codes.empty()) throw std::runtime_error("no variables");
    L = fields_layout(sim);
    if (c.rank == 0) {
      remove_field_dir(tmp);
      if (::mkdir(tmp.c_str(), 0777) != 0) throw std::runtime_error("cannot create " + tmp + ": " + std::strerror(errno));
    }
  } catch (const std::exception &e) {
    err = e.what();
  }
  bool failed = vote(sim, !err.empty());
  if (!failed) {
    try {
      std::vector<char> host(gather_fields(sim, req, nullptr, nullptr));
      gather_fields(sim, req, host.data(), nullptr);
      write_file(tmp + "/rank" + std::to_string(c.rank) + ".bin", host.data(), host.size());
    } catch (const std::exception &e) {
      err = e.what();
    }
    failed = vote(sim, !err.empty());
  }
  if (!failed) {
    try {
      if (c.rank == 0) {
        const std::string meta = meta_json(c, L, req);
        write_file(tmp + "/meta.json", meta.data(), meta.size()); // last: a directory with it has all its parts
        remove_field_dir(dir);
        if (std::rename(tmp.c_str(), dir.c_str()) != 0) throw std::runtime_error("cannot rename " + tmp + " to " + dir + ": " + std::strerror(errno));
      }
    } catch (const std::exception &e) {
      err = e.what();
    }
    failed = vote(sim, !err.empty());
  }
  if (!failed) return;
  if (c.rank == 0) {
    try {
      remove_field_dir(tmp);
    } catch (const std::exception &) {
    }
  }
  throw std::runtime_error("write_fields: " + dir + ": " + (err.empty() ? std::string("another rank failed") : err));
}

void write_field_dump(artemis_sim_t *sim, State &st, OutBlock &b, bool final) {
  char num[16];
  std::snprintf(num, sizeof num, "%05ld", b.counter);
  b.path = st.dir + "/" + st.problem_id + ".out" + std::to_string(b.index) + "." + (final ? std::string("final") : std::string(num)) + ".fld";
  write_fields(sim, b.path, request_of(b));
  if (!final) b.counter++;
}

} // namespace

void destroy(State *st) { delete st; }
bool enabled(const State *st) { return st && st->on; }

double deadline(const State *st) {
  double t = HUGE_VAL;
  if (st && st->on)
    for (const OutBlock &b : st->blocks)
      if (acted_on(b)) t = std::min(t, b.next_time);
  return t;
}

bool write_due(artemis_sim_t *sim, bool history_only) {
  State *st = state_of(sim);
  if (!enabled(st)) return false;
  bool dump_due = false;
  for (OutBlock &b : st->blocks) {
    if (!acted_on(b)) continue;
    const Clock c = clock_of(sim);
    if (c.time < b.next_time) continue;
    if (b.kind != HST && history_only) {
      dump_due = true;
      continue;
    }
    if (b.kind == HST) write_history(sim, *st, b);
    else if (b.kind == FLD) write_field_dump(sim, *st, b, false);
    else write_dump(sim, *st, b, false);
    b.written++, b.last_cycle = c.ncycle;
    b.next_time = next_multiple(c.time, b.dt);
  }
  return dump_due;
}

void write_final(artemis_sim_t *sim) {
  State *st = state_of(sim);
  if (!enabled(st)) return;
  for (OutBlock &b : st->blocks) {
    if (!acted_on(b)) continue;
    const Clock c = clock_of(sim);
    if (b.kind == HST) {
      if (b.last_cycle == c.ncycle) continue; // this cycle has its row
      write_history(sim, *st, b);
      b.written++, b.last_cycle = c.ncycle;
    } else {
      if (b.last_final_cycle == c.ncycle) continue;
      if (b.kind == FLD) write_field_dump(sim, *st, b, true);
      else write_dump(sim, *st, b, true);
      b.written++, b.last_final_cycle = c.ncycle;
    }
  }
}

} // namespace artemis_out

extern "C" {

int artemis_sim_enable_outputs(artemis_sim_t *sim, const char *dir) {
  using namespace artemis_out;
  try {
    if (!sim || !dir || !*dir) throw std::runtime_error("enable_outputs: no simulation or no directory");
    const std::string dead = artemis_ckpt::dead_reason(sim);
    if (!dead.empty()) throw std::runtime_error(dead);
    std::unique_ptr<State> st = parse(sim);
    st->on = true, st->dir = dir;
    while (st->dir.size() > 1 && st->dir.back() == '/') st->dir.pop_back();
    make_dirs(st->dir);
    const Clock c = clock_of(sim);
    const bool fresh = c.ncycle == 0 && c.time == 0.0;
    for (OutBlock &b : st->blocks) {
      if (!acted_on(b)) continue;
      long m = 0;
      b.next_time = fresh ? 0.0 : next_multiple(c.time, b.dt, &m);
      b.counter = m; // a continued run goes on numbering its dumps where an unbroken one would be
    }
    destroy(state_of(sim));
    state_of(sim) = st.release();
    return 0;
  } catch (const std::exception &e) {
    artemis_ckpt::set_error(e.what());
    return 1;
  }
}

// The artemis_sim_write_fields* entry points: the names become the codes of `req`, then the dump
static int write_entry(artemis_sim_t *sim, const char *path, int nvar, const char *const *names, artemis_out::FieldRequest req) {
  using namespace artemis_out;
  try {
    if (!sim || !path || !*path) throw std::runtime_error("write_fields: no simulation or no path");
    const Clock c = clock_of(sim);
    for (int v = 0; v < nvar; ++v) {
      const std::string name = (names && names[v]) ? names[v] : "";
      const int code = field_var_code(name);
      if (code < 0 || field_var_components(code, c.ns_gas, c.ns_dust) == 0) throw std::runtime_error("write_fields: unknown variable " + name);
      req.codes.push_back(code);
    }
    // (every rank holds blocks of the same shape: all refuse the axes or none.  A shift that breaks a rule throws inside
    //  the gather, on the ranks that hold such a block, and the vote spreads it)
    const std::string rule = req.axes ? reduce_rule(req.axes, c.mbnx) : "";
    if (!rule.empty()) throw std::runtime_error("write_fields: " + rule);
    write_fields(sim, path, req);
    return 0;
  } catch (const std::exception &e) {
    artemis_ckpt::set_error(e.what());
    return 1;
  }
}
int artemis_sim_write_fields(artemis_sim_t *sim, const char *path, int nvar, const char *const *names, int single) {
  return write_entry(sim, path, nvar, names, {{}, single != 0, 0, false, 0});
}
int artemis_sim_write_fields_level(artemis_sim_t *sim, const char *path, int nvar, const char *const *names, int single, int level) {
  return write_entry(sim, path, nvar, names, {{}, single != 0, 0, true, level});
}
int artemis_sim_write_fields_reduced(artemis_sim_t *sim, const char *path, int nvar, const char *const *names, int single, int axes) {
  return write_entry(sim, path, nvar, names, {{}, single != 0, artemis_out::reducing_axes(axes), false, 0});
}
int artemis_sim_write_fields_reduced_level(artemis_sim_t *sim, const char *path, int nvar, const char *const *names, int single, int axes,
                                           int level) {
  return write_entry(sim, path, nvar, names, {{}, single != 0, artemis_out::reducing_axes(axes), true, level});
}

long artemis_sim_scatter_fields(artemis_sim_t *sim, int nvar, const char *const *names, int single, const void *host_in, double time) {
  using namespace artemis_out;
  try {
    if (!sim) throw std::runtime_error("scatter_fields: no simulation");
    const std::string dead = artemis_ckpt::dead_reason(sim);
    if (!dead.empty()) throw std::runtime_error(dead);
    const Clock c = clock_of(sim);
    std::vector<int> codes;
    for (int v = 0; v < nvar; ++v) {
      const std::string name = (names && names[v]) ? names[v] : "";
      const int code = field_var_code(name);
      if (code >= 0 && field_var_is_derived(code)) throw std::runtime_error("scatter_fields: " + name + " is an output, not part of a state");
      if (code < 0 || field_var_components(code, c.ns_gas, c.ns_dust) == 0) throw std::runtime_error("scatter_fields: unknown variable " + name);
      codes.push_back(code);
    }
    return static_cast<long>(scatter_fields(sim, codes, single != 0, host_in, time));
  } catch (const std::exception &e) {
    artemis_ckpt::set_error(e.what());
    return -1;
  }
}

int artemis_sim_outputs_describe(const artemis_sim_t *sim, char *json_out, long capacity) {
  using namespace artemis_out;
  try {
    if (!sim) throw std::runtime_error("outputs_describe: no simulation");
    std::unique_ptr<State> parsed;
    const State *st = state_of(sim);
    if (!st) parsed = parse(sim), st = parsed.get();
    std::string j = "{\"enabled\": " + std::string(st->on ? "true" : "false") + ", \"dir\": " + (st->on ? json_str(st->dir) : "null") +
                    ", \"problem_id\": " + json_str(st->problem_id) + ", \"blocks\": [";
    bool first = true;
    for (const OutBlock &b : st->blocks) {
      if (!first) j += ", ";
      first = false;
      const bool live = st->on && acted_on(b);
      j += "{\"block\": " + json_str(b.name) + ", \"index\": " + std::to_string(b.index) + ", \"file_type\": " + json_str(b.file_type) +
           ", \"dt\": " + json_num(b.dt) + ", \"status\": " + json_str(status_of(*st, b)) +
           ", \"next_time\": " + (live ? json_num(b.next_time) : "null") + ", \"written\": " + std::to_string(b.written) +
           ", \"last_cycle\": " + (b.last_cycle >= 0 ? std::to_string(b.last_cycle) : "null") +
           ", \"path\": " + (b.path.empty() ? "null" : json_str(b.path));
      if (b.is_fld) {
        j += ", \"variables\": [";
        for (size_t v = 0; v < b.variables.size(); ++v) j += (v ? ", " : "") + json_str(b.variables[v]);
        j += std::string("], \"single_precision\": ") + (b.single ? "true" : "false");
        if (b.has_level) j += ", \"level\": " + std::to_string(b.level);
        if (b.reduce) {
          j += ", \"reduce\": [";
          for (int d = 0, n = 0; d < 3; ++d)
            if ((b.reduce >> d) & 1) j += std::string(n++ ? ", " : "") + "\"x" + std::to_string(d + 1) + "\"";
          j += "]";
        }
        if (b.has_reduce_level) j += ", \"reduce_level\": " + std::to_string(b.reduce_level);
      }
      j += "}";
    }
    j += "]}";
    if (json_out && capacity > static_cast<long>(j.size())) std::memcpy(json_out, j.c_str(), j.size() + 1);
    return static_cast<int>(j.size());
  } catch (const std::exception &e) {
    artemis_ckpt::set_error(e.what());
    return -1;
  }
}

} // extern "C"
