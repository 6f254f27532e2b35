// Deck-driven periodic outputs of the host driver (include/artemis_driver.h: artemis_sim_enable_outputs /
// _outputs_describe): the scheduler of the deck's <parthenon/outputN> blocks and the writer of history files.  Plain C++
// like the rest of the driver; the state is reached through outputs_hooks.hpp, dumps go through artemis_sim_save.
//
// Schedule (parthenon's Outputs::MakeOutputs, upstream): a block is due when time >= next_time; after it has been
// written next_time is the smallest m * dt, m an integer, above time -- by multiplication, so the times do not drift.  A
// fresh run starts with next_time = 0 (every block at cycle 0), a continued one with the first multiple above its clock.
// An output time is never passed to the time step.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <sys/stat.h>
#include <sys/types.h>
#include <vector>

#include "artemis_driver.h"
#include "checkpoint_hooks.hpp"
#include "outputs_hooks.hpp"
#include "parameter_input.hpp"

namespace artemis_out {

namespace {
enum Kind { HST, RST, SKIPPED };

struct OutBlock {
  std::string name, file_type; // "parthenon/output0", "hst"
  int index = 0;               // the N of outputN
  Kind kind = SKIPPED;
  double dt = 0.0, next_time = 0.0;
  long written = 0, last_cycle = -1, last_final_cycle = -1;
  long counter = 0;          // rst: number of the next dump
  bool header_done = false;  // hst: this run has written its header section
  std::string path;          // hst: the file; rst: the last dump
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
    st->blocks.push_back(b);
  }
  // (BlocksWithPrefix walks a sorted set: output10 would come before output2)
  for (size_t a = 1; a < st->blocks.size(); ++a)
    for (size_t q = a; q > 0 && st->blocks[q].index < st->blocks[q - 1].index; --q) std::swap(st->blocks[q], st->blocks[q - 1]);
  return st;
}

bool acted_on(const OutBlock &b) { return b.kind != SKIPPED && b.dt > 0.0 && std::isfinite(b.dt); }

std::string status_of(const State &st, const OutBlock &b) {
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
    if (b.kind == RST && history_only) {
      dump_due = true;
      continue;
    }
    if (b.kind == HST) write_history(sim, *st, b);
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
      write_dump(sim, *st, b, true);
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
           ", \"path\": " + (b.path.empty() ? "null" : json_str(b.path)) + "}";
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
