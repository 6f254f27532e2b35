// What csrc/driver/outputs.cpp (the scheduler of the deck's <parthenon/output*> blocks) and driver.cpp need from each
// other.  The schedule lives with the C handle, not with the simulation state an adaptive mesh rebuilds.  Everything
// here throws std::exception on failure; none of it is part of the C ABI.
#pragma once
#include <string>
#include <vector>

#include "artemis_driver.h"
#include "../fields_form.hpp"
#include "../fields_shape.hpp"

namespace artemis_out {

struct State; // parsed blocks, their next_time and counters (outputs.cpp)

struct Clock { // the driver's clock after a cycle and what a history row records next to it
  double time = 0.0, dt = 0.0, tlim = -1.0;
  long ncycle = 0, nlim = -1, nblocks_global = 0;
  int ns_gas = 0, ns_dust = 0, rank = 0;
  int finest_level = 0, mbnx[3] = {1, 1, 1}; // the finest level the mesh can ever hold; zones of a block
};

// ---- driver.cpp ------------------------------------------------------------------------------------------------------
Clock clock_of(const artemis_sim_t *sim);
const std::string &deck_of(const artemis_sim_t *sim);
const std::vector<std::string> &overrides_of(const artemis_sim_t *sim);
State *&state_of(artemis_sim_t *sim);
const State *state_of(const artemis_sim_t *sim);
// 6 ns_gas + 4 ns_dust volume integrals of the current state, reduced over the ranks (collective): the device kernel
// (artemis_hip_history_sums) where the library has it, the host sum otherwise
int history_sums(artemis_sim_t *sim, double *out);

// ---- field output ----------------------------------------------------------------------------------------------------
// The variables a `fld` block may name: those of enum artemis_field_var (include/artemis_hip.h) in its order, and the derived
// ones -- outputs only, formed from a zone and its face neighbours -- at their codes, a second range
constexpr int kFieldVars = 12, kDerived0 = 16, kDerivedEnd = 20;
inline bool field_var_known(int code) { return (code >= 0 && code < kFieldVars) || (code >= kDerived0 && code < kDerivedEnd); }
inline bool field_var_is_derived(int code) { return code >= kDerived0 && code < kDerivedEnd; }
inline const char *field_var_name(int code) {
  static const char *const names[kFieldVars] = {"gas.prim.density", "gas.prim.velocity", "gas.prim.pressure", "gas.prim.sie",
                                                "gas.cons.density", "gas.cons.momentum", "gas.cons.total_energy",
                                                "gas.cons.internal_energy", "dust.prim.density", "dust.prim.velocity",
                                                "dust.cons.density", "dust.cons.momentum"};
  if (field_var_is_derived(code)) return artemis::field_var_text(code); // (fields_form.hpp has the one copy of these names)
  return (code >= 0 && code < kFieldVars) ? names[code] : "";
}
inline int field_var_code(const std::string &name) { // -1: no such variable
  for (int c = 0; c < kDerivedEnd; ++c)
    if (field_var_known(c) && name == field_var_name(c)) return c;
  return -1;
}
inline bool field_var_is_dust(int code) { return field_var_is_derived(code) ? code >= 18 : code >= 8; }
inline bool field_var_is_vector(int code) { return code == 1 || code == 5 || code == 9 || code == 11 || code == 17 || code == 19; }
// components of a variable on a run with these species counts; 0: its fluid is absent
inline int field_var_components(int code, int ns_gas, int ns_dust) {
  return (field_var_is_vector(code) ? 3 : 1) * (field_var_is_dust(code) ? ns_dust : ns_gas);
}

struct FieldBlock { // one mesh block of the global mesh as meta.json lists it
  long gid = 0;
  int level = 0, rank = 0, index = 0; // index: its place among the blocks of `rank`
  double bounds[6] = {0, 0, 0, 0, 0, 0};
};
struct FieldsLayout {
  std::string coordinates;
  int ndim = 0, nx[3] = {1, 1, 1}, rank = 0, nranks = 1;
  double gamma = 0.0;
  std::vector<FieldBlock> blocks; // every block of the mesh, in gid order
};
// (driver.cpp) the global block table: every rank contributes its rows (collective)
FieldsLayout fields_layout(artemis_sim_t *sim);
// ---- one request for every mode of a gather: two independent choices.  axes (a mask, bit 0 x1, bit 1 x2, bit 2 x3, of
// ACTIVE directions; 0: none): every block integrated over them -- per component the sum of V q, and the volume as one
// more, last, row.  level: a block on level l has shift s = l - level; s >= 1 brings it down s times, s <= -1 up, along
// the ACTIVE directions (more than one zone) it keeps -- means by the volume-weighted restriction or by replication,
// integrals by pair sums or by an even share (artemis_hip.h, artemis_hip_pack_fields_level and _reduce_fields_level).
struct FieldRequest {
  std::vector<int> codes; // enum artemis_field_var
  bool single = false;
  int axes = 0;
  bool has_level = false;
  int level = 0;
};
// the mask of an entry point that always reduces: its 0 is not "none" but an empty mask, which reduce_rule refuses like
// every other mask outside 1 .. 7
inline int reducing_axes(int axes) { return axes ? axes : -1; }
using artemis_fields::reduce_level_extent;
// "" or what is wrong with a list "x2,x3" (axes filled: the mask)
inline std::string reduce_parse(const std::string &list, int &axes) {
  axes = 0;
  for (size_t at = 0; at <= list.size();) {
    size_t end = list.find(',', at);
    if (end == std::string::npos) end = list.size();
    std::string name = list.substr(at, end - at);
    const size_t a = name.find_first_not_of(" \t"), z = name.find_last_not_of(" \t");
    name = a == std::string::npos ? "" : name.substr(a, z - a + 1);
    if (name == "x1") axes |= 1;
    else if (name == "x2") axes |= 2;
    else if (name == "x3") axes |= 4;
    else if (!name.empty()) return "reduce: unknown direction " + name + " (x1, x2, x3)";
    at = end + 1;
  }
  return axes ? "" : "reduce: no direction";
}
// "" or the rule a block of nx zones breaks with these axes
inline std::string reduce_rule(int axes, const int nx[3]) {
  const std::string bad = artemis_fields::axes_rule(axes, nx, "no direction");
  return bad.empty() ? bad : "reduce: " + bad;
}
// "" or the rule a block of nx zones breaks at this shift along the directions these axes (0: none) keep
inline std::string level_rule(int shift, int axes, const int nx[3]) {
  const std::string bad = artemis_fields::shift_rule(shift, axes, nx);
  return bad.empty() ? bad : "would need " + bad;
}
// (driver.cpp) this rank's blocks one after the other, block b as [rows][nk'][nj'][ni'] of interior zones, double or float,
// rows = the components, and the volume where axes are set: through the artemis_hip_* entry point of the mode and a
// bounded staging buffer, or -- a library without that kernel -- a host loop over the downloaded primitives.  offsets
// (nblocks_local + 1 longs, or null): element offset of every block and the total.  host_out = NULL: sizes only.  Throws,
// before anything is written, where reduce_rule or -- for any block -- level_rule does.  Returns the bytes of the gather.
size_t gather_fields(artemis_sim_t *sim, const FieldRequest &req, void *host_out, long *offsets);
// (driver.cpp) the inverse: host_in in that layout, holding one complete form of the state per fluid (csrc/fields_form.hpp),
// becomes the interior primitives of the current buffer -- artemis_hip_unpack_fields out of the same staging buffer, or the
// host loop -- and the state is completed as a problem generator's is; time = NaN keeps the clock, dt is estimated afresh.
// host_in = NULL: validates only.  Collective.  Returns the bytes of the buffer.
size_t scatter_fields(artemis_sim_t *sim, const std::vector<int> &codes, bool single, const void *host_in, double time);

// ---- outputs.cpp -----------------------------------------------------------------------------------------------------
void destroy(State *st);
bool enabled(const State *st);
// earliest next_time of a block that is acted on; +infinity without one
double deadline(const State *st);
// Write every block that is due at the simulation's clock (time >= next_time) and move its next_time on.  history_only:
// called from inside the batched time loop, where a dump is not taken -- returns true if an `rst` or `fld` block is still due, and
// the loop then hands control back to the handle, which calls again with history_only = false.  Collective.
bool write_due(artemis_sim_t *sim, bool history_only);
// The run has ended at tlim or nlim: every block once more, unless this cycle has written it already.  Collective.
void write_final(artemis_sim_t *sim);

} // namespace artemis_out
