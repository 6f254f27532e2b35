// What a list of field variables (enum artemis_field_var) means as an INPUT: artemis_hip_unpack_fields and the host
// driver's scatter both take, per fluid, exactly one complete form of the state or nothing.  Plain C++ (the driver's
// translation units include it next to abi.hip): one place decides what a selection is and what is wrong with it.
//   gas    primitive: prim.density + prim.velocity + exactly one of prim.sie / prim.pressure
//          conserved: cons.density + cons.momentum + cons.total_energy (+ cons.internal_energy)
//   dust   primitive: prim.density + prim.velocity;  conserved: cons.density + cons.momentum
#pragma once
#include <string>

#include "../../include/artemis_hip.h"

namespace artemis {

enum FieldForm { FORM_NONE = 0, FORM_PRIM_SIE = 1, FORM_PRIM_PRESSURE = 2, FORM_CONS = 3, FORM_PRIM = 1 };

// The selection as the unpack kernel takes it (a wave-uniform kernel argument): the form of each fluid and the first
// component, of a block's ncomp, of each of its parts; g_eint < 0: no cons.internal_energy, the input is 0
struct FieldUnpack {
  int gas_form, dust_form, ncomp;
  int g_rho, g_vec, g_en, g_eint; // density, velocity | momentum, sie | pressure | total energy, internal energy
  int d_rho, d_vec;
};

inline const char *field_var_text(int code) {
  static const char *const names[ARTEMIS_VAR_COUNT] = {"gas.prim.density", "gas.prim.velocity", "gas.prim.pressure", "gas.prim.sie",
                                                       "gas.cons.density", "gas.cons.momentum", "gas.cons.total_energy",
                                                       "gas.cons.internal_energy", "dust.prim.density", "dust.prim.velocity",
                                                       "dust.cons.density", "dust.cons.momentum"};
  static const char *const derived[ARTEMIS_VAR_DERIVED_END - ARTEMIS_VAR_DERIVED0] = {"gas.derived.divergence", "gas.derived.vorticity",
                                                                                     "dust.derived.divergence", "dust.derived.vorticity"};
  if (code >= ARTEMIS_VAR_DERIVED0 && code < ARTEMIS_VAR_DERIVED_END) return derived[code - ARTEMIS_VAR_DERIVED0];
  return (code >= 0 && code < ARTEMIS_VAR_COUNT) ? names[code] : "?";
}

// "" and U filled, or what is wrong with the selection.  nsg / nsd: species of the pack (0: the fluid is absent).
inline std::string field_unpack_plan(int nsel, const int *sel, int nsg, int nsd, FieldUnpack &U) {
  U = FieldUnpack{FORM_NONE, FORM_NONE, 0, -1, -1, -1, -1, -1, -1};
  if (nsel < 0 || nsel > ARTEMIS_VAR_COUNT || (nsel > 0 && !sel)) return "unpack fields: 0 to 12 variable codes are taken, each once";
  int at[ARTEMIS_VAR_COUNT];
  for (int c = 0; c < ARTEMIS_VAR_COUNT; ++c) at[c] = -1;
  for (int e = 0; e < nsel; ++e) {
    const int code = sel[e];
    if (code >= ARTEMIS_VAR_DERIVED0 && code < ARTEMIS_VAR_DERIVED_END)
      return std::string("unpack fields: ") + field_var_text(code) + " is an output, not part of a state";
    if (code < 0 || code >= ARTEMIS_VAR_COUNT) return "unpack fields: unknown variable code " + std::to_string(code);
    if (at[code] >= 0) return std::string("unpack fields: ") + field_var_text(code) + " is given twice";
    const bool dust = code >= ARTEMIS_VAR_DUST_PRIM_DENSITY;
    const int ns = dust ? nsd : nsg;
    if (ns < 1) return std::string("unpack fields: ") + field_var_text(code) + (dust ? " on a pack without dust" : " on a pack without gas");
    const bool vec = code == ARTEMIS_VAR_GAS_PRIM_VELOCITY || code == ARTEMIS_VAR_GAS_CONS_MOMENTUM ||
                     code == ARTEMIS_VAR_DUST_PRIM_VELOCITY || code == ARTEMIS_VAR_DUST_CONS_MOMENTUM;
    at[code] = U.ncomp, U.ncomp += (vec ? 3 : 1) * ns;
  }
  auto has = [&](int code) { return at[code] >= 0; };
  auto missing = [&](const char *form, int code) {
    return std::string("unpack fields: the ") + form + " form is incomplete, " + field_var_text(code) + " is missing";
  };
  const bool gp = has(ARTEMIS_VAR_GAS_PRIM_DENSITY) || has(ARTEMIS_VAR_GAS_PRIM_VELOCITY) || has(ARTEMIS_VAR_GAS_PRIM_PRESSURE) ||
                  has(ARTEMIS_VAR_GAS_PRIM_SIE);
  const bool gc = has(ARTEMIS_VAR_GAS_CONS_DENSITY) || has(ARTEMIS_VAR_GAS_CONS_MOMENTUM) || has(ARTEMIS_VAR_GAS_CONS_TOTAL_ENERGY) ||
                  has(ARTEMIS_VAR_GAS_CONS_INTERNAL_ENERGY);
  if (gp && gc) return "unpack fields: the gas variables mix the primitive and the conserved form";
  if (gp) {
    if (!has(ARTEMIS_VAR_GAS_PRIM_DENSITY)) return missing("primitive gas", ARTEMIS_VAR_GAS_PRIM_DENSITY);
    if (!has(ARTEMIS_VAR_GAS_PRIM_VELOCITY)) return missing("primitive gas", ARTEMIS_VAR_GAS_PRIM_VELOCITY);
    if (has(ARTEMIS_VAR_GAS_PRIM_SIE) && has(ARTEMIS_VAR_GAS_PRIM_PRESSURE))
      return "unpack fields: gas.prim.sie and gas.prim.pressure are both given, the primitive gas form takes one of them";
    if (!has(ARTEMIS_VAR_GAS_PRIM_SIE) && !has(ARTEMIS_VAR_GAS_PRIM_PRESSURE))
      return "unpack fields: the primitive gas form is incomplete, gas.prim.sie or gas.prim.pressure is missing";
    const bool sie = has(ARTEMIS_VAR_GAS_PRIM_SIE);
    U.gas_form = sie ? FORM_PRIM_SIE : FORM_PRIM_PRESSURE;
    U.g_rho = at[ARTEMIS_VAR_GAS_PRIM_DENSITY], U.g_vec = at[ARTEMIS_VAR_GAS_PRIM_VELOCITY];
    U.g_en = sie ? at[ARTEMIS_VAR_GAS_PRIM_SIE] : at[ARTEMIS_VAR_GAS_PRIM_PRESSURE];
  } else if (gc) {
    for (int code : {ARTEMIS_VAR_GAS_CONS_DENSITY, ARTEMIS_VAR_GAS_CONS_MOMENTUM, ARTEMIS_VAR_GAS_CONS_TOTAL_ENERGY})
      if (!has(code)) return missing("conserved gas", code);
    U.gas_form = FORM_CONS;
    U.g_rho = at[ARTEMIS_VAR_GAS_CONS_DENSITY], U.g_vec = at[ARTEMIS_VAR_GAS_CONS_MOMENTUM];
    U.g_en = at[ARTEMIS_VAR_GAS_CONS_TOTAL_ENERGY], U.g_eint = at[ARTEMIS_VAR_GAS_CONS_INTERNAL_ENERGY];
  }
  const bool dp = has(ARTEMIS_VAR_DUST_PRIM_DENSITY) || has(ARTEMIS_VAR_DUST_PRIM_VELOCITY);
  const bool dc = has(ARTEMIS_VAR_DUST_CONS_DENSITY) || has(ARTEMIS_VAR_DUST_CONS_MOMENTUM);
  if (dp && dc) return "unpack fields: the dust variables mix the primitive and the conserved form";
  if (dp) {
    if (!has(ARTEMIS_VAR_DUST_PRIM_DENSITY)) return missing("primitive dust", ARTEMIS_VAR_DUST_PRIM_DENSITY);
    if (!has(ARTEMIS_VAR_DUST_PRIM_VELOCITY)) return missing("primitive dust", ARTEMIS_VAR_DUST_PRIM_VELOCITY);
    U.dust_form = FORM_PRIM, U.d_rho = at[ARTEMIS_VAR_DUST_PRIM_DENSITY], U.d_vec = at[ARTEMIS_VAR_DUST_PRIM_VELOCITY];
  } else if (dc) {
    if (!has(ARTEMIS_VAR_DUST_CONS_DENSITY)) return missing("conserved dust", ARTEMIS_VAR_DUST_CONS_DENSITY);
    if (!has(ARTEMIS_VAR_DUST_CONS_MOMENTUM)) return missing("conserved dust", ARTEMIS_VAR_DUST_CONS_MOMENTUM);
    U.dust_form = FORM_CONS, U.d_rho = at[ARTEMIS_VAR_DUST_CONS_DENSITY], U.d_vec = at[ARTEMIS_VAR_DUST_CONS_MOMENTUM];
  }
  return "";
}

} // namespace artemis
