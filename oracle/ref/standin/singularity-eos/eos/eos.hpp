// Stand-in for <singularity-eos/eos/eos.hpp>: an ideal gas inside a one-alternative Variant, with the single
// call the reference's Riemann solvers make (the Gruneisen parameter of an ideal gas is gamma - 1).
#ifndef ORACLE_REF_STANDIN_SINGULARITY_EOS_HPP_
#define ORACLE_REF_STANDIN_SINGULARITY_EOS_HPP_

namespace singularity {

struct IdealGas {
  double gm1 = 0.0, Cv = 1.0;
  IdealGas() {}
  IdealGas(double gm1_, double Cv_) : gm1(gm1_), Cv(Cv_) {}
  double GruneisenParamFromDensityTemperature(const double, const double, double * = nullptr) const { return gm1; }
};

template <class EOS>
struct Variant {
  EOS eos;
  Variant() {}
  Variant(const EOS &e) : eos(e) {}
  double GruneisenParamFromDensityTemperature(const double rho, const double temp, double *lambda = nullptr) const {
    return eos.GruneisenParamFromDensityTemperature(rho, temp, lambda);
  }
};

} // namespace singularity

#endif // ORACLE_REF_STANDIN_SINGULARITY_EOS_HPP_
