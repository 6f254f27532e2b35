// Stand-in for <parthenon/driver.hpp>: the leaf headers need nothing of the driver beyond the namespace artemis.hpp
// opens.  See package.hpp beside this file.
#ifndef ORACLE_REF_STANDIN_PARTHENON_DRIVER_HPP_
#define ORACLE_REF_STANDIN_PARTHENON_DRIVER_HPP_

#include "package.hpp"

namespace parthenon {
namespace driver {
namespace prelude {}
} // namespace driver
} // namespace parthenon

#endif // ORACLE_REF_STANDIN_PARTHENON_DRIVER_HPP_
