// copra_hip_axis.hip -- instantiations of the one-(instance, axis)-per-lane solver (lmpc_axis.hpp): the entries "axis" of axis_builds.hpp,
// chains of two states and one control in two and three dimensions, horizons up to 20 and up to 31.
// A translation unit of its own: it compiles next to copra_hip.hip (make -j).
#include "axis_kernels.hpp"

#define COPRA_AXIS_UNIT_axis(...) __VA_ARGS__
#define COPRA_AXIS_UNIT_axis3(...)
#define COPRA_AXIS_UNIT_axis_w(...)
COPRA_AXIS_BUILDS(COPRA_AXIS_INST)
