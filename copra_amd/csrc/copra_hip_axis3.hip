// copra_hip_axis3.hip -- more instantiations of the one-(instance, axis)-per-lane solver (lmpc_axis.hpp): the entries "axis3" of
// axis_builds.hpp, one state per control, chains of two states at N = 21, and chains of three states per control (the jerk-controlled CoM model).
// A translation unit of its own: it compiles next to copra_hip_axis.hip (make -j).
#include "axis_kernels.hpp"

#define COPRA_AXIS_UNIT_axis(...)
#define COPRA_AXIS_UNIT_axis3(...) __VA_ARGS__
#define COPRA_AXIS_UNIT_axis_w(...)
COPRA_AXIS_BUILDS(COPRA_AXIS_INST)
