// copra_hip_axis_w.hip -- instantiations of the one-(instance, axis)-per-lane solver (lmpc_axis.hpp) that read per-instance cost weights
// (copra_batch_set_cost_weights): the entries "axis_w" of axis_builds.hpp, the headline's shape, its first launch and its second chance.
// A translation unit of its own (make -j).
#include "axis_kernels.hpp"

#define COPRA_AXIS_UNIT_axis(...)
#define COPRA_AXIS_UNIT_axis3(...)
#define COPRA_AXIS_UNIT_axis_w(...) __VA_ARGS__
COPRA_AXIS_BUILDS(COPRA_AXIS_INST)
