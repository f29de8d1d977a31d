// copra_hip_ric.hip -- the Riccati-factor tier (lmpc_fused_ric.hpp) and the one-instance-per-lane pass (lmpc_lane.hpp) with a RUN-TIME
// horizon, for the shapes the library covers at every horizon (plan_builder.hpp::ric_aot_shape: the double integrators in one, two and
// three dimensions).  Round 3 shipped these kernels for (6, 3) at N = 10, 15, 20 only; every other horizon ran on the round-1 tiers unless
// the user's box had hipcc for copra_batch_specialise.  A translation unit of its own: it compiles next to copra_hip.hip (make -j).  Its builds: the
// entries of tier_builds.hpp with UNIT ric.
#include "ric_kernels.hpp"

#define COPRA_FIRST_INST(UNIT, KIND, ...) COPRA_UNIT_##UNIT(template, COPRA_FIRST_KERNEL_##KIND(__VA_ARGS__))
#define COPRA_LANE_INST(UNIT, ...) COPRA_UNIT_##UNIT(template, COPRA_LANE_KERNEL(__VA_ARGS__))
COPRA_FIRST_TIER_BUILDS(COPRA_FIRST_INST)
COPRA_LANE_BUILDS(COPRA_LANE_INST)
