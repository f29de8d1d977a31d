// copra_hip_axis_w.hip -- instantiations of the one-(instance, axis)-per-lane solver (lmpc_axis.hpp) that read per-instance cost weights
// (copra_batch_set_cost_weights): the headline's shape, its first launch and its second chance.  A translation unit of its own (make -j).
#include "axis_kernels.hpp"

#define COPRA_AXIS_W_INST(NXA, NU, NMAX, QMAX, EXACT, CT, RPA) template __global__ void copra_lmpc_axis_w_kernel<NXA, NU, NMAX, QMAX, EXACT, CT, RPA>(const FusedPlan);
COPRA_AXIS_W_KERNELS(COPRA_AXIS_W_INST)
#define COPRA_AXIS_LIST_W_INST(NXA, NU, NMAX, QMAX, CT, RPA) template __global__ void copra_lmpc_axis_list_w_kernel<NXA, NU, NMAX, QMAX, CT, RPA>(const FusedPlan);
COPRA_AXIS_LIST_W_KERNELS(COPRA_AXIS_LIST_W_INST)
