// axis_kernels.hpp -- the __global__ templates of the one-(instance, axis)-per-lane solver (lmpc_axis.hpp), shared by the translation units
// that instantiate its builds (copra_hip_axis*.hip: the entries of axis_builds.hpp) and the one that launches them (copra_hip.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "axis_builds.hpp"
#include "lmpc_axis.hpp"

using namespace copra_hip;

// One wave = 64 / NU instances x NU axes.  K, 1 / M_uu, U and the recursion's t of every stage live in registers (5 NMAX doubles), next to the
// lane's active set (S: QMAX (QMAX + 1) / 2 doubles).
#ifndef COPRA_AXIS_WAVES
#define COPRA_AXIS_WAVES 1 // waves per SIMD the register budget is cut for
#endif
template <int NXA, int NU, int NMAX, int QMAX, bool EXACT, bool CT, int RPA>
__global__ __launch_bounds__(64, COPRA_AXIS_WAVES) void copra_lmpc_axis_kernel(const FusedPlan P)
{
    lmpc_axis_body<NXA, NU, NMAX, QMAX, EXACT, CT, RPA>(P, (int)blockIdx.x);
}

// ... the builds that read per-instance cost weights (lmpc_axis.hpp, WTS)
template <int NXA, int NU, int NMAX, int QMAX, bool EXACT, bool CT, int RPA>
__global__ __launch_bounds__(64, COPRA_AXIS_WAVES) void copra_lmpc_axis_w_kernel(const FusedPlan P)
{
    lmpc_axis_body<NXA, NU, NMAX, QMAX, EXACT, CT, RPA, false, true>(P, (int)blockIdx.x);
}

// The second chance of what that launch lists: the same solver with room for kAxisQmaxBig active constraints per lane, instances taken from the
// list (a grid-stride loop over it: the launch does not know its length).  One wave per CU at most (its lanes' LDS): a handful of waves.
template <int NXA, int NU, int NMAX, int QMAX, bool CT, int RPA>
__global__ __launch_bounds__(64, 1) void copra_lmpc_axis_list_kernel(const FusedPlan P)
{
    constexpr int IPW = 64 / NU;
    const int count = *P.axis_list_count;
    for (int g = (int)blockIdx.x; g * IPW < count; g += (int)gridDim.x) {
        lmpc_axis_body<NXA, NU, NMAX, QMAX, false, CT, RPA, true>(P, g);
        __syncthreads();
    }
}
template <int NXA, int NU, int NMAX, int QMAX, bool CT, int RPA>
__global__ __launch_bounds__(64, 1) void copra_lmpc_axis_list_w_kernel(const FusedPlan P)
{
    constexpr int IPW = 64 / NU;
    const int count = *P.axis_list_count;
    for (int g = (int)blockIdx.x; g * IPW < count; g += (int)gridDim.x) {
        lmpc_axis_body<NXA, NU, NMAX, QMAX, false, CT, RPA, true, true>(P, g);
        __syncthreads();
    }
}

// The kernel of an entry of COPRA_AXIS_BUILDS, by its family (the list builds take no EXACT: false) ...
#define COPRA_AXIS_KERNEL_first(NXA, NU, NMAX, QMAX, EXACT, CT, RPA) copra_lmpc_axis_kernel<NXA, NU, NMAX, QMAX, EXACT, CT, RPA>
#define COPRA_AXIS_KERNEL_first_w(NXA, NU, NMAX, QMAX, EXACT, CT, RPA) copra_lmpc_axis_w_kernel<NXA, NU, NMAX, QMAX, EXACT, CT, RPA>
#define COPRA_AXIS_KERNEL_list(NXA, NU, NMAX, QMAX, EXACT, CT, RPA) copra_lmpc_axis_list_kernel<NXA, NU, NMAX, QMAX, CT, RPA>
#define COPRA_AXIS_KERNEL_list_w(NXA, NU, NMAX, QMAX, EXACT, CT, RPA) copra_lmpc_axis_list_w_kernel<NXA, NU, NMAX, QMAX, CT, RPA>
// ... its instantiation, in the unit that holds it: copra_hip_<UNIT>.hip defines COPRA_AXIS_UNIT_<UNIT>(...) as its arguments, the other units'
// as nothing ...
#define COPRA_AXIS_INST(UNIT, FAMILY, ...) COPRA_AXIS_UNIT_##UNIT(template __global__ void COPRA_AXIS_KERNEL_##FAMILY(__VA_ARGS__)(const FusedPlan);)
// ... and its declaration everywhere else
#define COPRA_AXIS_DECL(UNIT, FAMILY, ...) extern template __global__ void COPRA_AXIS_KERNEL_##FAMILY(__VA_ARGS__)(const FusedPlan);
