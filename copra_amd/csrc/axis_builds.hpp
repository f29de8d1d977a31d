// axis_builds.hpp -- the builds of the one-(instance, axis)-per-lane solver (lmpc_axis.hpp) and the rule that picks a controller's.  One list,
// read by the translation units that instantiate the builds (copra_hip_axis*.hip: each its own entries), by the library that launches them
// (copra_hip.hip: select_axis_kernel, select_axis_list_kernel) and by the CPU emulator that runs their bodies (tests/emu/emu_harness.cpp).
// Host code only.  (The builds of the other tiers: tier_builds.hpp; whether the solver runs at all: front_end.hpp, axis_solver_covers.)
#pragma once
#include "plan_builder.hpp" // axis_solver_nmax, kAxisQmax, kAxisQmaxBig

namespace copra_hip {

// X(UNIT, FAMILY, NXA, NU, NMAX, QMAX, EXACT, CT, RPA): one build.  UNIT: the translation unit copra_hip_<UNIT>.hip that instantiates it.
// FAMILY: first -- the first launch, copra_lmpc_axis_kernel --, first_w -- the same with per-instance cost weights (WTS), copra_lmpc_axis_w_kernel --,
// list -- the second chance of what the first launch lists, copra_lmpc_axis_list_kernel -- and list_w.  NXA states per axis, NU axes, horizons
// up to NMAX (axis_solver_nmax), QMAX active constraints per lane; EXACT: the horizon NMAX compiled in; CT: the tables in registers
// (FusedPlan::axis_const); RPA: constraint rows per axis and step it takes.
#define COPRA_AXIS_BUILDS(X)                                                                                                                   \
    /* chains of two states per control: the headline's horizon exactly, every horizon up to 20 and -- two axes -- up to 31; the tables in */ \
    /* registers with one and with two rows per axis and step, or read from LDS stage by stage */                                              \
    X(axis, first, 2, 3, 20, kAxisQmax, true, true, 1)                                                                                         \
    X(axis, first, 2, 3, 20, kAxisQmax, false, true, 1)                                                                                        \
    X(axis, first, 2, 2, 20, kAxisQmax, false, true, 1)                                                                                        \
    X(axis, first, 2, 2, 31, kAxisQmax, false, true, 1)                                                                                        \
    X(axis, first, 2, 3, 20, kAxisQmax, true, true, 2)                                                                                         \
    X(axis, first, 2, 3, 20, kAxisQmax, false, true, 2)                                                                                        \
    X(axis, first, 2, 2, 20, kAxisQmax, false, true, 2)                                                                                        \
    X(axis, first, 2, 2, 31, kAxisQmax, false, true, 2)                                                                                        \
    X(axis, first, 2, 3, 20, kAxisQmax, false, false, 2)                                                                                       \
    X(axis, first, 2, 2, 20, kAxisQmax, false, false, 2)                                                                                       \
    X(axis, first, 2, 2, 31, kAxisQmax, false, false, 2)                                                                                       \
    X(axis, list, 2, 3, 20, kAxisQmaxBig, false, true, 2)                                                                                      \
    X(axis, list, 2, 2, 20, kAxisQmaxBig, false, true, 2)                                                                                      \
    X(axis, list, 2, 2, 31, kAxisQmaxBig, false, true, 2)                                                                                      \
    X(axis, list, 2, 3, 20, kAxisQmaxBig, false, false, 2)                                                                                     \
    X(axis, list, 2, 2, 20, kAxisQmaxBig, false, false, 2)                                                                                     \
    X(axis, list, 2, 2, 31, kAxisQmaxBig, false, false, 2)                                                                                     \
    /* one state per control (kinematic models) in two dimensions up to 31 steps and in two and three up to 20; chains of two states in */    \
    /* three dimensions at N = 21; chains of THREE states per control (the jerk-controlled CoM model) in two and three dimensions: the */      \
    /* tables in registers with one row per axis and step, or read from LDS */                                                                \
    X(axis3, first, 1, 2, 31, kAxisQmax, false, true, 1)                                                                                       \
    X(axis3, first, 1, 2, 31, kAxisQmax, false, false, 2)                                                                                      \
    X(axis3, first, 1, 2, 20, kAxisQmax, false, true, 1)                                                                                       \
    X(axis3, first, 1, 2, 20, kAxisQmax, false, false, 2)                                                                                      \
    X(axis3, first, 1, 3, 20, kAxisQmax, false, true, 1)                                                                                       \
    X(axis3, first, 1, 3, 20, kAxisQmax, false, false, 2)                                                                                      \
    X(axis3, first, 2, 3, 21, kAxisQmax, false, true, 1)                                                                                       \
    X(axis3, first, 2, 3, 21, kAxisQmax, false, false, 2)                                                                                      \
    X(axis3, first, 3, 2, 20, kAxisQmax, false, true, 1)                                                                                       \
    X(axis3, first, 3, 2, 20, kAxisQmax, false, false, 2)                                                                                      \
    X(axis3, first, 3, 3, 20, kAxisQmax, false, true, 1)                                                                                       \
    X(axis3, first, 3, 3, 20, kAxisQmax, false, false, 2)                                                                                      \
    X(axis3, list, 1, 2, 31, kAxisQmaxBig, false, false, 2)                                                                                    \
    X(axis3, list, 1, 2, 20, kAxisQmaxBig, false, false, 2)                                                                                    \
    X(axis3, list, 1, 3, 20, kAxisQmaxBig, false, false, 2)                                                                                    \
    X(axis3, list, 2, 3, 21, kAxisQmaxBig, false, false, 2)                                                                                    \
    X(axis3, list, 3, 2, 20, kAxisQmaxBig, false, false, 2)                                                                                    \
    X(axis3, list, 3, 3, 20, kAxisQmaxBig, false, false, 2)                                                                                    \
    /* per-instance cost weights (copra_batch_set_cost_weights): the headline's shape, the first launch with its tables in registers */       \
    X(axis_w, first_w, 2, 3, 20, kAxisQmax, true, true, 1)                                                                                     \
    X(axis_w, first_w, 2, 3, 20, kAxisQmax, true, true, 2)                                                                                     \
    X(axis_w, first_w, 2, 3, 20, kAxisQmax, false, true, 1)                                                                                    \
    X(axis_w, first_w, 2, 3, 20, kAxisQmax, false, true, 2)                                                                                    \
    X(axis_w, list_w, 2, 3, 20, kAxisQmaxBig, false, true, 2)                                                                                  \
    X(axis_w, list_w, 2, 3, 20, kAxisQmaxBig, false, false, 2)

enum class AxisFamily { first, first_w, list, list_w };
struct AxisBuild {
    AxisFamily family;
    int nxa, nu, nmax, qmax;
    bool exact, ct;
    int rpa;
};
#define COPRA_AXIS_ENTRY(UNIT, FAMILY, NXA, NU, NMAX, QMAX, EXACT, CT, RPA) { AxisFamily::FAMILY, NXA, NU, NMAX, QMAX, EXACT, CT, RPA },
inline constexpr AxisBuild kAxisBuilds[] = { COPRA_AXIS_BUILDS(COPRA_AXIS_ENTRY) };
#undef COPRA_AXIS_ENTRY

// The build a controller gets: of the family asked for, the entries of its shape (nx / nu states per axis, nu axes, the largest horizon of its
// builds: axis_solver_nmax) that can run it -- EXACT only at that horizon and without reference trajectories, CT only where the tables are the
// same at every step, room for its rows per axis and step --; of those the one with the horizon compiled in, then the one with its tables in
// registers, then the one with the fewest rows.  nullptr: the library holds none.  (Several calls per solve: no allocation, no lock.)
inline const AxisBuild* pick_axis_build(int nx, int nu, int N, bool axis_const, int axis_rpa, bool stage_refs, bool weights, bool list)
{
    const int nmax = axis_solver_nmax(nx, nu, N);
    if (nmax == 0) return nullptr;
    const AxisFamily family = list ? (weights ? AxisFamily::list_w : AxisFamily::list) : (weights ? AxisFamily::first_w : AxisFamily::first);
    const int rpa = axis_rpa > 1 ? axis_rpa : 1;
    auto better = [](const AxisBuild& a, const AxisBuild& b) { return a.exact != b.exact ? a.exact : a.ct != b.ct ? a.ct : a.rpa < b.rpa; };
    const AxisBuild* pick = nullptr;
    for (const AxisBuild& b : kAxisBuilds) {
        if (b.family != family || b.nxa != nx / nu || b.nu != nu || b.nmax != nmax) continue;
        if ((b.exact && (N != nmax || stage_refs)) || (b.ct && !axis_const) || b.rpa < rpa) continue;
        if (!pick || better(b, *pick)) pick = &b;
    }
    return pick;
}

} // namespace copra_hip
