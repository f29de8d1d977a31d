// front_end.hpp -- which front end a solve may run in front of the first tier, as far as the plan and the per-solve inputs it carries decide it
// (the device_plan of a handle, or the emulator's: cost_p, cost_w, row_f_inst, lb_inst, ub_inst, the axis order's tables), and the layout a controller
// with per-instance cost weights runs on.  Read by the library (copra_hip.hip: axis_solver_wanted, lane_pass_wanted, weights_route -- which add what
// is state of the handle or of the machine) and by the CPU emulator (tests/emu/emu_harness.cpp).  Host code only.
#pragma once
#include "axis_builds.hpp"
#include "tier_builds.hpp"

namespace copra_hip {

// per-instance cost weights in the launch's plan (copra_batch_set_cost_weights): only the builds that read them may run
inline bool plan_has_weights(const FusedPlan& P)
{
    for (int t = 0; t < kMaxCosts; ++t)
        if (P.cost_w[t]) return true;
    return false;
}

// The one-(instance, axis)-per-lane solver (lmpc_axis.hpp) covers the controller with these inputs.  hp: the creation weights (HostPlan::params: P.params
// may be a device address) and the options.
inline bool axis_solver_covers(const HostPlan& hp, const FusedPlan& P)
{
    const bool weights = plan_has_weights(P);
    if (weights) { // per-instance weights: only where BOTH the solver and its second chance run builds that read them (lmpc_axis.hpp, WTS) --
        // a lane rebuilds its tables from the coefficients of FusedPlan::axis_cref divided by the creation weight, which must be non-zero, and
        // the cost's weights must repeat along the horizon (a reference-trajectory cost: the kernels read the first step's)
        if (P.axis_cref < 0 || !pick_axis_build(P.nx, P.nu, P.N, P.axis_const, P.axis_rpa, P.stage_refs, true, false)
            || !pick_axis_build(P.nx, P.nu, P.N, P.axis_const, P.axis_rpa, P.stage_refs, true, true))
            return false;
        for (int t = 0; t < P.ncost; ++t) {
            if (!P.cost_w[t]) continue;
            const CostTerm& ct = P.cost[t];
            if (ct.full) return false;
            for (int r = 0; r < ct.rows; ++r)
                if (hp.params[(size_t)ct.offW + r] == 0.0) return false;
        }
    }
    if (hp.opt.no_axis_solver || hp.opt.no_lane_pass || P.axis_tab < 0 || hp.large || P.initial_state) return false;
    // (per-instance limits: the builds that keep bounds and right-hand sides in registers, CT, take this lane's own -- where they are the same
    //  along the horizon, else the instance goes to the tier: lmpc_axis.hpp.  The other builds read the controller's, so BOTH launches must
    //  be CT ones: the second chance re-solves what the first lists, with the same limits)
    if (P.row_f_inst || P.lb_inst || P.ub_inst) {
        if (!P.axis_const || (P.lb_inst == nullptr) != (P.ub_inst == nullptr)) return false;
        const AxisBuild* const first = pick_axis_build(P.nx, P.nu, P.N, P.axis_const, P.axis_rpa, P.stage_refs, weights, false);
        const AxisBuild* const list = pick_axis_build(P.nx, P.nu, P.N, P.axis_const, P.axis_rpa, P.stage_refs, weights, true);
        if (!first || !first->ct || !list || !list->ct) return false;
    }
    for (int t = 0; t < kMaxCosts; ++t) // (per-instance references: a lane rebuilds the affine terms of its axis from them -- FusedPlan::axis_cref)
        if (P.cost_p[t] && (P.axis_cref < 0 || t >= P.ncost)) return false;
    if (P.stage_refs) { // reference trajectories: the stages' h wait in the lane's sparse array for the sweep (lmpc_axis.hpp)
        int oB = 0, oR = 0, rcs = 0;
        (void)axis_lds_doubles(P.nx, P.nu, P.N, P.axis_rpa, kAxisQmax, oB, oR, rcs);
        if (P.axis_cref < 0 || P.N * (P.nx / P.nu + 1) > rcs) return false;
    }
    return pick_axis_build(P.nx, P.nu, P.N, P.axis_const, P.axis_rpa, P.stage_refs, weights, false) != nullptr;
}

// The one-instance-per-lane pass (lmpc_lane.hpp) covers it -- in front of the Riccati-factor tier, which takes the factor over, or of any other one-wave
// first tier, where it only filters.  Whether there is a build of the pass for the shape is the caller's to ask (pick_lane, or a code object of its own).
inline bool lane_pass_covers(const HostPlan& hp, const FusedPlan& P)
{
    if (plan_has_weights(P)) return false; // (its tables hold the creation weights)
    if (hp.opt.no_lane_pass || P.lane_tab < 0 || hp.large || P.initial_state) return false;
    for (int t = 0; t < kMaxCosts; ++t)
        if (P.cost_p[t] && P.lane_cref < 0) return false; // (per-instance references: the pass rebuilds its affine terms per lane)
    return !(P.stage_refs && P.lane_cref < 0); // (reference trajectories: ... per lane and stage)
}

// Per-instance weights: the Riccati-factor tier reads its stage costs from tables the plan builder weighted with the creation weights, so a controller
// that has them runs the layout that tier's ladder ends on (adapt_layout: the compact or the full layout of the generic one-wave kernels, which evaluate
// the costs per instance).  false: the controller's own layout serves.
struct WeightsLayout {
    LdsLayout lds;
    bool two_tier, dense;
};
inline bool weights_layout(const HostPlan& hp, WeightsLayout& w)
{
    if (!hp.plan.lds.ric || hp.large || hp.plan.initial_state) return false;
    w.two_tier = hp.dense && hp.safe_two_tier && !hp.lds_safe.ric;
    w.dense = false;
    w.lds = w.two_tier ? hp.lds_safe : hp.lds_full;
    return true;
}

} // namespace copra_hip
