// tier_builds.hpp -- the builds of the one-wave tiers and of the one-instance-per-lane pass, and the rules that pick a controller's.  One list per
// selector of copra_hip.hip (select_fused_kernel, select_tier2_kernel, select_lane_kernel, select_lane_shared_kernel, select_shared_kernel), read by
// the library that launches the builds, by copra_hip_ric.hip that instantiates some of them, and by the CPU emulator that runs their bodies
// (tests/emu/emu_harness.cpp) -- as axis_builds.hpp is for the (instance, axis)-per-lane solver.  Host code only.
#pragma once
#include "plan_builder.hpp" // ric_aot_shape, ric_aot_exact, specialised_cost_rows

namespace copra_hip {

// UNIT in every list: the translation unit that instantiates the build: core -- copra_hip.hip, where it is launched -- or ric -- copra_hip_ric.hip.

// First tier.  X(UNIT, KIND, NX, NU, NH, RP, QR, SREFS).  KIND: ric -- the Riccati-factor tier, copra_lmpc_fused_ric_kernel<NX, NU, NH, QR, SREFS>: QR columns
// of Q1 in registers, SREFS stage references --, tri -- the factor-only tier, copra_lmpc_fused_tri_kernel<NX, NU, NH, RP, QR> --, square -- the
// square layout, copra_lmpc_fused_kernel<NX, NU, NH, RP> -- and w4 -- copra_lmpc_fused_kernel_w4, the generic body at four waves per SIMD.
// <0, 0, 0, 0>: the run-time shape; NH == 0 alone: the run-time horizon of the shapes of ric_aot_shape; RP: padded cost rows (0: as the plan has them).
#define COPRA_RIC_BUILDS_OF(X, UNIT, NX, NU, NH)                                                                                             \
    X(UNIT, ric, NX, NU, NH, 6, kFusedQ1Regs, false) X(UNIT, ric, NX, NU, NH, 6, 0, false) X(UNIT, ric, NX, NU, NH, 6, kFusedQ1Regs, true) X(UNIT, ric, NX, NU, NH, 6, 0, true)
#define COPRA_FIRST_TIER_BUILDS(X)                                                                                                           \
    COPRA_RIC_BUILDS_OF(X, core, 6, 3, 10) COPRA_RIC_BUILDS_OF(X, core, 6, 3, 15) COPRA_RIC_BUILDS_OF(X, core, 6, 3, 20)                     \
    COPRA_RIC_BUILDS_OF(X, ric, 6, 3, 0) COPRA_RIC_BUILDS_OF(X, ric, 4, 2, 0) COPRA_RIC_BUILDS_OF(X, ric, 2, 1, 0)                           \
    /* the headline shape with its six cost rows and with full-size costs, Q1 in registers or in LDS; every other shape */                  \
    X(core, tri, 6, 3, 20, 6, kFusedQ1Regs, false) X(core, tri, 6, 3, 20, 6, 0, false)                                                       \
    X(core, tri, 6, 3, 20, 0, kFusedQ1Regs, false) X(core, tri, 6, 3, 20, 0, 0, false) X(core, tri, 0, 0, 0, 0, 0, false)                     \
    /* the BASELINE.json shapes; generic shapes whose layout lets more than eight share a CU, and the others */                             \
    X(core, square, 6, 3, 20, 6, 0, false) X(core, square, 2, 1, 10, 2, 0, false) X(core, square, 6, 3, 20, 0, 0, false)                     \
    X(core, w4, 0, 0, 0, 0, 0, false) X(core, square, 0, 0, 0, 0, 0, false)
// Second tier, copra_lmpc_fused_tier2_kernel<NX, NU, NH, RP>.  X(UNIT, NX, NU, NH, RP)
#define COPRA_SECOND_TIER_BUILDS(X) X(core, 6, 3, 20, 6) X(core, 2, 1, 10, 2) X(core, 6, 3, 20, 0) X(core, 0, 0, 0, 0)
// The one-instance-per-lane pass, copra_lmpc_lane_kernel<NX, NU, SREFS, SPEC>: the CoM system, the reference's falling mass (BASELINE configs[1]), a
// planar point mass; SPEC: it takes the first steps of the iteration itself (FusedPlan::lane_spec).  X(UNIT, NX, NU, SREFS, SPEC)
#define COPRA_LANE_BUILDS_OF(X, UNIT, NX, NU) X(UNIT, NX, NU, false, true) X(UNIT, NX, NU, true, true) X(UNIT, NX, NU, false, false) X(UNIT, NX, NU, true, false)
#define COPRA_LANE_BUILDS(X) COPRA_LANE_BUILDS_OF(X, core, 6, 3) COPRA_LANE_BUILDS_OF(X, core, 2, 1) COPRA_LANE_BUILDS_OF(X, ric, 4, 2)
// ... and its shared-model form, copra_lmpc_lane_shared_kernel<NX, NU, SPEC>: the shapes of the tier's run-time-horizon builds.  X(UNIT, NX, NU, SPEC)
#define COPRA_LANE_SHARED_BUILDS(X) X(core, 6, 3, true) X(core, 6, 3, false) X(core, 4, 2, true) X(core, 4, 2, false) X(core, 2, 1, true) X(core, 2, 1, false)
// The shared-model kernels (lmpc_shared.hpp).  X(UNIT, KIND, NX, NU, NH).  KIND: tri -- copra_lmpc_shared_tri_kernel, the factor-only first tier --, first --
// copra_lmpc_shared_kernel --, w4 -- copra_lmpc_shared_kernel_w4 -- and tier2 -- copra_lmpc_shared_tier2_kernel.
#define COPRA_SHARED_BUILDS(X)                                                                                                               \
    X(core, tri, 6, 3, 20) X(core, tri, 0, 0, 0) X(core, first, 6, 3, 20) X(core, first, 2, 1, 10) X(core, w4, 0, 0, 0) X(core, first, 0, 0, 0) \
    X(core, tier2, 6, 3, 20) X(core, tier2, 2, 1, 10) X(core, tier2, 0, 0, 0)

// An entry of any of the lists: the fields its list does not have are zero
enum class TierKind { ric, tri, square, w4, second, lane, lane_shared, shared_tri, shared_first, shared_w4, shared_tier2 };
struct TierBuild {
    TierKind kind;
    int nx, nu, nh, rp, qr;
    bool srefs, spec;
    bool operator==(const TierBuild& o) const { return kind == o.kind && nx == o.nx && nu == o.nu && nh == o.nh && rp == o.rp && qr == o.qr && srefs == o.srefs && spec == o.spec; }
};
#define COPRA_FIRST_ENTRY(UNIT, KIND, NX, NU, NH, RP, QR, SREFS) { TierKind::KIND, NX, NU, NH, RP, QR, SREFS, false },
#define COPRA_SECOND_ENTRY(UNIT, NX, NU, NH, RP) { TierKind::second, NX, NU, NH, RP, 0, false, false },
#define COPRA_LANE_ENTRY(UNIT, NX, NU, SREFS, SPEC) { TierKind::lane, NX, NU, 0, 0, 0, SREFS, SPEC },
#define COPRA_LANE_SHARED_ENTRY(UNIT, NX, NU, SPEC) { TierKind::lane_shared, NX, NU, 0, 0, 0, false, SPEC },
#define COPRA_SHARED_ENTRY(UNIT, KIND, NX, NU, NH) { TierKind::shared_##KIND, NX, NU, NH, 0, 0, false, false },
inline constexpr TierBuild kFirstTierBuilds[] = { COPRA_FIRST_TIER_BUILDS(COPRA_FIRST_ENTRY) };
inline constexpr TierBuild kSecondTierBuilds[] = { COPRA_SECOND_TIER_BUILDS(COPRA_SECOND_ENTRY) };
inline constexpr TierBuild kLaneBuilds[] = { COPRA_LANE_BUILDS(COPRA_LANE_ENTRY) };
inline constexpr TierBuild kLaneSharedBuilds[] = { COPRA_LANE_SHARED_BUILDS(COPRA_LANE_SHARED_ENTRY) };
inline constexpr TierBuild kSharedBuilds[] = { COPRA_SHARED_BUILDS(COPRA_SHARED_ENTRY) };

// the entry of a list with these fields; nullptr: the list holds none.  (Several calls per solve: no allocation, no lock.)
template <size_t K>
inline const TierBuild* find_build(const TierBuild (&list)[K], const TierBuild& want)
{
    for (const TierBuild& b : list)
        if (b == want) return &b;
    return nullptr;
}

// does the run-time-shape body put more than eight instances on a CU?  (the _w4 kernels: four waves per SIMD)
inline bool more_than_eight_per_cu(const FusedPlan& P) { return (size_t)P.lds.total * sizeof(double) * 9 <= 160u * 1024u; }

// The first tier of a plan with this layout; every return names its entry.  specialised = false (the emulator's use_specialised = 0 only): the
// run-time-shape build for a shape that has a build of its own.
inline const TierBuild* pick_first_tier(const FusedPlan& P, bool specialised = true)
{
    auto entry = [](TierKind kind, int nx, int nu, int nh, int rp, int qr, bool srefs = false) { return find_build(kFirstTierBuilds, { kind, nx, nu, nh, rp, qr, srefs, false }); };
    const int rp = specialised ? specialised_cost_rows(P.nx, P.nu, P.N, P.rmax, P.rfull) : 0;
    const bool full = specialised && P.rfull > 0 && P.nx == 6 && P.nu == 3 && P.N == 20; // headline shape, full-size costs
    const int q = P.lds.q1regs == kFusedQ1Regs ? kFusedQ1Regs : 0;
    if (P.lds.tri) {
        if (P.lds.ric) { // (plan_builder.hpp: only these shapes get the layout -- one that copra_batch_specialise gave it launches its own code object, and
            // is answered with a (6, 3) build nobody launches --; Q1 in registers, or in LDS further down the ladder; SREFS: reference trajectories)
            const int rq = P.lds.q1regs ? kFusedQ1Regs : 0;
            if (!ric_aot_exact(P.nx, P.nu, P.N) && ric_aot_shape(P.nx, P.nu)) return entry(TierKind::ric, P.nx, P.nu, 0, 6, rq, P.stage_refs != 0); // run-time horizon (copra_hip_ric.hip)
            return entry(TierKind::ric, 6, 3, P.N == 10 || P.N == 15 ? P.N : 20, 6, rq, P.stage_refs != 0);
        }
        if (P.nx == 6 && rp == 6) return entry(TierKind::tri, 6, 3, 20, 6, q);
        if (full) return entry(TierKind::tri, 6, 3, 20, 0, q);
        return entry(TierKind::tri, 0, 0, 0, 0, 0);
    }
    if (P.nx == 6 && rp == 6) return entry(TierKind::square, 6, 3, 20, 6, 0);
    if (P.nx == 2 && rp == 2) return entry(TierKind::square, 2, 1, 10, 2, 0);
    if (full) return entry(TierKind::square, 6, 3, 20, 0, 0);
    if (more_than_eight_per_cu(P)) return entry(TierKind::w4, 0, 0, 0, 0, 0);
    return entry(TierKind::square, 0, 0, 0, 0, 0);
}
inline const TierBuild* pick_second_tier(const FusedPlan& P, bool specialised = true)
{
    auto entry = [](int nx, int nu, int nh, int rp) { return find_build(kSecondTierBuilds, { TierKind::second, nx, nu, nh, rp, 0, false, false }); };
    const int rp = specialised ? specialised_cost_rows(P.nx, P.nu, P.N, P.rmax, P.rfull) : 0;
    if (P.nx == 6 && rp == 6) return entry(6, 3, 20, 6);
    if (P.nx == 2 && rp == 2) return entry(2, 1, 10, 2);
    if (specialised && P.rfull > 0 && P.nx == 6 && P.nu == 3 && P.N == 20) return entry(6, 3, 20, 0);
    return entry(0, 0, 0, 0);
}
// The pass of a shape, in the form FusedPlan::lane_spec asks for; nullptr: the library holds none for the shape
inline const TierBuild* pick_lane(const FusedPlan& P) { return find_build(kLaneBuilds, { TierKind::lane, P.nx, P.nu, 0, 0, 0, P.stage_refs != 0, P.lane_spec != 0 }); }
inline const TierBuild* pick_lane_shared(const FusedPlan& P) { return find_build(kLaneSharedBuilds, { TierKind::lane_shared, P.nx, P.nu, 0, 0, 0, false, P.lane_spec != 0 }); }
inline const TierBuild* pick_shared(const FusedPlan& P, bool tier2)
{
    auto entry = [&](TierKind first, int nx, int nu, int nh) { return find_build(kSharedBuilds, { tier2 ? TierKind::shared_tier2 : first, nx, nu, nh, 0, 0, false, false }); };
    const bool head = P.nx == 6 && P.nu == 3 && P.N == 20;
    if (P.lds.tri && !tier2) return head ? entry(TierKind::shared_tri, 6, 3, 20) : entry(TierKind::shared_tri, 0, 0, 0);
    if (head) return entry(TierKind::shared_first, 6, 3, 20);
    if (P.nx == 2 && P.nu == 1 && P.N == 10) return entry(TierKind::shared_first, 2, 1, 10);
    if (!tier2 && more_than_eight_per_cu(P)) return entry(TierKind::shared_w4, 0, 0, 0);
    return entry(TierKind::shared_first, 0, 0, 0);
}

} // namespace copra_hip
