// plant_step.hpp -- the second half of a receding-horizon tick, on the device: apply the first control of the last solve to a plant and make the
// result the next initial state (copra_batch_advance / copra_batch_rollout, copra_hip_plant.hip).  Replaces the reference's
//   u = lmpc.control().head(nu);  x = plant(x, u);  ps->xInit(x);            (include/LMPC.h:108, include/PreviewSystem.h:52)
// for every instance b of the batch:
//   ok = status[b] == COPRA_QP_OK;   u = ok ? control[b][0 .. nu) : fallback_u ? fallback_u[b] : none
//   x+ = (ok || fallback_u) ? Ap[b] x0[b] + Bp[b] u + dp[b] (+ w[b]) : x0[b]            (no fallback: the state is HELD, bit for bit)
// A failed instance's control holds NaN: the status is looked at FIRST, the control of a failed instance is never loaded.
// With backup plans (copra_batch_set_backup_steps, K = backup_steps > 0) an instance without a fresh solution plays the tail of its last plan
// that did solve before it falls back or is held; per instance the store is plan[b][K][nu] and next[b] (0: no plan, > K: used up):
//   fresh && status[b] == COPRA_QP_OK : u = control[b][0 .. nu);  plan[b] = control[b][nu .. (K + 1) nu);  next[b] = 1;  age 0
//   else 1 <= next[b] <= K            : u = plan[b][next[b] - 1];  age = next[b];  next[b] += 1
//   else                              : fallback_u[b] (age -1) or held (age -2) as above, next[b] unchanged
// next[b] is READ in phase 1 (by the nu threads that fetch the instance's control) and WRITTEN in phase 2, behind the barrier, by the one
// thread that owns the instance; the age found in phase 1 goes through the LDS image beside the status.  An instance that reads plan[b] never
// writes it in the same tick.  backup_steps == 0 takes the bodies below with kBackup = false: the image, the copies and the sums of ABI 9.
//
// A streaming kernel (about 600 B read, 50-130 B written per instance at xDim 6, uDim 3).  One workgroup takes `group` consecutive instances:
// their A, B, d, x0, w blocks are ONE contiguous range per array, copied into LDS with wide coalesced loads (16 B per lane where the
// pointers allow it); then one thread per (instance, row) forms its sum from LDS and the new states leave as one contiguous range again.
// No lane walks a column with stride nx in global memory; only `control` is read with its stride nu N (its first nu entries).  No scratch, no
// atomics, nothing depends on the grid beyond the bounds of the last group.  In place (x0_next == x0) is the normal case: an instance belongs
// to one workgroup, whose old states are all in LDS (phase 1) before the barrier that precedes the first store (phase 2).
//
// The two phases are COPRA_DEV functions of (workgroup, thread) that also compile on the host: tests/emu/emu_plant.cpp walks them thread by
// thread with a host buffer in the place of LDS.
//
// The disturbance estimator (copra_batch_set_bias_estimator, PlantStepArgs::est) adds a third phase to the same kernel, built with kEst = true;
// est == 0 launches the kernel built with kEst = false: the two phases, the image and the copies above, nothing else.  With dhat the
// controller's d (the buffer the next solve reads), Am / Bm the controller's MODEL of the instance and u the control this tick applied:
//   pred_r = dhat_r + sum_j Am[r,j] x_j + sum_c Bm[r,c] u_c      (no w);      e_r = x+_r - pred_r
//   dhat+_r = dhat_r + sum_j L[r,j] e_j  (dense gain, column-major)    |    dhat_r + l_r e_r  (diagonal gain);      d_out = dhat+
// and an instance whose state is held keeps dhat bit for bit.  Phase 1 also stages Am, Bm, dhat and the gain -- with no plant of its own the
// plant IS the model with d = dhat: A, B, d are then the same arrays and are staged once (same_model); a gain shared by the batch once per
// workgroup.  Phase 2 leaves x+ in LDS as well.  Phase 3 (plant_estimate, behind the second barrier) forms e per (instance, row) into LDS;
// the dense gain reads all rows' e of its instance, so the update (plant_estimate_store) stands behind a third barrier and stores dhat and
// d_out as one contiguous range per group.  dhat is updated in place: every read of it is into LDS in phase 1, one workgroup owns an instance.
//
// The state observer (copra_batch_set_observer, PlantObsArgs) is a third build, copra_plant_observer_kernel: the two phases of the tick on the
// plant's OWN state xp, then the innovation of ny measured outputs and the update of the estimate xhat (the controller's x0) and, optionally,
// of dhat -- its rule, image and phases stand in front of its code below.  The two builds above do not know of it.
//
// Noise drawn on the device (copra_batch_set_noise, ABI 13; plant_noise.hpp): with kNoise phase 1 fills the w slot of the image -- and the
// observer's yv slot -- from a counter-based generator, w = (w given ? w : 0) + sigma_w n, one thread per pair of rows, which reads the given
// w of its two rows itself (no barrier between a copy and the sum).  kNoise is a template value of every phase and of the kernels: the builds
// without it hold none of the generator's code and never load the sigmas -- they are the code of ABI 12; plant_has_w / plant_obs_has_yv say
// for every build whether the image has the slot.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "plant_noise.hpp"

#ifndef COPRA_DEV
#if defined(__HIPCC__)
#define COPRA_DEV __device__ __forceinline__
#else
#define COPRA_DEV inline
#endif
#endif

#if defined(__HIPCC__)
#define COPRA_PLANT_HD __host__ __device__ inline // (the launch sizes the LDS image with the function the kernel lays it out with)
#else
#define COPRA_PLANT_HD inline
#endif

namespace copra_hip {

struct PlantStepArgs {
    int batch, nx, nu;
    int ctrl_stride; // doubles between two instances' controls: nu N
    int group; // instances per workgroup (even wherever vec2 is set)
    int shared; // A, B, d hold ONE system for the batch
    int vec2; // every pointer below is 16-byte aligned and every group's range starts on 16 bytes: copy two doubles per lane and load
    const double *A, *B, *d; // the plant, layout of copra_batch_set_system
    const double* x0; // [batch][nx]
    const double* w; // [batch][nx] or null
    const double* fallback_u; // [batch][nu] or null
    const int* status; // [batch], of the last launched solve
    const double* control; // [batch][ctrl_stride], of the last launched solve
    double* x0_next; // [batch][nx]; may be x0
    double *x_out, *u_out; // optional copies
    int* status_out;
    int backup_steps; // K: controls of horizon steps 1 .. K kept per instance; 0: no backup plans (plan, next, fresh are not looked at)
    int fresh; // a solve has been launched since the previous plant step: status / control are of THIS tick
    double* plan; // [batch][backup_steps][nu]
    int* next; // [batch]: the step of plan[b] the next tick without a fresh solution applies; 0: no plan yet, > backup_steps: used up
    int* age_out; // optional [batch]: 0 fresh solution | j >= 1 step j of the plan | kPlantAgeFallback | kPlantAgeHeld
    int est; // the disturbance estimator is on (everything below is looked at only then)
    int same_model; // no plant of its own: A, B ARE the model and d IS dhat (per instance, never `shared`); Am, Bm are not looked at
    int gain_dense, gain_shared; // gain: [nx x nx] column-major | [nx];  one for the batch | one per instance
    const double *Am, *Bm; // the controller's model, [batch][nx x nx], [batch][nx x nu]
    const double* gain;
    double* dhat; // [batch][nx]: the controller's d, read in phase 1, written behind the last barrier
    double* d_out; // optional [batch][nx]: a copy of the new estimates
    // noise drawn on the device (plant_noise.hpp; all zero: off -- the builds without kNoise never look at them)
    const double* sigma_w; // [nx] or [batch][nx]: process noise, w = (w given ? w : 0) + sigma_w n; null: none
    int sigma_per_instance; // sigma_w (and the observer's sigma_v) hold one block per instance
    NoiseGen noise; // seed, global index of instance 0, noise tick
};

// whether the image has a w slot: a w is given or process noise is drawn -- what every caller of the layout functions passes as has_w.
// kNoise = false is the answer of the builds without noise, which are launched only while sigma_w is null and do not load it
template <bool kNoise = true>
COPRA_PLANT_HD bool plant_has_w(const PlantStepArgs& P) { return P.w != nullptr || (kNoise && P.sigma_w != nullptr); }

constexpr int kPlantAgeFallback = -1, kPlantAgeHeld = -2; // (COPRA_PLAN_FALLBACK, COPRA_PLAN_HELD of include/copra_hip.h)

struct alignas(16) PlantPair {
    double a, b;
};

// (host) whether a launch may copy two doubles per lane: an even group -- every group's range then starts on 16 bytes -- and aligned arrays
inline bool plant_vec2_ok(const PlantStepArgs& P)
{
    const auto ok = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    if (P.est && !(ok(P.Am) && ok(P.Bm) && ok(P.gain) && ok(P.dhat))) return false;
    return P.group % 2 == 0 && ok(P.A) && ok(P.B) && ok(P.d) && ok(P.x0) && ok(P.w);
}

COPRA_PLANT_HD int plant_even(int v) { return (v + 1) & ~1; }

// LDS image of one workgroup, in doubles: A | B | d | x0 | w | u | status (ints) [| age (ints), with backup plans]; every part starts on 16 bytes
struct PlantLds {
    int oA, oB, od, ox, ow, ou, ost, total, oag;
};
COPRA_PLANT_HD PlantLds plant_lds(int nx, int nu, int group, int shared, int has_w, int backup = 0)
{
    const int gs = shared ? 1 : group;
    PlantLds L;
    L.oA = 0;
    L.oB = L.oA + plant_even(gs * nx * nx);
    L.od = L.oB + plant_even(gs * nx * nu);
    L.ox = L.od + plant_even(gs * nx);
    L.ow = L.ox + plant_even(group * nx);
    L.ou = L.ow + (has_w ? plant_even(group * nx) : 0);
    L.ost = L.ou + plant_even(group * nu);
    L.total = L.ost + plant_even((group + 1) / 2);
    L.oag = L.total;
    if (backup) L.total += plant_even((group + 1) / 2);
    return L;
}

// ... and with the estimator, behind it: [Am | Bm | dhat, with a plant of its own] | gain | x+ | e; with same_model dhat is the image's d
struct PlantEstLds {
    PlantLds base;
    int oAm, oBm, odh, oG, oxn, oe, total;
};
COPRA_PLANT_HD PlantEstLds plant_est_lds(int nx, int nu, int group, int shared, int has_w, int backup, int same_model, int gain_dense, int gain_shared)
{
    PlantEstLds E;
    E.base = plant_lds(nx, nu, group, shared, has_w, backup);
    int o = E.base.total;
    E.oAm = E.base.oA, E.oBm = E.base.oB, E.odh = E.base.od;
    if (!same_model) {
        E.oAm = o, o += plant_even(group * nx * nx);
        E.oBm = o, o += plant_even(group * nx * nu);
        E.odh = o, o += plant_even(group * nx);
    }
    E.oG = o, o += plant_even((gain_shared ? 1 : group) * (gain_dense ? nx * nx : nx));
    E.oxn = o, o += plant_even(group * nx);
    E.oe = o, o += plant_even(group * nx);
    E.total = o;
    return E;
}
template <bool kNoise = false>
COPRA_DEV PlantEstLds plant_est_lds(const PlantStepArgs& P, int backup)
{
    return plant_est_lds(P.nx, P.nu, P.group, P.shared, plant_has_w<kNoise>(P), backup, P.same_model, P.gain_dense, P.gain_shared);
}

// dst[0 .. count) = src[0 .. count), thread `tid` of `T`: consecutive lanes, consecutive addresses
COPRA_DEV void plant_copy(double* dst, const double* src, int count, int tid, int T, int vec2)
{
    if (vec2) {
        const int pairs = count >> 1;
        const PlantPair* s2 = reinterpret_cast<const PlantPair*>(src);
        PlantPair* d2 = reinterpret_cast<PlantPair*>(dst);
        for (int e = tid; e < pairs; e += T) d2[e] = s2[e];
        if ((count & 1) && tid == 0) dst[count - 1] = src[count - 1];
    } else {
        for (int e = tid; e < count; e += T) dst[e] = src[e];
    }
}

// row r of  A x + B u + d (+ w)  for one instance: A [nx x nx], B [nx x nu] column-major
COPRA_DEV double plant_row(int nx, int nu, int r, const double* A, const double* B, const double* d, const double* w, const double* x, const double* u)
{
    double acc = d[r];
    for (int j = 0; j < nx; ++j) acc += A[r + nx * j] * x[j];
    for (int c = 0; c < nu; ++c) acc += B[r + nx * c] * u[c];
    if (w) acc += w[r];
    return acc;
}

// where instance b's control of this tick comes from (backup plans): 0, the step of its plan, kPlantAgeFallback or kPlantAgeHeld
COPRA_DEV int plant_age(const PlantStepArgs& P, size_t b)
{
    if (P.fresh && P.status[b] == 0) return 0;
    const int nxt = P.next[b];
    if (nxt >= 1 && nxt <= P.backup_steps) return nxt;
    return P.fallback_u ? kPlantAgeFallback : kPlantAgeHeld;
}

// phase 1: everything workgroup `wg` reads, into its image `lds`
template <bool kBackup, bool kEst = false, bool kNoise = false>
COPRA_DEV void plant_stage_body(const PlantStepArgs& P, int wg, int tid, int T, double* lds)
{
    const int nx = P.nx, nu = P.nu, b0 = wg * P.group;
    const int cnt = (P.batch - b0 < P.group) ? P.batch - b0 : P.group;
    if (cnt <= 0) return;
    const PlantLds L = plant_lds(nx, nu, P.group, P.shared, plant_has_w<kNoise>(P), kBackup);
    const size_t s0 = P.shared ? 0 : (size_t)b0;
    const int scnt = P.shared ? 1 : cnt;
    plant_copy(lds + L.oA, P.A + s0 * nx * nx, scnt * nx * nx, tid, T, P.vec2);
    plant_copy(lds + L.oB, P.B + s0 * nx * nu, scnt * nx * nu, tid, T, P.vec2);
    plant_copy(lds + L.od, P.d + s0 * nx, scnt * nx, tid, T, P.vec2);
    plant_copy(lds + L.ox, P.x0 + (size_t)b0 * nx, cnt * nx, tid, T, P.vec2);
    if (kNoise && P.sigma_w) // (the thread that draws a pair reads the given w of its two rows itself: no barrier between a copy and the sum)
        noise_stage(P.noise, 0, P.sigma_w, P.sigma_per_instance, P.w, (size_t)b0, cnt, nx, lds + L.ow, tid, T);
    else if (P.w) plant_copy(lds + L.ow, P.w + (size_t)b0 * nx, cnt * nx, tid, T, P.vec2);
    int* st = reinterpret_cast<int*>(lds + L.ost);
    for (int i = tid; i < cnt; i += T) st[i] = P.status[b0 + i];
    if (kBackup) {
        int* ag = reinterpret_cast<int*>(lds + L.oag);
        for (int i = tid; i < cnt; i += T) ag[i] = plant_age(P, (size_t)b0 + i);
    }
    for (int e = tid; e < cnt * nu; e += T) { // the control that is applied: the status decides BEFORE anything of `control` is touched
        const int i = e / nu, c = e - i * nu;
        const size_t b = (size_t)b0 + i;
        double u = NAN;
        if (kBackup) { // (next[b] is only read here: its new value is written behind the barrier)
            const int age = plant_age(P, b);
            if (age == 0) u = P.control[b * P.ctrl_stride + c];
            else if (age > 0) u = P.plan[(b * P.backup_steps + (age - 1)) * nu + c];
            else if (age == kPlantAgeFallback) u = P.fallback_u[b * nu + c];
        } else {
            if (P.status[b] == 0) u = P.control[b * P.ctrl_stride + c];
            else if (P.fallback_u) u = P.fallback_u[b * nu + c];
        }
        lds[L.ou + e] = u;
    }
    if (kEst) { // the model, the estimates and the gain (same_model: A, B, d above were the model and the estimates)
        const PlantEstLds E = plant_est_lds<kNoise>(P, kBackup);
        if (!P.same_model) {
            plant_copy(lds + E.oAm, P.Am + (size_t)b0 * nx * nx, cnt * nx * nx, tid, T, P.vec2);
            plant_copy(lds + E.oBm, P.Bm + (size_t)b0 * nx * nu, cnt * nx * nu, tid, T, P.vec2);
            plant_copy(lds + E.odh, P.dhat + (size_t)b0 * nx, cnt * nx, tid, T, P.vec2);
        }
        const int g1 = P.gain_dense ? nx * nx : nx;
        plant_copy(lds + E.oG, P.gain + (P.gain_shared ? 0 : (size_t)b0 * g1), (P.gain_shared ? 1 : cnt) * g1, tid, T, P.vec2);
    }
}
template <bool kNoise = false>
COPRA_DEV void plant_stage(const PlantStepArgs& P, int wg, int tid, int T, double* lds)
{
    if (P.backup_steps > 0) plant_stage_body<true, false, kNoise>(P, wg, tid, T, lds);
    else plant_stage_body<false, false, kNoise>(P, wg, tid, T, lds);
}

// phase 2 (behind a barrier): the new states and the optional copies; with backup plans the tails of the fresh plans and every next[b]
template <bool kBackup, bool kEst = false, bool kPlant = true, bool kNoise = false>
COPRA_DEV void plant_apply_body(const PlantStepArgs& P, int wg, int tid, int T, const double* lds, double* xn_lds = nullptr)
{
    const int nx = P.nx, nu = P.nu, b0 = wg * P.group;
    const int cnt = (P.batch - b0 < P.group) ? P.batch - b0 : P.group;
    if (cnt <= 0) return;
    const PlantLds L = plant_lds(nx, nu, P.group, P.shared, plant_has_w<kNoise>(P), kBackup);
    const int* st = reinterpret_cast<const int*>(lds + L.ost);
    const int* ag = reinterpret_cast<const int*>(lds + L.oag); // (read with backup plans only)
    for (int e = tid; kPlant && e < cnt * nx; e += T) { // (kPlant = false: the observer fed with measured outputs moves no plant)
        const int i = e / nx, r = e - i * nx, is = P.shared ? 0 : i;
        double xn = lds[L.ox + e]; // held
        if (kBackup ? ag[i] != kPlantAgeHeld : (st[i] == 0 || P.fallback_u))
            xn = plant_row(nx, nu, r, lds + L.oA + is * nx * nx, lds + L.oB + is * nx * nu, lds + L.od + is * nx, plant_has_w<kNoise>(P) ? lds + L.ow + i * nx : nullptr,
                lds + L.ox + i * nx, lds + L.ou + i * nu);
        const size_t o = (size_t)b0 * nx + e;
        P.x0_next[o] = xn;
        if (P.x_out) P.x_out[o] = xn;
        if (kEst) xn_lds[e] = xn; // (with the estimator: row r of x+ stays in the image for phase 3)
    }
    if (P.u_out)
        for (int e = tid; e < cnt * nu; e += T) P.u_out[(size_t)b0 * nu + e] = lds[L.ou + e];
    if (P.status_out)
        for (int i = tid; i < cnt; i += T) P.status_out[b0 + i] = st[i];
    if (!kBackup) {
        if (P.age_out)
            for (int i = tid; i < cnt; i += T) P.age_out[b0 + i] = st[i] == 0 ? 0 : P.fallback_u ? kPlantAgeFallback : kPlantAgeHeld;
        return;
    }
    // the tail of every fresh plan: controls of steps 1 .. K, K nu doubles per instance out of `control` (stride nu N; K <= N - 1: nothing
    // beyond control[b][(K + 1) nu) is read) into the group's contiguous range of `plan`; only instances with a fresh solution are read
    const int kn = P.backup_steps * nu;
    const bool pairs = (nu & 1) == 0 && ((reinterpret_cast<uintptr_t>(P.plan) | reinterpret_cast<uintptr_t>(P.control)) & 15u) == 0;
    if (pairs) { // (nu even: nu N, nu and K nu are even, every instance's tail starts on 16 bytes in both arrays)
        const int kn2 = kn >> 1;
        for (int e = tid; e < cnt * kn2; e += T) {
            const int i = e / kn2, j = e - i * kn2;
            const size_t b = (size_t)b0 + i;
            if (ag[i] == 0) reinterpret_cast<PlantPair*>(P.plan + b * kn)[j] = reinterpret_cast<const PlantPair*>(P.control + b * P.ctrl_stride + nu)[j];
        }
    } else {
        for (int e = tid; e < cnt * kn; e += T) {
            const int i = e / kn, j = e - i * kn;
            const size_t b = (size_t)b0 + i;
            if (ag[i] == 0) P.plan[b * kn + j] = P.control[b * P.ctrl_stride + nu + j];
        }
    }
    for (int i = tid; i < cnt; i += T) { // one thread per instance: the only writer of next[b], behind the barrier
        const int age = ag[i];
        if (age >= 0) P.next[b0 + i] = age + 1;
        if (P.age_out) P.age_out[b0 + i] = age;
    }
}
template <bool kNoise = false>
COPRA_DEV void plant_apply(const PlantStepArgs& P, int wg, int tid, int T, const double* lds)
{
    if (P.backup_steps > 0) plant_apply_body<true, false, true, kNoise>(P, wg, tid, T, lds);
    else plant_apply_body<false, false, true, kNoise>(P, wg, tid, T, lds);
}


// ---- the same two phases with the estimator (est != 0), and its own ----
template <bool kNoise = false>
COPRA_DEV void plant_stage_est(const PlantStepArgs& P, int wg, int tid, int T, double* lds)
{
    if (P.backup_steps > 0) plant_stage_body<true, true, kNoise>(P, wg, tid, T, lds);
    else plant_stage_body<false, true, kNoise>(P, wg, tid, T, lds);
}
template <bool kNoise = false>
COPRA_DEV void plant_apply_est(const PlantStepArgs& P, int wg, int tid, int T, double* lds)
{
    if (P.backup_steps > 0) plant_apply_body<true, true, true, kNoise>(P, wg, tid, T, lds, lds + plant_est_lds<kNoise>(P, 1).oxn);
    else plant_apply_body<false, true, true, kNoise>(P, wg, tid, T, lds, lds + plant_est_lds<kNoise>(P, 0).oxn);
}

// whether instance i of the group had a control applied (phase 2's own condition)
COPRA_DEV bool plant_moved(const PlantStepArgs& P, const PlantLds& L, const double* lds, int i)
{
    if (P.backup_steps > 0) return reinterpret_cast<const int*>(lds + L.oag)[i] != kPlantAgeHeld;
    return reinterpret_cast<const int*>(lds + L.ost)[i] == 0 || P.fallback_u;
}

// phase 3 (behind the second barrier): e_r = x+_r - pred_r per (instance, row), into the image; the model's prediction has no w
template <bool kNoise = false>
COPRA_DEV void plant_estimate(const PlantStepArgs& P, int wg, int tid, int T, double* lds)
{
    const int nx = P.nx, nu = P.nu, b0 = wg * P.group;
    const int cnt = (P.batch - b0 < P.group) ? P.batch - b0 : P.group;
    if (cnt <= 0) return;
    const PlantEstLds E = plant_est_lds<kNoise>(P, P.backup_steps > 0);
    const PlantLds& L = E.base;
    for (int e = tid; e < cnt * nx; e += T) {
        const int i = e / nx, r = e - i * nx;
        double err = 0.0; // held: nothing was applied, nothing is learnt
        if (plant_moved(P, L, lds, i))
            err = lds[E.oxn + e]
                - plant_row(nx, nu, r, lds + E.oAm + i * nx * nx, lds + E.oBm + i * nx * nu, lds + E.odh + i * nx, nullptr, lds + L.ox + i * nx, lds + L.ou + i * nu);
        lds[E.oe + e] = err;
    }
}

// ... and behind a third barrier (the dense gain reads every row's e of its instance): dhat+ and its copy, one contiguous range per group
template <bool kNoise = false>
COPRA_DEV void plant_estimate_store(const PlantStepArgs& P, int wg, int tid, int T, const double* lds)
{
    const int nx = P.nx, b0 = wg * P.group;
    const int cnt = (P.batch - b0 < P.group) ? P.batch - b0 : P.group;
    if (cnt <= 0) return;
    const PlantEstLds E = plant_est_lds<kNoise>(P, P.backup_steps > 0);
    for (int e = tid; e < cnt * nx; e += T) {
        const int i = e / nx, r = e - i * nx;
        double dn = lds[E.odh + e]; // held: bit for bit
        if (plant_moved(P, E.base, lds, i)) {
            if (P.gain_dense) {
                const double* G = lds + E.oG + (P.gain_shared ? 0 : i * nx * nx);
                for (int j = 0; j < nx; ++j) dn += G[r + nx * j] * lds[E.oe + i * nx + j];
            } else {
                dn += lds[E.oG + (P.gain_shared ? r : e)] * lds[E.oe + e];
            }
        }
        const size_t o = (size_t)b0 * nx + e;
        P.dhat[o] = dn;
        if (P.d_out) P.d_out[o] = dn;
    }
}

// ---- the state observer (copra_batch_set_observer, ABI 12): output feedback in the same launch, a third build of the kernel ----
// The plant has a state of its OWN, xp, and the controller's x0 is the estimate xhat.  With C [ny x nx], Lx, Ld [nx x ny] column-major:
//   xp+ = Ap xp + Bp u + dp (+ w);   y = C xp+ (+ v)  |  y_meas;   xpred = Am xhat + Bm u + dhat;   inn = y - C xpred
//   xhat+ = xpred + Lx inn;   dhat+ = dhat + Ld inn  (Ld optional);   a held instance keeps xp, xhat, dhat bit for bit, y_out = C xp (+ v)
// `s` is the tick WITHOUT an estimator whose state is the plant's: s.x0 = s.x0_next = xp, s.A, s.B, s.d the plant -- phase 1 and phase 2 are
// the bodies above over the image of plant_lds, so u, the ages, the plans and every copy are theirs.  With measured outputs (meas) no plant
// is simulated: s.x0 IS xhat (staged once, xp is not looked at), s.A, s.B, s.d are the model and phase 2 runs without its plant loop.
// Behind the image of plant_lds:  [Am | Bm | dhat, with a plant of its own] | [xhat, unless meas] | C | Lx | [Ld] | [v or y_meas] | xp+ |
// xpred | inn.  Phases, a barrier between two:
//   1  stage       everything the workgroup reads: xp, xhat and dhat are complete in LDS before the first barrier
//   2  apply       xp+ (global, x_out, LDS) per (instance, row);  xpred per (instance, row) into LDS -- both read only what phase 1 staged
//   3  innovate    per (instance, output): y, y_out, inn into LDS (0 for a held instance)
//   4  update      per (instance, row): xhat+ and dhat+ as contiguous ranges per group, with their copies
// xp is written in phase 2, xhat and dhat in phase 4: each behind the barrier that follows its last read (phase 1).
// LDS banks: lanes of phase 3 read C[o + ny j] with consecutive o inside an instance and a stride of ny nx doubles between instances, lanes
// of phase 4 read Lx[r + nx o] likewise -- the pattern of plant_row over A; the blocks cannot be padded apart without giving up the one
// contiguous copy per array.  A C or gain shared by the batch is one block staged once: every instance's lanes read the same words (broadcast).
struct PlantObsArgs {
    PlantStepArgs s; // est == 0
    int ny;
    int meas; // yv is y_meas: no plant
    int same_model; // no plant of its own (or meas): s.A, s.B ARE the model and s.d IS dhat; Am, Bm are not looked at
    int gain_shared; // C, Lx, Ld hold one block for the batch
    const double *Am, *Bm; // the controller's model
    const double* dhat; // [batch][nx]: the controller's d
    double* dhat_next; // == dhat with Ld (updated in place), null without
    const double* xhat; // [batch][nx]: the controller's x0
    double* xhat_next; // [batch][nx]; may be xhat
    const double *C, *Lx, *Ld; // Ld may be null
    const double* yv; // [batch][ny]: v (may be null) or y_meas
    double *y_out, *xhat_out, *d_out; // optional copies
    const double* sigma_v; // [ny] or [batch][ny] (s.sigma_per_instance): sensor noise drawn on the device, v = (v given ? v : 0) + sigma_v n; null: none
};

// whether the image has a yv slot: y_meas or a v is given, or sensor noise is drawn (never with y_meas, where v is ignored)
template <bool kNoise = true>
COPRA_PLANT_HD bool plant_obs_has_yv(const PlantObsArgs& Q) { return Q.yv != nullptr || (kNoise && !Q.meas && Q.sigma_v != nullptr); }

inline bool plant_obs_vec2_ok(const PlantObsArgs& Q)
{
    const auto ok = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    if (!Q.same_model && !(ok(Q.Am) && ok(Q.Bm))) return false;
    return plant_vec2_ok(Q.s) && ok(Q.dhat) && ok(Q.xhat) && ok(Q.C) && ok(Q.Lx) && ok(Q.Ld) && ok(Q.yv);
}

struct PlantObsLds {
    PlantLds base;
    int oAm, oBm, odh, oxh, oC, oLx, oLd, oyv, oxn, oxp, oin, total;
};
COPRA_PLANT_HD PlantObsLds plant_obs_lds(int nx, int nu, int ny, int group, int shared, int has_w, int backup, int same_model, int meas, int has_Ld,
    int gain_shared, int has_yv)
{
    PlantObsLds E;
    E.base = plant_lds(nx, nu, group, shared, has_w, backup);
    int o = E.base.total;
    E.oAm = E.base.oA, E.oBm = E.base.oB, E.odh = E.base.od, E.oxh = E.base.ox;
    if (!same_model) {
        E.oAm = o, o += plant_even(group * nx * nx);
        E.oBm = o, o += plant_even(group * nx * nu);
        E.odh = o, o += plant_even(group * nx);
    }
    if (!meas) E.oxh = o, o += plant_even(group * nx);
    const int gs = gain_shared ? 1 : group;
    E.oC = o, o += plant_even(gs * ny * nx);
    E.oLx = o, o += plant_even(gs * nx * ny);
    E.oLd = o, o += has_Ld ? plant_even(gs * nx * ny) : 0;
    E.oyv = o, o += has_yv ? plant_even(group * ny) : 0;
    E.oxn = o, o += meas ? 0 : plant_even(group * nx);
    E.oxp = o, o += plant_even(group * nx);
    E.oin = o, o += plant_even(group * ny);
    E.total = o;
    return E;
}
template <bool kNoise = false>
COPRA_DEV PlantObsLds plant_obs_lds(const PlantObsArgs& Q)
{
    return plant_obs_lds(Q.s.nx, Q.s.nu, Q.ny, Q.s.group, Q.s.shared, plant_has_w<kNoise>(Q.s), Q.s.backup_steps > 0, Q.same_model, Q.meas, Q.Ld != nullptr,
        Q.gain_shared, plant_obs_has_yv<kNoise>(Q));
}

// ---- the launch geometry (host): what copra_hip_plant.hip sizes every build's grid and image with, and what tests/emu asks ----
constexpr size_t kPlantLdsTarget = 24 * 1024; // a group's image: small enough for several workgroups per CU
constexpr size_t kPlantLdsMax = 160 * 1024; // one instance's image at most (the CU's LDS)
constexpr int kPlantGroupMax = 32;

// instances per workgroup: an image of about kPlantLdsTarget bytes, an even number of instances so that every group starts on 16 bytes;
// `one` is one instance's image in bytes
inline int plant_group(size_t one)
{
    int group = (int)(kPlantLdsTarget / one);
    group = group > kPlantGroupMax ? kPlantGroupMax : group < 1 ? 1 : group;
    if (group > 1) group &= ~1;
    return group;
}

// one instance's image of the plain tick, in bytes: the widest the tick can ask for (a plant of its own, w, ages)
inline size_t plant_image_bytes(int nx, int nu)
{
    return (size_t)plant_lds(nx, nu, 1, 0, 1, 1).total * sizeof(double);
}

// ... with the disturbance estimator: the widest the tick can ask for with this gain (a plant of its own, w, ages)
inline size_t bias_image_bytes(int nx, int nu, int dense)
{
    return (size_t)plant_est_lds(nx, nu, 1, 0, 1, 1, 0, dense, 0).total * sizeof(double);
}

// ... and with the observer: the widest the tick can ask for at this ny (a plant of its own, w, ages, Ld, per-instance gains, v)
inline size_t observer_image_bytes(int nx, int nu, int ny)
{
    return (size_t)plant_obs_lds(nx, nu, ny, 1, 0, 1, 1, 0, 0, 1, 0, 1).total * sizeof(double);
}

// phase 1: the image of the tick, then what the observer reads beside it
template <bool kNoise = false>
COPRA_DEV void plant_obs_stage(const PlantObsArgs& Q, int wg, int tid, int T, double* lds)
{
    const PlantStepArgs& P = Q.s;
    plant_stage<kNoise>(P, wg, tid, T, lds);
    const int nx = P.nx, nu = P.nu, ny = Q.ny, b0 = wg * P.group;
    const int cnt = (P.batch - b0 < P.group) ? P.batch - b0 : P.group;
    if (cnt <= 0) return;
    const PlantObsLds E = plant_obs_lds<kNoise>(Q);
    if (!Q.same_model) {
        plant_copy(lds + E.oAm, Q.Am + (size_t)b0 * nx * nx, cnt * nx * nx, tid, T, P.vec2);
        plant_copy(lds + E.oBm, Q.Bm + (size_t)b0 * nx * nu, cnt * nx * nu, tid, T, P.vec2);
        plant_copy(lds + E.odh, Q.dhat + (size_t)b0 * nx, cnt * nx, tid, T, P.vec2);
    }
    if (!Q.meas) plant_copy(lds + E.oxh, Q.xhat + (size_t)b0 * nx, cnt * nx, tid, T, P.vec2);
    const int g1 = ny * nx, gcnt = Q.gain_shared ? 1 : cnt;
    const size_t g0 = Q.gain_shared ? 0 : (size_t)b0 * g1;
    plant_copy(lds + E.oC, Q.C + g0, gcnt * g1, tid, T, P.vec2);
    plant_copy(lds + E.oLx, Q.Lx + g0, gcnt * g1, tid, T, P.vec2);
    if (Q.Ld) plant_copy(lds + E.oLd, Q.Ld + g0, gcnt * g1, tid, T, P.vec2);
    if (kNoise && !Q.meas && Q.sigma_v) noise_stage(P.noise, 1, Q.sigma_v, P.sigma_per_instance, Q.yv, (size_t)b0, cnt, ny, lds + E.oyv, tid, T);
    else if (Q.yv) plant_copy(lds + E.oyv, Q.yv + (size_t)b0 * ny, cnt * ny, tid, T, P.vec2);
}

// phase 2 (behind a barrier): the plant's new state -- the tick's own phase 2 on xp, which leaves xp+ in the image -- and the model's prediction
template <bool kNoise = false>
COPRA_DEV void plant_obs_apply(const PlantObsArgs& Q, int wg, int tid, int T, double* lds)
{
    const PlantStepArgs& P = Q.s;
    const PlantObsLds E = plant_obs_lds<kNoise>(Q);
    if (Q.meas) {
        if (P.backup_steps > 0) plant_apply_body<true, false, false, kNoise>(P, wg, tid, T, lds);
        else plant_apply_body<false, false, false, kNoise>(P, wg, tid, T, lds);
    } else {
        if (P.backup_steps > 0) plant_apply_body<true, true, true, kNoise>(P, wg, tid, T, lds, lds + E.oxn);
        else plant_apply_body<false, true, true, kNoise>(P, wg, tid, T, lds, lds + E.oxn);
    }
    const int nx = P.nx, nu = P.nu, b0 = wg * P.group;
    const int cnt = (P.batch - b0 < P.group) ? P.batch - b0 : P.group;
    // (the rows are handed out from the LAST thread down: the plant's rows above went to the first threads, so with fewer than T / 2 rows --
    //  the launch's group at small xDim -- the two sums of a row run on different waves, side by side)
    for (int e = T - 1 - tid; e < cnt * nx; e += T) {
        const int i = e / nx, r = e - i * nx;
        double xp = lds[E.oxh + e]; // held: the estimate itself
        if (plant_moved(P, E.base, lds, i))
            xp = plant_row(nx, nu, r, lds + E.oAm + i * nx * nx, lds + E.oBm + i * nx * nu, lds + E.odh + i * nx, nullptr, lds + E.oxh + i * nx, lds + E.base.ou + i * nu);
        lds[E.oxp + e] = xp;
    }
}

// phase 3 (behind the second barrier): y and the innovation per (instance, output)
template <bool kNoise = false>
COPRA_DEV void plant_obs_innovate(const PlantObsArgs& Q, int wg, int tid, int T, double* lds)
{
    const PlantStepArgs& P = Q.s;
    const int nx = P.nx, ny = Q.ny, b0 = wg * P.group;
    const int cnt = (P.batch - b0 < P.group) ? P.batch - b0 : P.group;
    if (cnt <= 0) return;
    const PlantObsLds E = plant_obs_lds<kNoise>(Q);
    for (int e = tid; e < cnt * ny; e += T) {
        const int i = e / ny, o = e - i * ny;
        const double* Cm = lds + E.oC + (Q.gain_shared ? 0 : i * ny * nx);
        double y;
        if (Q.meas) {
            y = lds[E.oyv + e];
        } else { // (a held instance's xp+ in the image is its unchanged xp)
            y = plant_obs_has_yv<kNoise>(Q) ? lds[E.oyv + e] : 0.0;
            for (int j = 0; j < nx; ++j) y += Cm[o + ny * j] * lds[E.oxn + i * nx + j];
        }
        double inn = 0.0; // held: nothing was applied, nothing is learnt
        if (plant_moved(P, E.base, lds, i)) {
            double cp = 0.0;
            for (int j = 0; j < nx; ++j) cp += Cm[o + ny * j] * lds[E.oxp + i * nx + j];
            inn = y - cp;
        }
        lds[E.oin + e] = inn;
        if (Q.y_out) Q.y_out[(size_t)b0 * ny + e] = y;
    }
}

// phase 4 (behind the third barrier: a row reads every innovation of its instance): xhat+, dhat+ and their copies
template <bool kNoise = false>
COPRA_DEV void plant_obs_update(const PlantObsArgs& Q, int wg, int tid, int T, const double* lds)
{
    const PlantStepArgs& P = Q.s;
    const int nx = P.nx, ny = Q.ny, b0 = wg * P.group;
    const int cnt = (P.batch - b0 < P.group) ? P.batch - b0 : P.group;
    if (cnt <= 0) return;
    const PlantObsLds E = plant_obs_lds<kNoise>(Q);
    for (int e = tid; e < cnt * nx; e += T) {
        const int i = e / nx, r = e - i * nx;
        const int g = Q.gain_shared ? 0 : i * nx * ny;
        double xn = lds[E.oxp + e]; // held: phase 2 left the old estimate here, bit for bit
        if (plant_moved(P, E.base, lds, i))
            for (int o = 0; o < ny; ++o) xn += lds[E.oLx + g + r + nx * o] * lds[E.oin + i * ny + o];
        const size_t at = (size_t)b0 * nx + e;
        Q.xhat_next[at] = xn;
        if (Q.xhat_out) Q.xhat_out[at] = xn;
    }
    if (!Q.Ld) return;
    for (int e = T - 1 - tid; e < cnt * nx; e += T) { // (from the last thread down, as in phase 2: beside the rows of xhat+)
        const int i = e / nx, r = e - i * nx;
        const int g = Q.gain_shared ? 0 : i * nx * ny;
        double dn = lds[E.odh + e]; // held: bit for bit
        if (plant_moved(P, E.base, lds, i))
            for (int o = 0; o < ny; ++o) dn += lds[E.oLd + g + r + nx * o] * lds[E.oin + i * ny + o];
        const size_t at = (size_t)b0 * nx + e;
        Q.dhat_next[at] = dn;
        if (Q.d_out) Q.d_out[at] = dn;
    }
}

#if defined(__HIPCC__) && !defined(COPRA_PLANT_PHASES_ONLY) // (copra_hip_score.hip takes the phase bodies alone: the kernels have ONE home, copra_hip_plant.hip)
constexpr int kPlantThreads = 256;
// (kNoise: phase 1 draws the process noise -- builds of their own, so that the builds without it hold none of the generator's code)
template <bool kEst, bool kNoise = false>
__global__ __launch_bounds__(kPlantThreads) void copra_plant_step_kernel(const PlantStepArgs P)
{
    extern __shared__ __align__(16) double plant_image[];
    const int wg = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (!kEst) {
        plant_stage<kNoise>(P, wg, tid, kPlantThreads, plant_image);
        __syncthreads();
        plant_apply<kNoise>(P, wg, tid, kPlantThreads, plant_image);
        return;
    }
    plant_stage_est<kNoise>(P, wg, tid, kPlantThreads, plant_image);
    __syncthreads();
    plant_apply_est<kNoise>(P, wg, tid, kPlantThreads, plant_image);
    __syncthreads();
    plant_estimate<kNoise>(P, wg, tid, kPlantThreads, plant_image);
    __syncthreads();
    plant_estimate_store<kNoise>(P, wg, tid, kPlantThreads, plant_image);
}

// the third build: the tick with the state observer (its arguments carry the tick's own as their first member)
template <bool kNoise>
__device__ __forceinline__ void plant_observer_tick(const PlantObsArgs& Q, double* image)
{
    const int wg = (int)blockIdx.x, tid = (int)threadIdx.x;
    plant_obs_stage<kNoise>(Q, wg, tid, kPlantThreads, image);
    __syncthreads();
    plant_obs_apply<kNoise>(Q, wg, tid, kPlantThreads, image);
    __syncthreads();
    plant_obs_innovate<kNoise>(Q, wg, tid, kPlantThreads, image);
    __syncthreads();
    plant_obs_update<kNoise>(Q, wg, tid, kPlantThreads, image);
}
__global__ __launch_bounds__(kPlantThreads) void copra_plant_observer_kernel(const PlantObsArgs Q)
{
    extern __shared__ __align__(16) double plant_image[];
    plant_observer_tick<false>(Q, plant_image);
}
// ... and its build that draws process and sensor noise in phase 1
__global__ __launch_bounds__(kPlantThreads) void copra_plant_observer_noise_kernel(const PlantObsArgs Q)
{
    extern __shared__ __align__(16) double plant_image[];
    plant_observer_tick<true>(Q, plant_image);
}
#endif

} // namespace copra_hip
