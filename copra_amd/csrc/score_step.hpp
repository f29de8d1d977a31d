// score_step.hpp -- closed-loop scores on the device (copra_batch_set_score, ABI 14; host side: copra_hip_score.hip).  Behind the plant step
// of every tick a kernel of its own updates one 64-byte record per instance from the true state x after the tick, the control u the tick
// applied and its age (what age_out reports), against a measure the caller handed over once.  For instance b, rows in ASCENDING order:
//   e_r  = x_r - x_ref_r                                   (x_ref: the row min(tau, ref_steps - 1) of the reference signal; none: e = x)
//   cx_r = (qx_r e_r) e_r   |   e_r (sum_j Qx[r,j] e_j, j ascending from 0.0)          diagonal | dense, column-major;  no qx: cx_r = 0
//   cu_c = (ru_c u_c) u_c   |   u_c (sum_j Ru[c,j] u_j, j ascending from 0.0)          a HELD instance: cu_c = 0, u is never read
//   v_r  = 0;  if (lo_r - z_r > v_r) v_r = lo_r - z_r;  if (z_r - hi_r > v_r) v_r = z_r - hi_r        z = x, then u (held: no u rows)
//   lx = ((0.0 + cx_0) + cx_1) + ...;   lu likewise over cu;   vs = ((0.0 + v_0) + ...) over the nx rows of x, then the nu rows of u;
//   vmax = the largest v_r (comparisons with `>` from 0.0: a NaN never wins);   l = lx + lu
//   jx += lx;   ju += lu (not held: a held instance's ju keeps its bits);   viol_sum += vs;   if (vmax > viol_max) viol_max = vmax;
//   if (l > peak) peak = l;   ticks += 1;   held += age == HELD;   replayed += age >= 1;   fallback += age == FALLBACK;
//   if (vmax > tol) { violating += 1;  if (first_violation == 0) first_violation = ticks; }
// A NaN state or reference makes jx NaN (defined: the summary counts it out); the NaN a held instance's u_out row holds is copied with its
// group's range into LDS and never enters arithmetic -- the age is looked at first, as the tick does with a failed instance's control.
//
// The kernel has the shape of plant_step.hpp and reuses its plant_copy, PlantPair, plant_even, plant_group and LDS target: one workgroup
// takes `group` consecutive instances; phase 1 copies each array's contiguous range into the image (a measure shared by the batch once per
// workgroup, the reference row picked by tau); phase 2, one thread per (instance, row) over the nx + nu rows, forms cx / cu and v into the
// image; phase 3, one thread per instance, folds its rows and updates the record IN the image; phase 4 stores the group's records as one
// contiguous range.  A barrier stands between two phases.  No scratch, no static LDS, no atomics, nothing depends on the grid beyond the
// bounds of the last group.  The phases are COPRA_DEV functions of (workgroup, thread) that compile on the host (tests/emu/emu_score.cpp).
//
// The summary (copra_batch_score_summary) reduces the records with the pairwise update of (n, mean, m2, min, max, argmin, argmax) --
// score_stat_merge below -- in an order that depends on the batch size alone:
//   stage 1  chunk c is records [kScoreChunk c, kScoreChunk (c + 1)); one workgroup of kScoreThreads threads per chunk.  Thread t starts
//            from the empty partial and merges records kScoreChunk c + t, + kScoreThreads, + 2 kScoreThreads, ... in ascending order
//            (acc = merge(acc, record)).  Then inside every wave of 64 lanes, for off = 32, 16, 8, 4, 2, 1: lane l <- merge(lane l,
//            lane l + off) (__shfl_down); lane 0 holds the wave's partial.  Then thread 0 merges the waves' partials in ascending order,
//            (((w0, w1), w2), w3), and stores partial c.
//   stage 2  ONE workgroup over the partials: thread t merges partials t, t + kScoreThreads, ... in ascending order from the empty one, then
//            the same lane tree and the same fold of the waves.
// Only finite values of a field are counted; ties of min / max go to the lowest index (compared explicitly: the tree does not merge
// index-ordered sets); an empty side returns the other unchanged; the counters are integer sums.  No floating-point atomics.
#pragma once
#include "plant_step.hpp"

namespace copra_hip {

struct ScoreRecord { // copra_score_record_t of include/copra_hip.h: 64 bytes, all-zero bytes are the initial state
    double jx, ju, viol_sum, viol_max, peak;
    int ticks, held, replayed, fallback, violating, first_violation;
};
static_assert(sizeof(ScoreRecord) == 64, "one record is 64 bytes");
constexpr int kScoreRecDoubles = (int)(sizeof(ScoreRecord) / sizeof(double));

struct ScoreArgs {
    int batch, nx, nu;
    int group; // instances per workgroup (even wherever vec2 is set)
    int vec2; // every array's range of every group starts on 16 bytes (score_vec2_ok)
    int dense, per_instance;
    const double* x; // [batch][nx]: the true state after the tick
    const double* u; // [batch][nu]: the control the tick applied (NaN rows for held instances)
    const int* age; // [batch]
    const double *qx, *ru; // [nx] | [nx x nx], [nu] | [nu x nu]; once or per instance; null: no term
    const double* x_ref; // [per_instance ? batch : 1][ref_steps][nx] or null
    long long ref_steps, ref_row; // ref_row = min(tau, ref_steps - 1), formed by the launch
    const double *x_lo, *x_hi, *u_lo, *u_hi; // each may be null
    double tol;
    ScoreRecord* rec; // [batch]
};

// (host) whether a launch may copy two doubles per lane: the rule of plant_vec2_ok over the score's arrays
inline bool score_vec2_ok(const ScoreArgs& S)
{
    const auto ok = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    const double* const ref = S.x_ref && !S.per_instance ? S.x_ref + (size_t)S.ref_row * S.nx : S.x_ref;
    return S.group % 2 == 0 && ok(S.x) && ok(S.u) && ok(S.rec) && ok(S.qx) && ok(S.ru) && ok(ref) && ok(S.x_lo) && ok(S.x_hi) && ok(S.u_lo) && ok(S.u_hi);
}

// LDS image of one workgroup, in doubles: x | u | age (ints) | records | qx | ru | x_ref | x_lo | x_hi | u_lo | u_hi | terms | violations;
// every part starts on 16 bytes; a part whose array is not given takes no room
struct ScoreLds {
    int ox, ou, oag, orec, oqx, oru, oref, oxl, oxh, oul, ouh, oc, ov, total;
};
COPRA_PLANT_HD ScoreLds score_lds(int nx, int nu, int group, int dense, int per_instance, int has_qx, int has_ru, int has_ref, int has_xlo, int has_xhi, int has_ulo,
    int has_uhi)
{
    const int gs = per_instance ? group : 1;
    ScoreLds L;
    int o = 0;
    L.ox = o, o += plant_even(group * nx);
    L.ou = o, o += plant_even(group * nu);
    L.oag = o, o += plant_even((group + 1) / 2);
    L.orec = o, o += group * kScoreRecDoubles;
    L.oqx = o, o += has_qx ? plant_even(gs * (dense ? nx * nx : nx)) : 0;
    L.oru = o, o += has_ru ? plant_even(gs * (dense ? nu * nu : nu)) : 0;
    L.oref = o, o += has_ref ? plant_even(gs * nx) : 0;
    L.oxl = o, o += has_xlo ? plant_even(gs * nx) : 0;
    L.oxh = o, o += has_xhi ? plant_even(gs * nx) : 0;
    L.oul = o, o += has_ulo ? plant_even(gs * nu) : 0;
    L.ouh = o, o += has_uhi ? plant_even(gs * nu) : 0;
    L.oc = o, o += plant_even(group * (nx + nu));
    L.ov = o, o += plant_even(group * (nx + nu));
    L.total = o;
    return L;
}
COPRA_PLANT_HD ScoreLds score_lds(const ScoreArgs& S)
{
    return score_lds(S.nx, S.nu, S.group, S.dense, S.per_instance, S.qx != nullptr, S.ru != nullptr, S.x_ref != nullptr, S.x_lo != nullptr, S.x_hi != nullptr,
        S.u_lo != nullptr, S.u_hi != nullptr);
}

// ---- the launch geometry: one instance's widest image in bytes (every array given, per instance), the group from plant_group ----
inline size_t score_image_bytes(int nx, int nu, int dense) { return (size_t)score_lds(nx, nu, 1, dense, 1, 1, 1, 1, 1, 1, 1, 1).total * sizeof(double); }
inline int score_group(int nx, int nu, int dense) { return plant_group(score_image_bytes(nx, nu, dense)); }

// Several contiguous copies at once, dst[0 .. count) = src[0 .. count) each, the elements handed to the threads as plant_copy hands them out.
// A thread's FIRST element of every array is loaded before any is stored: the loads of all arrays are in flight together.  One copy loop
// per array waits for its own load before the next array's is issued -- eleven round trips to memory in a row for a workgroup that moves
// a few kilobytes (measured: profiles/closed_loop/score_rates.txt).
#if defined(__HIPCC__)
#define COPRA_SCORE_UNROLL _Pragma("unroll")
#else
#define COPRA_SCORE_UNROLL
#endif
constexpr int kScoreCopies = 10;
struct ScoreCopy {
    double* dst;
    const double* src;
    int count; // 0: not given
};
COPRA_DEV void score_copy_all(const ScoreCopy (&c)[kScoreCopies], int tid, int T, int vec2)
{
    if (vec2) {
        PlantPair first[kScoreCopies];
        COPRA_SCORE_UNROLL
        for (int k = 0; k < kScoreCopies; ++k) first[k].a = first[k].b = 0.0;
COPRA_SCORE_UNROLL
        for (int k = 0; k < kScoreCopies; ++k)
            if (tid < (c[k].count >> 1)) first[k] = reinterpret_cast<const PlantPair*>(c[k].src)[tid];
COPRA_SCORE_UNROLL
        for (int k = 0; k < kScoreCopies; ++k)
            if (tid < (c[k].count >> 1)) reinterpret_cast<PlantPair*>(c[k].dst)[tid] = first[k];
COPRA_SCORE_UNROLL
        for (int k = 0; k < kScoreCopies; ++k) {
            const int pairs = c[k].count >> 1;
            for (int e = tid + T; e < pairs; e += T) reinterpret_cast<PlantPair*>(c[k].dst)[e] = reinterpret_cast<const PlantPair*>(c[k].src)[e];
            if ((c[k].count & 1) && tid == 0) c[k].dst[c[k].count - 1] = c[k].src[c[k].count - 1];
        }
    } else {
        double first[kScoreCopies];
        COPRA_SCORE_UNROLL
        for (int k = 0; k < kScoreCopies; ++k) first[k] = 0.0;
COPRA_SCORE_UNROLL
        for (int k = 0; k < kScoreCopies; ++k)
            if (tid < c[k].count) first[k] = c[k].src[tid];
COPRA_SCORE_UNROLL
        for (int k = 0; k < kScoreCopies; ++k)
            if (tid < c[k].count) c[k].dst[tid] = first[k];
COPRA_SCORE_UNROLL
        for (int k = 0; k < kScoreCopies; ++k)
            for (int e = tid + T; e < c[k].count; e += T) c[k].dst[e] = c[k].src[e];
    }
}

// phase 1: everything workgroup `wg` reads, into its image
COPRA_DEV void score_stage(const ScoreArgs& S, int wg, int tid, int T, double* lds)
{
    const int nx = S.nx, nu = S.nu, b0 = wg * S.group;
    const int cnt = (S.batch - b0 < S.group) ? S.batch - b0 : S.group;
    if (cnt <= 0) return;
    const ScoreLds L = score_lds(S);
    const size_t m0 = S.per_instance ? (size_t)b0 : 0;
    const int mcnt = S.per_instance ? cnt : 1;
    const int q1 = S.dense ? nx * nx : nx, r1 = S.dense ? nu * nu : nu;
    // the reference rows of the group are one contiguous range for a shared signal (its row) and for a constant goal per instance
    const bool ref_gather = S.x_ref && S.per_instance && S.ref_steps != 1;
    const double* const ref = !S.x_ref || ref_gather ? nullptr : !S.per_instance ? S.x_ref + (size_t)S.ref_row * nx : S.x_ref + (size_t)b0 * nx;
    const auto part = [&](int at, const double* src, int count) { return ScoreCopy { lds + at, src, src ? count : 0 }; };
    const ScoreCopy copies[kScoreCopies] = {
        part(L.ox, S.x + (size_t)b0 * nx, cnt * nx),
        part(L.ou, S.u + (size_t)b0 * nu, cnt * nu), // (a held instance's NaN row travels, it is never used)
        part(L.orec, reinterpret_cast<const double*>(S.rec + b0), cnt * kScoreRecDoubles),
        part(L.oqx, S.qx ? S.qx + m0 * q1 : nullptr, mcnt * q1),
        part(L.oru, S.ru ? S.ru + m0 * r1 : nullptr, mcnt * r1),
        part(L.oref, ref, mcnt * nx),
        part(L.oxl, S.x_lo ? S.x_lo + m0 * nx : nullptr, mcnt * nx),
        part(L.oxh, S.x_hi ? S.x_hi + m0 * nx : nullptr, mcnt * nx),
        part(L.oul, S.u_lo ? S.u_lo + m0 * nu : nullptr, mcnt * nu),
        part(L.ouh, S.u_hi ? S.u_hi + m0 * nu : nullptr, mcnt * nu),
    };
    int* ag = reinterpret_cast<int*>(lds + L.oag);
    const int age0 = tid < cnt ? S.age[b0 + tid] : 0; // (in flight with the loads below)
    score_copy_all(copies, tid, T, S.vec2);
    if (tid < cnt) ag[tid] = age0;
    for (int i = tid + T; i < cnt; i += T) ag[i] = S.age[b0 + i];
    if (ref_gather) // every instance's row of its own signal: nx consecutive doubles, ref_steps nx apart
        for (int e = tid; e < cnt * nx; e += T) {
            const int i = e / nx, r = e - i * nx;
            lds[L.oref + e] = S.x_ref[(((size_t)b0 + i) * (size_t)S.ref_steps + (size_t)S.ref_row) * nx + r];
        }
}

// one row's violation of its box
COPRA_DEV double score_violation(double z, const double* lo, const double* hi, int r)
{
    double v = 0.0;
    if (lo && lo[r] - z > v) v = lo[r] - z;
    if (hi && z - hi[r] > v) v = z - hi[r];
    return v;
}

// phase 2 (behind a barrier): the cost term and the violation of every (instance, row), rows 0 .. nx - 1 of x, then nx .. nx + nu - 1 of u
COPRA_DEV void score_rows(const ScoreArgs& S, int wg, int tid, int T, double* lds)
{
    const int nx = S.nx, nu = S.nu, nr = nx + nu, b0 = wg * S.group;
    const int cnt = (S.batch - b0 < S.group) ? S.batch - b0 : S.group;
    if (cnt <= 0) return;
    const ScoreLds L = score_lds(S);
    const int* ag = reinterpret_cast<const int*>(lds + L.oag);
    for (int e = tid; e < cnt * nr; e += T) {
        const int i = e / nr, k = e - i * nr, im = S.per_instance ? i : 0;
        double c = 0.0, v = 0.0;
        if (k < nx) {
            const double* x = lds + L.ox + i * nx;
            const double* ref = S.x_ref ? lds + L.oref + im * nx : nullptr;
            const double er = ref ? x[k] - ref[k] : x[k];
            if (S.qx && S.dense) {
                const double* Q = lds + L.oqx + im * nx * nx;
                double acc = 0.0;
                for (int j = 0; j < nx; ++j) acc += Q[k + nx * j] * (ref ? x[j] - ref[j] : x[j]);
                c = er * acc;
            } else if (S.qx) {
                c = lds[L.oqx + im * nx + k] * er * er;
            }
            v = score_violation(x[k], S.x_lo ? lds + L.oxl + im * nx : nullptr, S.x_hi ? lds + L.oxh + im * nx : nullptr, k);
        } else if (ag[i] != kPlantAgeHeld) { // (the age decides BEFORE anything of u is touched)
            const int cidx = k - nx;
            const double* u = lds + L.ou + i * nu;
            if (S.ru && S.dense) {
                const double* R = lds + L.oru + im * nu * nu;
                double acc = 0.0;
                for (int j = 0; j < nu; ++j) acc += R[cidx + nu * j] * u[j];
                c = u[cidx] * acc;
            } else if (S.ru) {
                c = lds[L.oru + im * nu + cidx] * u[cidx] * u[cidx];
            }
            v = score_violation(u[cidx], S.u_lo ? lds + L.oul + im * nu : nullptr, S.u_hi ? lds + L.ouh + im * nu : nullptr, cidx);
        }
        lds[L.oc + e] = c;
        lds[L.ov + e] = v;
    }
}

// phase 3 (behind a barrier): one thread per instance folds its rows in ascending order and updates the record in the image
COPRA_DEV void score_fold(const ScoreArgs& S, int wg, int tid, int T, double* lds)
{
    const int nx = S.nx, nu = S.nu, nr = nx + nu, b0 = wg * S.group;
    const int cnt = (S.batch - b0 < S.group) ? S.batch - b0 : S.group;
    if (cnt <= 0) return;
    const ScoreLds L = score_lds(S);
    const int* ag = reinterpret_cast<const int*>(lds + L.oag);
    for (int i = tid; i < cnt; i += T) {
        const double *c = lds + L.oc + i * nr, *v = lds + L.ov + i * nr;
        const int age = ag[i];
        double lx = 0.0, lu = 0.0, vs = 0.0, vmax = 0.0;
        for (int r = 0; r < nx; ++r) lx += c[r];
        for (int r = nx; r < nr; ++r) lu += c[r];
        for (int r = 0; r < nr; ++r) {
            vs += v[r];
            if (v[r] > vmax) vmax = v[r];
        }
        ScoreRecord* R = reinterpret_cast<ScoreRecord*>(lds + L.orec) + i;
        const double l = lx + lu;
        R->jx += lx;
        if (age != kPlantAgeHeld) R->ju += lu;
        R->viol_sum += vs;
        if (vmax > R->viol_max) R->viol_max = vmax;
        if (l > R->peak) R->peak = l;
        R->ticks += 1;
        R->held += age == kPlantAgeHeld;
        R->replayed += age >= 1;
        R->fallback += age == kPlantAgeFallback;
        if (vmax > S.tol) {
            R->violating += 1;
            if (R->first_violation == 0) R->first_violation = R->ticks;
        }
    }
}

// phase 4 (behind a barrier): the group's records, one contiguous range
COPRA_DEV void score_store(const ScoreArgs& S, int wg, int tid, int T, const double* lds)
{
    const int b0 = wg * S.group;
    const int cnt = (S.batch - b0 < S.group) ? S.batch - b0 : S.group;
    if (cnt <= 0) return;
    plant_copy(reinterpret_cast<double*>(S.rec + b0), lds + score_lds(S).orec, cnt * kScoreRecDoubles, tid, T, S.vec2);
}

// ---- the summary ----
#if defined(__HIPCC__)
#define COPRA_SCORE_HD __host__ __device__ __forceinline__ // (a partial is 336 bytes: returned through the stack unless the merge is inlined)
#else
#define COPRA_SCORE_HD inline
#endif

constexpr int kScoreFields = 5; // jx, ju, viol_sum, viol_max, peak
constexpr int kScoreThreads = 256; // of both kernels
constexpr int kScoreChunk = 1024; // records per partial of stage 1

struct ScoreStat { // copra_score_stat_t
    long long n;
    double mean, m2, min, max;
    long long argmin, argmax;
};
struct ScoreCounts { // the integer totals of copra_score_summary_t
    long long ticks, held, replayed, fallback, violating;
    long long instances_violating, instances_held;
};
struct ScoreSummary { // copra_score_summary_t; also a partial of the reduction
    ScoreStat f[kScoreFields];
    ScoreCounts c;
};

COPRA_SCORE_HD ScoreStat score_stat_empty()
{
    ScoreStat s;
    s.n = 0, s.mean = 0.0, s.m2 = 0.0, s.min = (double)__builtin_inf(), s.max = -(double)__builtin_inf(), s.argmin = -1, s.argmax = -1;
    return s;
}
COPRA_SCORE_HD ScoreStat score_stat_one(double v, long long index)
{
    ScoreStat s = score_stat_empty();
    if (!__builtin_isfinite(v)) return s;
    s.n = 1, s.mean = v, s.min = v, s.max = v, s.argmin = index, s.argmax = index;
    return s;
}
// the pairwise update: a, then b
COPRA_SCORE_HD ScoreStat score_stat_merge(const ScoreStat a, const ScoreStat b)
{
    ScoreStat s = a;
    if (b.n == 0) return s;
    s = b;
    if (a.n == 0) return s;
    const double na = (double)a.n, nb = (double)b.n, n = (double)(a.n + b.n);
    const double delta = b.mean - a.mean;
    s.n = a.n + b.n;
    s.mean = a.mean + delta * nb / n;
    s.m2 = a.m2 + b.m2 + delta * delta * na * nb / n;
    const bool bmin = b.min < a.min || (b.min == a.min && b.argmin < a.argmin);
    const bool bmax = b.max > a.max || (b.max == a.max && b.argmax < a.argmax);
    s.min = bmin ? b.min : a.min, s.argmin = bmin ? b.argmin : a.argmin;
    s.max = bmax ? b.max : a.max, s.argmax = bmax ? b.argmax : a.argmax;
    return s;
}
COPRA_SCORE_HD ScoreCounts score_counts_empty()
{
    ScoreCounts c;
    c.ticks = c.held = c.replayed = c.fallback = c.violating = c.instances_violating = c.instances_held = 0;
    return c;
}
COPRA_SCORE_HD ScoreCounts score_counts_one(const ScoreRecord& r)
{
    ScoreCounts c;
    c.ticks = r.ticks, c.held = r.held, c.replayed = r.replayed, c.fallback = r.fallback, c.violating = r.violating;
    c.instances_violating = r.violating != 0, c.instances_held = r.held != 0;
    return c;
}
COPRA_SCORE_HD ScoreCounts score_counts_merge(const ScoreCounts& a, const ScoreCounts& b)
{
    ScoreCounts c;
    c.ticks = a.ticks + b.ticks, c.held = a.held + b.held, c.replayed = a.replayed + b.replayed, c.fallback = a.fallback + b.fallback;
    c.violating = a.violating + b.violating;
    c.instances_violating = a.instances_violating + b.instances_violating, c.instances_held = a.instances_held + b.instances_held;
    return c;
}
inline ScoreSummary score_empty()
{
    ScoreSummary p;
    for (int f = 0; f < kScoreFields; ++f) p.f[f] = score_stat_empty();
    p.c = score_counts_empty();
    return p;
}

// The kernel takes the six parts of a summary one after the other -- the five fields, then the counters: a partial in flight is 56 bytes,
// not 336, and every part goes through the same fold, tree and fold
struct ScoreReduceArgs {
    int stage; // 1: records -> partials, one workgroup per chunk; 2: partials -> out[0], one workgroup
    long long count; // records (stage 1) | partials (stage 2)
    const ScoreRecord* rec;
    const ScoreSummary* partials;
    ScoreSummary* out; // stage 1: [chunks]; stage 2: [1]
};
inline long long score_chunks(long long batch) { return (batch + kScoreChunk - 1) / kScoreChunk; }

// a thread's own fold of field f: thread `tid` of workgroup `wg`, ascending from the empty statistic
COPRA_DEV ScoreStat score_fold_stat(const ScoreReduceArgs& R, int wg, int tid, int f)
{
    ScoreStat acc = score_stat_empty();
    if (R.stage == 1) {
        const long long first = (long long)wg * kScoreChunk, end = first + kScoreChunk < R.count ? first + kScoreChunk : R.count;
        for (long long i = first + tid; i < end; i += kScoreThreads) // (the five doubles lead the record)
            acc = score_stat_merge(acc, score_stat_one(reinterpret_cast<const double*>(R.rec + i)[f], i));
    } else {
        for (long long i = tid; i < R.count; i += kScoreThreads) acc = score_stat_merge(acc, R.partials[i].f[f]);
    }
    return acc;
}
// ... and of the counters
COPRA_DEV ScoreCounts score_fold_counts(const ScoreReduceArgs& R, int wg, int tid)
{
    ScoreCounts acc = score_counts_empty();
    if (R.stage == 1) {
        const long long first = (long long)wg * kScoreChunk, end = first + kScoreChunk < R.count ? first + kScoreChunk : R.count;
        for (long long i = first + tid; i < end; i += kScoreThreads) acc = score_counts_merge(acc, score_counts_one(R.rec[i]));
    } else {
        for (long long i = tid; i < R.count; i += kScoreThreads) acc = score_counts_merge(acc, R.partials[i].c);
    }
    return acc;
}

#if defined(__HIPCC__) && !defined(COPRA_SCORE_HELPERS_ONLY) // (copra_hip_trace.hip takes the helpers alone: the kernels have ONE home, copra_hip_score.hip)
__global__ __launch_bounds__(kScoreThreads) void copra_score_kernel(const ScoreArgs S)
{
    extern __shared__ __align__(16) double score_image[];
    const int wg = (int)blockIdx.x, tid = (int)threadIdx.x;
    score_stage(S, wg, tid, kScoreThreads, score_image);
    __syncthreads();
    score_rows(S, wg, tid, kScoreThreads, score_image);
    __syncthreads();
    score_fold(S, wg, tid, kScoreThreads, score_image);
    __syncthreads();
    score_store(S, wg, tid, kScoreThreads, score_image);
}
#endif

#if defined(__HIPCC__)
__device__ __forceinline__ ScoreStat score_shfl_down(const ScoreStat& p, int off)
{
    ScoreStat q;
    q.n = __shfl_down(p.n, off, 64), q.mean = __shfl_down(p.mean, off, 64), q.m2 = __shfl_down(p.m2, off, 64);
    q.min = __shfl_down(p.min, off, 64), q.max = __shfl_down(p.max, off, 64);
    q.argmin = __shfl_down(p.argmin, off, 64), q.argmax = __shfl_down(p.argmax, off, 64);
    return q;
}
__device__ __forceinline__ ScoreCounts score_shfl_down(const ScoreCounts& p, int off)
{
    ScoreCounts q;
    q.ticks = __shfl_down(p.ticks, off, 64), q.held = __shfl_down(p.held, off, 64), q.replayed = __shfl_down(p.replayed, off, 64);
    q.fallback = __shfl_down(p.fallback, off, 64), q.violating = __shfl_down(p.violating, off, 64);
    q.instances_violating = __shfl_down(p.instances_violating, off, 64), q.instances_held = __shfl_down(p.instances_held, off, 64);
    return q;
}

#endif

#if defined(__HIPCC__) && !defined(COPRA_SCORE_HELPERS_ONLY)
static_assert(sizeof(ScoreStat) == sizeof(ScoreCounts), "the waves' words in LDS serve both");
__global__ __launch_bounds__(kScoreThreads) void copra_score_reduce_kernel(const ScoreReduceArgs R)
{
    extern __shared__ __align__(16) double score_waves[]; // one part of kScoreThreads / 64 waves
    const int wg = (int)blockIdx.x, tid = (int)threadIdx.x;
    ScoreSummary* const out = R.out + (R.stage == 1 ? wg : 0);
    for (int f = 0; f < kScoreFields; ++f) {
        ScoreStat* const waves = reinterpret_cast<ScoreStat*>(score_waves);
        ScoreStat acc = score_fold_stat(R, wg, tid, f);
        for (int off = 32; off >= 1; off >>= 1) acc = score_stat_merge(acc, score_shfl_down(acc, off));
        if ((tid & 63) == 0) waves[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kScoreThreads / 64; ++w) acc = score_stat_merge(acc, waves[w]);
            out->f[f] = acc;
        }
        __syncthreads(); // (the waves' words are written again by the next part)
    }
    ScoreCounts* const waves = reinterpret_cast<ScoreCounts*>(score_waves);
    ScoreCounts acc = score_fold_counts(R, wg, tid);
    for (int off = 32; off >= 1; off >>= 1) acc = score_counts_merge(acc, score_shfl_down(acc, off));
    if ((tid & 63) == 0) waves[tid >> 6] = acc;
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < kScoreThreads / 64; ++w) acc = score_counts_merge(acc, waves[w]);
    out->c = acc;
}
#endif

} // namespace copra_hip
