// trace_step.hpp -- ensemble traces on the device (copra_batch_set_trace, ABI 17; host side: copra_hip_trace.hip).  Behind the score of a recorded
// tick two launches reduce the batch to ONE slot of the trace: a head of integer counts and `rows` statistics (ScoreStat of score_step.hpp),
// in the order x | u | err | viol.  For instance i of that tick, from the true state x after the tick, the applied control u, its age and --
// while the observer simulates a plant -- the estimate e of the same tick:
//   x rows    x_r                                          u rows    u_c, a HELD instance has none (the age decides: u is never read)
//   err rows  e_r - x_r  (one subtraction)  on a tick with an estimate beside a true state; else no instance has a value
//   viol      vmax = the largest of  max(0, lo_r - z_r, z_r - hi_r)  over the rows of x, then of u (held: no u rows) -- score_violation,
//             comparisons with `>` from 0.0, so a NaN never wins
//   head      solved = #(age == 0), replayed = #(age >= 1), fallback = #(age == FALLBACK), held = #(age == HELD), violating = #(vmax > tol)
// A value that is not finite is counted out of its row (score_stat_one); "has none" is the same thing: the row sees a NaN.
//
// The order is the summary's (score_step.hpp), with "record i" read as "instance i's value of row r":
//   stage 1  chunk c is instances [kScoreChunk c, kScoreChunk (c + 1)); one workgroup of kScoreThreads threads per chunk.  For every row, thread t
//            merges from the empty statistic the instances kScoreChunk c + t, + kScoreThreads, ... in ascending order; inside every wave of 64
//            lanes, for off = 32 .. 1: lane l <- merge(lane l, lane l + off); thread 0 merges the waves' partials in ascending order and stores
//            row r of partial c.  The counts go through the same fold, tree and fold as integer sums (ScoreCounts, score_counts_merge).
//   stage 2  ONE workgroup over the partials: thread t merges partials t, t + kScoreThreads, ... in ascending order from the empty one, the same
//            tree and fold, and writes the slot -- the head with the tick and the schedule tick the launch was given.
// A partial has the shape of a slot (its first 56 bytes are the ScoreCounts); a partial in flight through the tree is one ScoreStat.
// WHO computes is free, and a merge is two FP64 divisions deep: one wave does a whole row (trace_part) -- its lane l plays the threads l,
// 64 + l, 128 + l, 192 + l, the four waves' trees run side by side and hide each other's latency -- and the workgroup's waves take the rows in
// turn, without a barrier or LDS between two rows.
//
// How a chunk reaches its threads.  x, u and e of a chunk are contiguous ranges, but thread t's own values lie nx doubles apart and every row
// pass wants them again.  So phase 1 of stage 1 copies the chunk's ranges and ages into the LDS image -- consecutive lanes, consecutive
// addresses, 16 bytes per lane where the ranges start on 16 bytes, kTraceInFlight loads of every thread in flight before their first store (a
// workgroup is four waves on four SIMDs: nothing else hides the latency) -- and the row passes read the image.  (6, 3) with all three groups:
// 1024 x 15 doubles and the ages, 124 KB.  Where the image does not fit (trace_in_lds) the row passes read global memory directly: the same
// values, the same bits.  The limits are batch-wide and read where they lie.  No scratch, no atomics, no counter on the device: the slot is an
// argument.  The phase bodies are COPRA_DEV functions of (workgroup, thread) that compile on the host (tests/emu/emu_trace.cpp).
#pragma once
#include "score_step.hpp"

namespace copra_hip {

constexpr int kTraceX = 1, kTraceU = 2, kTraceErr = 4; // COPRA_TRACE_* of include/copra_hip.h
constexpr int kTraceInFlight = 8; // loads of one thread issued before their first store (phase 1)

struct TraceHead { // copra_trace_head_t
    long long tick, tau, solved, replayed, fallback, held, violating, reserved;
};
static_assert(sizeof(TraceHead) == 64 && sizeof(ScoreCounts) <= sizeof(TraceHead), "a slot's head is 64 bytes; a partial keeps its counts there");

struct TraceArgs {
    int batch, nx, nu;
    int what; // kTrace* bits
    int err_live; // this tick has an estimate beside a true state (else the err rows are empty)
    int in_lds; // stage 1 copies its chunk into the image (trace_in_lds), else reads global memory
    int vec2; // the arrays this tick copies start on 16 bytes (a chunk's range then does too: kScoreChunk is even)
    const double* x; // [batch][nx]: the true state after the tick
    const double* u; // [batch][nu]: the applied control (NaN rows for held instances, never read)
    const double* est; // [batch][nx]: the estimate of the same tick; read only with err_live
    const int* age; // [batch]
    const double *x_lo, *x_hi, *u_lo, *u_hi; // [nx], [nu], one for the batch; each may be null
    double tol;
    long long tick, tau; // what the head reports
    long long chunks; // partials of stage 1
    unsigned char* part; // [chunks] partials, slot-shaped
    unsigned char* slot; // stage 2 writes this one
};

// (host) which ticks are recorded, and where: the trace's own tick count moves at every tick; the ticks t with t % every == 0 take the next
// free slot, and once the trace is full they are counted in `missed` instead -- a full trace never fails a tick
struct TraceClock {
    long long tick, recorded, missed, capacity;
    int every;
};
inline long long trace_next_slot(TraceClock& c, long long* tick_recorded) // the slot to write, or -1: this tick writes none
{
    const long long t = c.tick;
    c.tick += 1;
    if (t % (c.every > 0 ? c.every : 1) != 0) return -1;
    if (c.recorded >= c.capacity) {
        c.missed += 1;
        return -1;
    }
    *tick_recorded = t;
    return c.recorded++;
}

COPRA_PLANT_HD int trace_has_limits(const TraceArgs& T) { return T.x_lo || T.x_hi || T.u_lo || T.u_hi; }
COPRA_PLANT_HD int trace_rows(int what, int nx, int nu, int limits) { return ((what & kTraceX) ? nx : 0) + ((what & kTraceU) ? nu : 0) + ((what & kTraceErr) ? nx : 0) + (limits ? 1 : 0); }
COPRA_PLANT_HD int trace_rows(const TraceArgs& T) { return trace_rows(T.what, T.nx, T.nu, trace_has_limits(T)); }
COPRA_PLANT_HD size_t trace_slot_bytes(int rows) { return sizeof(TraceHead) + (size_t)rows * sizeof(ScoreStat); }
// which arrays a tick reads at all
COPRA_PLANT_HD int trace_reads_x(const TraceArgs& T) { return (T.what & kTraceX) || ((T.what & kTraceErr) && T.err_live) || T.x_lo || T.x_hi; }
COPRA_PLANT_HD int trace_reads_u(const TraceArgs& T) { return (T.what & kTraceU) || T.u_lo || T.u_hi; }
COPRA_PLANT_HD int trace_reads_est(const TraceArgs& T) { return (T.what & kTraceErr) && T.err_live; }

// LDS image of one workgroup of stage 1, in doubles: x | u | est | age (ints); every part starts on 16 bytes, a part not read takes no room;
// stage 2 has none
struct TraceLds {
    int ox, ou, oe, oag, total;
};
COPRA_PLANT_HD TraceLds trace_lds(int nx, int nu, int reads_x, int reads_u, int reads_est)
{
    TraceLds L;
    int o = 0;
    L.ox = o, o += reads_x ? kScoreChunk * nx : 0;
    L.ou = o, o += reads_u ? kScoreChunk * nu : 0;
    L.oe = o, o += reads_est ? kScoreChunk * nx : 0;
    L.oag = o, o += kScoreChunk / 2;
    L.total = o;
    return L;
}
COPRA_PLANT_HD TraceLds trace_lds(const TraceArgs& T) { return trace_lds(T.nx, T.nu, trace_reads_x(T), trace_reads_u(T), trace_reads_est(T)); }
// (host) the launch's choice: the image of the widest tick of this trace inside the CU's LDS
inline bool trace_in_lds(int nx, int nu, int what, int x_limits, int u_limits)
{
    const int rx = (what & (kTraceX | kTraceErr)) || x_limits, ru = (what & kTraceU) || u_limits, re = (what & kTraceErr) != 0;
    if (nx > 4096 || nu > 4096) return false; // (before an int can overflow)
    return (size_t)trace_lds(nx, nu, rx, ru, re).total * sizeof(double) <= kPlantLdsMax;
}
inline bool trace_vec2_ok(const TraceArgs& T)
{
    const auto ok = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    return (!trace_reads_x(T) || ok(T.x)) && (!trace_reads_u(T) || ok(T.u)) && (!trace_reads_est(T) || ok(T.est)); // (only what this tick copies)
}

// dst[0 .. count) = src[0 .. count), the elements handed to the threads as plant_copy hands them out, kTraceInFlight loads of a thread issued
// before the first of them is stored
COPRA_DEV void trace_copy(double* dst, const double* src, int count, int tid, int T, int vec2)
{
    if (vec2) {
        const int pairs = count >> 1;
        const PlantPair* s2 = reinterpret_cast<const PlantPair*>(src);
        PlantPair* d2 = reinterpret_cast<PlantPair*>(dst);
        for (int e0 = tid; e0 < pairs; e0 += kTraceInFlight * T) {
            PlantPair v[kTraceInFlight];
            COPRA_SCORE_UNROLL
            for (int j = 0; j < kTraceInFlight; ++j) v[j].a = v[j].b = 0.0;
COPRA_SCORE_UNROLL
            for (int j = 0; j < kTraceInFlight; ++j)
                if (e0 + j * T < pairs) v[j] = s2[e0 + j * T];
COPRA_SCORE_UNROLL
            for (int j = 0; j < kTraceInFlight; ++j)
                if (e0 + j * T < pairs) d2[e0 + j * T] = v[j];
        }
        if ((count & 1) && tid == 0) dst[count - 1] = src[count - 1];
    } else {
        for (int e0 = tid; e0 < count; e0 += kTraceInFlight * T) {
            double v[kTraceInFlight];
            COPRA_SCORE_UNROLL
            for (int j = 0; j < kTraceInFlight; ++j) v[j] = 0.0;
COPRA_SCORE_UNROLL
            for (int j = 0; j < kTraceInFlight; ++j)
                if (e0 + j * T < count) v[j] = src[e0 + j * T];
COPRA_SCORE_UNROLL
            for (int j = 0; j < kTraceInFlight; ++j)
                if (e0 + j * T < count) dst[e0 + j * T] = v[j];
        }
    }
}

// instances of chunk `wg`
COPRA_DEV int trace_chunk_count(const TraceArgs& T, int wg)
{
    const long long left = (long long)T.batch - (long long)wg * kScoreChunk;
    return left < kScoreChunk ? (left > 0 ? (int)left : 0) : kScoreChunk;
}

// stage 1, phase 1: what chunk `wg` reads, into its image (nothing without in_lds)
COPRA_DEV void trace_stage(const TraceArgs& T, int wg, int tid, int nthreads, double* lds)
{
    const int cnt = trace_chunk_count(T, wg);
    if (!T.in_lds || cnt <= 0) return;
    const TraceLds L = trace_lds(T);
    const size_t b0 = (size_t)wg * kScoreChunk;
    int* ag = reinterpret_cast<int*>(lds + L.oag);
    for (int i = tid; i < cnt; i += nthreads) ag[i] = T.age[b0 + i];
    if (trace_reads_x(T)) trace_copy(lds + L.ox, T.x + b0 * T.nx, cnt * T.nx, tid, nthreads, T.vec2);
    if (trace_reads_u(T)) trace_copy(lds + L.ou, T.u + b0 * T.nu, cnt * T.nu, tid, nthreads, T.vec2); // (a held instance's NaN row travels, it is never used)
    if (trace_reads_est(T)) trace_copy(lds + L.oe, T.est + b0 * T.nx, cnt * T.nx, tid, nthreads, T.vec2);
}

// a chunk as its row passes index it: instance `il` of the chunk, whether the image or global memory lies behind
struct TraceView {
    const double *x, *u, *est;
    const int* age;
};
COPRA_DEV TraceView trace_view(const TraceArgs& T, int wg, const double* lds)
{
    TraceView V;
    if (T.in_lds) {
        const TraceLds L = trace_lds(T);
        V.x = lds + L.ox, V.u = lds + L.ou, V.est = lds + L.oe, V.age = reinterpret_cast<const int*>(lds + L.oag);
    } else {
        const size_t b0 = (size_t)wg * kScoreChunk;
        V.x = T.x + b0 * T.nx, V.u = T.u + b0 * T.nu, V.est = T.est ? T.est + b0 * T.nx : nullptr, V.age = T.age + b0;
    }
    return V;
}

// the largest violation of instance il's boxes: the score's rule
COPRA_DEV double trace_vmax(const TraceArgs& T, const TraceView& V, int il)
{
    double vmax = 0.0;
    if (T.x_lo || T.x_hi)
        for (int r = 0; r < T.nx; ++r) {
            const double v = score_violation(V.x[(size_t)il * T.nx + r], T.x_lo, T.x_hi, r);
            if (v > vmax) vmax = v;
        }
    if ((T.u_lo || T.u_hi) && V.age[il] != kPlantAgeHeld) // (the age decides BEFORE anything of u is touched)
        for (int c = 0; c < T.nu; ++c) {
            const double v = score_violation(V.u[(size_t)il * T.nu + c], T.u_lo, T.u_hi, c);
            if (v > vmax) vmax = v;
        }
    return vmax;
}

// instance il's value of row `row` of the slot; NaN: it has none
COPRA_DEV double trace_value(const TraceArgs& T, const TraceView& V, int il, int row)
{
    const double none = __builtin_nan("");
    int r = row;
    if (T.what & kTraceX) {
        if (r < T.nx) return V.x[(size_t)il * T.nx + r];
        r -= T.nx;
    }
    if (T.what & kTraceU) {
        if (r < T.nu) return V.age[il] != kPlantAgeHeld ? V.u[(size_t)il * T.nu + r] : none;
        r -= T.nu;
    }
    if (T.what & kTraceErr) {
        if (r < T.nx) return T.err_live ? V.est[(size_t)il * T.nx + r] - V.x[(size_t)il * T.nx + r] : none;
        r -= T.nx;
    }
    return trace_vmax(T, V, il);
}

// stage 1: a thread's own fold of row `row`, ascending from the empty statistic
COPRA_DEV ScoreStat trace_fold_stat(const TraceArgs& T, const TraceView& V, int wg, int tid, int row)
{
    ScoreStat acc = score_stat_empty();
    const int cnt = trace_chunk_count(T, wg);
    const long long first = (long long)wg * kScoreChunk;
    for (int il = tid; il < cnt; il += kScoreThreads) acc = score_stat_merge(acc, score_stat_one(trace_value(T, V, il, row), first + il));
    return acc;
}
// ... and of the counts: ticks stands for `solved`, the instance totals stay 0
COPRA_DEV ScoreCounts trace_fold_counts(const TraceArgs& T, const TraceView& V, int wg, int tid)
{
    ScoreCounts acc = score_counts_empty();
    const int cnt = trace_chunk_count(T, wg);
    const bool limits = trace_has_limits(T);
    for (int il = tid; il < cnt; il += kScoreThreads) {
        const int age = V.age[il];
        ScoreCounts c = score_counts_empty();
        c.ticks = age == 0, c.held = age == kPlantAgeHeld, c.replayed = age >= 1, c.fallback = age == kPlantAgeFallback;
        c.violating = limits && trace_vmax(T, V, il) > T.tol;
        acc = score_counts_merge(acc, c);
    }
    return acc;
}
// stage 2: the folds over the partials
COPRA_DEV const unsigned char* trace_partial(const TraceArgs& T, long long c) { return T.part + (size_t)c * trace_slot_bytes(trace_rows(T)); }
COPRA_DEV ScoreStat trace_fold_stat2(const TraceArgs& T, int tid, int row)
{
    ScoreStat acc = score_stat_empty();
    for (long long c = tid; c < T.chunks; c += kScoreThreads)
        acc = score_stat_merge(acc, reinterpret_cast<const ScoreStat*>(trace_partial(T, c) + sizeof(TraceHead))[row]);
    return acc;
}
COPRA_DEV ScoreCounts trace_fold_counts2(const TraceArgs& T, int tid)
{
    ScoreCounts acc = score_counts_empty();
    for (long long c = tid; c < T.chunks; c += kScoreThreads) acc = score_counts_merge(acc, *reinterpret_cast<const ScoreCounts*>(trace_partial(T, c)));
    return acc;
}
// what thread 0 stores: a row and the head of partial `wg` (stage 1) or of the slot (stage 2)
COPRA_DEV void trace_store_stat(const TraceArgs& T, int stage, int wg, int row, const ScoreStat& s)
{
    unsigned char* const out = stage == 1 ? T.part + (size_t)wg * trace_slot_bytes(trace_rows(T)) : T.slot;
    reinterpret_cast<ScoreStat*>(out + sizeof(TraceHead))[row] = s;
}
COPRA_DEV void trace_store_counts(const TraceArgs& T, int stage, int wg, const ScoreCounts& c)
{
    if (stage == 1) {
        *reinterpret_cast<ScoreCounts*>(T.part + (size_t)wg * trace_slot_bytes(trace_rows(T))) = c;
        return;
    }
    TraceHead h;
    h.tick = T.tick, h.tau = T.tau, h.solved = c.ticks, h.replayed = c.replayed, h.fallback = c.fallback, h.held = c.held, h.violating = c.violating, h.reserved = 0;
    *reinterpret_cast<TraceHead*>(T.slot) = h;
}

#if defined(__HIPCC__) && !defined(COPRA_TRACE_HELPERS_ONLY) // (copra_hip_trace_quant.hip takes the helpers alone: the kernels have ONE home, copra_hip_trace.hip)
// One part (a row, or the counts) of one workgroup, done by ONE wave: its lane l plays the threads l, 64 + l, 128 + l, 192 + l of the written
// order -- four folds, then the lane tree of the four waves side by side, four chains that do not depend on each other and hide each other's
// latency (a merge is two divisions deep) --, and lane 0 folds the four in ascending order.  Which wave computes a part changes no bit of it:
// the order of the merges is the written one.  No barrier and no LDS stands between two parts, and the workgroup's waves take parts in turn.
template <class Part, class Fold, class Merge>
__device__ __forceinline__ Part trace_part(int lane, Fold fold, Merge merge)
{
    constexpr int W = kScoreThreads / 64;
    Part acc[W];
    COPRA_SCORE_UNROLL
    for (int w = 0; w < W; ++w) acc[w] = fold(64 * w + lane);
    for (int off = 32; off >= 1; off >>= 1) {
        COPRA_SCORE_UNROLL
        for (int w = 0; w < W; ++w) acc[w] = merge(acc[w], score_shfl_down(acc[w], off));
    }
    Part all = acc[0];
    COPRA_SCORE_UNROLL
    for (int w = 1; w < W; ++w) all = merge(all, acc[w]);
    return all; // (lane 0's is the workgroup's)
}

template <int kStage>
__global__ __launch_bounds__(kScoreThreads) void copra_trace_kernel(const TraceArgs T)
{
    extern __shared__ __align__(16) double trace_image[];
    const int wg = (int)blockIdx.x, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    TraceView V {};
    if (kStage == 1) {
        trace_stage(T, wg, tid, kScoreThreads, trace_image);
        __syncthreads();
        V = trace_view(T, wg, trace_image);
    }
    const int rows = trace_rows(T);
    for (int part = wave; part <= rows; part += kScoreThreads / 64) { // (part `rows`: the counts)
        if (part < rows) {
            const ScoreStat all = trace_part<ScoreStat>(
                lane, [&](int t) { return kStage == 1 ? trace_fold_stat(T, V, wg, t, part) : trace_fold_stat2(T, t, part); },
                [](const ScoreStat& a, const ScoreStat& b) { return score_stat_merge(a, b); });
            if (lane == 0) trace_store_stat(T, kStage, wg, part, all);
        } else {
            const ScoreCounts all = trace_part<ScoreCounts>(
                lane, [&](int t) { return kStage == 1 ? trace_fold_counts(T, V, wg, t) : trace_fold_counts2(T, t); },
                [](const ScoreCounts& a, const ScoreCounts& b) { return score_counts_merge(a, b); });
            if (lane == 0) trace_store_counts(T, kStage, wg, all);
        }
    }
}
#endif

} // namespace copra_hip
