// emu_trace.cpp -- the trace kernel's bodies (copra_amd/csrc/trace_step.hpp) on the host: stage 1's copy walked thread by thread over a NaN-filled
// image with the guard words and the walk orders of emu_walk.h, every thread's own fold, and the documented tree applied lane by lane; stage 2
// over the partials likewise.  Compile with -ffp-contract=off: the expectation (tests/trace_ref.py) rounds every product and every sum.
#include "emu_trace.h"

#include "../../copra_amd/csrc/trace_step.hpp"
#include "emu_walk.h"

#include <vector>

using namespace copra_hip;

static_assert(sizeof(EmuTraceClock) == sizeof(TraceClock), "the clock of the header is trace_step.hpp's");

// one workgroup's part of the kernel: every thread's fold in the walk's order, the lane tree of every wave, thread 0's fold of the waves
template <class Part, class Fold, class Merge>
static Part workgroup_part(const std::vector<int>& threads, Fold fold, Merge merge)
{
    std::vector<Part> lane((size_t)kScoreThreads);
    for (int tid : threads) lane[(size_t)tid] = fold(tid);
    for (int w = 0; w < kScoreThreads / 64; ++w)
        for (int off = 32; off >= 1; off >>= 1)
            for (int l = 0; l + off < 64; ++l) // (ascending: lane l + off still holds the value of before this step)
                lane[(size_t)(64 * w + l)] = merge(lane[(size_t)(64 * w + l)], lane[(size_t)(64 * w + l + off)]);
    Part acc = lane[0];
    for (int w = 1; w < kScoreThreads / 64; ++w) acc = merge(acc, lane[(size_t)(64 * w)]);
    return acc;
}
static const auto merge_stat = [](const ScoreStat& a, const ScoreStat& b) { return score_stat_merge(a, b); };
static const auto merge_counts = [](const ScoreCounts& a, const ScoreCounts& b) { return score_counts_merge(a, b); };

static void stage2(const TraceArgs& T, int order, unsigned long long seed)
{
    const int rows = trace_rows(T);
    const std::vector<int> threads = emu::order_of(kScoreThreads, order, seed, 99);
    for (int row = 0; row < rows; ++row)
        trace_store_stat(T, 2, 0, row, workgroup_part<ScoreStat>(threads, [&](int tid) { return trace_fold_stat2(T, tid, row); }, merge_stat));
    trace_store_counts(T, 2, 0, workgroup_part<ScoreCounts>(threads, [&](int tid) { return trace_fold_counts2(T, tid); }, merge_counts));
}

extern "C" {

int emu_trace_tick(EmuTraceTick* t)
{
    TraceArgs T {};
    T.batch = t->batch, T.nx = t->nx, T.nu = t->nu, T.what = t->what;
    T.err_live = t->est != nullptr;
    T.x = t->x, T.u = t->u, T.est = t->est, T.age = t->age;
    T.x_lo = t->x_lo, T.x_hi = t->x_hi, T.u_lo = t->u_lo, T.u_hi = t->u_hi;
    T.tol = t->tol, T.tick = t->tick, T.tau = t->tau;
    T.chunks = score_chunks(T.batch);
    T.in_lds = t->lds_mode < 0 ? trace_in_lds(T.nx, T.nu, T.what, T.x_lo || T.x_hi, T.u_lo || T.u_hi) : t->lds_mode;
    T.vec2 = t->vec2_mode < 0 ? trace_vec2_ok(T) : 0;
    const int rows = trace_rows(T);
    t->rows = rows, t->lds_used = T.in_lds, t->vec2_used = T.vec2;
    std::vector<unsigned char> part((size_t)T.chunks * trace_slot_bytes(rows));
    T.part = part.data();
    T.slot = static_cast<unsigned char*>(t->slot);
    const TraceLds L = trace_lds(T);
    t->lds_doubles = T.in_lds ? L.total : 0;
    emu::Image img((size_t)t->lds_doubles);
    if (!img.lds) return emu::kEmuNoMemory;
    for (int wg : emu::order_of((int)T.chunks, t->order, t->seed, 0)) {
        img.fill_nan();
        for (int tid : emu::order_of(kScoreThreads, t->order, t->seed, 1 + (uint64_t)wg * 8)) trace_stage(T, wg, tid, kScoreThreads, img.lds);
        const TraceView V = trace_view(T, wg, img.lds);
        const std::vector<int> threads = emu::order_of(kScoreThreads, t->order, t->seed, 2 + (uint64_t)wg * 8);
        for (int row = 0; row < rows; ++row)
            trace_store_stat(T, 1, wg, row, workgroup_part<ScoreStat>(threads, [&](int tid) { return trace_fold_stat(T, V, wg, tid, row); }, merge_stat));
        trace_store_counts(T, 1, wg, workgroup_part<ScoreCounts>(threads, [&](int tid) { return trace_fold_counts(T, V, wg, tid); }, merge_counts));
        if (!img.guard_intact()) return emu::kEmuGuardTouched;
    }
    stage2(T, t->order, t->seed);
    return 0;
}

long long emu_trace_record(EmuTraceTick* t, EmuTraceClock* clock, void* buffer)
{
    TraceClock c { clock->tick, clock->recorded, clock->missed, clock->capacity, clock->every };
    long long tick = 0;
    const long long slot = trace_next_slot(c, &tick);
    clock->tick = c.tick, clock->recorded = c.recorded, clock->missed = c.missed;
    if (slot < 0) return -1;
    const int limits = t->x_lo || t->x_hi || t->u_lo || t->u_hi;
    t->tick = tick;
    t->slot = static_cast<unsigned char*>(buffer) + (size_t)slot * trace_slot_bytes(trace_rows(t->what, t->nx, t->nu, limits));
    const int rc = emu_trace_tick(t);
    return rc == 0 ? slot : -10 + rc;
}

int emu_trace_stage2(int rows, long long chunks, const void* partials, long long tick, long long tau, void* slot)
{
    TraceArgs T {};
    T.what = kTraceX, T.nx = rows, T.nu = 0; // (rows of one group and no limits: the slot's shape is all stage 2 looks at)
    T.chunks = chunks, T.tick = tick, T.tau = tau;
    T.part = const_cast<unsigned char*>(static_cast<const unsigned char*>(partials));
    T.slot = static_cast<unsigned char*>(slot);
    stage2(T, 0, 0);
    return 0;
}

int emu_trace_rows(int what, int nx, int nu, int limits) { return trace_rows(what, nx, nu, limits); }
long long emu_trace_slot_bytes(int rows) { return (long long)trace_slot_bytes(rows); }
int emu_trace_in_lds(int nx, int nu, int what, int x_limits, int u_limits) { return trace_in_lds(nx, nu, what, x_limits, u_limits); }
int emu_trace_sizes(int* head, int* stat)
{
    *head = (int)sizeof(TraceHead), *stat = (int)sizeof(ScoreStat);
    return 0;
}
}
