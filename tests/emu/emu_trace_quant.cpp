// emu_trace_quant.cpp -- the quantile kernel's bodies (copra_amd/csrc/trace_quant_step.hpp) on the host: one workgroup per row; every pass
// walked thread by thread in the walk orders of emu_walk.h with a plain increment where the device makes an LDS atomic add (integer sums have
// no order); the scan of every level lane by lane, the sum of the lanes before a lane where the device shuffles.  The LDS block and the key
// buffer start out as garbage -- what is read must have been written -- and a guard stands behind the keys.  The expectation
// (tests/trace_quant_ref.py) is a sort.
#include "emu_trace_quant.h"

#include "../../copra_amd/csrc/trace_quant_step.hpp"
#include "emu_walk.h"

#include <vector>

using namespace copra_hip;

static_assert(sizeof(EmuQuantClock) == sizeof(TraceClock), "the clock of the header is trace_step.hpp's");

static const auto add_plain = [](unsigned* hist, unsigned bin, bool active) {
    if (active) hist[bin] += 1;
};

// the kernel, for one row
static void walk_row(const QuantArgs& Q, int row, int order, unsigned long long seed)
{
    QuantLds L;
    std::memset(&L, 0xA5, sizeof L);
    uint64_t salt = 1 + (uint64_t)row * 64;
    for (int tid : emu::order_of(kQuantThreads, order, seed, salt++)) quant_clear(L, tid, kQuantThreads);
    for (int pass = 0; pass < kQuantPasses; ++pass) {
        for (int tid : emu::order_of(kQuantThreads, order, seed, salt++)) {
            if (pass == 0) quant_pass0(Q, L, row, tid, kQuantThreads, add_plain);
            else quant_pass(Q, L, row, tid, kQuantThreads, pass, add_plain);
        }
        for (int q : emu::order_of(Q.nq, order, seed, salt++)) { // wave q scans level q
            unsigned own[64], below[64], total = 0;
            for (int lane = 0; lane < 64; ++lane) own[lane] = quant_lane_sum(L, q, lane);
            for (int lane = 0; lane < 64; ++lane) below[lane] = total, total += own[lane];
            const unsigned k = pass == 0 ? (total ? quant_rank(Q.level[q], total) : 0u) : L.k[q]; // (read by every lane before one of them writes)
            if (pass == 0 && q == 0) L.n = total;
            if (total)
                for (int lane : emu::order_of(64, order, seed, salt++)) quant_lane_pick(L, q, lane, below[lane], own[lane], k);
        }
        if (L.n == 0) break;
        if (pass + 1 < kQuantPasses)
            for (int tid : emu::order_of(kQuantThreads, order, seed, salt++)) quant_regroup(L, Q.nq, tid, kQuantThreads);
    }
    for (int tid : emu::order_of(kQuantThreads, order, seed, salt++)) quant_store(Q, L, row, tid);
}

extern "C" {

int emu_trace_quant_tick(EmuQuantTick* t)
{
    QuantArgs Q {};
    TraceArgs& T = Q.T;
    T.batch = t->batch, T.nx = t->nx, T.nu = t->nu, T.what = t->what;
    T.err_live = t->est != nullptr;
    T.x = t->x, T.u = t->u, T.est = t->est, T.age = t->age;
    T.x_lo = t->x_lo, T.x_hi = t->x_hi, T.u_lo = t->u_lo, T.u_hi = t->u_hi;
    T.in_lds = 0, T.vec2 = 0;
    const int rows = trace_rows(T);
    t->rows = rows;
    if (t->nq < 1 || t->nq > kQuantMax) return emu::kEmuNoMemory;
    Q.nq = t->nq;
    for (int q = 0; q < kQuantMax; ++q) Q.level[q] = q < t->nq ? t->level[q] : 0.0;
    const size_t count = (size_t)rows * (size_t)T.batch;
    std::vector<unsigned long long> keys(count + emu::kEmuGuard);
    for (size_t i = 0; i < count; ++i) keys[i] = 0x8000000000000000ull + i; // (garbage that would count as a finite key)
    for (int i = 0; i < emu::kEmuGuard; ++i) keys[count + i] = emu::kEmuGuardBits;
    Q.keys = keys.data();
    Q.out = t->out;
    for (int row : emu::order_of(rows, t->order, t->seed, 0)) walk_row(Q, row, t->order, t->seed);
    for (int i = 0; i < emu::kEmuGuard; ++i)
        if (keys[count + i] != emu::kEmuGuardBits) return emu::kEmuGuardTouched;
    return 0;
}

long long emu_trace_quant_record(EmuQuantTick* t, EmuQuantClock* clock, double* buffer)
{
    TraceClock c { clock->tick, clock->recorded, clock->missed, clock->capacity, clock->every };
    long long tick = 0;
    const long long slot = trace_next_slot(c, &tick);
    clock->tick = c.tick, clock->recorded = c.recorded, clock->missed = c.missed;
    if (slot < 0) return -1;
    const int limits = t->x_lo || t->x_hi || t->u_lo || t->u_hi;
    t->out = buffer + (size_t)slot * (size_t)trace_rows(t->what, t->nx, t->nu, limits) * (size_t)t->nq;
    const int rc = emu_trace_quant_tick(t);
    return rc == 0 ? slot : -10 + rc;
}

unsigned long long emu_trace_quant_key(double v) { return quant_key(v); }
long long emu_trace_quant_rank(double p, long long n) { return (long long)quant_rank(p, (unsigned)n); }
int emu_trace_quant_sizes(int* max_levels, int* threads, int* lds_bytes)
{
    *max_levels = kQuantMax, *threads = kQuantThreads, *lds_bytes = (int)sizeof(QuantLds);
    return 0;
}
}
