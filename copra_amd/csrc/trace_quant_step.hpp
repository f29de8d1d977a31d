// trace_quant_step.hpp -- trace quantiles on the device (copra_batch_set_trace_quantiles, ABI 18; host side: copra_hip_trace_quant.hip).  Behind the
// two launches of a recorded tick's trace ONE more launch selects, for every row of the slot and every level p, an order statistic of the
// row's finite values -- the values trace_value / trace_vmax of trace_step.hpp form, the same rows in the same order x | u | err | viol:
//   V    the instances whose value is finite, n = |V| (the n of the row's statistic in the slot)
//   key  of the value's 64 bits b:  key = b ^ (b >> 63 ? ~0ull : 1ull << 63)  -- ascending keys are ascending numbers, -0.0 before +0.0
//   k    c = ceil(p * (double)n), one FP64 multiply, then k = min(n - 1, max(0, c - 1)); the quantile is the k-th key of V ascending, 0-based
//   n == 0: the quiet NaN 0x7FF8000000000000
// An order statistic is an element of the data: whatever way it is found, the result has one right set of bytes.  The way here is a
// most-significant-digit-first radix select, one workgroup of kQuantThreads threads per row, eight passes of eight bits:
//   pass 0   every thread forms its instances' values, stores their keys into the key buffer [rows][batch] (the passes behind read keys 8
//            bytes apart, not values nx doubles apart, and the viol row is computed once) and counts the finite ones by their top digit in a
//            histogram of 256 counts in LDS.  The histogram's total is n; every level's k follows from it.
//   scan     wave q takes level q: lane l sums bins 4 l .. 4 l + 3, a shuffle scan gives what lies below, the lane whose range holds k picks
//            the digit, subtracts what lies below it from k and extends the level's prefix by the digit.
//   pass d   a key whose top d digits are a level's prefix counts in that level's histogram by digit d.  Levels with the same prefix share
//            one histogram (the lowest such level's: its `leader`): the top digits of a physical row are the same for every level.
//   after pass 7 the prefix is the key; the transform is inverted and stored.
// The counts are LDS integer atomics.  In the first passes most lanes of a wave hit ONE bin and an atomic to one address serialises, so the
// wave counts first (quant_add_wave): ballot on the first active lane's digit, one add of the popcount, kQuantRounds times; lanes left over
// add one each -- the low digits are close to uniform, where that is the cheaper way.  A key is finite exactly when it lies in
// [kQuantKeyLo, kQuantKeyHi): no marker is stored.  No floating-point atomics, no scratch, no workgroup waits for another, nothing on the
// device counts slots.  The phase bodies are COPRA_DEV functions of (row, thread) or (level, lane) that compile on the host
// (tests/emu/emu_trace_quant.cpp); `add` is the one thing the two sides do differently, and integer sums have no order.
#pragma once
#include "trace_step.hpp"

#include <cmath>

namespace copra_hip {

constexpr int kQuantMax = 8; // COPRA_TRACE_QUANT_MAX
constexpr int kQuantThreads = 1024; // one workgroup per row: sixteen waves hide each other's loads
constexpr int kQuantBins = 256, kQuantPasses = 8;
constexpr int kQuantInFlight = 4; // loads of one thread issued before the first of them is counted
#ifndef COPRA_QUANT_ROUNDS
#define COPRA_QUANT_ROUNDS 2 // ballot rounds of the wave-level pre-count; 0: plain atomics
#endif
constexpr int kQuantRounds = COPRA_QUANT_ROUNDS;
constexpr unsigned long long kQuantKeyLo = 0x0010000000000000ull, kQuantKeyHi = 0xFFF0000000000000ull; // keys of -DBL_MAX and of +inf
constexpr unsigned long long kQuantNaN = 0x7FF8000000000000ull;
static_assert(kQuantThreads / 64 >= kQuantMax && kQuantBins == 4 * 64, "a wave per level, four bins per lane");

struct QuantArgs {
    TraceArgs T; // the tick as the trace saw it, in_lds = 0: the values are read from global memory
    int nq;
    double level[kQuantMax];
    unsigned long long* keys; // [rows][batch], work buffer of the setter
    double* out; // [rows][nq] of the slot the host counted
};

struct QuantLds {
    unsigned hist[kQuantMax][kQuantBins];
    unsigned long long prefix[kQuantMax]; // the top digits chosen so far
    unsigned k[kQuantMax]; // the rank among the keys with that prefix
    int leader[kQuantMax]; // the lowest level with the same prefix: its histogram counts for this one too
    unsigned n;
};

COPRA_PLANT_HD unsigned long long quant_bits(double v)
{
    unsigned long long b;
    __builtin_memcpy(&b, &v, sizeof b);
    return b;
}
COPRA_PLANT_HD unsigned long long quant_key(double v)
{
    const unsigned long long b = quant_bits(v);
    return b ^ ((b >> 63) ? ~0ull : 1ull << 63);
}
COPRA_PLANT_HD unsigned long long quant_unkey(unsigned long long key) { return key ^ ((key >> 63) ? 1ull << 63 : ~0ull); } // (the value's bits)
COPRA_PLANT_HD bool quant_key_finite(unsigned long long key) { return key - kQuantKeyLo < kQuantKeyHi - kQuantKeyLo; }
// the rank of level p among n > 0 values
COPRA_PLANT_HD unsigned quant_rank(double p, unsigned n)
{
    const double c = ceil(p * (double)n);
    const long long k = (long long)c - 1;
    return k < 0 ? 0u : (k > (long long)n - 1 ? n - 1 : (unsigned)k);
}

// before pass 0: empty histograms, empty prefixes, every level led by level 0
COPRA_DEV void quant_clear(QuantLds& L, int tid, int nthreads)
{
    for (int i = tid; i < kQuantMax * kQuantBins; i += nthreads) L.hist[i / kQuantBins][i % kQuantBins] = 0;
    if (tid < kQuantMax) L.prefix[tid] = 0, L.k[tid] = 0, L.leader[tid] = 0;
    if (tid == 0) L.n = 0;
}

// the whole batch as trace_value indexes it, where it lies in global memory
COPRA_DEV TraceView quant_view(const TraceArgs& T)
{
    TraceView V;
    V.x = T.x, V.u = T.u, V.est = T.est, V.age = T.age;
    return V;
}

// pass 0 of row `row`: the values, their keys into the key buffer, the finite ones counted by their top digit.  add(hist, bin, active) is
// called by every thread of a wave together
template <class Add>
COPRA_DEV void quant_pass0(const QuantArgs& Q, QuantLds& L, int row, int tid, int nthreads, Add add)
{
    const TraceView V = quant_view(Q.T);
    unsigned long long* const keys = Q.keys + (size_t)row * (size_t)Q.T.batch;
    for (long long base = 0; base < Q.T.batch; base += (long long)kQuantInFlight * nthreads) {
        unsigned long long key[kQuantInFlight];
        COPRA_SCORE_UNROLL
        for (int j = 0; j < kQuantInFlight; ++j) {
            const long long i = base + (long long)j * nthreads + tid;
            key[j] = i < Q.T.batch ? quant_key(trace_value(Q.T, V, (int)i, row)) : 0; // (0 is no finite key)
        }
        COPRA_SCORE_UNROLL
        for (int j = 0; j < kQuantInFlight; ++j) {
            const long long i = base + (long long)j * nthreads + tid;
            if (i < Q.T.batch) keys[i] = key[j];
            add(L.hist[0], (unsigned)(key[j] >> 56), quant_key_finite(key[j]));
        }
    }
}

// pass d = 1 .. 7: the keys whose top d digits are a leader's prefix, counted by digit d in the leader's histogram
template <class Add>
COPRA_DEV void quant_pass(const QuantArgs& Q, QuantLds& L, int row, int tid, int nthreads, int pass, Add add)
{
    const unsigned long long* const keys = Q.keys + (size_t)row * (size_t)Q.T.batch;
    unsigned long long want[kQuantMax]; // a leader's prefix; ~0 (no prefix of fewer than 64 bits) for the others
    COPRA_SCORE_UNROLL
    for (int q = 0; q < kQuantMax; ++q) want[q] = q < Q.nq && L.leader[q] == q ? L.prefix[q] : ~0ull;
    const int above = 64 - 8 * pass, at = 56 - 8 * pass;
    for (long long base = 0; base < Q.T.batch; base += (long long)kQuantInFlight * nthreads) {
        unsigned long long key[kQuantInFlight];
        COPRA_SCORE_UNROLL
        for (int j = 0; j < kQuantInFlight; ++j) {
            const long long i = base + (long long)j * nthreads + tid;
            key[j] = i < Q.T.batch ? keys[i] : 0;
        }
        COPRA_SCORE_UNROLL
        for (int j = 0; j < kQuantInFlight; ++j) {
            const bool finite = quant_key_finite(key[j]);
            const unsigned long long top = key[j] >> above;
            const unsigned bin = (unsigned)(key[j] >> at) & (kQuantBins - 1);
            COPRA_SCORE_UNROLL
            for (int q = 0; q < kQuantMax; ++q) {
                if (q >= Q.nq) break;
                add(L.hist[q], bin, finite && top == want[q]);
            }
        }
    }
}

// the scan of level q, lane by lane: the lane's four bins of the level's histogram ...
COPRA_DEV unsigned quant_lane_sum(const QuantLds& L, int q, int lane)
{
    const unsigned* const h = L.hist[L.leader[q]] + 4 * lane;
    return h[0] + h[1] + h[2] + h[3];
}
// ... and, with `below` the sum of the lanes before it and k the level's rank, the pick: the lane whose bins hold rank k extends the prefix
COPRA_DEV void quant_lane_pick(QuantLds& L, int q, int lane, unsigned below, unsigned own, unsigned k)
{
    if (k < below || k - below >= own) return;
    const unsigned* const h = L.hist[L.leader[q]] + 4 * lane;
    unsigned left = k - below;
    int d = 0;
    while (left >= h[d]) left -= h[d], ++d; // (d < 4: left < own)
    L.prefix[q] = (L.prefix[q] << 8) | (unsigned long long)(4 * lane + d);
    L.k[q] = left;
}

// between two passes: who leads whom, and empty histograms
COPRA_DEV void quant_regroup(QuantLds& L, int nq, int tid, int nthreads)
{
    for (int i = tid; i < kQuantMax * kQuantBins; i += nthreads) L.hist[i / kQuantBins][i % kQuantBins] = 0;
    if (tid < nq) {
        int lead = tid;
        for (int q = tid - 1; q >= 0; --q)
            if (L.prefix[q] == L.prefix[tid]) lead = q;
        L.leader[tid] = lead;
    }
}

// after the last scan (or with n == 0): the row's quantiles
COPRA_DEV void quant_store(const QuantArgs& Q, const QuantLds& L, int row, int tid)
{
    if (tid >= Q.nq) return;
    const unsigned long long bits = L.n ? quant_unkey(L.prefix[tid]) : kQuantNaN;
    __builtin_memcpy(Q.out + (size_t)row * Q.nq + tid, &bits, sizeof bits);
}

#if defined(__HIPCC__) && !defined(COPRA_TRACE_QUANT_HELPERS_ONLY)
// the wave-level pre-count: while lanes remain (and for kQuantRounds rounds at most), the lanes with the first active lane's bin are counted
// by a ballot and that lane adds their number; what is left adds one each.  Called by all 64 lanes together.
struct QuantAddWave {
    int lane;
    __device__ __forceinline__ void operator()(unsigned* hist, unsigned bin, bool active) const
    {
        unsigned long long todo = __ballot(active);
        for (int r = 0; r < kQuantRounds && todo; ++r) {
            const int first = __ffsll((unsigned long long)todo) - 1;
            const unsigned b0 = (unsigned)__shfl((int)bin, first);
            const bool same = active && bin == b0;
            const unsigned long long m = __ballot(same);
            if (lane == first) atomicAdd(&hist[b0], (unsigned)__popcll(m));
            if (same) active = false;
            todo &= ~m;
        }
        if (active) atomicAdd(&hist[bin], 1u);
    }
};

__global__ __launch_bounds__(kQuantThreads) void copra_trace_quant_kernel(const QuantArgs Q)
{
    __shared__ QuantLds L;
    const int row = (int)blockIdx.x, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const QuantAddWave add { lane };
    quant_clear(L, tid, kQuantThreads);
    __syncthreads();
    for (int pass = 0; pass < kQuantPasses; ++pass) {
        if (pass == 0) quant_pass0(Q, L, row, tid, kQuantThreads, add);
        else quant_pass(Q, L, row, tid, kQuantThreads, pass, add);
        __syncthreads();
        if (wave < Q.nq) { // wave q scans level q
            const unsigned own = quant_lane_sum(L, wave, lane);
            unsigned upto = own;
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned t = (unsigned)__shfl_up((int)upto, off);
                if (lane >= off) upto += t;
            }
            const unsigned total = (unsigned)__shfl((int)upto, 63);
            const unsigned k = pass == 0 ? (total ? quant_rank(Q.level[wave], total) : 0u) : L.k[wave];
            if (pass == 0 && wave == 0 && lane == 0) L.n = total;
            if (total) quant_lane_pick(L, wave, lane, upto - own, own, k);
        }
        __syncthreads();
        if (L.n == 0) break; // (the same for every thread: pass 0 found no finite value)
        if (pass + 1 < kQuantPasses) {
            quant_regroup(L, Q.nq, tid, kQuantThreads);
            __syncthreads();
        }
    }
    quant_store(Q, L, row, tid);
}
#endif

} // namespace copra_hip
