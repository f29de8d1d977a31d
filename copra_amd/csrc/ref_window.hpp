// ref_window.hpp -- the window of a reference schedule that the horizon sees, on the device (copra_batch_set_reference_schedule,
// copra_batch_schedule_seek and the tick of copra_batch_advance / copra_batch_rollout; launched from copra_hip_plant.hip).  The reference
// moves its reference by replacing the cost object between solves (include/costFunctions.h:103-219, src/LMPC.cpp:233-247); here the caller
// hands the whole signal over once and every tick, for every scheduled cost and every instance b,
//   p[b][s r + i] = sched[b or 0][min(first + s, steps - 1)][i],   s = 0 .. S-1,  first = tau + offset
// is written into the per-instance reference buffer every kernel already reads (the last block is held beyond the end of the schedule).
//
// A streaming gather.  A window is ONE contiguous range of the schedule -- `live` blocks from block f0 = min(first, steps - 1) -- followed by
// S - live copies of the last block, which only exist near the end of the signal.  One launch serves all scheduled costs (descriptors in the
// kernel argument, at most kRefWindowMax); a workgroup takes `group` consecutive instances of every cost.  Its T threads form lx x ly, lx
// the power of two that covers one window: consecutive lanes write consecutive doubles (16 bytes per lane where the host found the pointers
// and sizes to allow it, ref_window_prepare), the ly rows walk the instances, whose windows are contiguous in the output.
//   shared schedule:  a lane loads its piece of the window ONCE (it stays in L2 for the other workgroups) and stores it to its instances;
//                     the clamp is applied per loaded double, so only the output decides about 16-byte stores
//   per instance:     a copy of live r doubles per instance, then the held tail (the only place with a division; empty until the end)
// Index arithmetic stays outside the store loops: they advance pointers.  No atomics, no LDS, no scratch, ordinary (cached) stores -- the
// next kernel reads them.  The body is a COPRA_DEV function of (workgroup, thread) that also compiles on the host: tests/emu/emu_ref_window.cpp
// walks it thread by thread.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef COPRA_DEV
#if defined(__HIPCC__)
#define COPRA_DEV __device__ __forceinline__
#else
#define COPRA_DEV inline
#endif
#endif

#if defined(__HIPCC__)
#define COPRA_REFWIN_HD __host__ __device__ inline // (the launch is shaped with the functions the kernel reads its windows with)
#else
#define COPRA_REFWIN_HD inline
#endif

namespace copra_hip {

constexpr int kRefWindowMax = 8; // scheduled costs one launch serves
constexpr int kRefWindowGroup = 64; // instances per workgroup

struct RefWindowCost {
    const double* sched; // [per_instance ? batch : 1][steps][r]
    double* out; // [batch][S r]
    long long steps;
    long long first; // tau + offset: the block step 0 of the window reads
    int r, S;
    int per_instance;
    int vec2; // (ref_window_prepare) two doubles per lane
    int lx_log2; // (ref_window_prepare) lanes along one window: 1 << lx_log2 of the workgroup's threads
};

struct RefWindowArgs {
    int batch, ncost;
    int group; // instances per workgroup
    RefWindowCost c[kRefWindowMax];
};

struct alignas(16) RefPair {
    double a, b;
};

COPRA_REFWIN_HD bool ref_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the contiguous part of a window: it starts at block f0 and holds liveW doubles of the S r
struct RefWindowSpan {
    long long f0r, lastr; // offsets (doubles, within one schedule) of block f0 and of the last block
    int W, liveW;
};
COPRA_REFWIN_HD RefWindowSpan ref_window_span(const RefWindowCost& c)
{
    RefWindowSpan s;
    const long long last = c.steps - 1, f0 = c.first < last ? c.first : last, rem = c.steps - f0;
    s.W = c.r * c.S;
    s.liveW = (rem < c.S ? (int)rem : c.S) * c.r;
    s.f0r = f0 * c.r;
    s.lastr = last * c.r;
    return s;
}

// (host) how one launch of T threads (a power of two) per workgroup copies: 16 bytes per lane where every address of the copy is a multiple of
// 16 -- the output's base and an even window; for a per-instance schedule also its base, an even schedule per instance, an even start and an
// even contiguous part (a shared schedule is loaded once per lane: its alignment is looked at there) -- and how many lanes cover one window
inline void ref_window_prepare(RefWindowArgs& P, int T)
{
    int tlog = 0;
    while ((1 << (tlog + 1)) <= T) ++tlog;
    for (int k = 0; k < P.ncost; ++k) {
        RefWindowCost& c = P.c[k];
        const RefWindowSpan s = ref_window_span(c);
        bool v = ref_aligned16(c.out) && s.W % 2 == 0;
        if (c.per_instance) v = v && ref_aligned16(c.sched) && (c.steps * c.r) % 2 == 0 && s.f0r % 2 == 0 && s.liveW % 2 == 0;
        c.vec2 = v ? 1 : 0;
        const int units = v ? s.W / 2 : s.W;
        c.lx_log2 = 0;
        while (c.lx_log2 < tlog && (1 << c.lx_log2) < units) ++c.lx_log2;
    }
}

// entry e of a window whose schedule starts at src
COPRA_DEV double ref_window_at(const double* src, const RefWindowSpan& s, int r, int e)
{
    return e < s.liveW ? src[s.f0r + e] : src[s.lastr + (e - s.liveW) % r];
}

// the windows of instances b0 .. b0 + cnt of one cost, thread tid of T
COPRA_DEV void ref_window_cost(const RefWindowCost& c, int b0, int cnt, int tid, int T)
{
    const RefWindowSpan s = ref_window_span(c);
    const int lx = 1 << c.lx_log2, ly = T >> c.lx_log2, tx = tid & (lx - 1), ty = tid >> c.lx_log2;
    double* const out0 = c.out + (size_t)b0 * s.W;
    if (!c.per_instance) {
        if (c.vec2) {
            const int W2 = s.W >> 1;
            const bool pair_src = ref_aligned16(c.sched) && (s.f0r & 1) == 0;
            for (int k = tx; k < W2; k += lx) {
                RefPair v;
                if (pair_src && 2 * k + 1 < s.liveW) {
                    v = *reinterpret_cast<const RefPair*>(c.sched + s.f0r + 2 * k);
                } else {
                    v.a = ref_window_at(c.sched, s, c.r, 2 * k);
                    v.b = ref_window_at(c.sched, s, c.r, 2 * k + 1);
                }
                RefPair* d = reinterpret_cast<RefPair*>(out0) + (size_t)ty * W2 + k;
                for (int i = ty; i < cnt; i += ly, d += (size_t)ly * W2) *d = v;
            }
        } else {
            for (int k = tx; k < s.W; k += lx) {
                const double v = ref_window_at(c.sched, s, c.r, k);
                double* d = out0 + (size_t)ty * s.W + k;
                for (int i = ty; i < cnt; i += ly, d += (size_t)ly * s.W) *d = v;
            }
        }
        return;
    }
    const size_t per = (size_t)c.steps * c.r;
    const double* src = c.sched + (size_t)(b0 + ty) * per;
    double* dst = out0 + (size_t)ty * s.W;
    for (int i = ty; i < cnt; i += ly, src += (size_t)ly * per, dst += (size_t)ly * s.W) {
        if (c.vec2) {
            const RefPair* s2 = reinterpret_cast<const RefPair*>(src + s.f0r);
            RefPair* d2 = reinterpret_cast<RefPair*>(dst);
            for (int k = tx; k < (s.liveW >> 1); k += lx) d2[k] = s2[k];
        } else {
            const double* s1 = src + s.f0r;
            for (int k = tx; k < s.liveW; k += lx) dst[k] = s1[k];
        }
        for (int e = s.liveW + tx; e < s.W; e += lx) dst[e] = src[s.lastr + (e - s.liveW) % c.r]; // held beyond the end
    }
}

COPRA_DEV void ref_window_body(const RefWindowArgs& P, int wg, int tid, int T)
{
    const int b0 = wg * P.group;
    const int cnt = (P.batch - b0 < P.group) ? P.batch - b0 : P.group;
    if (cnt <= 0) return;
    for (int k = 0; k < P.ncost; ++k) ref_window_cost(P.c[k], b0, cnt, tid, T);
}

#if defined(__HIPCC__)
constexpr int kRefWindowThreads = 256;
__global__ __launch_bounds__(kRefWindowThreads) void copra_ref_window_kernel(const RefWindowArgs P)
{
    ref_window_body(P, (int)blockIdx.x, (int)threadIdx.x, kRefWindowThreads);
}
#endif

} // namespace copra_hip
