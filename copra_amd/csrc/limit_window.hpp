// limit_window.hpp -- the window of a LIMIT schedule that the horizon sees, on the device (copra_batch_set_constraint_schedule,
// copra_batch_set_control_bound_schedule, copra_batch_schedule_seek and the tick of copra_batch_advance / copra_batch_rollout; launched from
// copra_hip_plant.hip behind the reference windows).  The reference moves a limit by replacing the constraint object between solves
// (include/constraints.h:114-308, src/LMPC.cpp:233-247); here the caller hands the whole signal over once and every tick, for every live
// window and every instance b,
//   out[b stride + row0 + s r + i] = sched[b or 0][preview ? min(first + s, steps - 1) : min(first, steps - 1)][i],  s = 0 .. S-1, first = tau + offset
// is written into the per-instance limit buffers every solver kernel already reads: row_f_inst ([batch][mgen], stride = mgen, row0 the
// constraint's first stacked row) and lb_inst / ub_inst ([batch][n], stride = n, row0 = 0).
//
// A streaming gather like ref_window.hpp, with three differences.  The output is STRIDED: a window is W = S r doubles inside an instance's
// `stride` doubles, and the doubles between windows belong to other constraints -- they are never touched.  preview == 0 BROADCASTS one
// block (the limit of the present tick at every step: what the axis solver's register builds keep).  And one launch serves all live limit
// windows (descriptors in the kernel argument, at most kLimitWindowMax; lower and upper bounds count as one each).
// A workgroup takes `group` consecutive instances of every window.  Its T threads form lx x ly, lx the power of two that covers one
// window: consecutive lanes write consecutive doubles of ONE window, the ly rows walk the instances.  A lane owns a piece of the window --
// one double, or two where limit_window_prepare found every address of the copy to be a multiple of 16 -- and works out where that piece
// comes from ONCE (the clamp, the held tail's division); the store loop over the instances only advances pointers.  A shared schedule is
// loaded once per lane (it stays in L2 for the other workgroups) and stored to the lane's instances.  No atomics, no LDS, no scratch,
// ordinary (cached) stores -- the solve reads them next.  The body is a COPRA_DEV function of (workgroup, thread) that also compiles on the
// host: tests/emu/emu_limit_window.cpp walks it thread by thread.
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
#define COPRA_LIMWIN_HD __host__ __device__ inline // (the launch is shaped with the functions the kernel reads its windows with)
#else
#define COPRA_LIMWIN_HD inline
#endif

namespace copra_hip {

constexpr int kLimitWindowMax = 8; // live limit windows one launch serves
constexpr int kLimitWindowGroup = 64; // instances per workgroup

struct LimitWindow {
    const double* sched; // [per_instance ? batch : 1][steps][r]
    double* out; // [batch][stride]: the window of instance b starts at out + b stride + row0
    long long steps;
    long long first; // tau + offset: the block step 0 of the window reads
    int stride, row0;
    int r, S;
    int per_instance;
    int preview; // 0: block min(first, steps - 1) at every step
    int vec2; // (limit_window_prepare) two doubles per lane
    int lx_log2; // (limit_window_prepare) lanes along one window: 1 << lx_log2 of the workgroup's threads
};

struct LimitWindowArgs {
    int batch, nwin;
    int group; // instances per workgroup
    LimitWindow w[kLimitWindowMax];
};

// two doubles moved as 16 bytes (a vector type of the compiler, host and device: a struct of two doubles as a local made the device compiler
// park it in LDS)
typedef double LimitPair __attribute__((vector_size(16)));

COPRA_LIMWIN_HD bool limit_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// A window is `liveW` doubles read contiguously from block f0 on, then copies of ONE held block: the last block of the schedule (near the
// end of the signal), or -- preview == 0 -- block f0 itself, with no contiguous part at all.
struct LimitWindowSpan {
    long long f0r, heldr; // offsets (doubles, within one schedule) of block f0 and of the held block
    int W, liveW;
};
COPRA_LIMWIN_HD LimitWindowSpan limit_window_span(const LimitWindow& c)
{
    LimitWindowSpan s;
    const long long last = c.steps - 1, f0 = c.first < last ? c.first : last, rem = c.steps - f0;
    s.W = c.r * c.S;
    s.f0r = f0 * c.r;
    if (c.preview) {
        s.liveW = (rem < c.S ? (int)rem : c.S) * c.r;
        s.heldr = last * c.r;
    } else {
        s.liveW = 0;
        s.heldr = s.f0r;
    }
    return s;
}
// where entry e of a window comes from (doubles, within one schedule)
COPRA_LIMWIN_HD long long limit_window_from(const LimitWindowSpan& s, int r, int e)
{
    return e < s.liveW ? s.f0r + e : s.heldr + (e - s.liveW) % r;
}

// (host) how one launch of T threads (a power of two) per workgroup copies.  16 bytes per lane only where EVERY address of the copy is a multiple
// of 16: the output's base, an even stride, an even first row and an even window; for a per-instance schedule the same on the source side -- its
// base, an even schedule per instance, an even start and an even contiguous part.  (A shared schedule is loaded once per lane, and so is the
// held block: whether such a load may take 16 bytes is looked at where it is made.)  The source-side conditions are stricter than safety
// needs -- the kernel decides per piece whether a 16-byte load is legal and otherwise loads twice 8 bytes into one 16-byte store --, so a
// per-instance schedule with odd r gives up store width at every second tick; they could be relaxed to the output side.  And how many
// lanes cover one window.
inline void limit_window_prepare(LimitWindowArgs& P, int T)
{
    int tlog = 0;
    while ((1 << (tlog + 1)) <= T) ++tlog;
    for (int k = 0; k < P.nwin; ++k) {
        LimitWindow& c = P.w[k];
        const LimitWindowSpan s = limit_window_span(c);
        bool v = limit_aligned16(c.out) && c.stride % 2 == 0 && c.row0 % 2 == 0 && s.W % 2 == 0;
        if (c.per_instance) v = v && limit_aligned16(c.sched) && (c.steps * c.r) % 2 == 0 && s.f0r % 2 == 0 && s.liveW % 2 == 0;
        c.vec2 = v ? 1 : 0;
        const int units = v ? s.W / 2 : s.W;
        c.lx_log2 = 0;
        while (c.lx_log2 < tlog && (1 << c.lx_log2) < units) ++c.lx_log2;
    }
}

// the windows of instances b0 .. b0 + cnt of one descriptor, thread tid of T
COPRA_DEV void limit_window_one(const LimitWindow& c, int b0, int cnt, int tid, int T)
{
    const LimitWindowSpan s = limit_window_span(c);
    const int lx = 1 << c.lx_log2, ly = T >> c.lx_log2, tx = tid & (lx - 1), ty = tid >> c.lx_log2;
    if (ty >= cnt) return;
    const size_t per = c.per_instance ? (size_t)c.steps * c.r : 0; // (a shared schedule: every instance reads the same doubles)
    const double* const src0 = c.sched + (size_t)(b0 + ty) * per;
    double* const out0 = c.out + (size_t)(b0 + ty) * c.stride + c.row0;
    const size_t sstep = (size_t)ly * per, dstep = (size_t)ly * c.stride;
    if (c.vec2) {
        const bool src16 = limit_aligned16(c.sched) && (per & 1) == 0;
        const int W2 = s.W >> 1;
        for (int k = tx; k < W2; k += lx) {
            const long long o0 = limit_window_from(s, c.r, 2 * k), o1 = limit_window_from(s, c.r, 2 * k + 1);
            double* d = out0 + 2 * k;
            if (src16 && o1 == o0 + 1 && (o0 & 1) == 0) { // the two doubles lie side by side on 16 bytes: one load
                const double* p = src0 + o0;
                if (!c.per_instance) {
                    const LimitPair v = *reinterpret_cast<const LimitPair*>(p);
                    for (int i = ty; i < cnt; i += ly, d += dstep) *reinterpret_cast<LimitPair*>(d) = v;
                } else {
                    for (int i = ty; i < cnt; i += ly, d += dstep, p += sstep) *reinterpret_cast<LimitPair*>(d) = *reinterpret_cast<const LimitPair*>(p);
                }
            } else {
                const double *p0 = src0 + o0, *p1 = src0 + o1;
                if (!c.per_instance) {
                    const LimitPair v = { *p0, *p1 };
                    for (int i = ty; i < cnt; i += ly, d += dstep) *reinterpret_cast<LimitPair*>(d) = v;
                } else {
                    for (int i = ty; i < cnt; i += ly, d += dstep, p0 += sstep, p1 += sstep) *reinterpret_cast<LimitPair*>(d) = LimitPair { *p0, *p1 };
                }
            }
        }
        return;
    }
    for (int k = tx; k < s.W; k += lx) {
        const double* p = src0 + limit_window_from(s, c.r, k);
        double* d = out0 + k;
        if (!c.per_instance) {
            const double v = *p;
            for (int i = ty; i < cnt; i += ly, d += dstep) *d = v;
        } else {
            for (int i = ty; i < cnt; i += ly, d += dstep, p += sstep) *d = *p;
        }
    }
}

COPRA_DEV void limit_window_body(const LimitWindowArgs& P, int wg, int tid, int T)
{
    const int b0 = wg * P.group;
    const int cnt = (P.batch - b0 < P.group) ? P.batch - b0 : P.group;
    if (cnt <= 0) return;
    for (int k = 0; k < P.nwin; ++k) limit_window_one(P.w[k], b0, cnt, tid, T);
}

#if defined(__HIPCC__)
constexpr int kLimitWindowThreads = 256;
__global__ __launch_bounds__(kLimitWindowThreads) void copra_limit_window_kernel(const LimitWindowArgs P)
{
    limit_window_body(P, (int)blockIdx.x, (int)threadIdx.x, kLimitWindowThreads);
}
#endif

} // namespace copra_hip
