// delay_step.hpp -- input delay in the tick, on the device (copra_batch_set_input_delay, ABI 16; launched from copra_hip_delay.hip): the
// command the solve of tick t issues reaches the plant at tick t + D.  The library keeps, per instance b, a ring of the D commands already
// issued, q[b][D][nu], the status of the solve that issued each, qs[D][batch], and the state at the current tick, xnow[b][nx]; one
// handle-wide `head` names the slot the plant applies next.  The plant step reads slot `head` through its own pointer and stride fields
// (plant_step.hpp is untouched); this kernel runs behind it and
//   push     slot `head` <- the last solve's control[b][0 .. nu) and status[b] (the status is looked at FIRST: a failed instance's control
//            is never loaded, its slot holds NaN), and head <- (head + 1) % D, which the host passes in already advanced
//   predict  x <- xnow[b];  for the D pending entries, OLDEST first (slots head, head + 1, ... cyclically; the newest is head + D - 1):
//              status == COPRA_QP_OK : x <- Am x + Bm u + d         (the controller's model, no w; the sum in the order of plant_row)
//              else, fallback_u given: the same with u = fallback_u[b]
//              else                  : x is kept -- the plant will hold that instance at that tick
//            x0[b] <- x: what the next solve reads
// With push == 0 (the setters that move xnow, d or the model) the queue is only read.
//
// A streaming kernel of the shape of plant_step.hpp / score_step.hpp (at (6, 3), D = 2 about 600 B read, 70 B written per instance).  One
// workgroup takes `group` consecutive instances: A, B, d, xnow, the instances' queue blocks and fallback controls are ONE contiguous range
// per array, copied into an LDS image with wide coalesced loads (16 B per lane where delay_vec2_ok allows it, 8 B otherwise), every array's
// first load issued before the first store; a shared model is staged once per workgroup.  The statuses are gathered (stride batch), the new
// command is read with the solve's stride, written to its ring slot in global memory and to a slot of its own in the image (the copy of the
// queue block beside it may still hold that slot's old command: the newest entry is read from the image's own slot, never from there).
// Behind a barrier D prediction steps, one thread per (instance, row): the state ping-pongs between two slots of the image with a barrier
// between two steps -- an instance's rows may sit in different waves.  The last step's states leave as one contiguous range per group.  No
// scratch, no atomics, nothing depends on the grid beyond the bounds of the last group; D is a run-time value, uniform across the grid.
//
// The phases are COPRA_DEV functions of (workgroup, thread) that also compile on the host: tests/emu/emu_delay.cpp walks them thread by
// thread with a host buffer in the place of LDS.
#pragma once
#include "plant_step.hpp" // plant_row, plant_even, PlantPair, plant_group and the LDS bounds: the helpers, none of the kernels' phases

namespace copra_hip {

constexpr int kDelayMax = 8; // COPRA_DELAY_MAX of include/copra_hip.h

struct DelayArgs {
    int batch, nx, nu;
    int D; // 1 .. kDelayMax
    int head; // the slot applied next: the OLDEST pending entry (after this launch's push)
    int push; // write the last solve's command into slot (head + D - 1) % D first
    int ctrl_stride; // doubles between two instances' controls of the solve: nu N
    int group; // instances per workgroup (even wherever vec2 is set)
    int shared; // A, B, d hold ONE system for the batch
    int vec2; // delay_vec2_ok
    const double *A, *B, *d; // the controller's model
    const double* xnow; // [batch][nx]
    double* q; // [batch][D][nu]
    int* qs; // [D][batch]
    const double* fallback_u; // [batch][nu] or null
    const int* status; // [batch], of the last launched solve (push only)
    const double* control; // [batch][ctrl_stride] (push only)
    double* x0; // [batch][nx]: the prediction
};

// LDS image of one workgroup, in doubles: A | B | d | xa | xb | q | fb | unew | status (ints: [group][D], then the new entries' [group]);
// every part starts on 16 bytes
struct DelayLds {
    int oA, oB, od, oxa, oxb, oq, ofb, oun, ost, total;
};
COPRA_PLANT_HD DelayLds delay_lds(int nx, int nu, int D, int group, int shared, int has_fb)
{
    const int gs = shared ? 1 : group;
    DelayLds L;
    L.oA = 0;
    L.oB = L.oA + plant_even(gs * nx * nx);
    L.od = L.oB + plant_even(gs * nx * nu);
    L.oxa = L.od + plant_even(gs * nx);
    L.oxb = L.oxa + plant_even(group * nx);
    L.oq = L.oxb + plant_even(group * nx);
    L.ofb = L.oq + plant_even(group * D * nu);
    L.oun = L.ofb + (has_fb ? plant_even(group * nu) : 0);
    L.ost = L.oun + plant_even(group * nu);
    L.total = L.ost + plant_even((group * (D + 1) + 1) / 2);
    return L;
}
COPRA_PLANT_HD DelayLds delay_lds(const DelayArgs& P) { return delay_lds(P.nx, P.nu, P.D, P.group, P.shared, P.fallback_u != nullptr); }

// ---- the launch geometry (host): one instance's widest image in bytes (a model of its own, fallback controls), the group from plant_group ----
inline size_t delay_image_bytes(int nx, int nu, int D) { return (size_t)delay_lds(nx, nu, D, 1, 0, 1).total * sizeof(double); }
inline int delay_group(int nx, int nu, int D) { return plant_group(delay_image_bytes(nx, nu, D)); }

// (host) whether a launch may copy two doubles per lane: an even group -- every group's range of every array then starts on 16 bytes
// whatever nx, nu and D -- and aligned arrays
inline bool delay_vec2_ok(const DelayArgs& P)
{
    const auto ok = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    return P.group % 2 == 0 && ok(P.A) && ok(P.B) && ok(P.d) && ok(P.xnow) && ok(P.q) && ok(P.fallback_u);
}

// Several contiguous copies at once, the elements handed to the threads as plant_copy hands them out; a thread's FIRST element of every
// array is loaded before any is stored, so that the loads of all arrays are in flight together (score_step.hpp: score_copy_all)
#if defined(__HIPCC__)
#define COPRA_DELAY_UNROLL _Pragma("unroll")
#else
#define COPRA_DELAY_UNROLL
#endif
constexpr int kDelayCopies = 6;
struct DelayCopy {
    double* dst;
    const double* src;
    int count; // 0: not given
};
COPRA_DEV void delay_copy_all(const DelayCopy (&c)[kDelayCopies], int tid, int T, int vec2)
{
    if (vec2) {
        PlantPair first[kDelayCopies];
        COPRA_DELAY_UNROLL
        for (int k = 0; k < kDelayCopies; ++k) first[k].a = first[k].b = 0.0;
        COPRA_DELAY_UNROLL
        for (int k = 0; k < kDelayCopies; ++k)
            if (tid < (c[k].count >> 1)) first[k] = reinterpret_cast<const PlantPair*>(c[k].src)[tid];
        COPRA_DELAY_UNROLL
        for (int k = 0; k < kDelayCopies; ++k)
            if (tid < (c[k].count >> 1)) reinterpret_cast<PlantPair*>(c[k].dst)[tid] = first[k];
        COPRA_DELAY_UNROLL
        for (int k = 0; k < kDelayCopies; ++k) {
            const int pairs = c[k].count >> 1;
            for (int e = tid + T; e < pairs; e += T) reinterpret_cast<PlantPair*>(c[k].dst)[e] = reinterpret_cast<const PlantPair*>(c[k].src)[e];
            if ((c[k].count & 1) && tid == 0) c[k].dst[c[k].count - 1] = c[k].src[c[k].count - 1];
        }
    } else {
        double first[kDelayCopies];
        COPRA_DELAY_UNROLL
        for (int k = 0; k < kDelayCopies; ++k) first[k] = 0.0;
        COPRA_DELAY_UNROLL
        for (int k = 0; k < kDelayCopies; ++k)
            if (tid < c[k].count) first[k] = c[k].src[tid];
        COPRA_DELAY_UNROLL
        for (int k = 0; k < kDelayCopies; ++k)
            if (tid < c[k].count) c[k].dst[tid] = first[k];
        COPRA_DELAY_UNROLL
        for (int k = 0; k < kDelayCopies; ++k)
            for (int e = tid + T; e < c[k].count; e += T) c[k].dst[e] = c[k].src[e];
    }
}

// the slot of the newest entry: the one a push writes
COPRA_PLANT_HD int delay_newest(int head, int D) { return (head + D - 1) % D; }

// phase 1: everything workgroup `wg` reads, into its image `lds`; with push the new command into its ring slot
COPRA_DEV void delay_stage(const DelayArgs& P, int wg, int tid, int T, double* lds)
{
    const int nx = P.nx, nu = P.nu, D = P.D, b0 = wg * P.group;
    const int cnt = (P.batch - b0 < P.group) ? P.batch - b0 : P.group;
    if (cnt <= 0) return;
    const DelayLds L = delay_lds(P);
    const size_t s0 = P.shared ? 0 : (size_t)b0;
    const int scnt = P.shared ? 1 : cnt;
    const int newest = delay_newest(P.head, D);
    // the new entries' statuses first: they decide whether anything of `control` is touched
    int* st = reinterpret_cast<int*>(lds + L.ost);
    int* stn = st + P.group * D;
    if (P.push) {
        for (int e = tid; e < cnt * nu; e += T) {
            const int i = e / nu, c = e - i * nu;
            const size_t b = (size_t)b0 + i;
            double u = NAN; // (a failed entry's slot: never applied, never read for the prediction)
            if (P.status[b] == 0) u = P.control[b * P.ctrl_stride + c];
            P.q[(b * D + newest) * nu + c] = u;
            lds[L.oun + e] = u;
        }
        for (int i = tid; i < cnt; i += T) {
            const int s = P.status[b0 + i];
            P.qs[(size_t)newest * P.batch + b0 + i] = s;
            stn[i] = s;
        }
    }
    const DelayCopy copies[kDelayCopies] = {
        { lds + L.oA, P.A + s0 * nx * nx, scnt * nx * nx },
        { lds + L.oB, P.B + s0 * nx * nu, scnt * nx * nu },
        { lds + L.od, P.d + s0 * nx, scnt * nx },
        { lds + L.oxa, P.xnow + (size_t)b0 * nx, cnt * nx },
        { lds + L.oq, P.q + (size_t)b0 * D * nu, cnt * D * nu },
        { lds + L.ofb, P.fallback_u ? P.fallback_u + (size_t)b0 * nu : nullptr, P.fallback_u ? cnt * nu : 0 },
    };
    delay_copy_all(copies, tid, T, P.vec2);
    for (int e = tid; e < cnt * D; e += T) { // (with push the newest slot's word may be the old or the new one: it is read from stn)
        const int j = e / cnt, i = e - j * cnt;
        st[i * D + j] = P.qs[(size_t)j * P.batch + b0 + i];
    }
}

// phase 2 + j (behind a barrier each), j = 0 .. D - 1: pending entry j, oldest first, applied to every (instance, row); the state is read
// from slot j & 1 of the image (xa, xb) and written to the other; the last step stores the group's predictions
COPRA_DEV void delay_predict(const DelayArgs& P, int wg, int tid, int T, double* lds, int j)
{
    const int nx = P.nx, nu = P.nu, D = P.D, b0 = wg * P.group;
    const int cnt = (P.batch - b0 < P.group) ? P.batch - b0 : P.group;
    if (cnt <= 0) return;
    const DelayLds L = delay_lds(P);
    const int slot = (P.head + j) % D;
    const bool fresh = P.push && j == D - 1; // the entry this launch pushed: its own slot of the image
    const int* st = reinterpret_cast<const int*>(lds + L.ost);
    const int* stn = st + P.group * D;
    const double* xs = lds + ((j & 1) ? L.oxb : L.oxa);
    double* xd = lds + ((j & 1) ? L.oxa : L.oxb);
    for (int e = tid; e < cnt * nx; e += T) {
        const int i = e / nx, r = e - i * nx, is = P.shared ? 0 : i;
        const int s = fresh ? stn[i] : st[i * D + slot];
        const double* u = nullptr;
        if (s == 0) u = fresh ? lds + L.oun + i * nu : lds + L.oq + (i * D + slot) * nu;
        else if (P.fallback_u) u = lds + L.ofb + i * nu;
        double xn = xs[e]; // held
        if (u) xn = plant_row(nx, nu, r, lds + L.oA + is * nx * nx, lds + L.oB + is * nx * nu, lds + L.od + is * nx, nullptr, xs + i * nx, u);
        xd[e] = xn;
        if (j == D - 1) P.x0[(size_t)b0 * nx + e] = xn;
    }
}

#if defined(__HIPCC__) && defined(COPRA_DELAY_KERNEL) // (the kernel has ONE home, copra_hip_delay.hip)
constexpr int kDelayThreads = 256;
__global__ __launch_bounds__(kDelayThreads) void copra_delay_kernel(const DelayArgs P)
{
    extern __shared__ __align__(16) double delay_image[];
    const int wg = (int)blockIdx.x, tid = (int)threadIdx.x;
    delay_stage(P, wg, tid, kDelayThreads, delay_image);
    for (int j = 0; j < P.D; ++j) { // (P.D is a kernel argument: the trip count and every barrier are uniform)
        __syncthreads();
        delay_predict(P, wg, tid, kDelayThreads, delay_image, j);
    }
}
#endif

} // namespace copra_hip
