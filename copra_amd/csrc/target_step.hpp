// target_step.hpp -- steady-state targets on the device (copra_batch_set_target, ABI 15; host side: copra_hip_target.hip).  The third block of an
// offset-free loop beside the estimator and the observer: per instance b the steady state (xs, us) that is consistent with the model in
// force, its current d and a setpoint r on nr == nu controlled outputs H x, made the reference of the driven costs.  With n = nx + nu:
//   M = [ A - I   B ]      rhs = [ -d ]        M z = rhs,   z = [xs ; us]
//       [   H     0 ]            [  r ]
//   p_c[s r_c + i] = (T_c z)[i]      for every driven cost c, every block s = 0 .. S_c - 1 and every row i = 0 .. r_c - 1
// r is block min(tau + offset, steps - 1) of a signal [per_instance ? batch : 1][steps][nu] (the block is formed by the launch), T_c is
// [r_c x n] column-major and shared by the batch.  The reference's costs are |Mx - p|, |Nu - p|, |Mx + Nu - p|
// (include/costFunctions.h:101-190), so T_c = [M_c N_c] gives the p at which cost c vanishes in (xs, us).
//
// The arithmetic, in the order it is done (every product and every sum is one operation on the host; the device may contract a product
// and the sum behind it):
//   scale      amax = the largest |M_ij| over the n x n entries, scanned column by column, rows ascending, `>` from 0.0;
//              finite = every M_ij and every rhs_i is finite;   tol = (n * 2^-52) * amax
//   for k = 0 .. n - 1 (Gaussian elimination with partial pivoting on the augmented rows [M | rhs])
//     pivot    p = the row among k .. n - 1 with the largest |M_ik|, rows ascending, `>` from |M_kk|: ties go to the LOWEST row
//              singular |= !(|M_pk| > tol)                       (a NaN pivot is singular as well)
//     swap     rows k and p exchange their entries of columns k .. n (n: the rhs)
//     for i = k + 1 .. n - 1:   f = M_ik / M_kk;   for j = k + 1 .. n ascending:   M_ij = M_ij - f * M_kj
//   for i = n - 1 .. 0 (back substitution into the rhs column)
//     acc = rhs_i;   for j = i + 1 .. n - 1 ascending:   acc = acc - M_ij * z_j;     z_i = acc / M_ii
//   p_c[s r_c + i] = ((0.0 + T_c[i,0] z_0) + T_c[i,1] z_1) + ... + T_c[i,n-1] z_{n-1}
// An instance is SINGULAR when a pivot has |pivot| <= n 2^-52 max|M_ij| or M or rhs holds a non-finite value: status 1, and neither its z nor
// its references are stored -- they keep their bits; nothing of its neighbours changes.  Otherwise status 0.  Pivoting is not optional:
// for a double integrator A - I has a zero diagonal, the first pivot of an unpivoted elimination is 0.
//
// The kernel is stateless: it factorises from A, B, H every time (about n^3 / 3 multiply-adds, under 600 at n = 12, against about 12 000
// FLOP of a solve; it reads no more than the plant step reads; nothing cached can go stale).  It has the shape of plant_step.hpp: one
// workgroup takes `group` consecutive instances, whose A, B, d blocks are one contiguous range per array.  Mapping: ONE INSTANCE PER LANE in
// the elimination.  The image is entry-major: entry (row i, column j) of instance l of the group sits at (j n + i) group + l, so the lanes of a
// wave touch consecutive doubles whatever row a lane's pivot chose -- no bank conflict that the data could cause, and the row swaps are made
// in LDS (a run-time index into registers would go to scratch).
//   phase 1  target_stage   every thread: the ranges of A, B, d (and r) are read with coalesced loads, four in flight per thread, 16 bytes
//                           each where the pointers allow it, and scattered into the image (A - I, B, -d, r); H and the T_c are staged
//                           once per workgroup
//   phase 2  target_fill    every thread: the rows [H 0] of every lane's image from the staged H
//   phase 3  target_solve   thread l < group: scale, elimination, back substitution of instance l, all in the image; its status
//   phase 4  target_store   every thread: z [batch][n], status [batch] and, per driven cost, the S_c blocks leave as contiguous ranges; 16-byte
//                           stores only where every address allows it (the rule of limit_window_prepare): an aligned base and an even
//                           length per instance, so that no pair straddles two instances and a singular instance is skipped pair by pair
// A barrier stands between two phases.  No scratch, no atomics, no static LDS, nothing depends on the grid beyond the bounds of the last
// group.  The phases are COPRA_DEV functions of (workgroup, thread) that compile on the host (tests/emu/emu_target.cpp).
#pragma once
#include "plant_step.hpp"

namespace copra_hip {

constexpr int kTargetMaxCosts = 8; // driven costs of one launch
constexpr int kTargetThreads = 256; // of the kernel
constexpr int kTargetWave = 64; // a group is a whole number of waves of the elimination

struct TargetCost {
    const double* map; // T_c [r x n] column-major, one for the batch
    double* out; // [batch][S r]: the per-instance reference buffer the solve reads
    int r, S;
    int vec2; // out is 16-byte aligned and S r is even (target_prepare)
};

struct TargetArgs {
    int batch, nx, nu;
    int group; // instances per workgroup: a multiple of kTargetWave, at most kTargetThreads (target_group)
    int vec2_in; // A, B, d start on 16 bytes (the group is even: so does every group's range)
    int vec2_z; // z starts on 16 bytes and n is even
    int per_instance; // r holds one signal per instance
    const double *A, *B, *d; // the model in force, layout of copra_batch_set_system: [batch][nx x nx], [batch][nx x nu], [batch][nx]
    const double* H; // [nu x nx] column-major
    const double* r; // [per_instance ? batch : 1][steps][nu]
    long long steps, row; // row = min(tau + offset, steps - 1), formed by the launch
    int ncost;
    TargetCost c[kTargetMaxCosts];
    double* z; // [batch][nx + nu]
    int* status; // [batch]
};

// LDS image of one workgroup, in doubles: the augmented systems, entry-major | H | the maps, one after the other | status (ints); every
// part starts on 16 bytes.  map_doubles: the sum over the driven costs of plant_even(r_c n)
struct TargetLds {
    int oM, oH, oT, ost, total;
};
COPRA_PLANT_HD TargetLds target_lds(int nx, int nu, int group, int map_doubles)
{
    const int n = nx + nu;
    TargetLds L;
    L.oM = 0;
    L.oH = L.oM + n * (n + 1) * group;
    L.oT = L.oH + plant_even(nu * nx);
    L.ost = L.oT + map_doubles;
    L.total = L.ost + plant_even((group + 1) / 2);
    return L;
}
COPRA_PLANT_HD int target_map_doubles(const TargetArgs& S)
{
    int m = 0;
    for (int k = 0; k < S.ncost; ++k) m += plant_even(S.c[k].r * (S.nx + S.nu));
    return m;
}
COPRA_PLANT_HD TargetLds target_lds(const TargetArgs& S) { return target_lds(S.nx, S.nu, S.group, target_map_doubles(S)); }

// ---- the launch geometry (host), next to plant_group: one WAVE's image in bytes, and the group from it ----
constexpr size_t kTargetLdsTarget = 64 * 1024; // a group's image: room for a second workgroup on the CU
inline size_t target_image_bytes(int nx, int nu, int map_doubles) { return (size_t)target_lds(nx, nu, kTargetWave, map_doubles).total * sizeof(double); }
// instances per workgroup: as many waves (4, 2, 1) as keep the image within kTargetLdsTarget; one wave beyond it, up to kPlantLdsMax
inline int target_group(int nx, int nu, int map_doubles)
{
    for (int waves = kTargetThreads / kTargetWave; waves > 1; waves >>= 1)
        if ((size_t)target_lds(nx, nu, waves * kTargetWave, map_doubles).total * sizeof(double) <= kTargetLdsTarget) return waves * kTargetWave;
    return kTargetWave;
}

// (host) where a launch may move 16 bytes per lane
inline void target_prepare(TargetArgs& S)
{
    const auto ok = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    S.vec2_in = S.group % 2 == 0 && ok(S.A) && ok(S.B) && ok(S.d);
    S.vec2_z = ok(S.z) && (S.nx + S.nu) % 2 == 0;
    for (int k = 0; k < S.ncost; ++k) S.c[k].vec2 = ok(S.c[k].out) && (S.c[k].r * S.c[k].S) % 2 == 0;
}

#if defined(__HIPCC__)
#define COPRA_TARGET_UNROLL _Pragma("unroll")
#else
#define COPRA_TARGET_UNROLL
#endif

// src[0 .. count) handed to put(index, value), the elements dealt to the threads as plant_copy deals them, FOUR loads of a thread in flight
// before the first is used: one load per trip waits a round trip to memory per trip
template <class Put>
COPRA_DEV void target_read(const double* src, int count, int tid, int T, int vec2, Put put)
{
    if (vec2) {
        const int pairs = count >> 1;
        const PlantPair* s2 = reinterpret_cast<const PlantPair*>(src);
        for (int e = tid; e < pairs; e += 4 * T) {
            PlantPair v[4];
            COPRA_TARGET_UNROLL
            for (int q = 0; q < 4; ++q) v[q].a = v[q].b = 0.0;
COPRA_TARGET_UNROLL
            for (int q = 0; q < 4; ++q)
                if (e + q * T < pairs) v[q] = s2[e + q * T];
COPRA_TARGET_UNROLL
            for (int q = 0; q < 4; ++q)
                if (e + q * T < pairs) put(2 * (e + q * T), v[q].a), put(2 * (e + q * T) + 1, v[q].b);
        }
        if ((count & 1) && tid == 0) put(count - 1, src[count - 1]);
    } else {
        for (int e = tid; e < count; e += 4 * T) {
            double v[4];
            COPRA_TARGET_UNROLL
            for (int q = 0; q < 4; ++q) v[q] = 0.0;
COPRA_TARGET_UNROLL
            for (int q = 0; q < 4; ++q)
                if (e + q * T < count) v[q] = src[e + q * T];
COPRA_TARGET_UNROLL
            for (int q = 0; q < 4; ++q)
                if (e + q * T < count) put(e + q * T, v[q]);
        }
    }
}

// phase 1: everything workgroup `wg` reads, into its image
COPRA_DEV void target_stage(const TargetArgs& S, int wg, int tid, int T, double* lds)
{
    const int nx = S.nx, nu = S.nu, n = nx + nu, G = S.group, b0 = wg * G;
    const int cnt = (S.batch - b0 < G) ? S.batch - b0 : G;
    if (cnt <= 0) return;
    const TargetLds L = target_lds(S);
    double* const M = lds + L.oM;
    const int na = nx * nx, nb = nx * nu;
    target_read(S.A + (size_t)b0 * na, cnt * na, tid, T, S.vec2_in, [&](int e, double v) { // A - I: rows 0 .. nx - 1, columns 0 .. nx - 1
        const int i = e / na, w = e - i * na, j = w / nx, r = w - j * nx;
        M[(j * n + r) * G + i] = r == j ? v - 1.0 : v;
    });
    target_read(S.B + (size_t)b0 * nb, cnt * nb, tid, T, S.vec2_in, [&](int e, double v) { // B: columns nx .. n - 1
        const int i = e / nb, w = e - i * nb, c = w / nx, r = w - c * nx;
        M[((nx + c) * n + r) * G + i] = v;
    });
    target_read(S.d + (size_t)b0 * nx, cnt * nx, tid, T, S.vec2_in, [&](int e, double v) { // -d: the rhs column, rows 0 .. nx - 1
        const int i = e / nx, r = e - i * nx;
        M[(n * n + r) * G + i] = -v;
    });
    if (S.per_instance) { // every instance's block of its own signal: nu consecutive doubles, steps nu apart
        for (int e = tid; e < cnt * nu; e += T) {
            const int i = e / nu, a = e - i * nu;
            M[(n * n + nx + a) * G + i] = S.r[(((size_t)b0 + i) * (size_t)S.steps + (size_t)S.row) * nu + a];
        }
    } else { // one block for the batch
        const double* const r = S.r + (size_t)S.row * nu;
        for (int e = tid; e < cnt * nu; e += T) {
            const int a = e / cnt, i = e - a * cnt;
            M[(n * n + nx + a) * G + i] = r[a];
        }
    }
    plant_copy(lds + L.oH, S.H, nu * nx, tid, T, 0);
    int at = L.oT;
    for (int k = 0; k < S.ncost; ++k) {
        plant_copy(lds + at, S.c[k].map, S.c[k].r * n, tid, T, 0);
        at += plant_even(S.c[k].r * n);
    }
}

// phase 2 (behind a barrier): rows nx .. n - 1 of every lane's system, [H 0]
COPRA_DEV void target_fill(const TargetArgs& S, int wg, int tid, int T, double* lds)
{
    const int nx = S.nx, nu = S.nu, n = nx + nu, G = S.group, b0 = wg * G;
    const int cnt = (S.batch - b0 < G) ? S.batch - b0 : G;
    if (cnt <= 0) return;
    const TargetLds L = target_lds(S);
    double* const M = lds + L.oM;
    const double* const H = lds + L.oH;
    for (int e = tid; e < cnt * nu * n; e += T) { // (consecutive threads, consecutive lanes of one entry)
        const int w = e / cnt, i = e - w * cnt, j = w / nu, a = w - j * nu;
        M[(j * n + nx + a) * G + i] = j < nx ? H[a + nu * j] : 0.0;
    }
}

// phase 3 (behind a barrier): thread l solves instance l of the group in its column of the image; z ends in the rhs column
COPRA_DEV void target_solve(const TargetArgs& S, int wg, int tid, int T, double* lds)
{
    const int n = S.nx + S.nu, G = S.group, b0 = wg * G;
    const int cnt = (S.batch - b0 < G) ? S.batch - b0 : G;
    if (cnt <= 0) return;
    const TargetLds L = target_lds(S);
    int* const st = reinterpret_cast<int*>(lds + L.ost);
    for (int l = tid; l < cnt; l += T) {
        double* const M = lds + L.oM + l; // entry (i, j): M[(j n + i) G]
        double amax = 0.0;
        bool finite = true;
        for (int e = 0; e < n * n; ++e) {
            const double v = M[e * G], a = v < 0.0 ? -v : v;
            if (a > amax) amax = a;
            finite = finite && a <= 1.7976931348623157e308;
        }
        for (int i = 0; i < n; ++i) {
            const double v = M[(n * n + i) * G], a = v < 0.0 ? -v : v;
            finite = finite && a <= 1.7976931348623157e308;
        }
        const double tol = ((double)n * 2.220446049250313e-16) * amax;
        bool singular = !finite;
        for (int k = 0; k < n; ++k) {
            int p = k;
            double best = M[(k * n + k) * G];
            best = best < 0.0 ? -best : best;
            for (int i = k + 1; i < n; ++i) {
                const double v = M[(k * n + i) * G], a = v < 0.0 ? -v : v;
                if (a > best) best = a, p = i;
            }
            singular = singular || !(best > tol);
            for (int j = k; j <= n; ++j) { // (p == k: both rows are the same entry, written back unchanged)
                const double top = M[(j * n + k) * G], low = M[(j * n + p) * G];
                M[(j * n + k) * G] = low;
                M[(j * n + p) * G] = top;
            }
            const double piv = M[(k * n + k) * G];
            for (int i = k + 1; i < n; ++i) {
                const double f = M[(k * n + i) * G] / piv;
                for (int j = k + 1; j <= n; ++j) M[(j * n + i) * G] = M[(j * n + i) * G] - f * M[(j * n + k) * G];
            }
        }
        for (int i = n - 1; i >= 0; --i) {
            double acc = M[(n * n + i) * G];
            for (int j = i + 1; j < n; ++j) acc = acc - M[(j * n + i) * G] * M[(n * n + j) * G];
            M[(n * n + i) * G] = acc / M[(i * n + i) * G];
        }
        st[l] = singular ? 1 : 0;
    }
}

// row i of T z for instance l of the group: ascending from 0.0
COPRA_DEV double target_row(const double* map, int r, int i, const double* z, int n, int G)
{
    double acc = 0.0;
    for (int j = 0; j < n; ++j) acc += map[i + r * j] * z[j * G];
    return acc;
}

// phase 4 (behind a barrier): the group's results as contiguous ranges; a singular instance stores its status alone
COPRA_DEV void target_store(const TargetArgs& S, int wg, int tid, int T, const double* lds)
{
    const int n = S.nx + S.nu, G = S.group, b0 = wg * G;
    const int cnt = (S.batch - b0 < G) ? S.batch - b0 : G;
    if (cnt <= 0) return;
    const TargetLds L = target_lds(S);
    const int* const st = reinterpret_cast<const int*>(lds + L.ost);
    const double* const Z = lds + L.oM + n * n * G; // z_j of instance i: Z[j G + i]
    for (int i = tid; i < cnt; i += T) S.status[b0 + i] = st[i];
    double* const zo = S.z + (size_t)b0 * n;
    if (S.vec2_z) {
        for (int e = tid; e < (cnt * n) >> 1; e += T) {
            const int i = (2 * e) / n, j = 2 * e - i * n;
            if (st[i]) continue;
            PlantPair v;
            v.a = Z[j * G + i], v.b = Z[(j + 1) * G + i];
            reinterpret_cast<PlantPair*>(zo)[e] = v;
        }
    } else {
        for (int e = tid; e < cnt * n; e += T) {
            const int i = e / n, j = e - i * n;
            if (!st[i]) zo[e] = Z[j * G + i];
        }
    }
    int at = L.oT;
    for (int k = 0; k < S.ncost; ++k) {
        const TargetCost& c = S.c[k];
        const double* const map = lds + at;
        at += plant_even(c.r * n);
        const int W = c.r * c.S;
        double* const out = c.out + (size_t)b0 * W;
        if (c.vec2) {
            for (int e = tid; e < (cnt * W) >> 1; e += T) {
                const int i = (2 * e) / W, w = 2 * e - i * W;
                if (st[i]) continue;
                PlantPair v;
                v.a = target_row(map, c.r, w % c.r, Z + i, n, G), v.b = target_row(map, c.r, (w + 1) % c.r, Z + i, n, G);
                reinterpret_cast<PlantPair*>(out)[e] = v;
            }
        } else {
            for (int e = tid; e < cnt * W; e += T) {
                const int i = e / W, w = e - i * W;
                if (!st[i]) out[e] = target_row(map, c.r, w % c.r, Z + i, n, G);
            }
        }
    }
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(kTargetThreads) void copra_target_kernel(const TargetArgs S)
{
    extern __shared__ __align__(16) double target_image[];
    const int wg = (int)blockIdx.x, tid = (int)threadIdx.x;
    target_stage(S, wg, tid, kTargetThreads, target_image);
    __syncthreads();
    target_fill(S, wg, tid, kTargetThreads, target_image);
    __syncthreads();
    target_solve(S, wg, tid, kTargetThreads, target_image);
    __syncthreads();
    target_store(S, wg, tid, kTargetThreads, target_image);
}
#endif

} // namespace copra_hip
