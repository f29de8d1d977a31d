// plant_noise.hpp -- process and sensor noise of the tick drawn ON THE DEVICE (copra_batch_set_noise, ABI 13): a counter-based generator, so
// that the draw of instance b at noise tick t is a function of (seed, first_instance + b, stream, row, t) and of nothing else -- not of the
// batch, the group, the build of the kernel or the GPU a shard of the batch runs on -- and costs no memory.
//
// Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53, 0xCD9E8D57, Weyl key increments 0x9E3779B9, 0xBB67AE85, round r with
// key + r x increment, new counter = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)).
// Rows 2j and 2j + 1 of instance b at tick t use ONE call; stream s is 0 for process noise w, 1 for sensor noise v:
//   key = (seed & 0xffffffff, seed >> 32);   counter = ((first_instance + b) & 0xffffffff, (s << 16) | j, t & 0xffffffff, t >> 32)
//   u1 = (((o0 << 32 | o1) >> 12) + 0.5) 2^-52,  u2 likewise from (o2, o3): exact in a double, inside (0, 1)
//   rad = sqrt(-2 log u1),  ang = 6.283185307179586 u2;   n[2j] = rad cos ang,  n[2j + 1] = rad sin ang   (odd row count: the last sin is dropped)
// The noise TERM of row r is sigma[r] n[r], one multiplication rounded once; the tick uses w = term, or w = w_given + term (v likewise).
// Neither the product nor that sum may be contracted into a neighbour: noise_mul / noise_add.  The stand-alone fill kernel
// (copra_batch_draw_noise) and phase 1 of the tick (plant_step.hpp) go through the SAME function, noise_stage, and agree bit for bit.
//
// Everything here is a COPRA_DEV function that also compiles on the host (tests/emu/emu_plant_noise.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifndef COPRA_DEV
#if defined(__HIPCC__)
#define COPRA_DEV __device__ __forceinline__
#else
#define COPRA_DEV inline
#endif
#endif

namespace copra_hip {

struct PhiloxOut {
    uint32_t o0, o1, o2, o3;
};

COPRA_DEV PhiloxOut philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return PhiloxOut { c0, c1, c2, c3 };
}

// the generator's words for pair j of stream s of global instance gi at noise tick t
COPRA_DEV PhiloxOut noise_words(uint64_t seed, uint64_t gi, int s, int j, uint64_t t)
{
    return philox4x32_10((uint32_t)gi, ((uint32_t)s << 16) | (uint32_t)j, (uint32_t)t, (uint32_t)(t >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}

// a product and a sum that stay a product and a sum: never half of a fused multiply-add
COPRA_DEV double noise_mul(double a, double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
    return a * b;
#else
    volatile double p = a * b;
    return p;
#endif
}
COPRA_DEV double noise_add(double a, double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
    return a + b;
#else
    volatile double p = a + b;
    return p;
#endif
}

struct NoisePair {
    double a, b;
};

// the two standard normals n[2j], n[2j + 1] ...
COPRA_DEV NoisePair noise_normals(uint64_t seed, uint64_t gi, int s, int j, uint64_t t)
{
    const PhiloxOut o = noise_words(seed, gi, s, j, t);
    const double k = 2.220446049250313e-16; // 2^-52
    const double u1 = ((double)((((uint64_t)o.o0 << 32) | o.o1) >> 12) + 0.5) * k;
    const double u2 = ((double)((((uint64_t)o.o2 << 32) | o.o3) >> 12) + 0.5) * k;
    const double rad = sqrt(noise_mul(-2.0, log(u1))), ang = noise_mul(6.283185307179586, u2);
    return NoisePair { noise_mul(rad, cos(ang)), noise_mul(rad, sin(ang)) };
}

// ... and the noise terms of the pair: sigma[2j] n[2j], sigma[2j + 1] n[2j + 1]
COPRA_DEV NoisePair noise_pair_terms(uint64_t seed, uint64_t gi, int s, int j, uint64_t t, double sig_a, double sig_b)
{
    const NoisePair n = noise_normals(seed, gi, s, j, t);
    return NoisePair { noise_mul(sig_a, n.a), noise_mul(sig_b, n.b) };
}

// Where the draws of one handle stand: the seed, the global index of its instance 0 and the noise tick
struct NoiseGen {
    uint64_t seed, first, tick;
};

// dst[i][r] = (given ? given[i][r] : 0 +) sigma[r] n[r] for instances b0 .. b0 + cnt of the batch, `rows` rows each; thread `tid` of `T`.
// One thread forms both rows of a pair: consecutive threads take consecutive pairs, so a per-instance sigma and a given array are read, and
// dst is written, at consecutive addresses (16 bytes per lane with an even row count); a sigma shared by the batch is `rows` words that
// every instance's lanes read alike.  sigma, given: the arrays of the WHOLE batch in global memory; dst: the group's own block (LDS in the
// tick, the output array at b0 in the fill kernel).  A sigma of 0 leaves the given value (or +0) exactly.
COPRA_DEV void noise_stage(const NoiseGen& G, int s, const double* sigma, int per_instance, const double* given, size_t b0, int cnt, int rows, double* dst, int tid,
    int T)
{
    const int pairs = (rows + 1) >> 1;
    for (int e = tid; e < cnt * pairs; e += T) {
        const int i = e / pairs, j = e - i * pairs, r = 2 * j;
        const bool both = r + 1 < rows;
        const size_t at = (b0 + i) * (size_t)rows + r;
        const double* sg = per_instance ? sigma + at : sigma + r;
        const NoisePair term = noise_pair_terms(G.seed, G.first + b0 + i, s, j, G.tick, sg[0], both ? sg[1] : 0.0);
        double* out = dst + (size_t)i * rows + r;
        out[0] = given ? noise_add(given[at], term.a) : term.a;
        if (both) out[1] = given ? noise_add(given[at + 1], term.b) : term.b;
    }
}

// ---- the fill kernel: the terms of one tick and one stream, [batch][rows] (copra_batch_draw_noise) ----
struct NoiseFillArgs {
    int batch, rows, stream, per_instance, group;
    NoiseGen gen;
    const double* sigma;
    double* out;
};

COPRA_DEV void noise_fill_body(const NoiseFillArgs& F, int wg, int tid, int T)
{
    const size_t b0 = (size_t)wg * F.group;
    if (b0 >= (size_t)F.batch) return;
    const int cnt = (size_t)F.batch - b0 < (size_t)F.group ? (int)((size_t)F.batch - b0) : F.group;
    noise_stage(F.gen, F.stream, F.sigma, F.per_instance, nullptr, b0, cnt, F.rows, F.out + b0 * F.rows, tid, T);
}

#if defined(__HIPCC__) && !defined(COPRA_PLANT_PHASES_ONLY) // (a unit that wants the phase bodies alone defines it: the kernels have ONE home, copra_hip_plant.hip)
constexpr int kNoiseFillThreads = 256;
__global__ __launch_bounds__(kNoiseFillThreads) void copra_noise_fill_kernel(const NoiseFillArgs F)
{
    noise_fill_body(F, (int)blockIdx.x, (int)threadIdx.x, kNoiseFillThreads);
}
#endif

} // namespace copra_hip
