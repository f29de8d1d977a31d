// emu_walk.h -- what the five walkers of this directory (emu_plant.cpp, _backup, _bias, _observer, _noise) share beside the kernel's own header:
// the order in which one phase's threads, and the grid's workgroups, are walked; the image with a guard zone behind it; and the launch
// geometry of copra_amd/csrc/plant_step.hpp as C functions (tests/test_tick_edges_abi.py and the *_abi.py files ask these, none restates
// the rule).  The walkers stay five files: each walks its own build's phases.  Included by exactly ONE translation unit of an emulator (the
// geometry functions below are defined, not only declared).
//
// On the device the threads of a phase run in no order that a program may rely on, and neither do the workgroups of a grid: a phase whose
// result depends on the order reads, somewhere, what another thread of the SAME phase wrote -- a race.  So every walker takes an order:
//   0  ascending (what the walkers did before they took one)      1  descending      2  a permutation drawn from `seed`, a new one for
//   every phase of every workgroup, and one for the workgroups
// and a result that differs between two orders by one bit is a defect of the phase bodies.
// The guard: the image is `total` doubles -- from the layout function the launch sizes it with -- and kEmuGuard doubles behind it that
// hold a fixed bit pattern no computation produces; they are looked at after every workgroup.  The image itself is filled with NaN as before.
#pragma once
#include "../../copra_amd/csrc/plant_step.hpp"

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

namespace emu {

constexpr int kEmuGuard = 64; // doubles behind the image
constexpr uint64_t kEmuGuardBits = 0x7ff4deadbeef5a5aull; // (a signalling NaN with a payload: nothing stores it by accident)
constexpr int kEmuNoMemory = -1, kEmuGuardTouched = -2; // the walkers' return codes beside 0

inline uint64_t splitmix(uint64_t& s)
{
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// 0 .. n - 1 in the order asked for; `salt` tells the phases and workgroups of one walk apart
inline std::vector<int> order_of(int n, int order, uint64_t seed, uint64_t salt)
{
    std::vector<int> idx((size_t)(n > 0 ? n : 0));
    std::iota(idx.begin(), idx.end(), 0);
    if (order == 1) {
        for (int i = 0; i < n / 2; ++i) std::swap(idx[(size_t)i], idx[(size_t)(n - 1 - i)]);
    } else if (order == 2) {
        uint64_t s = seed ^ (salt * 0xd1342543de82ef95ull + 0x2545f4914f6cdd1dull);
        for (int i = n - 1; i > 0; --i) std::swap(idx[(size_t)i], idx[(size_t)(splitmix(s) % (uint64_t)(i + 1))]);
    }
    return idx;
}

// the image of one workgroup with its guard
struct Image {
    double* lds = nullptr;
    size_t total = 0;
    explicit Image(size_t doubles) : total(doubles)
    {
        lds = static_cast<double*>(std::aligned_alloc(16, ((total + kEmuGuard) * sizeof(double) + 15) / 16 * 16));
        if (lds)
            for (int i = 0; i < kEmuGuard; ++i) std::memcpy(lds + total + i, &kEmuGuardBits, sizeof(double));
    }
    ~Image() { std::free(lds); }
    Image(const Image&) = delete;
    Image& operator=(const Image&) = delete;
    void fill_nan() // (LDS is not initialised: whatever is read must have been staged)
    {
        for (size_t i = 0; i < total; ++i) lds[i] = std::numeric_limits<double>::quiet_NaN();
    }
    bool guard_intact() const
    {
        for (int i = 0; i < kEmuGuard; ++i)
            if (std::memcmp(lds + total + i, &kEmuGuardBits, sizeof(double)) != 0) return false;
        return true;
    }
};

// One walk: `phases(wg, phase, tid)` runs thread tid of phase `phase` of workgroup wg; between two phases stands the barrier.  Returns 0 or
// kEmuGuardTouched
template <class Phases>
int walk(Image& img, int grid, int nphases, int threads, int order, uint64_t seed, Phases phases)
{
    for (int wg : order_of(grid, order, seed, 0)) {
        img.fill_nan();
        for (int ph = 0; ph < nphases; ++ph)
            for (int tid : order_of(threads, order, seed, 1 + (uint64_t)wg * 8 + (uint64_t)ph)) phases(wg, ph, tid);
        if (!img.guard_intact()) return kEmuGuardTouched;
    }
    return 0;
}

} // namespace emu

extern "C" {

// ---- the launch geometry of plant_step.hpp: kind 0 the plain tick, 1 the disturbance estimator (dense: its gain), 2 the observer (ny) ----
// one instance's widest image in bytes: what the launch checks against emu_plant_lds_max() and sizes the group from
long long emu_plant_image_bytes(int kind, int nx, int nu, int ny, int dense)
{
    using namespace copra_hip;
    return (long long)(kind == 0 ? plant_image_bytes(nx, nu) : kind == 1 ? bias_image_bytes(nx, nu, dense) : observer_image_bytes(nx, nu, ny));
}
int emu_plant_launch_group(int kind, int nx, int nu, int ny, int dense) { return copra_hip::plant_group((size_t)emu_plant_image_bytes(kind, nx, nu, ny, dense)); }
long long emu_plant_lds_max() { return (long long)copra_hip::kPlantLdsMax; }
long long emu_plant_lds_target() { return (long long)copra_hip::kPlantLdsTarget; }
int emu_plant_group_max() { return copra_hip::kPlantGroupMax; }
int emu_plant_guard_doubles() { return emu::kEmuGuard; }

// The layout structs themselves, as the phase bodies get them: every offset in doubles in the order of the image, then the total.  flags:
// shared, has_w, backup, same_model, gain_dense, gain_shared, meas, has_Ld, has_yv (a kind reads the ones its layout function takes).
// Returns the number of values written to out (at most 24).
int emu_plant_layout(int kind, int nx, int nu, int ny, int group, const int* f, int* out)
{
    using namespace copra_hip;
    int n = 0;
    const auto base = [&](const PlantLds& L, int total) {
        out[n++] = L.oA, out[n++] = L.oB, out[n++] = L.od, out[n++] = L.ox, out[n++] = L.ow, out[n++] = L.ou, out[n++] = L.ost, out[n++] = L.oag;
        out[n++] = total;
    };
    if (kind == 0) {
        const PlantLds L = plant_lds(nx, nu, group, f[0], f[1], f[2]);
        base(L, L.total);
    } else if (kind == 1) {
        const PlantEstLds E = plant_est_lds(nx, nu, group, f[0], f[1], f[2], f[3], f[4], f[5]);
        base(E.base, E.base.total);
        out[n++] = E.oAm, out[n++] = E.oBm, out[n++] = E.odh, out[n++] = E.oG, out[n++] = E.oxn, out[n++] = E.oe, out[n++] = E.total;
    } else {
        const PlantObsLds E = plant_obs_lds(nx, nu, ny, group, f[0], f[1], f[2], f[3], f[6], f[7], f[5], f[8]);
        base(E.base, E.base.total);
        out[n++] = E.oAm, out[n++] = E.oBm, out[n++] = E.odh, out[n++] = E.oxh, out[n++] = E.oC, out[n++] = E.oLx, out[n++] = E.oLd, out[n++] = E.oyv;
        out[n++] = E.oxn, out[n++] = E.oxp, out[n++] = E.oin, out[n++] = E.total;
    }
    return n;
}

// ... of n shapes at once (a sweep): p holds n rows of nx, nu, ny, group and the nine flags, out n rows of 24 values.  Returns the number of
// values of a row that are set.
int emu_plant_layouts(int kind, int n, const int* p, int* out)
{
    int count = 0;
    for (int i = 0; i < n; ++i) count = emu_plant_layout(kind, p[13 * i], p[13 * i + 1], p[13 * i + 2], p[13 * i + 3], p + 13 * i + 4, out + 24 * i);
    return count;
}

} // extern "C"
