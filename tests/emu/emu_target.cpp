// emu_target.cpp -- the target kernel's phase bodies (copra_amd/csrc/target_step.hpp) on the host: a walker over the four phases with a
// NaN-filled image, the guard words and the walk orders of emu_walk.h.  Compile with -ffp-contract=off: every product and every sum is
// rounded, the order is the one the header writes down.
#include "emu_target.h"

#include "../../copra_amd/csrc/target_step.hpp"
#include "emu_walk.h"

#include <cmath>

using namespace copra_hip;

extern "C" {

int emu_target_run(EmuTarget* t)
{
    if (t->ncost < 0 || t->ncost > kTargetMaxCosts) return emu::kEmuNoMemory;
    TargetArgs S {};
    S.batch = t->batch, S.nx = t->nx, S.nu = t->nu, S.group = t->group;
    S.per_instance = t->per_instance;
    S.A = t->A, S.B = t->B, S.d = t->d, S.H = t->H, S.r = t->r;
    S.steps = t->steps;
    const long long tau = t->tau < 0 ? 0 : t->tau;
    S.row = tau < S.steps - 1 ? tau : S.steps - 1;
    S.ncost = t->ncost;
    for (int k = 0; k < S.ncost; ++k) S.c[k].map = t->cost_map[k], S.c[k].out = t->cost_out[k], S.c[k].r = t->cost_rows[k], S.c[k].S = t->cost_blocks[k];
    S.z = t->z, S.status = t->status;
    if (t->vec2_mode < 0) target_prepare(S);
    t->vec2_used = S.vec2_in | (S.vec2_z << 1);
    for (int k = 0; k < S.ncost; ++k) t->vec2_used |= S.c[k].vec2 << (2 + k);
    const TargetLds L = target_lds(S);
    t->lds_doubles = L.total;
    t->nan_left = 0;
    emu::Image img((size_t)L.total);
    if (!img.lds) return emu::kEmuNoMemory;
    const int grid = (S.batch + S.group - 1) / S.group, n = S.nx + S.nu;
    return emu::walk(img, grid, 5, t->threads, t->order, t->seed, [&](int wg, int ph, int tid) {
        if (ph == 0) target_stage(S, wg, tid, t->threads, img.lds);
        else if (ph == 1) target_fill(S, wg, tid, t->threads, img.lds);
        else if (ph == 2) target_solve(S, wg, tid, t->threads, img.lds);
        else if (ph == 3) target_store(S, wg, tid, t->threads, img.lds);
        else if (tid == 0) { // (no phase of the kernel: the image after the last one is looked at once per workgroup)
            const int b0 = wg * S.group, cnt = S.batch - b0 < S.group ? S.batch - b0 : S.group;
            const int* st = reinterpret_cast<const int*>(img.lds + L.ost);
            for (int i = 0; i < cnt; ++i)
                for (int j = 0; j < n && !st[i]; ++j)
                    if (std::isnan(img.lds[L.oM + (n * n + j) * S.group + i])) t->nan_left = 1;
        }
    });
}

long long emu_target_image_bytes(int nx, int nu, int map_doubles) { return (long long)target_image_bytes(nx, nu, map_doubles); }
int emu_target_launch_group(int nx, int nu, int map_doubles) { return target_group(nx, nu, map_doubles); }
int emu_target_layout(int nx, int nu, int group, int map_doubles, int* out)
{
    const TargetLds L = target_lds(nx, nu, group, map_doubles);
    out[0] = L.oM, out[1] = L.oH, out[2] = L.oT, out[3] = L.ost, out[4] = L.total;
    return 5;
}
int emu_target_threads(void) { return kTargetThreads; }
int emu_target_max_costs(void) { return kTargetMaxCosts; }
long long emu_target_lds_max(void) { return (long long)kPlantLdsMax; }
}
