// emu_plant.cpp -- the plant-step kernel's two phases (copra_amd/csrc/plant_step.hpp) on the host: every workgroup's threads are walked one
// after the other through phase 1, then -- the barrier -- through phase 2, with a host buffer in the place of LDS.  Compiled by
// tests/test_closed_loop_abi.py itself (g++ -shared into its tmp_path); no part of the emulator's Makefile.
#include "emu_walk.h"

using namespace copra_hip;

extern "C" {

// Returns 0; -1: no memory; -2: the guard behind the image was written; vec2_used (may be null) says whether the launch copied two doubles
// per lane.  x0_next may be x0.  order, seed: the walk order of emu_walk.h.
int emu_plant_step_walk(int batch, int nx, int nu, int N, int group, int threads, int shared, const double* A, const double* B, const double* d, const double* x0,
    const double* w, const double* fallback_u, const int* status, const double* control, double* x0_next, double* x_out, double* u_out, int* status_out,
    int* vec2_used, int order, unsigned long long seed)
{
    PlantStepArgs P {};
    P.batch = batch, P.nx = nx, P.nu = nu, P.ctrl_stride = nu * N, P.group = group, P.shared = shared;
    P.A = A, P.B = B, P.d = d, P.x0 = x0, P.w = w, P.fallback_u = fallback_u, P.status = status, P.control = control;
    P.x0_next = x0_next, P.x_out = x_out, P.u_out = u_out, P.status_out = status_out;
    P.vec2 = plant_vec2_ok(P);
    if (vec2_used) *vec2_used = P.vec2;
    const size_t total = (size_t)plant_lds(nx, nu, group, shared, w != nullptr).total;
    emu::Image img(total);
    if (!img.lds) return emu::kEmuNoMemory;
    return emu::walk(img, (batch + group - 1) / group, 2, threads, order, seed, [&](int wg, int ph, int tid) {
        if (ph == 0) plant_stage(P, wg, tid, threads, img.lds);
        else plant_apply(P, wg, tid, threads, img.lds);
    });
}

// ... every phase and the grid walked in ascending order
int emu_plant_step(int batch, int nx, int nu, int N, int group, int threads, int shared, const double* A, const double* B, const double* d, const double* x0,
    const double* w, const double* fallback_u, const int* status, const double* control, double* x0_next, double* x_out, double* u_out, int* status_out,
    int* vec2_used)
{
    return emu_plant_step_walk(batch, nx, nu, N, group, threads, shared, A, B, d, x0, w, fallback_u, status, control, x0_next, x_out, u_out, status_out, vec2_used,
        0, 0);
}

int emu_plant_lds_doubles(int nx, int nu, int group, int shared, int has_w) { return plant_lds(nx, nu, group, shared, has_w).total; }

} // extern "C"
