// emu_plant.cpp -- the plant-step kernel's two phases (copra_amd/csrc/plant_step.hpp) on the host: every workgroup's threads are walked one
// after the other through phase 1, then -- the barrier -- through phase 2, with a host buffer in the place of LDS.  Compiled by
// tests/test_closed_loop_abi.py itself (g++ -shared into its tmp_path); no part of the emulator's Makefile.
#include "../../copra_amd/csrc/plant_step.hpp"

#include <cstdlib>
#include <limits>

using namespace copra_hip;

extern "C" {

// Returns 0; -1: no memory; vec2_used (may be null) says whether the launch copied two doubles per lane.  x0_next may be x0.
int emu_plant_step(int batch, int nx, int nu, int N, int group, int threads, int shared, const double* A, const double* B, const double* d, const double* x0,
    const double* w, const double* fallback_u, const int* status, const double* control, double* x0_next, double* x_out, double* u_out, int* status_out,
    int* vec2_used)
{
    PlantStepArgs P {};
    P.batch = batch, P.nx = nx, P.nu = nu, P.ctrl_stride = nu * N, P.group = group, P.shared = shared;
    P.A = A, P.B = B, P.d = d, P.x0 = x0, P.w = w, P.fallback_u = fallback_u, P.status = status, P.control = control;
    P.x0_next = x0_next, P.x_out = x_out, P.u_out = u_out, P.status_out = status_out;
    P.vec2 = plant_vec2_ok(P);
    if (vec2_used) *vec2_used = P.vec2;
    const size_t total = (size_t)plant_lds(nx, nu, group, shared, w != nullptr).total;
    double* lds = static_cast<double*>(std::aligned_alloc(16, (total * sizeof(double) + 15) / 16 * 16));
    if (!lds) return -1;
    const int grid = (batch + group - 1) / group;
    for (int wg = 0; wg < grid; ++wg) {
        for (size_t i = 0; i < total; ++i) lds[i] = std::numeric_limits<double>::quiet_NaN(); // (LDS is not initialised: whatever is read must have been staged)
        for (int tid = 0; tid < threads; ++tid) plant_stage(P, wg, tid, threads, lds);
        for (int tid = 0; tid < threads; ++tid) plant_apply(P, wg, tid, threads, lds);
    }
    std::free(lds);
    return 0;
}

int emu_plant_lds_doubles(int nx, int nu, int group, int shared, int has_w) { return plant_lds(nx, nu, group, shared, has_w).total; }

} // extern "C"
