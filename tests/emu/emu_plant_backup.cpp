// emu_plant_backup.cpp -- one tick of the plant-step kernel WITH its backup-plan arguments (copra_amd/csrc/plant_step.hpp: backup_steps, fresh,
// plan, next, age_out) on the host, walked as tests/emu/emu_plant.cpp walks it: every workgroup's threads one after the other through phase 1,
// then -- the barrier -- through phase 2, over an image filled with NaN.  The caller keeps plan / next between ticks.  Compiled by
// tests/test_backup_plan_abi.py itself: g++ -shared for ctypes, and with tests/emu/emu_plant_backup_main.cpp as a stand-alone program.
#include "../../copra_amd/csrc/plant_step.hpp"

#include <cstdlib>
#include <limits>

using namespace copra_hip;

extern "C" {

// Returns 0; -1: no memory.  backup_steps == 0: plan / next may be null and the tick is emu_plant_step's.  x0_next may be x0.
int emu_plant_backup_step(int batch, int nx, int nu, int N, int group, int threads, int shared, const double* A, const double* B, const double* d,
    const double* x0, const double* w, const double* fallback_u, const int* status, const double* control, double* x0_next, double* x_out, double* u_out,
    int* status_out, int* vec2_used, int backup_steps, int fresh, double* plan, int* next, int* age_out)
{
    PlantStepArgs P {};
    P.batch = batch, P.nx = nx, P.nu = nu, P.ctrl_stride = nu * N, P.group = group, P.shared = shared;
    P.A = A, P.B = B, P.d = d, P.x0 = x0, P.w = w, P.fallback_u = fallback_u, P.status = status, P.control = control;
    P.x0_next = x0_next, P.x_out = x_out, P.u_out = u_out, P.status_out = status_out;
    P.backup_steps = backup_steps, P.fresh = fresh, P.plan = plan, P.next = next, P.age_out = age_out;
    P.vec2 = plant_vec2_ok(P);
    if (vec2_used) *vec2_used = P.vec2;
    const size_t total = (size_t)plant_lds(nx, nu, group, shared, w != nullptr, backup_steps > 0).total;
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

int emu_plant_backup_lds_doubles(int nx, int nu, int group, int shared, int has_w, int backup) { return plant_lds(nx, nu, group, shared, has_w, backup).total; }

} // extern "C"
