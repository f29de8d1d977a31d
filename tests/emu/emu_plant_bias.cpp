// emu_plant_bias.cpp -- one tick of the plant-step kernel WITH its disturbance estimator (copra_amd/csrc/plant_step.hpp: est, same_model, gain,
// Am, Bm, dhat, d_out) on the host, walked as tests/emu/emu_plant_backup.cpp walks it: every workgroup's threads one after the other through
// phase 1, then -- a barrier each -- through phase 2, phase 3 (the errors) and the update, over an image filled with NaN.  est == 0 walks the
// two phases of the kernel built without the estimator over the image of plant_lds.  Compiled by tests/test_bias_estimator_abi.py itself:
// g++ -shared for ctypes, and with tests/emu/emu_plant_bias_main.cpp as a stand-alone program.
#include "emu_walk.h"

using namespace copra_hip;

extern "C" {

// Returns 0; -1: no memory.  A == NULL with est != 0: no plant of its own -- the plant is (Am, Bm, dhat), staged once.  vec2_mode: -1 as
// plant_vec2_ok decides, 0 never.  x0_next may be x0; dhat is updated in place.  -2: the guard behind the image was written.  order, seed: the
// walk order of emu_walk.h.
int emu_plant_bias_step_walk(int batch, int nx, int nu, int N, int group, int threads, int shared, const double* A, const double* B, const double* d,
    const double* x0, const double* w, const double* fallback_u, const int* status, const double* control, double* x0_next, double* x_out, double* u_out,
    int* status_out, int* vec2_used, int backup_steps, int fresh, double* plan, int* next, int* age_out, int est, int gain_dense, int gain_shared,
    const double* Am, const double* Bm, const double* gain, double* dhat, double* d_out, int vec2_mode, int order, unsigned long long seed)
{
    PlantStepArgs P {};
    P.batch = batch, P.nx = nx, P.nu = nu, P.ctrl_stride = nu * N, P.group = group, P.shared = shared;
    P.A = A, P.B = B, P.d = d, P.x0 = x0, P.w = w, P.fallback_u = fallback_u, P.status = status, P.control = control;
    P.x0_next = x0_next, P.x_out = x_out, P.u_out = u_out, P.status_out = status_out;
    P.backup_steps = backup_steps, P.fresh = fresh, P.plan = plan, P.next = next, P.age_out = age_out;
    if (est) {
        P.est = 1, P.gain_dense = gain_dense, P.gain_shared = gain_shared;
        P.Am = Am, P.Bm = Bm, P.gain = gain, P.dhat = dhat, P.d_out = d_out;
        if (!A) P.same_model = 1, P.shared = 0, P.A = Am, P.B = Bm, P.d = dhat;
    }
    P.vec2 = vec2_mode == 0 ? 0 : plant_vec2_ok(P);
    if (vec2_used) *vec2_used = P.vec2;
    const size_t total = est ? (size_t)plant_est_lds(nx, nu, group, P.shared, w != nullptr, backup_steps > 0, P.same_model, gain_dense, gain_shared).total
                             : (size_t)plant_lds(nx, nu, group, shared, w != nullptr, backup_steps > 0).total;
    emu::Image img(total);
    if (!img.lds) return emu::kEmuNoMemory;
    double* const lds = img.lds;
    const int grid = (batch + group - 1) / group;
    if (!est)
        return emu::walk(img, grid, 2, threads, order, seed, [&](int wg, int ph, int tid) {
            if (ph == 0) plant_stage(P, wg, tid, threads, lds);
            else plant_apply(P, wg, tid, threads, lds);
        });
    return emu::walk(img, grid, 4, threads, order, seed, [&](int wg, int ph, int tid) {
        if (ph == 0) plant_stage_est(P, wg, tid, threads, lds);
        else if (ph == 1) plant_apply_est(P, wg, tid, threads, lds);
        else if (ph == 2) plant_estimate(P, wg, tid, threads, lds);
        else plant_estimate_store(P, wg, tid, threads, lds);
    });
}

// ... every phase and the grid walked in ascending order
int emu_plant_bias_step(int batch, int nx, int nu, int N, int group, int threads, int shared, const double* A, const double* B, const double* d,
    const double* x0, const double* w, const double* fallback_u, const int* status, const double* control, double* x0_next, double* x_out, double* u_out,
    int* status_out, int* vec2_used, int backup_steps, int fresh, double* plan, int* next, int* age_out, int est, int gain_dense, int gain_shared,
    const double* Am, const double* Bm, const double* gain, double* dhat, double* d_out, int vec2_mode)
{
    return emu_plant_bias_step_walk(batch, nx, nu, N, group, threads, shared, A, B, d, x0, w, fallback_u, status, control, x0_next, x_out, u_out, status_out,
        vec2_used, backup_steps, fresh, plan, next, age_out, est, gain_dense, gain_shared, Am, Bm, gain, dhat, d_out, vec2_mode, 0, 0);
}

// the image of the kernel built WITHOUT the estimator
int emu_plant_bias_lds_doubles(int nx, int nu, int group, int shared, int has_w, int backup) { return plant_lds(nx, nu, group, shared, has_w, backup).total; }

// ... and with it
int emu_plant_bias_est_doubles(int nx, int nu, int group, int shared, int has_w, int backup, int same_model, int gain_dense, int gain_shared)
{
    return plant_est_lds(nx, nu, group, shared, has_w, backup, same_model, gain_dense, gain_shared).total;
}

} // extern "C"
