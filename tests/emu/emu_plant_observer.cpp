// emu_plant_observer.cpp -- one tick of the plant-step kernel WITH its state observer (copra_amd/csrc/plant_step.hpp: PlantObsArgs, the
// phases plant_obs_stage / _apply / _innovate / _update) on the host, walked as tests/emu/emu_plant_bias.cpp walks the estimator: every
// workgroup's threads one after the other through phase 1, then -- a barrier each -- through phases 2, 3 and 4, over an image filled with
// NaN.  Compiled by tests/test_observer_abi.py itself: g++ -shared for ctypes, and with tests/emu/emu_plant_observer_main.cpp as a
// stand-alone program.
#include "emu_walk.h"

using namespace copra_hip;

extern "C" {

// The arguments of one tick; every pointer as the library's launch would pass it.  A == NULL: no plant of its own -- the plant is
// (Am, Bm, dhat).  y_meas != NULL: no plant at all, xp is not looked at.  Ld == NULL: dhat is only read.  vec2_mode: -1 as
// plant_obs_vec2_ok decides, 0 never.  xhat_next may be xhat; xp and dhat are updated in place.
struct EmuObserverTick {
    int batch, nx, nu, ny, N, group, threads, shared;
    const double *A, *B, *d; // the plant
    double* xp;
    const double *w, *fallback_u;
    const int* status;
    const double* control;
    double *x_out, *u_out;
    int* status_out;
    int backup_steps, fresh;
    double* plan;
    int* next;
    int* age_out;
    int gain_shared;
    const double *Am, *Bm;
    double* dhat;
    const double* xhat;
    double* xhat_next;
    const double *C, *Lx, *Ld, *v, *y_meas;
    double *y_out, *xhat_out, *d_out;
    int vec2_mode, vec2_used;
};

// Returns 0; -1: no memory; -2: the guard behind the image was written.  order, seed: the walk order of emu_walk.h.
int emu_plant_observer_step_walk(EmuObserverTick* t, int order, unsigned long long seed)
{
    PlantObsArgs Q {};
    PlantStepArgs& P = Q.s;
    P.batch = t->batch, P.nx = t->nx, P.nu = t->nu, P.ctrl_stride = t->nu * t->N, P.group = t->group, P.shared = t->shared;
    P.A = t->A, P.B = t->B, P.d = t->d, P.x0 = t->xp, P.x0_next = t->xp, P.w = t->w, P.fallback_u = t->fallback_u;
    P.status = t->status, P.control = t->control, P.x_out = t->x_out, P.u_out = t->u_out, P.status_out = t->status_out;
    P.backup_steps = t->backup_steps, P.fresh = t->fresh, P.plan = t->plan, P.next = t->next, P.age_out = t->age_out;
    Q.ny = t->ny;
    Q.meas = t->y_meas != nullptr;
    Q.same_model = Q.meas || !t->A;
    Q.gain_shared = t->gain_shared;
    Q.Am = t->Am, Q.Bm = t->Bm, Q.dhat = t->dhat, Q.dhat_next = t->Ld ? t->dhat : nullptr;
    Q.xhat = t->xhat, Q.xhat_next = t->xhat_next;
    Q.C = t->C, Q.Lx = t->Lx, Q.Ld = t->Ld;
    Q.yv = Q.meas ? t->y_meas : t->v;
    Q.y_out = t->y_out, Q.xhat_out = t->xhat_out, Q.d_out = t->d_out;
    if (Q.same_model) P.A = t->Am, P.B = t->Bm, P.d = t->dhat, P.shared = 0;
    if (Q.meas) P.x0 = t->xhat, P.x0_next = nullptr, P.x_out = nullptr, P.w = nullptr;
    P.vec2 = t->vec2_mode == 0 ? 0 : plant_obs_vec2_ok(Q);
    t->vec2_used = P.vec2;
    const size_t total = (size_t)plant_obs_lds(P.nx, P.nu, Q.ny, P.group, P.shared, P.w != nullptr, P.backup_steps > 0, Q.same_model, Q.meas, Q.Ld != nullptr,
        Q.gain_shared, Q.yv != nullptr).total;
    emu::Image img(total);
    if (!img.lds) return emu::kEmuNoMemory;
    double* const lds = img.lds;
    const int T = t->threads;
    return emu::walk(img, (P.batch + P.group - 1) / P.group, 4, T, order, seed, [&](int wg, int ph, int tid) {
        if (ph == 0) plant_obs_stage(Q, wg, tid, T, lds);
        else if (ph == 1) plant_obs_apply(Q, wg, tid, T, lds);
        else if (ph == 2) plant_obs_innovate(Q, wg, tid, T, lds);
        else plant_obs_update(Q, wg, tid, T, lds);
    });
}

// ... every phase and the grid walked in ascending order
int emu_plant_observer_step(EmuObserverTick* t) { return emu_plant_observer_step_walk(t, 0, 0); }

// the image in doubles, as the launch sizes it
int emu_plant_observer_lds_doubles(int nx, int nu, int ny, int group, int shared, int has_w, int backup, int same_model, int meas, int has_Ld, int gain_shared,
    int has_yv)
{
    return plant_obs_lds(nx, nu, ny, group, shared, has_w, backup, same_model, meas, has_Ld, gain_shared, has_yv).total;
}

} // extern "C"
