// emu_plant_noise.cpp -- one tick of each build of the plant-step kernel (copra_amd/csrc/plant_step.hpp: the plain tick, the disturbance
// estimator, the state observer) on the host WITH noise drawn in phase 1 (copra_amd/csrc/plant_noise.hpp), walked as the other emulators of
// this directory walk them: every workgroup's threads one after the other through phase 1, then -- a barrier each -- through the later
// phases, over an image filled with NaN.  Beside it the body of the fill kernel, and the generator itself.  Compiled by
// tests/test_noise_abi.py: g++ -shared for ctypes, and with tests/emu/emu_plant_noise_main.cpp as a stand-alone program.
#include "emu_plant_noise.h"
#include "emu_walk.h"

using namespace copra_hip;

namespace {

template <bool kNoise>
int walk(const EmuNoiseTick& t, const PlantStepArgs& P, const PlantObsArgs& Q, emu::Image& img, int order, unsigned long long seed)
{
    const int grid = (P.batch + P.group - 1) / P.group, T = t.threads;
    double* const lds = img.lds;
    if (t.build == 0)
        return emu::walk(img, grid, 2, T, order, seed, [&](int wg, int ph, int tid) {
            if (ph == 0) plant_stage<kNoise>(P, wg, tid, T, lds);
            else plant_apply<kNoise>(P, wg, tid, T, lds);
        });
    if (t.build == 1)
        return emu::walk(img, grid, 4, T, order, seed, [&](int wg, int ph, int tid) {
            if (ph == 0) plant_stage_est<kNoise>(P, wg, tid, T, lds);
            else if (ph == 1) plant_apply_est<kNoise>(P, wg, tid, T, lds);
            else if (ph == 2) plant_estimate<kNoise>(P, wg, tid, T, lds);
            else plant_estimate_store<kNoise>(P, wg, tid, T, lds);
        });
    return emu::walk(img, grid, 4, T, order, seed, [&](int wg, int ph, int tid) {
        if (ph == 0) plant_obs_stage<kNoise>(Q, wg, tid, T, lds);
        else if (ph == 1) plant_obs_apply<kNoise>(Q, wg, tid, T, lds);
        else if (ph == 2) plant_obs_innovate<kNoise>(Q, wg, tid, T, lds);
        else plant_obs_update<kNoise>(Q, wg, tid, T, lds);
    });
}

} // namespace

extern "C" {

// Returns 0; -1: no memory; -2: the guard behind the image was written.  order, seed: the walk order of emu_walk.h; vec2_used (may be null)
// says whether the walk copied two doubles per lane.
int emu_plant_noise_tick_walk(EmuNoiseTick* t, int order, unsigned long long seed, int* vec2_used)
{
    PlantObsArgs Q {};
    PlantStepArgs& P = Q.s;
    P.batch = t->batch, P.nx = t->nx, P.nu = t->nu, P.ctrl_stride = t->nu * t->N, P.group = t->group, P.shared = t->shared;
    P.A = t->A, P.B = t->B, P.d = t->d, P.x0 = t->x, P.x0_next = t->x, P.w = t->w, P.fallback_u = t->fallback_u;
    P.status = t->status, P.control = t->control, P.x_out = t->x_out, P.u_out = t->u_out, P.status_out = t->status_out;
    P.backup_steps = t->backup_steps, P.fresh = t->fresh, P.plan = t->plan, P.next = t->next, P.age_out = t->age_out;
    P.sigma_w = t->sigma_w, P.sigma_per_instance = t->per_instance;
    P.noise = NoiseGen { t->seed, t->first, t->tick };
    size_t total = 0;
    if (t->build == 0) {
        P.vec2 = plant_vec2_ok(P);
        total = (size_t)plant_lds(P.nx, P.nu, P.group, P.shared, plant_has_w(P), P.backup_steps > 0).total;
    } else if (t->build == 1) {
        P.est = 1, P.gain_dense = t->gain_dense, P.gain_shared = t->gain_shared;
        P.Am = t->Am, P.Bm = t->Bm, P.gain = t->gain, P.dhat = t->dhat, P.d_out = t->d_out;
        if (!t->A) P.same_model = 1, P.shared = 0, P.A = t->Am, P.B = t->Bm, P.d = t->dhat;
        P.vec2 = plant_vec2_ok(P);
        total = (size_t)plant_est_lds(P.nx, P.nu, P.group, P.shared, plant_has_w(P), P.backup_steps > 0, P.same_model, P.gain_dense, P.gain_shared).total;
    } else {
        Q.ny = t->ny;
        Q.meas = t->y_meas != nullptr;
        Q.same_model = Q.meas || !t->A;
        Q.gain_shared = t->gain_shared;
        Q.Am = t->Am, Q.Bm = t->Bm, Q.dhat = t->dhat, Q.dhat_next = t->Ld ? t->dhat : nullptr;
        Q.xhat = t->xhat, Q.xhat_next = t->xhat;
        Q.C = t->C, Q.Lx = t->Lx, Q.Ld = t->Ld;
        Q.yv = Q.meas ? t->y_meas : t->v;
        Q.y_out = t->y_out, Q.xhat_out = t->xhat_out, Q.d_out = t->d_out;
        if (!Q.meas) Q.sigma_v = t->sigma_v;
        if (Q.same_model) P.A = t->Am, P.B = t->Bm, P.d = t->dhat, P.shared = 0;
        if (Q.meas) P.x0 = t->xhat, P.x0_next = nullptr, P.x_out = nullptr, P.w = nullptr, P.sigma_w = nullptr;
        P.vec2 = plant_obs_vec2_ok(Q);
        total = (size_t)plant_obs_lds(P.nx, P.nu, Q.ny, P.group, P.shared, plant_has_w(P), P.backup_steps > 0, Q.same_model, Q.meas, Q.Ld != nullptr,
            Q.gain_shared, plant_obs_has_yv(Q)).total;
    }
    t->lds_doubles = (int)total;
    if (vec2_used) *vec2_used = P.vec2;
    emu::Image img(total);
    if (!img.lds) return emu::kEmuNoMemory;
    return t->knoise ? walk<true>(*t, P, Q, img, order, seed) : walk<false>(*t, P, Q, img, order, seed);
}

// ... every phase and the grid walked in ascending order
int emu_plant_noise_tick(EmuNoiseTick* t) { return emu_plant_noise_tick_walk(t, 0, 0, nullptr); }

// the fill kernel's body over its grid: out[batch][rows]
void emu_noise_fill(int batch, int rows, int stream, int per_instance, int group, int threads, unsigned long long seed, unsigned long long first,
    unsigned long long tick, const double* sigma, double* out)
{
    NoiseFillArgs F {};
    F.batch = batch, F.rows = rows, F.stream = stream, F.per_instance = per_instance, F.group = group;
    F.gen = NoiseGen { seed, first, tick };
    F.sigma = sigma, F.out = out;
    const int grid = (batch + group - 1) / group;
    for (int wg = 0; wg < grid; ++wg)
        for (int tid = 0; tid < threads; ++tid) noise_fill_body(F, wg, tid, threads);
}

void emu_philox(const unsigned* counter, const unsigned* key, unsigned* out)
{
    const PhiloxOut o = philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
    out[0] = o.o0, out[1] = o.o1, out[2] = o.o2, out[3] = o.o3;
}

// the generator's words of `count` draws: gi = first_instance + b
void emu_noise_words(int count, const unsigned long long* seed, const unsigned long long* gi, const int* s, const int* j, const unsigned long long* t, unsigned* out)
{
    for (int i = 0; i < count; ++i) {
        const PhiloxOut o = noise_words(seed[i], gi[i], s[i], j[i], t[i]);
        out[4 * i] = o.o0, out[4 * i + 1] = o.o1, out[4 * i + 2] = o.o2, out[4 * i + 3] = o.o3;
    }
}

} // extern "C"
