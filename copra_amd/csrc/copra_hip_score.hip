// copra_hip_score.hip -- closed-loop scores of the C ABI (include/copra_hip.h, ABI 14): copra_batch_set_score hands the measure over and takes
// every buffer the feature needs; launch_score is what the tick (copra_hip_plant.hip, advance()) calls behind its plant step while scoring is
// on -- one launch of copra_score_kernel on the tick's stream, no synchronisation, no allocation; copra_batch_score_reset / _score_device /
// _get_score handle the records, copra_batch_score_summary reduces them with copra_score_reduce_kernel in the order score_step.hpp writes down.
#include "engine.hpp"
#define COPRA_PLANT_PHASES_ONLY // (plant_step.hpp through score_step.hpp: its helpers and geometry, not its kernels)
#include "score_step.hpp"

#include <cmath>
#include <cstddef>
#include <cstring>

static_assert(sizeof(copra_score_record_t) == sizeof(ScoreRecord) && sizeof(copra_score_record_t) == 64, "the record of the header is the kernel's");
static_assert(offsetof(copra_score_record_t, ticks) == offsetof(ScoreRecord, ticks) && offsetof(copra_score_record_t, first_violation) == offsetof(ScoreRecord, first_violation),
    "the record of the header is the kernel's");
static_assert(sizeof(copra_score_stat_t) == sizeof(ScoreStat) && sizeof(copra_score_summary_t) == sizeof(ScoreSummary), "the summary of the header is the kernel's");
static_assert(offsetof(copra_score_summary_t, ticks) == offsetof(ScoreSummary, c) && offsetof(copra_score_summary_t, peak) == 4 * sizeof(ScoreStat),
    "the summary of the header is the kernel's");

namespace {

copra_status_t check_handle(const copra_batch* h, const char* who)
{
    if (h->hp.plan.initial_state)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": the initial state of an InitialStateLMPC controller is a decision variable, not the plant's state");
    return COPRA_OK;
}

void score_off(copra_batch* h) // (a release waits for a tick that still uses the buffer)
{
    h->score_on = false;
    for (int k = 0; k < kScoreArrays; ++k) h->score_arr[k].reset();
    h->d_score.reset();
    h->d_score_u.reset();
    h->d_score_age.reset();
    h->d_score_part.reset();
    h->h_score_sum.reset();
}

} // namespace

copra_status_t launch_score(copra_batch* h, const double* x, const double* u, const int* age, hipStream_t s, const char* who)
{
    const FusedPlan& HP = h->hp.plan;
    if (!h->score_on || HP.batch <= 0) return COPRA_OK;
    if (!h->d_score || !x || !u || !age) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the score has lost its buffers");
    ScoreArgs S {};
    S.batch = HP.batch, S.nx = HP.nx, S.nu = HP.nu;
    S.dense = h->score_dense, S.per_instance = h->score_per_instance;
    S.x = x, S.u = u, S.age = age;
    S.qx = h->score_arr[0], S.ru = h->score_arr[1], S.x_ref = h->score_arr[2];
    S.x_lo = h->score_arr[3], S.x_hi = h->score_arr[4], S.u_lo = h->score_arr[5], S.u_hi = h->score_arr[6];
    S.ref_steps = S.x_ref ? h->score_ref_steps : 1;
    const long long tau = h->sched_tick < 0 ? 0 : h->sched_tick;
    S.ref_row = tau < S.ref_steps - 1 ? tau : S.ref_steps - 1;
    S.tol = h->score_tol;
    S.rec = reinterpret_cast<ScoreRecord*>((unsigned char*)h->d_score);
    S.group = score_group(S.nx, S.nu, S.dense); // (the geometry: score_step.hpp; checked against the LDS by the setter)
    S.vec2 = score_vec2_ok(S);
    const size_t lds_bytes = (size_t)score_lds(S).total * sizeof(double);
    if (lds_bytes > 48 * 1024) LDS_OPT_IN(copra_score_kernel, lds_bytes);
    const unsigned grid = (unsigned)((S.batch + S.group - 1) / S.group);
    hipLaunchKernelGGL(copra_score_kernel, dim3(grid), dim3(kScoreThreads), lds_bytes, s, S);
    HIP_TRY(hipGetLastError());
    return COPRA_OK;
}

extern "C" {

void copra_score_init(copra_score_t* score)
{
    if (!score) return;
    std::memset(score, 0, sizeof *score);
    score->struct_size = (int)sizeof *score;
}

copra_status_t copra_batch_set_score(copra_batch_t* h, const copra_score_t* score)
{
    const char* const who = "copra_batch_set_score";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    const copra_status_t rc = check_handle(h, who);
    if (rc != COPRA_OK) return rc;
    if (!score) { // scoring ends, the buffers go
        score_off(h);
        return COPRA_OK;
    }
    copra_score_t m;
    const copra_status_t rc_m = read_sized(m, score, who, "copra_score_t", "copra_score_init");
    if (rc_m != COPRA_OK) return rc_m;
    if (m.x_ref && m.ref_steps < 1) return fail(COPRA_ERR_ARG, std::string(who) + ": ref_steps < 1");
    if (!(m.tol >= 0.0)) return fail(COPRA_ERR_ARG, std::string(who) + ": a negative or NaN tol");
    const FusedPlan& P = h->hp.plan;
    const int dense = m.dense != 0, per = m.per_instance != 0;
    if ((double)P.nx * P.nx + (double)P.nu * P.nu > 1e6 || score_image_bytes(P.nx, P.nu, dense) > kPlantLdsMax)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": one instance's state, control and measure do not fit the LDS");
    const size_t b = (size_t)(P.batch > 0 ? P.batch : 1), lead = per ? b : 1;
    const size_t nx = (size_t)P.nx, nu = (size_t)P.nu;
    const double* arr[kScoreArrays] = { m.qx, m.ru, m.x_ref, m.x_lo, m.x_hi, m.u_lo, m.u_hi };
    const size_t count[kScoreArrays] = { lead * (dense ? nx * nx : nx), lead * (dense ? nu * nu : nu), lead * (size_t)(m.x_ref ? m.ref_steps : 0) * nx, lead * nx, lead * nx,
        lead * nu, lead * nu };
    if (!m.on_device) {
        for (int k = 0; k < 2; ++k)
            for (size_t i = 0; arr[k] && i < count[k]; ++i)
                if (std::isnan(arr[k][i])) return fail(COPRA_ERR_ARG, std::string(who) + ": a NaN weight");
        for (int k = 3; k < kScoreArrays; k += 2)
            for (size_t i = 0; arr[k] && arr[k + 1] && i < count[k]; ++i)
                if (!(arr[k][i] <= arr[k + 1][i])) return fail(COPRA_ERR_ARG, std::string(who) + ": a lower limit above its upper limit (or a NaN limit)");
        for (int k = 3; k < kScoreArrays; ++k)
            for (size_t i = 0; arr[k] && i < count[k]; ++i)
                if (std::isnan(arr[k][i])) return fail(COPRA_ERR_ARG, std::string(who) + ": a NaN limit");
    }
    h->score_on = false; // (a failed attempt leaves the feature off, never a measure half replaced)
    if (!m.on_device) HIP_TRY(hipStreamSynchronize(h->last_stream)); // the library's copies: a tick that still reads the old ones first
    for (int k = 0; k < kScoreArrays; ++k) {
        if (m.on_device || !arr[k]) h->score_arr[k].borrow(arr[k]);
        else OWN_TRY(h->score_arr[k].copy_in(arr[k], count[k]));
    }
    const size_t chunks = (size_t)score_chunks((long long)b);
    if (!h->d_score) OWN_TRY(h->d_score.alloc(b * sizeof(ScoreRecord)));
    if (!h->d_score_u) OWN_TRY(h->d_score_u.alloc(b * nu));
    if (!h->d_score_age) OWN_TRY(h->d_score_age.alloc(b));
    if (!h->d_score_part) OWN_TRY(h->d_score_part.alloc((chunks + 1) * sizeof(ScoreSummary)));
    if (!h->h_score_sum) OWN_TRY(h->h_score_sum.alloc(sizeof(ScoreSummary)));
    HIP_TRY(hipMemsetAsync(h->d_score, 0, b * sizeof(ScoreRecord), h->last_stream)); // behind the last solve / tick
    h->score_dense = dense, h->score_per_instance = per;
    h->score_ref_steps = m.x_ref ? m.ref_steps : 1;
    h->score_tol = m.tol;
    h->score_on = true;
    return COPRA_OK;
}

copra_status_t copra_batch_score_reset(copra_batch_t* h)
{
    const char* const who = "copra_batch_score_reset";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    if (!h->score_on || !h->d_score) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": scoring is not on (copra_batch_set_score)");
    const size_t b = (size_t)(h->hp.plan.batch > 0 ? h->hp.plan.batch : 1);
    HIP_TRY(hipMemsetAsync(h->d_score, 0, b * sizeof(ScoreRecord), h->last_stream));
    return COPRA_OK;
}

const copra_score_record_t* copra_batch_score_device(const copra_batch_t* h)
{
    return h && h->score_on ? reinterpret_cast<const copra_score_record_t*>((const unsigned char*)h->d_score) : nullptr;
}

copra_status_t copra_batch_get_score(copra_batch_t* h, copra_score_record_t* host)
{
    const char* const who = "copra_batch_get_score";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    if (!host) return fail(COPRA_ERR_ARG, std::string(who) + ": null destination");
    if (!h->score_on || !h->d_score) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": scoring is not on (copra_batch_set_score)");
    HIP_TRY(hipStreamSynchronize(h->last_stream));
    if (h->hp.plan.batch > 0) HIP_TRY(hipMemcpy(host, h->d_score, (size_t)h->hp.plan.batch * sizeof(ScoreRecord), hipMemcpyDeviceToHost));
    return COPRA_OK;
}

copra_status_t copra_batch_score_summary(copra_batch_t* h, copra_score_summary_t* out)
{
    const char* const who = "copra_batch_score_summary";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    if (!out) return fail(COPRA_ERR_ARG, std::string(who) + ": null destination");
    if (!h->score_on || !h->d_score || !h->d_score_part || !h->h_score_sum)
        return fail(COPRA_ERR_RUNTIME, std::string(who) + ": scoring is not on (copra_batch_set_score)");
    const long long batch = h->hp.plan.batch;
    if (batch <= 0) {
        const ScoreSummary none = score_empty();
        std::memcpy(out, &none, sizeof none);
        return COPRA_OK;
    }
    hipStream_t s = h->last_stream;
    const long long chunks = score_chunks(batch);
    ScoreSummary* const part = reinterpret_cast<ScoreSummary*>((unsigned char*)h->d_score_part);
    const size_t lds_bytes = (kScoreThreads / 64) * sizeof(ScoreStat);
    ScoreReduceArgs R {};
    R.stage = 1, R.count = batch, R.rec = reinterpret_cast<const ScoreRecord*>((const unsigned char*)h->d_score), R.out = part;
    hipLaunchKernelGGL(copra_score_reduce_kernel, dim3((unsigned)chunks), dim3(kScoreThreads), lds_bytes, s, R);
    HIP_TRY(hipGetLastError());
    R.stage = 2, R.count = chunks, R.rec = nullptr, R.partials = part, R.out = part + chunks;
    hipLaunchKernelGGL(copra_score_reduce_kernel, dim3(1), dim3(kScoreThreads), lds_bytes, s, R);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->h_score_sum, part + chunks, sizeof(ScoreSummary), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s)); // (waits for the last tick as well: the reduction stands behind it on its stream)
    std::memcpy(out, h->h_score_sum, sizeof(ScoreSummary));
    return COPRA_OK;
}

} // extern "C"
