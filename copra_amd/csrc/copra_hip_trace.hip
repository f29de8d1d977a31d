// copra_hip_trace.hip -- ensemble traces of the C ABI (include/copra_hip.h, ABI 17): copra_batch_set_trace takes every buffer the feature needs;
// launch_trace is what the tick (copra_hip_plant.hip, advance()) calls behind its score while tracing is on -- on a recorded tick two launches
// of copra_trace_kernel on the tick's stream into the slot the host counted, no synchronisation, no allocation, no counter on the device;
// copra_batch_trace_reset / _trace_info / _trace_device / _get_trace handle the slots.  The reduction and its order: trace_step.hpp.
#include "engine.hpp"
#define COPRA_PLANT_PHASES_ONLY // (plant_step.hpp and score_step.hpp through trace_step.hpp: their helpers and geometry, not their kernels)
#define COPRA_SCORE_HELPERS_ONLY
#include "trace_step.hpp"

#include <cmath>
#include <cstddef>
#include <cstring>

static_assert(sizeof(copra_trace_head_t) == sizeof(TraceHead) && sizeof(copra_trace_head_t) == 64, "the head of the header is the kernel's");
static_assert(offsetof(copra_trace_head_t, solved) == offsetof(TraceHead, solved) && offsetof(copra_trace_head_t, violating) == offsetof(TraceHead, violating),
    "the head of the header is the kernel's");
static_assert(COPRA_TRACE_X == kTraceX && COPRA_TRACE_U == kTraceU && COPRA_TRACE_ERR == kTraceErr, "the bits of the header are the kernel's");

namespace {

void trace_off(copra_batch* h) // (a release waits for a tick that still uses the buffer)
{
    h->trace_on = false;
    trace_quant_off(h); // (quantiles belong to the trace in force)
    for (int k = 0; k < kTraceArrays; ++k) h->trace_lim[k].reset();
    h->d_trace.reset();
    h->d_trace_part.reset();
    h->d_trace_u.reset();
    h->d_trace_age.reset();
    h->trace_tick = h->trace_recorded = h->trace_missed = 0;
}

size_t slot_bytes(const copra_batch* h) { return trace_slot_bytes(h->trace_rows); }

} // namespace

copra_status_t launch_trace(copra_batch* h, const double* x, const double* est, const double* u, const int* age, hipStream_t s, const char* who)
{
    const FusedPlan& HP = h->hp.plan;
    if (!h->trace_on || HP.batch <= 0) return COPRA_OK;
    if (!h->d_trace || !h->d_trace_part || !x || !u || !age) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the trace has lost its buffers");
    TraceClock clock { h->trace_tick, h->trace_recorded, h->trace_missed, h->trace_cap, h->trace_every };
    long long tick = 0;
    const long long slot = trace_next_slot(clock, &tick); // (the tick count moves at every tick; a full trace counts `missed`, it never fails the tick)
    h->trace_tick = clock.tick, h->trace_recorded = clock.recorded, h->trace_missed = clock.missed;
    if (slot < 0) return COPRA_OK;
    TraceArgs T {};
    T.batch = HP.batch, T.nx = HP.nx, T.nu = HP.nu;
    T.what = h->trace_what;
    T.err_live = est != nullptr;
    T.x = x, T.u = u, T.est = est, T.age = age;
    T.x_lo = h->trace_lim[0], T.x_hi = h->trace_lim[1], T.u_lo = h->trace_lim[2], T.u_hi = h->trace_lim[3];
    T.tol = h->trace_tol;
    T.tick = tick, T.tau = h->sched_tick;
    T.chunks = score_chunks(T.batch);
    T.part = h->d_trace_part;
    T.slot = (unsigned char*)h->d_trace + (size_t)slot * slot_bytes(h); // (the slot was counted here: nothing on the device counts)
    T.in_lds = h->trace_in_lds; // (decided by the setter for the trace's widest tick: trace_step.hpp)
    T.vec2 = trace_vec2_ok(T);
    const size_t lds1 = T.in_lds ? (size_t)trace_lds(T).total * sizeof(double) : 0;
    if (lds1 > 48 * 1024) LDS_OPT_IN(copra_trace_kernel<1>, lds1);
    hipLaunchKernelGGL(copra_trace_kernel<1>, dim3((unsigned)T.chunks), dim3(kScoreThreads), lds1, s, T);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(copra_trace_kernel<2>, dim3(1), dim3(kScoreThreads), 0, s, T);
    HIP_TRY(hipGetLastError());
    return launch_trace_quant(h, T, slot, s, who); // (copra_hip_trace_quant.hip: one launch more while quantiles are on, else nothing)
}

extern "C" {

void copra_trace_init(copra_trace_t* trace)
{
    if (!trace) return;
    std::memset(trace, 0, sizeof *trace);
    trace->struct_size = (int)sizeof *trace;
}

copra_status_t copra_batch_set_trace(copra_batch_t* h, const copra_trace_t* trace)
{
    const char* const who = "copra_batch_set_trace";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    if (!trace) { // tracing ends, the buffers go (on any controller: nothing to end is no error)
        trace_off(h);
        return COPRA_OK;
    }
    if (h->hp.plan.initial_state)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": the initial state of an InitialStateLMPC controller is a decision variable, not the plant's state");
    copra_trace_t m;
    const copra_status_t rc_m = read_sized(m, trace, who, "copra_trace_t", "copra_trace_init");
    if (rc_m != COPRA_OK) return rc_m;
    if (m.capacity < 1) return fail(COPRA_ERR_ARG, std::string(who) + ": capacity < 1");
    if ((m.what & (COPRA_TRACE_X | COPRA_TRACE_U | COPRA_TRACE_ERR)) == 0 || (m.what & ~(COPRA_TRACE_X | COPRA_TRACE_U | COPRA_TRACE_ERR)) != 0)
        return fail(COPRA_ERR_ARG, std::string(who) + ": `what` holds no COPRA_TRACE_* bit, or an unknown one");
    if (m.every < 0) return fail(COPRA_ERR_ARG, std::string(who) + ": every < 0");
    if (!(m.tol >= 0.0)) return fail(COPRA_ERR_ARG, std::string(who) + ": a negative or NaN tol");
    const FusedPlan& P = h->hp.plan;
    const size_t b = (size_t)(P.batch > 0 ? P.batch : 1), nx = (size_t)P.nx, nu = (size_t)P.nu;
    const double* arr[kTraceArrays] = { m.x_lo, m.x_hi, m.u_lo, m.u_hi };
    const size_t count[kTraceArrays] = { nx, nx, nu, nu };
    if (!m.on_device) {
        for (int k = 0; k < kTraceArrays; k += 2)
            for (size_t i = 0; arr[k] && arr[k + 1] && i < count[k]; ++i)
                if (!(arr[k][i] <= arr[k + 1][i])) return fail(COPRA_ERR_ARG, std::string(who) + ": a lower limit above its upper limit (or a NaN limit)");
        for (int k = 0; k < kTraceArrays; ++k)
            for (size_t i = 0; arr[k] && i < count[k]; ++i)
                if (std::isnan(arr[k][i])) return fail(COPRA_ERR_ARG, std::string(who) + ": a NaN limit");
    }
    const int limits = m.x_lo || m.x_hi || m.u_lo || m.u_hi;
    const int rows = trace_rows(m.what, P.nx, P.nu, limits);
    const size_t slot = trace_slot_bytes(rows);
    if ((double)m.capacity * (double)slot > 1e15) return fail(COPRA_ERR_ARG, std::string(who) + ": capacity beyond any device");
    h->trace_on = false; // (a failed attempt leaves the feature off, never a trace half replaced)
    HIP_TRY(hipStreamSynchronize(h->last_stream)); // a tick that still writes the old slots or reads the old limits first
    trace_quant_off(h); // (the quantiles of the trace this one replaces end with it: copra_batch_set_trace_quantiles)
    for (int k = 0; k < kTraceArrays; ++k) {
        if (m.on_device || !arr[k]) h->trace_lim[k].borrow(arr[k]);
        else OWN_TRY(h->trace_lim[k].copy_in(arr[k], count[k]));
    }
    OWN_TRY(h->d_trace.grow((size_t)m.capacity * slot));
    OWN_TRY(h->d_trace_part.grow((size_t)score_chunks((long long)b) * slot));
    if (!h->d_trace_u) OWN_TRY(h->d_trace_u.alloc(b * nu));
    if (!h->d_trace_age) OWN_TRY(h->d_trace_age.alloc(b));
    h->trace_what = m.what, h->trace_every = m.every > 0 ? m.every : 1, h->trace_rows = rows;
    h->trace_cap = m.capacity, h->trace_tol = m.tol;
    h->trace_in_lds = trace_in_lds(P.nx, P.nu, m.what, m.x_lo || m.x_hi, m.u_lo || m.u_hi);
    h->trace_tick = h->trace_recorded = h->trace_missed = 0;
    h->trace_on = true;
    return COPRA_OK;
}

copra_status_t copra_batch_trace_reset(copra_batch_t* h)
{
    const char* const who = "copra_batch_trace_reset";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    if (!h->trace_on) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": tracing is not on (copra_batch_set_trace)");
    h->trace_tick = h->trace_recorded = h->trace_missed = 0; // (the slot is a launch argument: the next recorded tick writes slot 0 behind everything launched so far)
    return COPRA_OK;
}

copra_status_t copra_batch_trace_info(const copra_batch_t* h, long long* recorded, long long* missed, int* rows, long long* slot_size)
{
    const char* const who = "copra_batch_trace_info";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    if (!h->trace_on) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": tracing is not on (copra_batch_set_trace)");
    if (recorded) *recorded = h->trace_recorded;
    if (missed) *missed = h->trace_missed;
    if (rows) *rows = h->trace_rows;
    if (slot_size) *slot_size = (long long)slot_bytes(h);
    return COPRA_OK;
}

const void* copra_batch_trace_device(const copra_batch_t* h) { return h && h->trace_on ? (const void*)(const unsigned char*)h->d_trace : nullptr; }

copra_status_t copra_batch_get_trace(copra_batch_t* h, long long first, long long count, void* host)
{
    const char* const who = "copra_batch_get_trace";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    if (!host) return fail(COPRA_ERR_ARG, std::string(who) + ": null destination");
    if (!h->trace_on || !h->d_trace) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": tracing is not on (copra_batch_set_trace)");
    if (first < 0 || count < 0 || first > h->trace_recorded || count > h->trace_recorded - first)
        return fail(COPRA_ERR_ARG, std::string(who) + ": first / count outside the recorded slots (copra_batch_trace_info)");
    HIP_TRY(hipStreamSynchronize(h->last_stream));
    if (count > 0) HIP_TRY(hipMemcpy(host, (const unsigned char*)h->d_trace + (size_t)first * slot_bytes(h), (size_t)count * slot_bytes(h), hipMemcpyDeviceToHost));
    return COPRA_OK;
}

} // extern "C"
