// copra_hip_trace_quant.hip -- trace quantiles of the C ABI (include/copra_hip.h, ABI 18): copra_batch_set_trace_quantiles takes the quantile
// buffer [capacity][rows][count] beside the trace's slots and the key buffer the kernel works in; launch_trace_quant is what launch_trace
// (copra_hip_trace.hip) calls behind its two launches on a recorded tick while quantiles are on -- one launch of copra_trace_quant_kernel on the
// tick's stream into the slot the host counted, no synchronisation, no allocation, no counter on the device; copra_batch_trace_quantile_info /
// _trace_quantiles_device / _get_trace_quantiles read the levels and the buffer.  The rule and the selection: trace_quant_step.hpp.
#include "engine.hpp"
#define COPRA_PLANT_PHASES_ONLY // (plant_step.hpp, score_step.hpp and trace_step.hpp through trace_quant_step.hpp: their helpers, not their kernels)
#define COPRA_SCORE_HELPERS_ONLY
#define COPRA_TRACE_HELPERS_ONLY
#include "trace_quant_step.hpp"

#include <cmath>
#include <cstring>

static_assert(COPRA_TRACE_QUANT_MAX == kQuantMax, "the level count of the header is the kernel's");

namespace {

size_t per_slot(const copra_batch* h) { return (size_t)h->trace_rows * (size_t)h->quant_count; } // doubles

} // namespace

void trace_quant_off(copra_batch* h) // (a release waits for a tick that still uses the buffers)
{
    h->quant_on = false;
    h->quant_count = 0;
    h->d_quant.reset();
    h->d_quant_keys.reset();
}

copra_status_t launch_trace_quant(copra_batch* h, const TraceArgs& T, long long slot, hipStream_t s, const char* who)
{
    if (!h->quant_on) return COPRA_OK;
    const int rows = trace_rows(T);
    if (!h->d_quant || !h->d_quant_keys || rows != h->trace_rows || slot < 0 || slot >= h->trace_cap)
        return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the trace quantiles have lost their buffers");
    QuantArgs Q {};
    Q.T = T;
    Q.T.in_lds = 0, Q.T.vec2 = 0; // (the values are read where they lie)
    Q.nq = h->quant_count;
    for (int q = 0; q < kQuantMax; ++q) Q.level[q] = q < Q.nq ? h->quant_level[q] : 0.0;
    Q.keys = h->d_quant_keys;
    Q.out = (double*)h->d_quant + (size_t)slot * per_slot(h);
    hipLaunchKernelGGL(copra_trace_quant_kernel, dim3((unsigned)rows), dim3(kQuantThreads), 0, s, Q);
    HIP_TRY(hipGetLastError());
    return COPRA_OK;
}

extern "C" {

copra_status_t copra_batch_set_trace_quantiles(copra_batch_t* h, const double* levels, int count)
{
    const char* const who = "copra_batch_set_trace_quantiles";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    if (count < 0 || count > COPRA_TRACE_QUANT_MAX) return fail(COPRA_ERR_ARG, std::string(who) + ": count outside 0 .. COPRA_TRACE_QUANT_MAX");
    for (int q = 0; levels && q < count; ++q)
        if (!(levels[q] >= 0.0 && levels[q] <= 1.0)) return fail(COPRA_ERR_ARG, std::string(who) + ": a level that is NaN or outside [0, 1]");
    if (!h->trace_on) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": tracing is not on (copra_batch_set_trace)");
    if (!levels || count == 0) { // quantiles end; the trace and its slots stay
        HIP_TRY(hipStreamSynchronize(h->last_stream));
        trace_quant_off(h);
        return COPRA_OK;
    }
    const size_t b = (size_t)(h->hp.plan.batch > 0 ? h->hp.plan.batch : 1), rows = (size_t)h->trace_rows;
    if ((double)h->trace_cap * (double)rows * (double)count * 8.0 > 1e15) return fail(COPRA_ERR_ARG, std::string(who) + ": capacity beyond any device");
    h->quant_on = false; // (a failed attempt leaves quantiles off)
    HIP_TRY(hipStreamSynchronize(h->last_stream)); // a tick that still writes the old buffer first
    OWN_TRY(h->d_quant.alloc((size_t)h->trace_cap * rows * (size_t)count));
    OWN_TRY(h->d_quant_keys.grow(rows * b));
    h->quant_count = count;
    for (int q = 0; q < count; ++q) h->quant_level[q] = levels[q];
    h->trace_tick = h->trace_recorded = h->trace_missed = 0; // the trace restarts: every recorded slot has its quantiles
    h->quant_on = true;
    return COPRA_OK;
}

copra_status_t copra_batch_trace_quantile_info(const copra_batch_t* h, int* count, double* levels)
{
    const char* const who = "copra_batch_trace_quantile_info";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    if (!h->trace_on || !h->quant_on) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": trace quantiles are not on (copra_batch_set_trace_quantiles)");
    if (count) *count = h->quant_count;
    for (int q = 0; levels && q < COPRA_TRACE_QUANT_MAX; ++q) levels[q] = q < h->quant_count ? h->quant_level[q] : 0.0;
    return COPRA_OK;
}

const double* copra_batch_trace_quantiles_device(const copra_batch_t* h) { return h && h->trace_on && h->quant_on ? (const double*)h->d_quant : nullptr; }

copra_status_t copra_batch_get_trace_quantiles(copra_batch_t* h, long long first, long long count, double* host)
{
    const char* const who = "copra_batch_get_trace_quantiles";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    if (!host) return fail(COPRA_ERR_ARG, std::string(who) + ": null destination");
    if (!h->trace_on || !h->quant_on || !h->d_quant) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": trace quantiles are not on (copra_batch_set_trace_quantiles)");
    if (first < 0 || count < 0 || first > h->trace_recorded || count > h->trace_recorded - first)
        return fail(COPRA_ERR_ARG, std::string(who) + ": first / count outside the recorded slots (copra_batch_trace_info)");
    HIP_TRY(hipStreamSynchronize(h->last_stream));
    if (count > 0) HIP_TRY(hipMemcpy(host, (const double*)h->d_quant + (size_t)first * per_slot(h), (size_t)count * per_slot(h) * sizeof(double), hipMemcpyDeviceToHost));
    return COPRA_OK;
}

} // extern "C"
