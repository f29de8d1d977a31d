// copra_hip_delay.hip -- input delay in the tick of the C ABI (include/copra_hip.h, ABI 16): copra_batch_set_input_delay takes the ring of
// pending commands, their statuses and the state at the current tick; launch_delay is the ONE helper that launches copra_delay_kernel
// (delay_step.hpp) -- stream-ordered, no synchronisation, no allocation -- and what the tick (copra_hip_plant.hip, advance()) calls behind
// its plant step with the push on, and the setter, copra_batch_set_x0, copra_batch_set_bias and the system setters with the push off;
// delay_adopt_x0 is what those that bring a new state call.  copra_batch_delay_state_device / _get_delay_state / _delay_queue_device /
// _get_delay_queue / copra_batch_input_delay hand the state out.  The kernel is compiled in this unit alone.
#include "engine.hpp"
#define COPRA_PLANT_PHASES_ONLY // (plant_step.hpp through delay_step.hpp: its helpers and geometry, not its kernels)
#define COPRA_DELAY_KERNEL
#include "delay_step.hpp"

#include <vector>

static_assert(kDelayMax == COPRA_DELAY_MAX, "the header's bound is the kernel's");

namespace {

void delay_off(copra_batch* h) // (a release waits for a tick that still uses the buffer)
{
    h->delay = 0, h->delay_head = 0;
    h->d_delay_q.reset();
    h->d_delay_qs.reset();
    h->d_delay_x.reset();
}

} // namespace

copra_status_t launch_delay(copra_batch* h, int push, const double* fallback_u, hipStream_t s, const char* who)
{
    const FusedPlan& HP = h->hp.plan;
    if (h->delay <= 0 || HP.batch <= 0) return COPRA_OK;
    if (!h->d_delay_q || !h->d_delay_qs || !h->d_delay_x || !h->own_x0) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the input delay has lost its buffers");
    DelayArgs P {};
    P.batch = HP.batch, P.nx = HP.nx, P.nu = HP.nu;
    P.D = h->delay;
    if (h->shared) { // ONE system for the batch ...
        const copra_status_t rc = shared_model_on_device(h);
        if (rc != COPRA_OK) return rc;
        P.A = h->d_shA, P.B = h->d_shB, P.d = h->d_shd;
        P.shared = 1;
    } else { // ... or every instance's own; d the estimates while the estimator or the observer's Ld is on
        if (!h->A || !h->B || !h->d) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": no preview system set (copra_batch_set_system)");
        P.A = h->A, P.B = h->B, P.d = h->d;
    }
    if (push) {
        if (!h->ad.last_status || !h->ad.last_control) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": no solve has been launched into the current result buffers");
        P.push = 1;
        P.status = h->ad.last_status, P.control = h->ad.last_control;
        P.ctrl_stride = HP.n;
        h->delay_head = (h->delay_head + 1) % h->delay; // the slot the plant step just applied takes the new command and becomes the newest
    }
    P.head = h->delay_head;
    P.xnow = h->d_delay_x;
    P.q = h->d_delay_q, P.qs = h->d_delay_qs;
    P.fallback_u = fallback_u;
    P.x0 = h->own_x0;
    P.group = delay_group(P.nx, P.nu, P.D); // (the geometry: delay_step.hpp; checked against the LDS by the setter)
    P.vec2 = delay_vec2_ok(P);
    const size_t lds_bytes = (size_t)delay_lds(P).total * sizeof(double);
    if (lds_bytes > kPlantLdsMax) return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": one instance's model and queue do not fit the LDS");
    if (lds_bytes > 48 * 1024) LDS_OPT_IN(copra_delay_kernel, lds_bytes);
    const copra_status_t behind = order_behind_last(h, s); // behind the plant step or the copy that moved xnow, d or the model
    if (behind != COPRA_OK) return behind;
    const unsigned grid = (unsigned)((P.batch + P.group - 1) / P.group);
    hipLaunchKernelGGL(copra_delay_kernel, dim3(grid), dim3(kDelayThreads), lds_bytes, s, P);
    HIP_TRY(hipGetLastError());
    h->x0 = h->own_x0; // what the next solve reads: the prediction
    h->last_stream = s;
    return COPRA_OK;
}

copra_status_t delay_adopt_x0(copra_batch* h, hipStream_t s, const char* who)
{
    const FusedPlan& HP = h->hp.plan;
    if (h->delay <= 0) return COPRA_OK;
    const size_t nd = (size_t)HP.batch * HP.nx;
    if (!h->own_x0) OWN_TRY(h->own_x0.alloc(nd ? nd : 1));
    if (!h->x0 || !h->d_delay_x) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": no initial states set");
    const copra_status_t behind = order_behind_last(h, s); // (a tick that still writes xnow)
    if (behind != COPRA_OK) return behind;
    if (nd) HIP_TRY(hipMemcpyAsync(h->d_delay_x, h->x0, nd * sizeof(double), hipMemcpyDeviceToDevice, s)); // (a caller's buffer: read this once, never written)
    h->last_stream = s;
    return launch_delay(h, 0, nullptr, s, who);
}

extern "C" {

copra_status_t copra_batch_set_input_delay(copra_batch_t* h, int steps, const double* u_init, int on_device)
{
    const char* const who = "copra_batch_set_input_delay";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    if (steps < 0 || steps > COPRA_DELAY_MAX) return fail(COPRA_ERR_ARG, std::string(who) + ": steps outside 0 .. COPRA_DELAY_MAX");
    const FusedPlan& P = h->hp.plan;
    if (P.initial_state)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": the initial state of an InitialStateLMPC controller is a decision variable, not the plant's state");
    const size_t nd = (size_t)P.batch * P.nx;
    if (steps == 0) { // off: x0 is the state at the current tick again, the buffers go
        if (h->delay > 0 && h->d_delay_x && h->own_x0 && nd) {
            HIP_TRY(hipMemcpyAsync(h->own_x0, h->d_delay_x, nd * sizeof(double), hipMemcpyDeviceToDevice, h->last_stream));
            h->x0 = h->own_x0;
        }
        delay_off(h);
        return COPRA_OK;
    }
    if (h->backup_steps > 0)
        return fail(COPRA_ERR_RUNTIME, std::string(who) + ": backup plans are on (copra_batch_set_backup_steps): the plan store reads the tail of the solve's controls");
    if (!h->shared && (!h->A || !h->B || !h->d)) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": no preview system set (copra_batch_set_system)");
    if (!h->x0) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": no initial states set");
    if ((double)P.nx * P.nx > 1e6 || delay_image_bytes(P.nx, P.nu, steps) > kPlantLdsMax)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": one instance's model and queue do not fit the LDS");
    const size_t b = (size_t)(P.batch > 0 ? P.batch : 1), nq = b * (size_t)steps * P.nu;
    const bool was_on = h->delay > 0;
    HIP_TRY(hipStreamSynchronize(h->last_stream)); // the one synchronisation: a tick that still reads the old queue
    if (steps != h->delay || !h->d_delay_q || !h->d_delay_qs) {
        h->delay = 0; // (a failed attempt leaves the feature off, never a queue of the wrong size)
        OWN_TRY(h->d_delay_q.alloc(nq));
        OWN_TRY(h->d_delay_qs.alloc(b * (size_t)steps));
    }
    if (!h->d_delay_x) OWN_TRY(h->d_delay_x.alloc(b * (size_t)P.nx));
    if (!was_on && nd) // turned on: the state at the current tick is the x0 in force (a repeated call keeps xnow: only the queue is reset)
        HIP_TRY(hipMemcpyAsync(h->d_delay_x, h->x0, nd * sizeof(double), hipMemcpyDeviceToDevice, h->last_stream));
    // every slot holds u_init (zeros without one) with status COPRA_QP_OK
    HIP_TRY(hipMemsetAsync(h->d_delay_qs, 0, b * (size_t)steps * sizeof(int), h->last_stream));
    if (!u_init) {
        HIP_TRY(hipMemsetAsync(h->d_delay_q, 0, nq * sizeof(double), h->last_stream));
    } else if (P.batch > 0 && on_device) {
        const size_t row = (size_t)P.nu * sizeof(double);
        for (int j = 0; j < steps; ++j) // slot j of every instance: rows of nu doubles, D nu apart
            HIP_TRY(hipMemcpy2DAsync((double*)h->d_delay_q + (size_t)j * P.nu, (size_t)steps * row, u_init, row, row, (size_t)P.batch, hipMemcpyDeviceToDevice, h->last_stream));
    } else if (P.batch > 0) {
        std::vector<double> rep(nq);
        for (size_t i = 0; i < (size_t)P.batch; ++i)
            for (int j = 0; j < steps; ++j) std::copy(u_init + i * P.nu, u_init + (i + 1) * P.nu, rep.begin() + (i * steps + j) * P.nu);
        HIP_TRY(hipMemcpy(h->d_delay_q, rep.data(), nq * sizeof(double), hipMemcpyHostToDevice));
    }
    if (!h->own_x0) OWN_TRY(h->own_x0.alloc(nd ? nd : 1));
    h->delay = steps, h->delay_head = 0;
    const copra_status_t rc = launch_delay(h, 0, nullptr, h->last_stream, who); // the first prediction: what the first solve reads
    if (rc != COPRA_OK) delay_off(h);
    return rc;
}

int copra_batch_input_delay(const copra_batch_t* h)
{
    return h ? h->delay : -1;
}

const double* copra_batch_delay_state_device(const copra_batch_t* h)
{
    return h && h->delay > 0 ? (const double*)h->d_delay_x : nullptr;
}

copra_status_t copra_batch_get_delay_state(copra_batch_t* h, double* x)
{
    const char* const who = "copra_batch_get_delay_state";
    if (!h || !x) return fail(COPRA_ERR_ARG, std::string(who) + ": null argument");
    if (h->delay <= 0 || !h->d_delay_x) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": input delay is not on (copra_batch_set_input_delay)");
    HIP_TRY(hipStreamSynchronize(h->last_stream));
    const size_t nd = (size_t)(h->hp.plan.batch > 0 ? h->hp.plan.batch : 0) * h->hp.plan.nx;
    if (nd) HIP_TRY(hipMemcpy(x, h->d_delay_x, nd * sizeof(double), hipMemcpyDeviceToHost));
    return COPRA_OK;
}

copra_status_t copra_batch_delay_queue_device(const copra_batch_t* h, const double** q, const int** status, int* head)
{
    const char* const who = "copra_batch_delay_queue_device";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    if (h->delay <= 0 || !h->d_delay_q || !h->d_delay_qs) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": input delay is not on (copra_batch_set_input_delay)");
    if (q) *q = h->d_delay_q;
    if (status) *status = h->d_delay_qs;
    if (head) *head = h->delay_head;
    return COPRA_OK;
}

copra_status_t copra_batch_get_delay_queue(copra_batch_t* h, double* q, int* status)
{
    const char* const who = "copra_batch_get_delay_queue";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    if (h->delay <= 0 || !h->d_delay_q || !h->d_delay_qs) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": input delay is not on (copra_batch_set_input_delay)");
    HIP_TRY(hipStreamSynchronize(h->last_stream));
    const size_t b = (size_t)(h->hp.plan.batch > 0 ? h->hp.plan.batch : 0), D = (size_t)h->delay, nu = (size_t)h->hp.plan.nu;
    if (!b) return COPRA_OK;
    std::vector<double> ring(q ? b * D * nu : 0);
    std::vector<int> rs(status ? D * b : 0);
    if (q) HIP_TRY(hipMemcpy(ring.data(), h->d_delay_q, ring.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (status) HIP_TRY(hipMemcpy(rs.data(), h->d_delay_qs, rs.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < b; ++i)
        for (size_t j = 0; j < D; ++j) { // entry j, oldest first, sits in slot (head + j) % D
            const size_t slot = ((size_t)h->delay_head + j) % D;
            if (q) std::copy(ring.begin() + (i * D + slot) * nu, ring.begin() + (i * D + slot + 1) * nu, q + (i * D + j) * nu);
            if (status) status[i * D + j] = rs[slot * b + i];
        }
    return COPRA_OK;
}

} // extern "C"
