// copra_hip_target.hip -- steady-state targets of the C ABI (include/copra_hip.h, ABI 15): copra_batch_set_target hands the controlled outputs,
// the setpoint signal and the driven costs over once and takes every buffer the feature needs; launch_target is the ONE helper that launches
// copra_target_kernel (target_step.hpp) -- stream-ordered, no synchronisation, no allocation -- and what the tick (copra_hip_plant.hip,
// advance()), copra_batch_schedule_seek, copra_batch_set_bias and the system setters call while targets are on; copra_batch_target_device /
// _target_status_device / _get_target hand the steady states out, copra_batch_get_cost_reference the per-instance reference of a cost in force
// (what the kernel, a schedule's window or copra_batch_set_cost_reference wrote).  The kernel is compiled in this unit alone.
#include "engine.hpp"
#define COPRA_PLANT_PHASES_ONLY // (plant_step.hpp through target_step.hpp: its helpers and geometry, not its kernels)
#include "target_step.hpp"

#include <cstring>

static_assert(kTargetMaxCosts == kTargetCosts, "the handle holds what one launch serves");

namespace {

void target_off(copra_batch* h) // (the buffers stay for the next time: copra_batch_target_device keeps no promise while off)
{
    h->target_on = false;
    h->target_ncost = 0;
}

} // namespace

copra_status_t launch_target(copra_batch* h, hipStream_t s, const char* who)
{
    const FusedPlan& HP = h->hp.plan;
    if (!h->target_on || HP.batch <= 0) return COPRA_OK;
    if (h->shared || !h->A || !h->B || !h->d || !h->d_target || !h->d_target_status || !h->target_H || !h->target_r)
        return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the targets have lost their model or their buffers");
    TargetArgs S {};
    S.batch = HP.batch, S.nx = HP.nx, S.nu = HP.nu;
    S.A = h->A, S.B = h->B, S.d = h->d;
    S.H = h->target_H, S.r = h->target_r;
    S.per_instance = h->target_per_instance;
    S.steps = h->target_steps;
    const long long tau = (h->sched_tick < 0 ? 0 : h->sched_tick) + h->target_offset;
    S.row = tau < S.steps - 1 ? tau : S.steps - 1;
    S.ncost = h->target_ncost;
    for (int k = 0; k < S.ncost; ++k) {
        const int t = h->target_cost[k];
        if (!h->d_cost_p[t] || !h->target_map[k]) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": a driven cost has lost its reference buffer");
        S.c[k].map = h->target_map[k];
        S.c[k].out = h->d_cost_p[t];
        S.c[k].r = h->target_rows[k];
        S.c[k].S = HP.cost[t].prows / h->target_rows[k];
    }
    S.z = h->d_target, S.status = h->d_target_status;
    const int maps = target_map_doubles(S);
    S.group = target_group(S.nx, S.nu, maps); // (the geometry: target_step.hpp; checked against the LDS by the setter)
    target_prepare(S);
    const size_t lds_bytes = (size_t)target_lds(S).total * sizeof(double);
    if (lds_bytes > kPlantLdsMax) return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": one wave's target systems do not fit the LDS");
    if (lds_bytes > 48 * 1024) LDS_OPT_IN(copra_target_kernel, lds_bytes);
    const bool other = s != h->last_stream;
    const copra_status_t behind = order_behind_last(h, s); // a solve or a tick that still reads the references or writes d: behind it ...
    if (behind != COPRA_OK) return behind;
    const unsigned grid = (unsigned)((S.batch + S.group - 1) / S.group);
    hipLaunchKernelGGL(copra_target_kernel, dim3(grid), dim3(kTargetThreads), lds_bytes, s, S);
    HIP_TRY(hipGetLastError());
    if (other) { // ... and what the handle's stream does next, behind this launch
        HIP_TRY(hipEventRecord(h->ev_plant, s));
        HIP_TRY(hipStreamWaitEvent(h->last_stream, h->ev_plant, 0));
    }
    return COPRA_OK;
}

extern "C" {

void copra_target_init(copra_target_t* target)
{
    if (!target) return;
    std::memset(target, 0, sizeof *target);
    target->struct_size = (int)sizeof *target;
}

copra_status_t copra_batch_set_target(copra_batch_t* h, const copra_target_t* target)
{
    const char* const who = "copra_batch_set_target";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    if (!target) { // the targets end; the last references stay in force (cost_p keeps pointing at them)
        target_off(h);
        return COPRA_OK;
    }
    copra_target_t m;
    const copra_status_t rc_m = read_sized(m, target, who, "copra_target_t", "copra_target_init");
    if (rc_m != COPRA_OK) return rc_m;
    if (m.steps < 1 || m.offset < 0) return fail(COPRA_ERR_ARG, std::string(who) + ": steps < 1 or offset < 0");
    if (m.n_costs < 1 || m.n_costs > kTargetMaxCosts) return fail(COPRA_ERR_ARG, std::string(who) + ": n_costs outside 1 .. 8");
    if (!m.H || !m.r || !m.cost_index || !m.cost_rows || !m.cost_map) return fail(COPRA_ERR_ARG, std::string(who) + ": a null array");
    for (int k = 0; k < m.n_costs; ++k) {
        if (!m.cost_map[k]) return fail(COPRA_ERR_ARG, std::string(who) + ": a null cost map");
        if (m.cost_index[k] < 0 || m.cost_index[k] >= (int)h->hp.cost_slot.size()) return fail(COPRA_ERR_ARG, std::string(who) + ": no such cost");
        for (int q = 0; q < k; ++q)
            if (m.cost_index[q] == m.cost_index[k]) return fail(COPRA_ERR_ARG, std::string(who) + ": a cost is driven twice");
    }
    const FusedPlan& P = h->hp.plan;
    if (P.initial_state)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": the initial state of an InitialStateLMPC controller is a decision variable, not the plant's state");
    if (m.nr != P.nu) return fail(COPRA_ERR_DOMAIN, std::string(who) + ": nr must equal uDim (a square target problem)");
    int slot[kTargetMaxCosts];
    for (int k = 0; k < m.n_costs; ++k) {
        const int t = h->hp.cost_slot[(size_t)m.cost_index[k]]; // (dense costs are not among the kernel-evaluated terms)
        if (t < 0) return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": a dense (host-evaluated) cost has no reference p");
        const CostTerm& ct = P.cost[t];
        if (ct.full) return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": a full-size cost the controller does not evaluate step by step has no step form");
        const int r = m.cost_rows[k];
        if (r < 1 || ct.prows % r != 0) return fail(COPRA_ERR_DOMAIN, std::string(who) + ": cost_rows does not divide the rows of the cost");
        if (ct.pstride && r != ct.pstride)
            return fail(COPRA_ERR_DOMAIN, std::string(who) + ": the controller evaluates this full-size cost step by step: cost_rows must be the rows of one step");
        slot[k] = t;
    }
    if (h->shared || h->shared_as_batch)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": one model for the batch (copra_batch_set_shared_system) has one d; write the model out with copra_batch_set_system");
    if (!h->A || !h->B || !h->d) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": no preview system set (copra_batch_set_system)");
    for (int k = 0; k < m.n_costs; ++k)
        if (h->ref_sched[slot[k]].sched)
            return fail(COPRA_ERR_RUNTIME, std::string(who) + ": a driven cost follows a reference schedule (copra_batch_set_reference_schedule): end it first");
    const int n = P.nx + P.nu;
    double map_total = 0.0;
    for (int k = 0; k < m.n_costs; ++k) map_total += (double)plant_even(m.cost_rows[k] * n);
    if ((double)n * (n + 1) > 1e5 || map_total > 1e6 || target_image_bytes(P.nx, P.nu, (int)map_total) > kPlantLdsMax)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": one wave's target systems do not fit the LDS (xDim + uDim beyond about 16)");
    const size_t b = (size_t)(P.batch > 0 ? P.batch : 1), lead = m.per_instance ? b : 1;
    const size_t nH = (size_t)P.nu * P.nx, nr = lead * (size_t)m.steps * P.nu;
    target_off(h); // (a failed attempt leaves the feature off, never a setpoint half replaced)
    HIP_TRY(hipStreamSynchronize(h->last_stream)); // the one synchronisation: a launch that still reads the old copies, a solve that reads the references
    if (m.on_device) {
        h->target_H.borrow(m.H), h->target_r.borrow(m.r);
        for (int k = 0; k < m.n_costs; ++k) h->target_map[k].borrow(m.cost_map[k]);
    } else { // the library's copies
        OWN_TRY(h->target_H.copy_in(m.H, nH));
        OWN_TRY(h->target_r.copy_in(m.r, nr));
        for (int k = 0; k < m.n_costs; ++k) OWN_TRY(h->target_map[k].copy_in(m.cost_map[k], (size_t)m.cost_rows[k] * n));
    }
    if (!h->d_target) {
        OWN_TRY(h->d_target.alloc(b * (size_t)n));
        HIP_TRY(hipMemsetAsync(h->d_target, 0, b * (size_t)n * sizeof(double), h->last_stream)); // (what a singular instance shows before its first good target)
    }
    if (!h->d_target_status) {
        OWN_TRY(h->d_target_status.alloc(b));
        HIP_TRY(hipMemsetAsync(h->d_target_status, 0, b * sizeof(int), h->last_stream));
    }
    // the driven costs go into per-instance-reference mode, as copra_batch_set_cost_reference_all puts them there: every instance starts from
    // the reference in force -- what a singular instance keeps
    for (int k = 0; k < m.n_costs; ++k) {
        const int t = slot[k];
        const size_t rows = (size_t)P.cost[t].prows;
        if (!h->d_cost_p[t]) OWN_TRY(h->d_cost_p[t].alloc(b * rows));
        if (h->cost_p[t] == h->d_cost_p[t]) continue;
        if (h->cost_p[t]) { // a caller's device references
            HIP_TRY(hipMemcpyAsync(h->d_cost_p[t], h->cost_p[t], b * rows * sizeof(double), hipMemcpyDeviceToDevice, h->last_stream));
        } else { // the controller-wide reference given at creation
            std::vector<double> rep(b * rows);
            const double* const p0 = h->hp.params.data() + P.cost[t].offP;
            for (size_t i = 0; i < b; ++i) std::copy(p0, p0 + rows, rep.begin() + i * rows);
            HIP_TRY(hipMemcpy(h->d_cost_p[t], rep.data(), rep.size() * sizeof(double), hipMemcpyHostToDevice));
            h->model_dirty = true; // shared model: c0 / C2 change
        }
        h->cost_p[t] = h->d_cost_p[t];
    }
    h->target_steps = m.steps, h->target_offset = m.offset, h->target_per_instance = m.per_instance != 0;
    h->target_ncost = m.n_costs;
    for (int k = 0; k < m.n_costs; ++k) h->target_cost[k] = slot[k], h->target_rows[k] = m.cost_rows[k];
    h->target_on = true;
    const copra_status_t rc = launch_target(h, h->last_stream, who); // so that the first solve is right
    if (rc != COPRA_OK) target_off(h);
    return rc;
}

const double* copra_batch_target_device(const copra_batch_t* h)
{
    return h && h->target_on ? (const double*)h->d_target : nullptr;
}

const int* copra_batch_target_status_device(const copra_batch_t* h)
{
    return h && h->target_on ? (const int*)h->d_target_status : nullptr;
}

copra_status_t copra_batch_get_target(copra_batch_t* h, double* z, int* status)
{
    const char* const who = "copra_batch_get_target";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    if (!h->target_on || !h->d_target || !h->d_target_status) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": targets are not on (copra_batch_set_target)");
    HIP_TRY(hipStreamSynchronize(h->last_stream));
    const size_t b = (size_t)(h->hp.plan.batch > 0 ? h->hp.plan.batch : 0), n = (size_t)(h->hp.plan.nx + h->hp.plan.nu);
    if (z && b) HIP_TRY(hipMemcpy(z, h->d_target, b * n * sizeof(double), hipMemcpyDeviceToHost));
    if (status && b) HIP_TRY(hipMemcpy(status, h->d_target_status, b * sizeof(int), hipMemcpyDeviceToHost));
    return COPRA_OK;
}

copra_status_t copra_batch_get_cost_reference(copra_batch_t* h, int cost_index, double* p)
{
    const char* const who = "copra_batch_get_cost_reference";
    if (!h || !p) return fail(COPRA_ERR_ARG, std::string(who) + ": null argument");
    if (cost_index < 0 || cost_index >= (int)h->hp.cost_slot.size()) return fail(COPRA_ERR_ARG, std::string(who) + ": no such cost");
    const int t = h->hp.cost_slot[(size_t)cost_index];
    if (t < 0) return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": a dense (host-evaluated) cost has no reference p");
    if (!h->cost_p[t]) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the cost has no per-instance reference (the controller-wide one given at creation is in force)");
    HIP_TRY(hipStreamSynchronize(h->last_stream));
    const size_t count = (size_t)(h->hp.plan.batch > 0 ? h->hp.plan.batch : 0) * h->hp.plan.cost[t].prows;
    if (count) HIP_TRY(hipMemcpy(p, h->cost_p[t], count * sizeof(double), hipMemcpyDeviceToHost));
    return COPRA_OK;
}

} // extern "C"
