// copra_hip_plant.hip -- the receding-horizon tick of the C ABI (include/copra_hip.h): copra_batch_advance applies the first control of the
// last solve to a plant and makes the result the controller's next initial state (kernel: plant_step.hpp), copra_batch_rollout enqueues
// `ticks` x (solve, advance) on one stream, copra_batch_x0_device / copra_batch_get_x0 hand the current state out.  A cost whose reference
// follows a schedule (copra_batch_set_reference_schedule) gets the window of the new tick behind every plant step (kernel: ref_window.hpp),
// and so does a limit that follows one (copra_batch_set_constraint_schedule, copra_batch_set_control_bound_schedule; kernel: limit_window.hpp).
// copra_batch_set_backup_steps: an instance without a fresh solution plays the tail of its last plan (the store: d_plan, d_plan_next).
// copra_batch_set_bias_estimator / _set_bias / _bias_device / _get_bias: the disturbance estimator -- the plant step moves every instance's d
// (d_bias, the controller's d while the estimates are in force) by a gain times the model's prediction error, in the same launch.
// copra_batch_set_observer / _set_plant_state / _plant_state_device / _get_plant_state: output feedback -- the plant keeps a state of its own
// (d_xp), the controller's x0 is the estimate, which the same launch corrects with the innovation of ny measured outputs.
// copra_batch_set_noise / _noise_seek / _noise_tick / _draw_noise: Monte-Carlo ticks -- phase 1 of the plant step draws process and sensor
// noise from a counter-based generator (plant_noise.hpp) at the handle's noise tick; builds of the kernels of their own, no memory.
// copra_batch_set_score (copra_hip_score.hip): while scoring is on, advance() hands the tick's state, control and age to launch_score.
// copra_batch_set_trace (copra_hip_trace.hip): while tracing is on, advance() hands the same, and the estimate, to launch_trace behind it.
// copra_batch_set_target (copra_hip_target.hip): while targets are on, advance(), copra_batch_schedule_seek and copra_batch_set_bias call
// launch_target behind what they did -- the steady states and the driven costs' references follow d and the setpoint.
#include "engine.hpp"
#include "limit_window.hpp"
#include "plant_step.hpp"
#include "ref_window.hpp"

#include <cstddef>
#include <cstring>

// the shared model of copra_batch_set_shared_system on the device (the solve keeps it on the host and in its prepared model)
copra_status_t shared_model_on_device(copra_batch* h)
{
    if (h->d_shA && !h->sh_dev_stale) return COPRA_OK;
    const size_t nA = h->shA.size(), nB = h->shB.size(), nd = h->shd.size();
    if (!h->d_shA) {
        OWN_TRY(h->d_shA.alloc(nA));
        OWN_TRY(h->d_shB.alloc(nB));
        OWN_TRY(h->d_shd.alloc(nd));
    }
    HIP_TRY(hipStreamSynchronize(h->last_stream)); // (an advance that still reads the old model: once per model)
    HIP_TRY(hipMemcpy(h->d_shA, h->shA.data(), nA * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_shB, h->shB.data(), nB * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_shd, h->shd.data(), nd * sizeof(double), hipMemcpyHostToDevice));
    h->sh_dev_stale = false;
    return COPRA_OK;
}

namespace {

// the caller's struct as THIS library knows it -- the widest form, copra_plant_step_obs_t, whose first bytes are the struct a caller of ABI 10
// (copra_plant_step_t) or ABI 11 (copra_plant_step_ex_t) passes: fields beyond the caller's struct_size keep their defaults (all zero)
copra_status_t read_step(const copra_plant_step_t* step, copra_plant_step_obs_t& wide, const char* who)
{
    const copra_status_t rc = read_sized(wide, step, who, "copra_plant_step_t", "copra_plant_step_init");
    if (rc != COPRA_OK) return rc;
    copra_plant_step_ex_t& out = wide.ex;
    out.step.struct_size = (int)sizeof wide;
    const int given = (out.step.A != nullptr) + (out.step.B != nullptr) + (out.step.d != nullptr);
    if (given != 0 && given != 3) return fail(COPRA_ERR_ARG, std::string(who) + ": a plant needs all of A, B and d (or none of them: the controller's model)");
    return COPRA_OK;
}
static_assert(offsetof(copra_plant_step_ex_t, d_out) == sizeof(copra_plant_step_t), "copra_plant_step_ex_t is copra_plant_step_t grown at its end");
static_assert(offsetof(copra_plant_step_obs_t, v) == sizeof(copra_plant_step_ex_t), "copra_plant_step_obs_t is copra_plant_step_ex_t grown at its end");

// what can be said before any solve: the handle takes part in closed-loop ticks at all
copra_status_t check_handle(const copra_batch* h, const char* who)
{
    if (h->hp.plan.initial_state)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": the initial state of an InitialStateLMPC controller is a decision variable, not the plant's state");
    return COPRA_OK;
}

// the windows of every scheduled cost at the controller's tick counter, one launch on `s`: no synchronisation, no allocation
copra_status_t write_ref_windows(copra_batch* h, hipStream_t s, const char* who)
{
    RefWindowArgs W {};
    W.batch = h->hp.plan.batch;
    W.group = kRefWindowGroup;
    for (int t = 0; t < kMaxCosts; ++t) {
        const RefSchedule& rs = h->ref_sched[t];
        if (!rs.sched) continue;
        if (W.ncost == kRefWindowMax) return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": more scheduled costs than one launch serves");
        RefWindowCost& c = W.c[W.ncost++];
        c.sched = rs.sched;
        c.out = h->d_cost_p[t];
        c.steps = rs.steps;
        c.first = h->sched_tick + rs.offset;
        c.r = rs.r, c.S = rs.S;
        c.per_instance = rs.per_instance;
    }
    if (W.ncost == 0 || W.batch <= 0) return COPRA_OK;
    ref_window_prepare(W, kRefWindowThreads);
    const unsigned grid = (unsigned)((W.batch + W.group - 1) / W.group);
    hipLaunchKernelGGL(copra_ref_window_kernel, dim3(grid), dim3(kRefWindowThreads), 0, s, W);
    HIP_TRY(hipGetLastError());
    return COPRA_OK;
}

// ... and the windows of every live limit schedule, one launch of its own on `s` -- made only where a limit schedule is live
copra_status_t write_limit_windows(copra_batch* h, hipStream_t s, const char* who)
{
    const FusedPlan& HP = h->hp.plan;
    if (live_limit_windows(h) == 0 || HP.batch <= 0) return COPRA_OK;
    LimitWindowArgs W {};
    W.batch = HP.batch;
    W.group = kLimitWindowGroup;
    auto add = [&](const LimitSchedule& ls, double* out, int stride) {
        if (!ls.sched) return true;
        if (W.nwin == kLimitWindowMax || !out) return false;
        LimitWindow& c = W.w[W.nwin++];
        c.sched = ls.sched;
        c.out = out;
        c.steps = ls.steps;
        c.first = h->sched_tick + ls.offset;
        c.stride = stride, c.row0 = ls.row0;
        c.r = ls.r, c.S = ls.S;
        c.per_instance = ls.per_instance, c.preview = ls.preview;
        return true;
    };
    bool ok = add(h->lb_sched, h->d_lb_inst, HP.n) && add(h->ub_sched, h->d_ub_inst, HP.n);
    for (const auto& kv : h->cstr_sched) ok = ok && add(kv.second, h->d_row_f_inst, HP.mgen);
    if (!ok) return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": more live limit windows than one launch serves");
    limit_window_prepare(W, kLimitWindowThreads);
    const unsigned grid = (unsigned)((W.batch + W.group - 1) / W.group);
    hipLaunchKernelGGL(copra_limit_window_kernel, dim3(grid), dim3(kLimitWindowThreads), 0, s, W);
    HIP_TRY(hipGetLastError());
    return COPRA_OK;
}

copra_status_t write_windows(copra_batch* h, hipStream_t s, const char* who)
{
    const copra_status_t rc = write_ref_windows(h, s, who);
    return rc != COPRA_OK ? rc : write_limit_windows(h, s, who);
}

// what one tick reads and writes beside the step's plant: the step's own pointers, or a rollout's rows of tick t
struct TickIO {
    const double* w;
    double *x_out, *u_out;
    int *status_out, *age_out;
    double* d_out;
    const double *v, *y_meas; // (the observer's, as the three below)
    double *y_out, *xhat_out;
};

// the tick with the observer on: P is the tick as filled in by advance() -- its plant, controls, plans and copies
copra_status_t launch_observer(copra_batch* h, const PlantStepArgs& P, const copra_plant_step_t& st, const TickIO& io, hipStream_t s, const char* who)
{
    const FusedPlan& HP = h->hp.plan;
    if (h->shared || !h->A || !h->B || !h->d || !h->d_xp || (h->obs_Ld && h->d != h->d_bias))
        return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the observer has lost its model");
    PlantObsArgs Q {};
    Q.s = P;
    Q.ny = h->obs_ny;
    Q.meas = io.y_meas != nullptr;
    Q.same_model = Q.meas || st.A == nullptr;
    Q.gain_shared = !h->obs_per_instance;
    Q.Am = h->A, Q.Bm = h->B;
    Q.dhat = h->d;
    Q.dhat_next = h->obs_Ld ? (double*)h->d_bias : nullptr;
    Q.xhat = h->x0; // (a caller's device buffer is read this once more, never written)
    Q.xhat_next = h->own_x0;
    if (h->delay > 0) Q.xhat = h->d_delay_x, Q.xhat_next = h->d_delay_x; // input delay: the estimate is xnow, x0 the prediction from it
    Q.C = h->obs_C, Q.Lx = h->obs_Lx, Q.Ld = h->obs_Ld;
    Q.yv = Q.meas ? io.y_meas : io.v;
    if (!Q.meas && h->noise_sv && h->noise_ny == Q.ny) Q.sigma_v = h->noise_sv;
    Q.y_out = io.y_out, Q.xhat_out = io.xhat_out, Q.d_out = io.d_out;
    if (Q.same_model) Q.s.A = h->A, Q.s.B = h->B, Q.s.d = h->d, Q.s.shared = 0;
    if (Q.meas) { // a real plant: the state of the tick's image is the estimate, nothing of the simulated plant is looked at
        Q.s.x0 = Q.xhat, Q.s.x0_next = nullptr, Q.s.x_out = nullptr, Q.s.w = nullptr, Q.s.sigma_w = nullptr;
    } else {
        Q.s.x0 = h->d_xp, Q.s.x0_next = h->d_xp;
    }
    const size_t one = observer_image_bytes(HP.nx, HP.nu, Q.ny);
    if (one > kPlantLdsMax) return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": one instance's model, plant and observer do not fit the LDS");
    const int group = plant_group(one);
    Q.s.group = group;
    Q.s.vec2 = plant_obs_vec2_ok(Q);
    const size_t lds_bytes = (size_t)plant_obs_lds(HP.nx, HP.nu, Q.ny, group, Q.s.shared, plant_has_w(Q.s), Q.s.backup_steps > 0, Q.same_model, Q.meas,
                                 Q.Ld != nullptr, Q.gain_shared, plant_obs_has_yv(Q)).total * sizeof(double);
    void (*const kernel)(const PlantObsArgs) = Q.s.sigma_w || Q.sigma_v ? copra_plant_observer_noise_kernel : copra_plant_observer_kernel;
    if (lds_bytes > 48 * 1024) LDS_OPT_IN(kernel, lds_bytes);
    const unsigned grid = (unsigned)((HP.batch + group - 1) / group);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kPlantThreads), lds_bytes, s, Q);
    HIP_TRY(hipGetLastError());
    return COPRA_OK;
}

// one plant step behind the last launched solve; `st` has been through read_step
copra_status_t advance(copra_batch* h, const copra_plant_step_t& st, const TickIO& io, hipStream_t s, const char* who)
{
    const double* const w = io.w;
    double *const x_out = io.x_out, *const u_out = io.u_out, *const d_out = io.d_out;
    int *const status_out = io.status_out, *const age_out = io.age_out;
    const FusedPlan& HP = h->hp.plan;
    if (!h->ad.solved_once) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": no solve has been launched (copra_batch_solve)");
    if (HP.batch == 0) return COPRA_OK;
    if (!h->ad.last_status || !h->ad.last_control)
        return fail(COPRA_ERR_RUNTIME, std::string(who) + ": no solve has been launched into the current result buffers (copra_batch_set_outputs, then copra_batch_solve)");
    if (!h->x0) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": no initial states set");
    PlantStepArgs P {};
    P.batch = HP.batch;
    P.nx = HP.nx;
    P.nu = HP.nu;
    P.ctrl_stride = HP.n;
    if (st.A) {
        P.A = st.A, P.B = st.B, P.d = st.d;
        P.shared = st.shared != 0;
    } else if (h->shared) { // the model the last solve read: ONE system ...
        const copra_status_t rc = shared_model_on_device(h);
        if (rc != COPRA_OK) return rc;
        P.A = h->d_shA, P.B = h->d_shB, P.d = h->d_shd;
        P.shared = 1;
    } else { // ... or every instance's own (a shared model written out per instance included)
        if (!h->A || !h->B || !h->d) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": no preview system set (copra_batch_set_system)");
        P.A = h->A, P.B = h->B, P.d = h->d;
    }
    const size_t nd = (size_t)HP.batch * HP.nx;
    if (!h->own_x0) OWN_TRY(h->own_x0.alloc(nd));
    P.x0 = h->x0; // (a caller's device buffer is read this once more, never written)
    P.x0_next = h->own_x0;
    P.w = w;
    if (h->noise_sw || h->noise_sv) { // drawn in phase 1, at the handle's noise tick
        P.sigma_w = h->noise_sw;
        P.sigma_per_instance = h->noise_per_instance;
        P.noise = NoiseGen { h->noise_seed, h->noise_first, h->noise_tick };
    }
    P.fallback_u = st.fallback_u;
    P.status = h->ad.last_status;
    P.control = h->ad.last_control;
    if (h->delay > 0) { // input delay: the command that reaches the plant is the ring's oldest, the state xnow (x0 is the prediction)
        if (!h->d_delay_q || !h->d_delay_qs || !h->d_delay_x) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the input delay has lost its buffers");
        P.control = (const double*)h->d_delay_q + (size_t)h->delay_head * P.nu;
        P.ctrl_stride = h->delay * P.nu;
        P.status = (const int*)h->d_delay_qs + (size_t)h->delay_head * P.batch;
        P.x0 = h->d_delay_x, P.x0_next = h->d_delay_x;
    }
    P.x_out = x_out;
    P.u_out = u_out;
    P.status_out = status_out;
    P.age_out = age_out;
    if (h->score_on) { // the score reads this tick's u_out / age_out: where the caller asked for none, the buffers copra_batch_set_score took
        if (!P.u_out) P.u_out = h->d_score_u;
        if (!P.age_out) P.age_out = h->d_score_age;
    }
    if (h->trace_on) { // ... and the trace likewise, with the buffers copra_batch_set_trace took
        if (!P.u_out) P.u_out = h->d_trace_u;
        if (!P.age_out) P.age_out = h->d_trace_age;
    }
    if (h->backup_steps > 0) {
        P.backup_steps = h->backup_steps;
        P.fresh = h->plan_fresh;
        P.plan = h->d_plan;
        P.next = h->d_plan_next;
    }
    if (h->bias_on) { // the disturbance estimator: the model beside the plant, the estimates (the controller's d) updated in place
        if (h->shared || !h->A || !h->B || h->d != h->d_bias) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the disturbance estimator has lost its model");
        P.est = 1;
        P.same_model = st.A == nullptr; // (P.A, P.B, P.d are h->A, h->B and the estimates then)
        P.Am = h->A, P.Bm = h->B;
        P.dhat = h->d_bias;
        P.gain = h->bias_gain;
        P.gain_dense = h->bias_dense, P.gain_shared = !h->bias_per_instance;
        P.d_out = d_out;
    }
    const size_t one = P.est ? bias_image_bytes(P.nx, P.nu, P.gain_dense) : plant_image_bytes(P.nx, P.nu); // (the geometry: plant_step.hpp)
    if (one > kPlantLdsMax) return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": one instance's plant does not fit the LDS (xDim beyond about 130)");
    const int group = plant_group(one);
    P.group = group;
    P.vec2 = plant_vec2_ok(P);
    const size_t lds_doubles = P.est ? (size_t)plant_est_lds(P.nx, P.nu, group, P.shared, plant_has_w(P), P.backup_steps > 0, P.same_model, P.gain_dense, P.gain_shared).total
                                     : (size_t)plant_lds(P.nx, P.nu, group, P.shared, plant_has_w(P), P.backup_steps > 0).total;
    const size_t lds_bytes = lds_doubles * sizeof(double);
    void (*const kernel)(const PlantStepArgs) = P.sigma_w ? (P.est ? copra_plant_step_kernel<true, true> : copra_plant_step_kernel<false, true>)
                                                          : (P.est ? copra_plant_step_kernel<true> : copra_plant_step_kernel<false>);
    if (lds_bytes > 48 * 1024 && !h->obs_on) LDS_OPT_IN(kernel, lds_bytes);
    const copra_status_t behind = order_behind_last(h, s); // behind the solve, whichever stream that was launched on
    if (behind != COPRA_OK) return behind;
    if (h->obs_on) { // the observer: its own build of the kernel, with a group and an image of its own
        const copra_status_t rc = launch_observer(h, P, st, io, s, who);
        if (rc != COPRA_OK) return rc;
    } else {
        const unsigned grid = (unsigned)((HP.batch + group - 1) / group);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kPlantThreads), lds_bytes, s, P);
        HIP_TRY(hipGetLastError());
    }
    h->x0 = h->own_x0;
    h->plan_fresh = false;
    h->last_stream = s; // (copra_batch_synchronize and the read-outs wait for the tick, not only for its solve)
    if (h->delay > 0) { // the last solve's command into the slot just applied, and the prediction into x0: behind the plant step
        const copra_status_t rc = launch_delay(h, 1, st.fallback_u, s, who);
        if (rc != COPRA_OK) return rc;
    }
    h->noise_tick += 1; // (counted whether noise is drawn or not: a seek or a new copra_batch_set_noise says where the draws stand)
    h->sched_tick += 1; // time moves on for every instance, a failed one included: the next solve reads the next window
    if (h->score_on) { // the records, against the true state: the plant's own while the observer simulates one, else the new x0 (the estimate
        const double* const now = h->delay > 0 ? (const double*)h->d_delay_x : h->x0; // (input delay: x0 is the prediction, the state is xnow)
        const double* const truth = h->obs_on && !io.y_meas ? (const double*)h->d_xp : now; // on a y_meas tick, where no truth exists)
        const copra_status_t rc = launch_score(h, truth, P.u_out, P.age_out, s, who);
        if (rc != COPRA_OK) return rc;
    }
    if (h->trace_on) { // the fleet's statistics of this tick, from the same true state; the estimate beside it where the observer simulates a plant
        const double* const now = h->delay > 0 ? (const double*)h->d_delay_x : h->x0;
        const bool simulated = h->obs_on && !io.y_meas;
        const copra_status_t rc = launch_trace(h, simulated ? (const double*)h->d_xp : now, simulated ? now : nullptr, P.u_out, P.age_out, s, who);
        if (rc != COPRA_OK) return rc;
    }
    const copra_status_t rc = write_windows(h, s, who);
    return rc != COPRA_OK ? rc : launch_target(h, s, who); // (behind the plant step, which moved d, at the new tick's block of the setpoint)
}

} // namespace

extern "C" {

void copra_plant_step_init(copra_plant_step_t* step)
{
    if (!step) return;
    std::memset(step, 0, sizeof *step);
    step->struct_size = (int)sizeof *step;
}

void copra_plant_step_ex_init(copra_plant_step_ex_t* step)
{
    if (!step) return;
    std::memset(step, 0, sizeof *step);
    step->step.struct_size = (int)sizeof *step;
}

void copra_plant_step_obs_init(copra_plant_step_obs_t* step)
{
    if (!step) return;
    std::memset(step, 0, sizeof *step);
    step->ex.step.struct_size = (int)sizeof *step;
}

copra_status_t copra_batch_advance(copra_batch_t* h, const copra_plant_step_t* step, void* hip_stream)
{
    if (!h) return fail(COPRA_ERR_ARG, "copra_batch_advance: null handle");
    copra_plant_step_obs_t obs;
    copra_status_t rc = read_step(step, obs, "copra_batch_advance");
    const copra_plant_step_t& st = obs.ex.step;
    if (rc == COPRA_OK) rc = check_handle(h, "copra_batch_advance");
    if (rc != COPRA_OK) return rc;
    const TickIO io { st.w, st.x_out, st.u_out, st.status_out, st.age_out, obs.ex.d_out, obs.v, obs.y_meas, obs.y_out, obs.xhat_out };
    return advance(h, st, io, (hipStream_t)hip_stream, "copra_batch_advance");
}

copra_status_t copra_batch_rollout(copra_batch_t* h, const copra_plant_step_t* step, int ticks, const double* w_seq, double* x_hist, double* u_hist,
    int* status_hist, void* hip_stream)
{
    if (!h) return fail(COPRA_ERR_ARG, "copra_batch_rollout: null handle");
    if (ticks < 0) return fail(COPRA_ERR_ARG, "copra_batch_rollout: negative number of ticks");
    copra_plant_step_obs_t obs;
    copra_status_t rc = read_step(step, obs, "copra_batch_rollout");
    const copra_plant_step_ex_t& ex = obs.ex;
    const copra_plant_step_t& st = ex.step;
    if (rc == COPRA_OK) rc = check_handle(h, "copra_batch_rollout");
    if (rc != COPRA_OK) return rc;
    if (obs.y_meas) return fail(COPRA_ERR_ARG, "copra_batch_rollout: y_meas is the measurement of a real plant, one tick at a time (copra_batch_advance)");
    const int every = st.solve_every;
    if (every < 0) return fail(COPRA_ERR_ARG, "copra_batch_rollout: negative solve_every");
    if (every > 1 && h->delay > 0)
        return fail(COPRA_ERR_RUNTIME, "copra_batch_rollout: solve_every > 1 with input delay on (copra_batch_set_input_delay): the ticks in between play the plan store");
    if (every > 1 && h->backup_steps < every - 1)
        return fail(COPRA_ERR_ARG, "copra_batch_rollout: solve_every = k needs backup plans of at least k - 1 steps (copra_batch_set_backup_steps)");
    hipStream_t s = (hipStream_t)hip_stream;
    const FusedPlan& HP = h->hp.plan;
    const size_t nd = (size_t)HP.batch * HP.nx, nc = (size_t)HP.batch * HP.nu, nb = (size_t)HP.batch;
    const size_t ny = h->obs_on ? (size_t)HP.batch * h->obs_ny : 0;
    if (x_hist && nd) { // the state the first solve reads -- with the observer on the plant's own state: the truth
        if (!h->x0) return fail(COPRA_ERR_RUNTIME, "copra_batch_rollout: no initial states set");
        const double* const now = h->delay > 0 ? (const double*)h->d_delay_x : h->x0; // (input delay: x0 is the prediction, the state is xnow)
        const double* const truth = h->obs_on && h->d_xp ? (const double*)h->d_xp : now;
        if ((h->obs_on || h->delay > 0) && s != h->last_stream) HIP_TRY(hipStreamSynchronize(h->last_stream)); // (xp may still be written on the last tick's stream)
        HIP_TRY(hipMemcpyAsync(x_hist, truth, nd * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    for (int t = 0; t < ticks; ++t) {
        if (every <= 1 || t % every == 0) { // (the ticks in between play the plan)
            rc = copra_batch_solve(h, hip_stream);
            if (rc != COPRA_OK) return rc;
        }
        const TickIO io { w_seq ? w_seq + (size_t)t * nd : st.w, x_hist ? x_hist + (size_t)(t + 1) * nd : st.x_out, u_hist ? u_hist + (size_t)t * nc : st.u_out,
            status_hist ? status_hist + (size_t)t * nb : st.status_out, st.age_hist ? st.age_hist + (size_t)t * nb : st.age_out,
            ex.d_hist ? ex.d_hist + (size_t)t * nd : ex.d_out, obs.v_seq ? obs.v_seq + (size_t)t * ny : obs.v, nullptr,
            obs.y_hist ? obs.y_hist + (size_t)t * ny : obs.y_out, obs.xhat_hist ? obs.xhat_hist + (size_t)t * nd : obs.xhat_out };
        rc = advance(h, st, io, s, "copra_batch_rollout");
        if (rc != COPRA_OK) return rc;
    }
    return COPRA_OK;
}

copra_status_t copra_batch_set_backup_steps(copra_batch_t* h, int steps)
{
    const char* const who = "copra_batch_set_backup_steps";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    const copra_status_t rc = check_handle(h, who);
    if (rc != COPRA_OK) return rc;
    const FusedPlan& P = h->hp.plan;
    if (steps < 0 || steps > P.N - 1) return fail(COPRA_ERR_ARG, std::string(who) + ": steps outside 0 .. N - 1");
    if (steps > 0 && h->delay > 0)
        return fail(COPRA_ERR_RUNTIME, std::string(who) + ": input delay is on (copra_batch_set_input_delay): the plan store reads the tail of the solve's controls");
    if (steps == 0) { // off: the store goes (the release waits for a tick that still uses it)
        h->backup_steps = 0;
        h->d_plan.reset();
        h->d_plan_next.reset();
        return COPRA_OK;
    }
    const size_t b = (size_t)(P.batch > 0 ? P.batch : 1);
    if (steps != h->backup_steps || !h->d_plan || !h->d_plan_next) {
        h->backup_steps = 0; // (a failed attempt leaves the feature off, never a store of the wrong size)
        OWN_TRY(h->d_plan.alloc(b * (size_t)steps * P.nu));
        if (!h->d_plan_next) OWN_TRY(h->d_plan_next.alloc(b));
    }
    HIP_TRY(hipMemsetAsync(h->d_plan_next, 0, b * sizeof(int), h->last_stream)); // every plan is forgotten, behind the last solve / tick
    h->backup_steps = steps;
    return COPRA_OK;
}

copra_status_t copra_batch_set_bias_estimator(copra_batch_t* h, const double* gain, int dense, int per_instance, int on_device)
{
    const char* const who = "copra_batch_set_bias_estimator";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    const copra_status_t rc = check_handle(h, who);
    if (rc != COPRA_OK) return rc;
    if (!gain) { // the estimator ends; the last estimates stay the model's d (h->d keeps pointing at them)
        h->bias_on = false;
        h->bias_gain.unset();
        return COPRA_OK;
    }
    if (h->obs_on) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the observer is on (copra_batch_set_observer): its gain Ld estimates d");
    if (h->shared || h->shared_as_batch)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": one model for the batch (copra_batch_set_shared_system) has one d; write the model out with copra_batch_set_system");
    if (!h->A || !h->B || !h->d) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": no preview system set (copra_batch_set_system)");
    const FusedPlan& P = h->hp.plan;
    if (bias_image_bytes(P.nx, P.nu, dense != 0) > kPlantLdsMax)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": one instance's model, plant and gain do not fit the LDS");
    if (!on_device) { // the library's copy: a tick that still reads the old one first
        const size_t count = (per_instance ? (size_t)(P.batch > 0 ? P.batch : 1) : 1) * (size_t)P.nx * (dense ? P.nx : 1);
        HIP_TRY(hipStreamSynchronize(h->last_stream));
        h->bias_on = false; // (a failed attempt leaves the estimator off, never a gain half replaced)
        OWN_TRY(h->bias_gain.copy_in(gain, count));
    }
    const copra_status_t rc_d = adopt_bias_buffer(h, h->last_stream); // the d in force seeds the estimates, behind the last solve / tick
    if (rc_d != COPRA_OK) return rc_d;
    if (on_device) h->bias_gain.borrow(gain);
    h->bias_dense = dense != 0, h->bias_per_instance = per_instance != 0;
    h->bias_on = true;
    return COPRA_OK;
}

copra_status_t copra_batch_set_bias(copra_batch_t* h, const double* d, int on_device)
{
    const char* const who = "copra_batch_set_bias";
    if (!h || !d) return fail(COPRA_ERR_ARG, std::string(who) + ": null argument");
    const copra_status_t rc = check_handle(h, who);
    if (rc != COPRA_OK) return rc;
    if (h->shared || h->shared_as_batch) return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": one model for the batch has no per-instance estimates");
    if (!h->d_bias || h->d != h->d_bias)
        return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the library's estimates are not the d in force (copra_batch_set_bias_estimator)");
    const size_t bytes = (size_t)h->hp.plan.batch * h->hp.plan.nx * sizeof(double);
    if (!bytes) return COPRA_OK;
    if (on_device) {
        HIP_TRY(hipMemcpyAsync(h->d_bias, d, bytes, hipMemcpyDeviceToDevice, h->last_stream));
    } else {
        HIP_TRY(hipStreamSynchronize(h->last_stream)); // (a tick that still writes the estimates)
        HIP_TRY(hipMemcpy(h->d_bias, d, bytes, hipMemcpyHostToDevice));
    }
    const copra_status_t rc_t = launch_target(h, h->last_stream, who);
    return rc_t != COPRA_OK ? rc_t : launch_delay(h, 0, nullptr, h->last_stream, who); // (input delay on: the prediction with the new d)
}

copra_status_t copra_batch_set_observer(copra_batch_t* h, int ny, const double* C, const double* Lx, const double* Ld, int per_instance, int on_device)
{
    const char* const who = "copra_batch_set_observer";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    const copra_status_t rc = check_handle(h, who);
    if (rc != COPRA_OK) return rc;
    if (!C) { // the observer ends; x0 and d stay as the last tick left them
        h->obs_on = false;
        h->obs_C.unset(), h->obs_Lx.unset(), h->obs_Ld.unset();
        return COPRA_OK;
    }
    if (ny < 1) return fail(COPRA_ERR_ARG, std::string(who) + ": ny < 1");
    if (!Lx) return fail(COPRA_ERR_ARG, std::string(who) + ": C needs a gain Lx");
    if (h->noise_sv && ny != h->noise_ny)
        return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the sensor noise in force was given for another ny: call copra_batch_set_noise again first");
    if (h->shared || h->shared_as_batch)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": one model for the batch (copra_batch_set_shared_system); write the model out with copra_batch_set_system");
    if (!h->A || !h->B || !h->d) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": no preview system set (copra_batch_set_system)");
    if (!h->x0) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": no initial states set");
    if (h->bias_on) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the disturbance estimator is on (copra_batch_set_bias_estimator): end it first, Ld takes its place");
    const FusedPlan& P = h->hp.plan;
    if ((double)ny * P.nx > 1e6 || observer_image_bytes(P.nx, P.nu, ny) > kPlantLdsMax)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": one instance's model, plant and observer do not fit the LDS");
    const size_t b = (size_t)(P.batch > 0 ? P.batch : 1), nd = (size_t)P.batch * P.nx;
    const bool was_on = h->obs_on;
    if (!on_device) { // the library's copies: a tick that still reads the old ones first
        const size_t count = (per_instance ? b : 1) * (size_t)P.nx * ny;
        HIP_TRY(hipStreamSynchronize(h->last_stream));
        h->obs_on = false; // (a failed attempt leaves the observer off, never its matrices half replaced)
        OWN_TRY(h->obs_C.copy_in(C, count));
        OWN_TRY(h->obs_Lx.copy_in(Lx, count));
        if (Ld) OWN_TRY(h->obs_Ld.copy_in(Ld, count));
        else h->obs_Ld.unset();
    }
    if (Ld) { // the estimates of d: the buffer and the seed of copra_batch_set_bias_estimator
        const copra_status_t rc_d = adopt_bias_buffer(h, h->last_stream);
        if (rc_d != COPRA_OK) return rc_d;
    }
    if (!was_on) { // turned on: the plant starts from the x0 in force, behind the last solve / tick
        if (!h->d_xp) OWN_TRY(h->d_xp.alloc(b * (size_t)P.nx));
        const double* const now = h->delay > 0 && h->d_delay_x ? (const double*)h->d_delay_x : h->x0; // (input delay: x0 is the prediction, the state is xnow)
        if (nd) HIP_TRY(hipMemcpyAsync(h->d_xp, now, nd * sizeof(double), hipMemcpyDeviceToDevice, h->last_stream));
    }
    h->obs_ny = ny, h->obs_per_instance = per_instance != 0;
    if (on_device) h->obs_C.borrow(C), h->obs_Lx.borrow(Lx), h->obs_Ld.borrow(Ld);
    h->obs_on = true;
    return COPRA_OK;
}

copra_status_t copra_batch_set_plant_state(copra_batch_t* h, const double* x, int on_device)
{
    const char* const who = "copra_batch_set_plant_state";
    if (!h || !x) return fail(COPRA_ERR_ARG, std::string(who) + ": null argument");
    if (!h->d_xp) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the plant has no state of its own: the observer was never on (copra_batch_set_observer)");
    const size_t bytes = (size_t)h->hp.plan.batch * h->hp.plan.nx * sizeof(double);
    if (!bytes) return COPRA_OK;
    if (on_device) {
        HIP_TRY(hipMemcpyAsync(h->d_xp, x, bytes, hipMemcpyDeviceToDevice, h->last_stream));
    } else {
        HIP_TRY(hipStreamSynchronize(h->last_stream)); // (a tick that still writes the state)
        HIP_TRY(hipMemcpy(h->d_xp, x, bytes, hipMemcpyHostToDevice));
    }
    return COPRA_OK;
}

const double* copra_batch_plant_state_device(const copra_batch_t* h)
{
    return h ? (const double*)h->d_xp : nullptr;
}

copra_status_t copra_batch_get_plant_state(copra_batch_t* h, double* x)
{
    const char* const who = "copra_batch_get_plant_state";
    if (!h || !x) return fail(COPRA_ERR_ARG, std::string(who) + ": null argument");
    if (!h->d_xp) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the plant has no state of its own: the observer was never on (copra_batch_set_observer)");
    HIP_TRY(hipStreamSynchronize(h->last_stream));
    HIP_TRY(hipMemcpy(x, h->d_xp, (size_t)h->hp.plan.batch * h->hp.plan.nx * sizeof(double), hipMemcpyDeviceToHost));
    return COPRA_OK;
}

void copra_noise_init(copra_noise_t* noise)
{
    if (!noise) return;
    std::memset(noise, 0, sizeof *noise);
    noise->struct_size = (int)sizeof *noise;
}

copra_status_t copra_batch_set_noise(copra_batch_t* h, const copra_noise_t* noise)
{
    const char* const who = "copra_batch_set_noise";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    const copra_status_t rc = check_handle(h, who);
    if (rc != COPRA_OK) return rc;
    copra_noise_t n;
    const copra_status_t rc_n = read_sized(n, noise, who, "copra_noise_t", "copra_noise_init");
    if (rc_n != COPRA_OK) return rc_n;
    if (!n.sigma_w && !n.sigma_v) { // off: nothing is drawn; the library's copies stay for the next time
        h->noise_sw.unset(), h->noise_sv.unset();
        h->noise_tick = 0;
        return COPRA_OK;
    }
    const FusedPlan& P = h->hp.plan;
    const unsigned long long top = 1ull << 32;
    if (n.first_instance > top || (unsigned long long)(P.batch > 0 ? P.batch : 0) > top - n.first_instance)
        return fail(COPRA_ERR_ARG, std::string(who) + ": first_instance + batch beyond 2^32");
    if (n.sigma_v && !h->obs_on) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": sensor noise needs the observer (copra_batch_set_observer)");
    const size_t b = (size_t)(P.batch > 0 ? P.batch : 1);
    const size_t cw = (n.per_instance ? b : 1) * (size_t)P.nx, cv = (n.per_instance ? b : 1) * (size_t)h->obs_ny;
    if (!n.on_device) {
        const auto bad = [](const double* a, size_t count) {
            for (size_t i = 0; a && i < count; ++i)
                if (!(a[i] >= 0.0)) return true;
            return false;
        };
        if (bad(n.sigma_w, cw) || bad(n.sigma_v, cv)) return fail(COPRA_ERR_ARG, std::string(who) + ": a negative or NaN sigma");
        HIP_TRY(hipStreamSynchronize(h->last_stream)); // the library's copies: a tick that still reads the old ones first
        h->noise_sw.unset(), h->noise_sv.unset(); // (a failed attempt leaves both streams off, never one with the other's layout)
        if (n.sigma_w) OWN_TRY(h->noise_sw.copy_in(n.sigma_w, cw));
        if (n.sigma_v) OWN_TRY(h->noise_sv.copy_in(n.sigma_v, cv));
    } else {
        h->noise_sw.borrow(n.sigma_w), h->noise_sv.borrow(n.sigma_v);
    }
    h->noise_per_instance = n.per_instance != 0;
    h->noise_ny = n.sigma_v ? h->obs_ny : 0;
    h->noise_seed = n.seed, h->noise_first = n.first_instance;
    h->noise_tick = 0;
    return COPRA_OK;
}

copra_status_t copra_batch_noise_seek(copra_batch_t* h, unsigned long long tick)
{
    if (!h) return fail(COPRA_ERR_ARG, "copra_batch_noise_seek: null handle");
    const copra_status_t rc = check_handle(h, "copra_batch_noise_seek");
    if (rc != COPRA_OK) return rc;
    h->noise_tick = tick;
    return COPRA_OK;
}

unsigned long long copra_batch_noise_tick(const copra_batch_t* h)
{
    return h ? h->noise_tick : 0;
}

copra_status_t copra_batch_draw_noise(copra_batch_t* h, unsigned long long tick, int stream, double* out_device, void* hip_stream)
{
    const char* const who = "copra_batch_draw_noise";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    if (stream != 0 && stream != 1) return fail(COPRA_ERR_ARG, std::string(who) + ": stream is 0 (process noise) or 1 (sensor noise)");
    if (!out_device) return fail(COPRA_ERR_ARG, std::string(who) + ": null out_device");
    const copra_status_t rc = check_handle(h, who);
    if (rc != COPRA_OK) return rc;
    if (stream == 1 && !h->obs_on) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": sensor noise needs the observer (copra_batch_set_observer)");
    const double* const sigma = stream == 0 ? h->noise_sw : (h->noise_ny == h->obs_ny ? h->noise_sv : nullptr);
    if (!sigma) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": no sigma set for this stream (copra_batch_set_noise)");
    const FusedPlan& P = h->hp.plan;
    if (P.batch <= 0) return COPRA_OK;
    NoiseFillArgs F {};
    F.batch = P.batch, F.rows = stream == 0 ? P.nx : h->obs_ny, F.stream = stream, F.per_instance = h->noise_per_instance;
    F.gen = NoiseGen { h->noise_seed, h->noise_first, tick };
    F.sigma = sigma, F.out = out_device;
    const int pairs = (F.rows + 1) / 2; // one thread per pair: a group fills the workgroup
    F.group = pairs >= kNoiseFillThreads ? 1 : kNoiseFillThreads / pairs;
    const unsigned grid = (unsigned)((F.batch + F.group - 1) / F.group);
    hipLaunchKernelGGL(copra_noise_fill_kernel, dim3(grid), dim3(kNoiseFillThreads), 0, (hipStream_t)hip_stream, F);
    HIP_TRY(hipGetLastError());
    return COPRA_OK;
}

const double* copra_batch_bias_device(const copra_batch_t* h)
{
    return h && !h->shared ? h->d : nullptr;
}

copra_status_t copra_batch_get_bias(copra_batch_t* h, double* d)
{
    if (!h || !d) return fail(COPRA_ERR_ARG, "copra_batch_get_bias: null argument");
    if (h->shared || !h->d) return fail(COPRA_ERR_RUNTIME, "copra_batch_get_bias: no per-instance preview system set (copra_batch_set_system)");
    HIP_TRY(hipStreamSynchronize(h->last_stream));
    HIP_TRY(hipMemcpy(d, h->d, (size_t)h->hp.plan.batch * h->hp.plan.nx * sizeof(double), hipMemcpyDeviceToHost));
    return COPRA_OK;
}

copra_status_t copra_batch_set_reference_schedule(copra_batch_t* h, int cost_index, const double* sched, long long steps, int r, int offset, int per_instance,
    int on_device)
{
    const char* const who = "copra_batch_set_reference_schedule";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    const FusedPlan& P = h->hp.plan;
    if (cost_index < 0 || cost_index >= (int)h->hp.cost_slot.size()) return fail(COPRA_ERR_ARG, std::string(who) + ": no such cost");
    const int t = h->hp.cost_slot[(size_t)cost_index]; // (dense costs are not among the kernel-evaluated terms)
    if (t < 0) return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": a dense (host-evaluated) cost has no reference p");
    RefSchedule& rs = h->ref_sched[t];
    if (!sched) { // the schedule ends, the window stays (cost_p keeps pointing at it)
        rs.sched.unset();
        return COPRA_OK;
    }
    if (steps < 1 || offset < 0) return fail(COPRA_ERR_ARG, std::string(who) + ": steps < 1 or offset < 0");
    const CostTerm& ct = P.cost[t];
    if (r < 1 || ct.prows % r != 0) return fail(COPRA_ERR_DOMAIN, std::string(who) + ": r does not divide the rows of the cost");
    if (ct.pstride && r != ct.pstride)
        return fail(COPRA_ERR_DOMAIN, std::string(who) + ": the controller evaluates this full-size cost step by step: r must be the rows of one step");
    const size_t b = (size_t)(P.batch > 0 ? P.batch : 1);
    if (!h->d_cost_p[t]) OWN_TRY(h->d_cost_p[t].alloc(b * ct.prows));
    if (!on_device) { // the library's copy: a window launch that still reads the old one first
        const size_t count = (per_instance ? b : 1) * (size_t)steps * r;
        HIP_TRY(hipStreamSynchronize(h->last_stream));
        OWN_TRY(rs.sched.copy_in(sched, count));
    } else {
        rs.sched.borrow(sched);
    }
    rs.steps = steps;
    rs.r = r, rs.S = ct.prows / r, rs.offset = offset, rs.per_instance = per_instance != 0;
    if (!h->cost_p[t]) h->model_dirty = true; // shared model: c0 / C2 change
    h->cost_p[t] = h->d_cost_p[t];
    target_drop_cost(h, t); // (a schedule on a cost the target calculation drives takes it off that list)
    return write_windows(h, h->last_stream, who);
}

copra_status_t copra_batch_schedule_seek(copra_batch_t* h, long long tick)
{
    if (!h) return fail(COPRA_ERR_ARG, "copra_batch_schedule_seek: null handle");
    if (tick < 0) return fail(COPRA_ERR_ARG, "copra_batch_schedule_seek: negative tick");
    h->sched_tick = tick;
    const copra_status_t rc = write_windows(h, h->last_stream, "copra_batch_schedule_seek");
    return rc != COPRA_OK ? rc : launch_target(h, h->last_stream, "copra_batch_schedule_seek");
}

copra_status_t copra_batch_set_constraint_schedule(copra_batch_t* h, int cstr_index, const double* sched, long long steps, int r, int offset, int preview,
    int per_instance, int on_device)
{
    const char* const who = "copra_batch_set_constraint_schedule";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    const FusedPlan& P = h->hp.plan;
    if (cstr_index < 0 || cstr_index >= (int)h->hp.cstr_kind.size() || h->hp.cstr_kind[(size_t)cstr_index] < 0)
        return fail(COPRA_ERR_ARG, std::string(who) + ": no such constraint");
    const int kind = h->hp.cstr_kind[(size_t)cstr_index], row0 = h->hp.cstr_row0[(size_t)cstr_index];
    if (kind == COPRA_CSTR_TRAJECTORY_BOUND || kind == COPRA_CSTR_CONTROL_BOUND || kind == COPRA_CSTR_DENSE || row0 < 0)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": not a Trajectory / Control / Mixed constraint of this controller "
                                                                "(control bounds: copra_batch_set_control_bound_schedule)");
    if (!sched) { // the schedule ends, the window stays in the per-instance right-hand sides
        auto it = h->cstr_sched.find(cstr_index);
        if (it != h->cstr_sched.end() && it->second.sched) {
            // (its last window launch may be in flight: it reads the schedule, which the caller may free now, and a right-hand side set by
            //  hand next must not be overtaken by it)
            HIP_TRY(hipStreamSynchronize(h->last_stream));
            it->second.sched.unset();
        }
        return COPRA_OK;
    }
    if (steps < 1 || offset < 0) return fail(COPRA_ERR_ARG, std::string(who) + ": steps < 1 or offset < 0");
    const int per_step = h->hp.cstr_per_step[(size_t)cstr_index], csteps = h->hp.cstr_steps[(size_t)cstr_index];
    int S = 0;
    if (csteps == 1) { // a full-size entry: any block size that divides its rows
        if (r < 1 || per_step % r != 0) return fail(COPRA_ERR_DOMAIN, std::string(who) + ": r does not divide the rows of this full-size constraint");
        S = per_step / r;
    } else {
        if (r != per_step) return fail(COPRA_ERR_DOMAIN, std::string(who) + ": r must be the rows of one step of this per-step constraint");
        S = csteps;
    }
    if (row0 + S * r > P.mgen) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the constraint's rows do not fit the plan");
    const bool was_live = h->cstr_sched.count(cstr_index) && h->cstr_sched[cstr_index].sched;
    if (!was_live && live_limit_windows(h) + 1 > kLimitWindowMax)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": more live limit windows than one launch serves (8; lower and upper bounds count as one each)");
    const size_t b = (size_t)(P.batch > 0 ? P.batch : 1);
    const copra_status_t rc_f = ensure_row_f_inst(h);
    if (rc_f != COPRA_OK) return rc_f;
    LimitSchedule& ls = h->cstr_sched[cstr_index];
    if (!on_device) { // the library's copy: a window launch that still reads the old one first
        HIP_TRY(hipStreamSynchronize(h->last_stream));
        OWN_TRY(ls.sched.copy_in(sched, (per_instance ? b : 1) * (size_t)steps * r));
    } else {
        ls.sched.borrow(sched);
    }
    ls.steps = steps;
    ls.r = r, ls.S = S, ls.row0 = row0, ls.offset = offset, ls.per_instance = per_instance != 0, ls.preview = preview != 0;
    return write_limit_windows(h, h->last_stream, who);
}

copra_status_t copra_batch_set_control_bound_schedule(copra_batch_t* h, const double* lower, const double* upper, long long steps, int offset, int preview,
    int per_instance, int on_device)
{
    const char* const who = "copra_batch_set_control_bound_schedule";
    if (!h) return fail(COPRA_ERR_ARG, std::string(who) + ": null handle");
    const FusedPlan& P = h->hp.plan;
    if ((lower == nullptr) != (upper == nullptr)) return fail(COPRA_ERR_ARG, std::string(who) + ": both of lower and upper are needed (or neither: the schedule ends)");
    if (!h->hp.has_control_bound || P.initial_state)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": the controller has no ControlBoundConstraint (or is an InitialStateLMPC controller)");
    if (!lower) { // the schedule ends, the window stays in the per-instance bounds
        if (h->lb_sched.sched || h->ub_sched.sched) HIP_TRY(hipStreamSynchronize(h->last_stream)); // (as for a constraint's schedule)
        h->lb_sched.sched.unset(), h->ub_sched.sched.unset();
        return COPRA_OK;
    }
    if (steps < 1 || offset < 0) return fail(COPRA_ERR_ARG, std::string(who) + ": steps < 1 or offset < 0");
    if (P.n != P.nu * P.N) return fail(COPRA_ERR_RUNTIME, std::string(who) + ": the plan's variables are not the controls of the horizon");
    const bool was_live = h->lb_sched.sched != nullptr;
    if (!was_live && live_limit_windows(h) + 2 > kLimitWindowMax)
        return fail(COPRA_ERR_UNSUPPORTED, std::string(who) + ": more live limit windows than one launch serves (8; lower and upper bounds count as one each)");
    const size_t b = (size_t)(P.batch > 0 ? P.batch : 1);
    // (first use: the window covers all nu N bounds of every instance -- nothing to start from)
    if (!h->d_lb_inst) OWN_TRY(h->d_lb_inst.alloc(b * (size_t)P.n));
    if (!h->d_ub_inst) OWN_TRY(h->d_ub_inst.alloc(b * (size_t)P.n));
    if (!on_device) {
        HIP_TRY(hipStreamSynchronize(h->last_stream));
        const size_t count = (per_instance ? b : 1) * (size_t)steps * P.nu;
        int e = h->lb_sched.sched.copy_in(lower, count);
        if (e == 0) e = h->ub_sched.sched.copy_in(upper, count);
        if (e != 0) h->lb_sched.sched.unset(), h->ub_sched.sched.unset(); // (both live or neither)
        OWN_TRY(e);
    } else {
        h->lb_sched.sched.borrow(lower), h->ub_sched.sched.borrow(upper);
    }
    for (LimitSchedule* ls : { &h->lb_sched, &h->ub_sched }) {
        ls->steps = steps;
        ls->r = P.nu, ls->S = P.N, ls->row0 = 0, ls->offset = offset, ls->per_instance = per_instance != 0, ls->preview = preview != 0;
    }
    return write_limit_windows(h, h->last_stream, who);
}

long long copra_batch_schedule_tick(const copra_batch_t* h)
{
    return h ? h->sched_tick : -1;
}

const double* copra_batch_x0_device(const copra_batch_t* h)
{
    return h ? h->x0 : nullptr;
}

copra_status_t copra_batch_get_x0(copra_batch_t* h, double* x0)
{
    if (!h || !x0) return fail(COPRA_ERR_ARG, "copra_batch_get_x0: null argument");
    if (!h->x0) return fail(COPRA_ERR_RUNTIME, "copra_batch_get_x0: no initial states set");
    HIP_TRY(hipStreamSynchronize(h->last_stream));
    HIP_TRY(hipMemcpy(x0, h->x0, (size_t)h->hp.plan.batch * h->hp.plan.nx * sizeof(double), hipMemcpyDeviceToHost));
    return COPRA_OK;
}

} // extern "C"
