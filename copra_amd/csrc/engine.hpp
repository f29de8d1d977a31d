// engine.hpp -- what the translation units of libcopra_hip.so share on the HOST side: the controller handle, the error slot, the HIP
// helpers and the handful of functions one unit calls in another.  Units:
//   copra_hip.hip          kernels of the controller paths, kernel selection, create / destroy, copra_batch_solve, shared-model and
//                          Riccati preparation, parity dump
//   copra_hip_ric.hip      run-time-horizon builds of the headline's kernels (ric_kernels.hpp)
//   copra_hip_setters.hip  everything that hands data in or out: set_* / get_* / results / timing / profile
//   copra_hip_jit.hip      copra_batch_specialise, copra_qp_dense_specialise (hipcc --genco at run time)
//   copra_hip_qp.hip       plug-in point 1: copra_qp_solve_dense_batch and its kernels
//   copra_hip_packed16/32.hip  the one-wave bodies with 16 / 32 lanes per instance
//   copra_hip_plant.hip    the receding-horizon tick: copra_batch_advance / copra_batch_rollout and their kernel (plant_step.hpp); reference
//                          schedules, whose windows the tick moves (copra_batch_set_reference_schedule, ref_window.hpp); limit schedules
//                          (copra_batch_set_constraint_schedule, copra_batch_set_control_bound_schedule, limit_window.hpp); noise drawn in
//                          the plant step and its fill kernel (copra_batch_set_noise, copra_batch_draw_noise, plant_noise.hpp)
//   copra_hip_score.hip    closed-loop scores: copra_batch_set_score / _score_reset / _get_score / _score_summary and their kernels
//                          (score_step.hpp); launch_score below is what the tick calls behind its plant step while scoring is on
//   copra_hip_target.hip   steady-state targets: copra_batch_set_target / _target_device / _target_status_device / _get_target and their
//                          kernel (target_step.hpp); launch_target below is what the tick and the setters that move d, the setpoint's
//                          block or the model call while targets are on
//   copra_hip_delay.hip    input delay in the tick: copra_batch_set_input_delay / _input_delay / _delay_state_device / _get_delay_state /
//                          _delay_queue_device / _get_delay_queue and their kernel (delay_step.hpp); launch_delay below is what the tick calls
//                          behind its plant step while delay is on, and what the setters that move the state, d or the model call
//   copra_hip_trace.hip    ensemble traces: copra_batch_set_trace / _trace_reset / _trace_info / _trace_device / _get_trace and their kernel
//                          (trace_step.hpp); launch_trace below is what the tick calls behind its score while tracing is on
//   copra_hip_trace_quant.hip  trace quantiles: copra_batch_set_trace_quantiles / _trace_quantile_info / _trace_quantiles_device /
//                          _get_trace_quantiles and their kernel (trace_quant_step.hpp); launch_trace_quant below is what launch_trace calls
//                          behind its own launches while quantiles are on
// and, host only and free of HIP: device_mem.hpp, the owners of device and pinned memory.  The two allocator policies below are the only
// place in the library that allocates or frees.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "../../include/copra_hip.h"
#include "device_mem.hpp"
#include "packed_launch.hpp"
#include "plan_builder.hpp"
#include "stage_plan.hpp"

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

using namespace copra_hip;

extern thread_local std::string g_copra_err; // what copra_last_error() returns
inline copra_status_t fail(copra_status_t code, const std::string& msg)
{
    g_copra_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                                                 \
    do {                                                                                                              \
        hipError_t e_ = (expr);                                                                                       \
        if (e_ != hipSuccess) return fail(COPRA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

// Dynamic LDS beyond 48 KiB is an opt-in PER KERNEL SYMBOL (copra_hip.hip); remembered per function
hipError_t lds_opt_in(const void* fn, size_t bytes);
#define LDS_OPT_IN(fn, bytes) HIP_TRY(lds_opt_in(reinterpret_cast<const void*>(fn), (bytes)))

// The allocator policies of device_mem.hpp.  release() of device memory WAITS for the device: a temporary that a just-launched kernel
// reads is kept alive by the release that follows the launch, so an owner's scope ends where that wait has to stand.
struct DeviceMem {
    static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static void release(void* p) { (void)hipFree(p); }
    static int copy_in(void* dst, const void* src, size_t bytes) { return (int)hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
};
struct PinnedMem {
    static int alloc(void** p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void release(void* p) { (void)hipHostFree(p); }
};
template <class T>
using Dev = DevBuf<T, DeviceMem>;
template <class T>
using PinnedBuf = DevBuf<T, PinnedMem>;
using Bag = DevBag<DeviceMem>;
template <class T>
using DevIn = DevArg<T, DeviceMem>;

// HIP_TRY for what an owner returns: OWN_TRY(h->d_x.alloc(n)), OWN_TRY(h->d_x.grow(n)), OWN_TRY(h->x_in.copy_in(x, n))
#define OWN_TRY(expr) HIP_TRY((hipError_t)(expr))

// a plan table on the device (at least one element, so that an empty table still has an address)
template <class T>
hipError_t upload(Dev<T>& dst, const std::vector<T>& src)
{
    int e = dst.alloc(src.empty() ? 1 : src.size());
    if (e == 0 && !src.empty()) e = DeviceMem::copy_in(dst, src.data(), src.size() * sizeof(T));
    return (hipError_t)e;
}

// persistent grids of the workgroup-per-instance kernels (copra_hip.hip)
int large_per_cu(const void* kernel, int threads, size_t lds_bytes);
int large_grid(const copra_options_t& opt, const void* kernel, int batch, int threads, size_t lds_bytes);
void see_axis_order(copra_batch* h, const double* A, const double* B, bool on_device);
bool prefer_w4(const copra_options_t& opt, const void* full, const void* w4, int threads, size_t lds_bytes);

constexpr size_t kSmallSlab = 1u << 20; // result slabs up to this size are fetched with one copy through pinned memory

// What the engine has LEARNT about a controller's workload.  Every decision that makes the choice of kernels (never their results) depend on
// earlier solves reads and writes this struct and nothing else: round-4 verdict -- four adaptive controllers spread over the handle were the
// place where the variants interacted.  copra_hip.hip: adapt_lane_pass, adapt_axis_solver, the list-length window (adapt_list_window and what
// reads it), adapt_layout, rechoose_layout, start_layout_from_histogram, the shared tier's choice.
struct AdaptState {
    bool solved_once = false;
    // the layout ladder of the first tier
    int adapt_left = 3; // solves after which the overflow count of a compact layout is still checked (adapt_layout)
    int lane_predict_left = 1; // solves whose first-tier layout is still chosen from the pass's violated-row histogram
    LdsLayout lds_top {}; // the layout the ladder started on: the choice is made again every 256 solves, from the top (rechoose_layout) -- a
    bool lds_top_set = false; // controller whose constraints relax gets its denser layout back
    long long layout_solves = 0; // solves completed on the current ladder
    // the one-instance-per-lane pass
    bool lane_ran = false; // the last solve ran it
    bool lane_off = false; // switched off for this controller: too few instances end in it (adapt_lane_pass), or no memory for its workspace
    bool lane_off_by_share = false; // ... the former: sampled again every 256 solves
    int lane_adapt_left = 2;
    bool lane_spec_shared_off = false; // the shared-model form of the pass does not take steps itself (too few instances end by them)
    bool lane_form_handover = false; // the pass runs in its hand-over form (too few instances end in the speculating one: adapt_lane_pass)
    bool lane_ws2_failed = false; // ... whose blocks found no room once (ensure_lane_buffers): the speculating form stays
    long long lane_solves = 0; // solves seen by adapt_lane_pass
    // the one-(instance, axis)-per-lane solver (lmpc_axis.hpp)
    bool axis_ran = false; // the last solve ran it
    bool axis_quiet = false; // ... without a second chance and a first tier behind it (its recent lists were empty: adapt_axis_quiet)
    bool axis_off = false; // switched off for this controller: it leaves more than half of the batch to the tier (adapt_axis_solver), or no memory for its list
    bool axis_off_by_share = false; // ... the former: sampled again every 256 solves
    int axis_adapt_left = 2; // solves after which its share is still looked at
    long long axis_solves = 0;
    // ... and the lengths of its recent lists, as they arrive in the handle's pinned words (h_lane_seen; adapt_list_window): the second chance's
    // grid, the first tier's grid and whether both are launched at all follow them
    int lane_seen_slot = 0, lane_seen_max = 0, lane_seen_first_max = 0; // (of the tier's list | of the first launch's list, which the second chance walks)
    long long lane_seen_solves = 0;
    // shared-model tick on the records tier
    long long shared_ric_solves = 0; // solves launched on the tier's shared-model mode
    bool shared_ric_off = false; // ... which a small, constraint-heavy controller leaves after its first solve
    // where the LAST LAUNCHED solve wrote its counters (round-4 advisor: rechoose_layout and the shared tier's choice read the buffers set for
    // the NEXT solve -- with rotating result slabs an uninitialised one)
    const int* last_iter = nullptr;
    const int* last_status = nullptr;
    const double* last_control = nullptr; // ... and its controls: what copra_batch_advance applies to the plant (copra_hip_plant.hip)
};

// A cost whose reference follows a schedule (copra_batch_set_reference_schedule): the tick writes its window into d_cost_p (copra_hip_plant.hip)
struct RefSchedule {
    DevIn<double> sched; // null: the cost has no schedule
    long long steps = 0;
    int r = 0, S = 0, offset = 0, per_instance = 0;
};

// A limit that follows a schedule (copra_batch_set_constraint_schedule: the right-hand sides of one constraint, written into d_row_f_inst at its
// stacked rows; copra_batch_set_control_bound_schedule: the lower / upper control bounds, into d_lb_inst / d_ub_inst): the tick writes its window
// behind the reference windows (copra_hip_plant.hip, limit_window.hpp)
struct LimitSchedule {
    DevIn<double> sched; // null: no schedule
    long long steps = 0;
    int r = 0, S = 0, row0 = 0, offset = 0, per_instance = 0, preview = 0;
};

constexpr int kScoreArrays = 7; // the arrays of a score's measure (copra_score_t)
constexpr int kTraceArrays = 4; // the limits of a trace (copra_trace_t)
constexpr int kTargetCosts = 8; // the costs one target calculation drives (copra_target_t; kTargetMaxCosts of target_step.hpp)

// Ownership is by type: a Dev<T> / PinnedBuf<T> / Bag member owns its memory and frees it with the handle; every raw pointer is borrowed
// from the caller or a view into an owned block.  An array that a setter accepts on the device (borrowed) or from the host (copied) is ONE
// DevIn<T> member: it reads as the pointer in force and holds the library's copy, which a borrow or an unset keeps for the next time.  Its
// setter waits for the handle's last stream once (a launch may still read the old copy), calls copy_in() per array and leaves its feature off
// when one fails.  Nothing owned refers to anything else owned, so the order of destruction is free.
// Deliberately NOT DevIn, because pointer and buffer mean more there than "theirs or our copy": A / B / d / x0 beside own_A / own_B / own_d /
// own_x0 (own_x0 is also the tick's write buffer, d also aliases d_bias, own_A / own_B are the targets of the row-major transposes) and
// cost_p / d_cost_p, cost_w / d_cost_w (the window and target kernels write d_cost_p, and equality with it is tested in several places).
struct copra_batch {
    HostPlan hp;
    AdaptState ad;
    // device copies of the plan tables
    Dev<int> d_row_step, d_row_ekind, d_row_eoff, d_row_gkind, d_row_goff;
    Dev<double> d_row_f, d_params, d_lb, d_ub;
    Dev<int> d_row_prev, d_warm; // warm start of the shared-model path (copra_batch_set_warm_start)
    // system (owned copies, or borrowed device pointers; not DevIn: see above)
    Dev<double> own_A, own_B, own_d, own_x0;
    int axis_order = 0; // the state order of this controller's systems as the (instance, axis)-per-lane solver sees it (FusedPlan::axis_order) ...
    bool axis_order_seen = false; // ... looked at when the first systems were set (see_axis_order, copra_hip.hip)
    bool shared_as_batch = false; // copra_batch_set_shared_system on a controller the (instance, axis)-per-lane solver takes: the model written out per instance (copra_hip.hip)
    const double *A = nullptr, *B = nullptr, *d = nullptr, *x0 = nullptr;
    // results
    double *d_control = nullptr, *d_traj = nullptr; // (carved from ONE allocation, d_results: small batches fetch it with one copy)
    int *d_status = nullptr, *d_iter = nullptr;
    Dev<unsigned char> d_results;
    size_t results_bytes = 0, off_traj = 0, off_status = 0, off_iter = 0;
    PinnedBuf<unsigned char> h_results; // pinned staging copy of the slab (batches whose slab is at most kSmallSlab bytes)
    // caller-provided device result buffers (copra_batch_set_outputs); override the engine-owned ones
    double *ext_control = nullptr, *ext_traj = nullptr;
    int *ext_status = nullptr, *ext_iter = nullptr;
    Dev<int> d_ovf_count, d_ovf_list; // two-tier queue (TWO counters, used in turn: begin_overflow_queue)
    int ovf_cur = 0; // the counter the last solve appended to
    bool ovf_clean[2] = { false, false }; // known to hold zero on the device
    // shared-model fast path: one (A, B, d) for the whole batch, factorised once (copra_batch_set_shared_system)
    bool shared = false, model_dirty = true, shared_attr_set = false;
    // shared-model mode of the Riccati-factor tier (lmpc_fused_ric.hpp, FusedPlan::ric_model): the layout the plan builder chose
    // for that tier (kept when copra_batch_set_shared_system moves the plan to an LDS-Q1 layout), whether the next solve uses it,
    // and the batch-wide records
    bool has_lds_ric = false, shared_ric = false;
    LdsLayout lds_ric {};
    Dev<double> d_ric_model;
    int model_ref_off[kMaxCosts]; // columns of C2 per cost as prepared (-1: none)
    int model_rtot = 0; // columns of C2 / K2 as prepared
    Dev<double> d_shA, d_shB, d_shd, d_model;
    std::vector<double> shA, shB, shd;
    bool sh_dev_stale = true; // d_shA / d_shB / d_shd (the shared model as a plant, copra_hip_plant.hip) are older than shA / shB / shd
    Dev<double> d_row_f_inst, d_lb_inst, d_ub_inst; // per-instance rhs / control bounds
    Dev<double> d_cost_p[kMaxCosts]; // per-instance cost references (owned copies; with cost_p and the weights below not DevIn: see above) ...
    const double* cost_p[kMaxCosts] = {}; // ... or borrowed device pointers (copra_batch_set_cost_reference)
    RefSchedule ref_sched[kMaxCosts]; // ... which the tick rewrites for the costs that follow a schedule,
    long long sched_tick = 0; // at the controller's tick counter tau: the advances so far, or what copra_batch_schedule_seek set
    std::map<int, LimitSchedule> cstr_sched; // limit schedules by constraint (position in the user's array) ...
    LimitSchedule lb_sched, ub_sched; // ... and of the control bounds (both live or neither)
    // backup plans of the tick (copra_batch_set_backup_steps; copra_hip_plant.hip, plant_step.hpp)
    int backup_steps = 0; // K: 0 is off
    Dev<double> d_plan; // [batch][K][nu]: controls of steps 1 .. K of every instance's last successful solve
    Dev<int> d_plan_next; // [batch]: the step of d_plan the next tick without a fresh solution applies (0: no plan, > K: used up)
    bool plan_fresh = false; // a solve has been launched since the previous plant step (set by copra_batch_solve, cleared by the tick)
    // disturbance estimator of the tick (copra_batch_set_bias_estimator; copra_hip_plant.hip, plant_step.hpp)
    bool bias_on = false;
    int bias_dense = 0, bias_per_instance = 0;
    DevIn<double> bias_gain;
    Dev<double> d_bias; // [batch][nx]: the estimates; the controller's d (h->d) from the moment the estimator is turned on -- never own_d
    // state observer of the tick (copra_batch_set_observer; copra_hip_plant.hip, plant_step.hpp): x0 is the estimate while it is on
    bool obs_on = false;
    int obs_ny = 0, obs_per_instance = 0;
    DevIn<double> obs_C, obs_Lx, obs_Ld; // obs_Ld null: d is not estimated
    Dev<double> d_xp; // [batch][nx]: the plant's own state, from the first time the observer is turned on
    // noise drawn on the device (copra_batch_set_noise; copra_hip_plant.hip, plant_noise.hpp)
    DevIn<double> noise_sw, noise_sv; // null: that stream is off
    int noise_per_instance = 0, noise_ny = 0; // (noise_ny: the observer's ny that noise_sv was given for)
    unsigned long long noise_seed = 0, noise_first = 0;
    unsigned long long noise_tick = 0; // plant steps since copra_batch_set_noise, or what copra_batch_noise_seek set
    // closed-loop scores (copra_batch_set_score; copra_hip_score.hip, score_step.hpp): every buffer is taken by the setter, never by the tick
    bool score_on = false;
    int score_dense = 0, score_per_instance = 0;
    long long score_ref_steps = 0;
    double score_tol = 0.0;
    DevIn<double> score_arr[kScoreArrays]; // qx, ru, x_ref, x_lo, x_hi, u_lo, u_hi; null: not given
    Dev<unsigned char> d_score; // [batch] records of 64 bytes
    Dev<double> d_score_u; // [batch][nu]: the tick's u_out where the caller gave none ...
    Dev<int> d_score_age; // ... and [batch] its age_out
    Dev<unsigned char> d_score_part; // the partials of the summary's first stage, then its result
    PinnedBuf<unsigned char> h_score_sum; // the result's way to the host
    // steady-state targets (copra_batch_set_target; copra_hip_target.hip, target_step.hpp): every buffer is taken by the setter, never by the tick
    bool target_on = false;
    int target_offset = 0, target_per_instance = 0;
    long long target_steps = 0;
    DevIn<double> target_H, target_r;
    int target_ncost = 0; // the driven costs: their slot among the kernel-evaluated terms, the rows of one block, the map T_c
    int target_cost[kTargetCosts] = {}, target_rows[kTargetCosts] = {};
    DevIn<double> target_map[kTargetCosts];
    Dev<double> d_target; // [batch][nx + nu]: z = [xs ; us]
    Dev<int> d_target_status; // [batch]: 1 where the last calculation found the instance singular
    // input delay of the tick (copra_batch_set_input_delay; copra_hip_delay.hip, delay_step.hpp): every buffer is taken by the setter, never by
    // the tick; while it is on x0 (own_x0) is the PREDICTION the next solve reads and d_delay_x the state at the current tick
    int delay = 0; // D: 0 is off
    int delay_head = 0; // the ring slot the next plant step applies: the oldest pending command
    Dev<double> d_delay_q; // [batch][D][nu]: the pending commands
    Dev<int> d_delay_qs; // [D][batch]: the status of the solve that issued each
    Dev<double> d_delay_x; // [batch][nx]: xnow -- the measured state, or the observer's estimate
    // ensemble traces (copra_batch_set_trace; copra_hip_trace.hip, trace_step.hpp): every buffer is taken by the setter, never by the tick; the
    // slot a recorded tick writes is counted HERE, on the host, and handed to its launches
    bool trace_on = false;
    int trace_what = 0, trace_every = 1, trace_rows = 0, trace_in_lds = 0;
    long long trace_cap = 0; // slots
    long long trace_tick = 0, trace_recorded = 0, trace_missed = 0; // ticks since the last set / reset; slots written; recordable ticks a full trace let pass
    double trace_tol = 0.0;
    DevIn<double> trace_lim[kTraceArrays]; // x_lo, x_hi, u_lo, u_hi; null: not given
    Dev<unsigned char> d_trace; // [capacity] slots
    Dev<unsigned char> d_trace_part; // [chunks] partials of a tick's first stage, slot-shaped
    Dev<double> d_trace_u; // [batch][nu]: the tick's u_out where neither the caller nor the score gave one ...
    Dev<int> d_trace_age; // ... and [batch] its age_out
    // trace quantiles (copra_batch_set_trace_quantiles; copra_hip_trace_quant.hip, trace_quant_step.hpp): they belong to the trace in force --
    // the slot index is the trace's, and whatever ends or replaces the trace ends them
    bool quant_on = false;
    int quant_count = 0; // levels
    double quant_level[COPRA_TRACE_QUANT_MAX] = {};
    Dev<double> d_quant; // [capacity][rows][levels]
    Dev<unsigned long long> d_quant_keys; // [rows][batch]: the keys of a recorded tick, written by the kernel's first pass
    Dev<double> d_cost_w[kMaxCosts]; // per-instance cost weights (owned copies) ...
    const double* cost_w[kMaxCosts] = {}; // ... or borrowed device pointers (copra_batch_set_cost_weights)
    // While a controller has per-instance weights its first tier must not be the Riccati-factor tier (its tables hold the creation
    // weights): the layout it had is kept here and given back once the weights are restored (weights_route, copra_hip.hip)
    bool wt_saved = false;
    LdsLayout wt_lds {};
    bool wt_two_tier = false, wt_dense = false;
    int wt_packed = 0;
    // copra_batch_specialise: this controller's shape compiled into its own kernels (hipcc --genco, cached on disk)
    hipModule_t jit_module = nullptr;
    hipFunction_t jit_fused = nullptr, jit_shared = nullptr;
    hipFunction_t jit_fused_q0 = nullptr; // Riccati-factor tier compiled for this shape: Q1 in LDS (further down the layout ladder)
    hipFunction_t jit_lane = nullptr; // ... and the one-instance-per-lane pass in front of it (lmpc_lane.hpp),
    hipFunction_t jit_lane_plain = nullptr; // ... its build without the speculative steps
    bool jit_ric = false; // the code object holds the Riccati-factor tier (lmpc_fused_ric.hpp) of this controller's shape
    int jit_lanes = 64; // lanes per instance the code object was compiled for
    int jit_tri = 0; // ... and whether for the factor-only layout
    // one-instance-per-lane pass in front of the Riccati-factor tier (lmpc_lane.hpp)
    Dev<int> d_lane_count, d_lane_list; // (two counters, used in turn like the overflow queue's)
    Dev<int> d_lane_hist; // histogram of the violated-row counts the pass leaves (kLaneHistBins; read once, before the first tier launch)
    Dev<double> d_lane_ws;
    int* d_lane_seen = nullptr; // ... the same words as the device sees them (a view of h_lane_seen)
    PinnedBuf<int> h_lane_seen; // pinned: [2] the lengths of the last solves' first-tier lists as they arrive (ensure_axis_buffers; read by adapt_list_window into AdaptState)
    Dev<int> d_axis_list2, d_axis_count2; // the list the second chance of the (instance, axis)-per-lane solver appends to (the first tier's, then) and its length
    Dev<int> d_axis_acc; // lmpc_axis.hpp: the words in which the counters of instances on spare lanes meet (FusedPlan::axis_acc; zero between solves)
    Dev<double> d_lane_ws2; // the instance-major hand-over blocks of the pass (FusedPlan::lane_ws2)
    int lane_cur = 0; // the counter the last solve appended to
    int packed = 0; // lanes per instance when several small problems share a wavefront (16 / 32; 0: one wave each)
    void (*large_fn)(const FusedPlan) = nullptr; // workgroup-per-instance kernel variant chosen at creation
    Dev<double> d_ws; // workgroup-per-instance kernel: [large_grid][ws_total] doubles (J, factor, Phi, ...)
    int large_grid = 0;
    // InitialStateLMPC variant
    Dev<double> d_isR, d_isr, d_x0opt;
    DevIn<double> x0lb, x0ub;
    // stage-wise Riccati interior-point path (copra_batch_select_solver; lmpc_riccati.hpp)
    int solver = COPRA_SOLVER_DEFAULT;
    HostStagePlan hs;
    bool ric_fast = false; // the LDS-resident kernel (lmpc_riccati_mfma.hpp) runs it
    bool ric_refs = false; // ... decided for this state of the per-instance cost references
    bool ric_built = false; // hs describes this controller (eligible or not) ...
    bool ric_all_bounds = false; // ... with bound rows for every control
    Bag ric_dev; // device copies of its tables
    Dev<double> d_ric_ws;
    Dev<int> d_ric_next; // work-queue counter of the Riccati kernel
    int ric_grid = 0;
    Dev<long long> d_prof_fine; // profiling builds only
    Dev<long long> d_prof; // optional per-instance phase cycle counts (copra_batch_enable_phase_profile)
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evm = nullptr; // start | end of the solve | end of its first launch (packet-borne timing)
    bool tier_timed = false; // evm was written by the last solve
    hipEvent_t ev_plant = nullptr; // orders copra_batch_advance on another stream behind the solve
    hipStream_t last_stream = nullptr;
    bool timed = false;
    bool lds_attr_set = false;
};

// Per-instance cost weights (copra_batch_set_cost_weights) are set.  Every kernel that bakes the weights into tables at plan time -- the
// (instance, axis)-per-lane solver, the one-instance-per-lane pass, the Riccati-factor tier, the shared-model kernels, the Riccati
// interior-point kernels -- is off while this holds; every selector of those kernels asks it.
inline bool own_weights(const copra_batch* h)
{
    for (int t = 0; t < kMaxCosts; ++t)
        if (h->cost_w[t]) return true;
    return false;
}
// ... and per-instance cost references (copra_batch_set_cost_reference): an instance's affine terms are its own
inline bool own_references(const copra_batch* h)
{
    for (int t = 0; t < kMaxCosts; ++t)
        if (h->cost_p[t]) return true;
    return false;
}

// Limit schedules that the tick still moves: how many windows one launch has to write
inline int live_limit_windows(const copra_batch* h)
{
    int n = (h->lb_sched.sched != nullptr) + (h->ub_sched.sched != nullptr);
    for (const auto& kv : h->cstr_sched) n += kv.second.sched != nullptr;
    return n;
}

// What is launched on `s` next stands behind the handle's last stream, where that is another one (ev_plant is the event of this alone)
inline copra_status_t order_behind_last(copra_batch* h, hipStream_t s)
{
    if (s == h->last_stream) return COPRA_OK;
    if (!h->ev_plant) HIP_TRY(hipEventCreateWithFlags(&h->ev_plant, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(h->ev_plant, h->last_stream));
    HIP_TRY(hipStreamWaitEvent(s, h->ev_plant, 0));
    return COPRA_OK;
}

// The library's estimates become the controller's d: d_bias, allocated on first use, is seeded on `s` from the d in force -- a caller's
// buffer is read, never written
inline copra_status_t adopt_bias_buffer(copra_batch* h, hipStream_t s)
{
    const FusedPlan& P = h->hp.plan;
    if (!h->d_bias) OWN_TRY(h->d_bias.alloc((size_t)(P.batch > 0 ? P.batch : 1) * P.nx));
    if (h->d == h->d_bias) return COPRA_OK;
    const size_t nd = (size_t)P.batch * P.nx;
    if (nd) HIP_TRY(hipMemcpyAsync(h->d_bias, h->d, nd * sizeof(double), hipMemcpyDeviceToDevice, s));
    h->d = h->d_bias;
    return COPRA_OK;
}

// A new system (h->d) while the disturbance estimator is on: the estimates restart from its d -- copied on `s`, behind the last tick (which
// may still write them), into the library's buffer, which stays the controller's d; the new d itself is only read.  The observer with a
// gain Ld estimates d the same way
inline copra_status_t bias_restart(copra_batch* h, hipStream_t s)
{
    const bool estimates = h->bias_on || (h->obs_on && h->obs_Ld);
    if (!estimates || !h->d_bias || h->d == h->d_bias) return COPRA_OK;
    const copra_status_t rc = order_behind_last(h, s);
    return rc != COPRA_OK ? rc : adopt_bias_buffer(h, s);
}

// A caller's struct up to its struct_size, zero beyond it: fields the caller's version of the header does not know keep their defaults.
// A null `src` reads as all zero
template <class D, class S>
copra_status_t read_sized(D& dst, const S* src, const char* who, const char* type_name, const char* init_name)
{
    static_assert(sizeof(D) >= sizeof(S), "the widest form of the struct");
    std::memset(&dst, 0, sizeof dst);
    if (!src) return COPRA_OK;
    if (src->struct_size < (int)sizeof(int))
        return fail(COPRA_ERR_ARG, std::string(who) + ": " + type_name + "::struct_size is not set (" + init_name + ")");
    std::memcpy(&dst, src, (size_t)src->struct_size < sizeof dst ? (size_t)src->struct_size : sizeof dst);
    return COPRA_OK;
}

// First use of the per-instance right-hand sides: every instance starts from the controller-wide ones
inline copra_status_t ensure_row_f_inst(copra_batch* h)
{
    if (h->d_row_f_inst) return COPRA_OK;
    const FusedPlan& P = h->hp.plan;
    const size_t b = (size_t)(P.batch > 0 ? P.batch : 1);
    OWN_TRY(h->d_row_f_inst.alloc(b * (size_t)P.mgen));
    std::vector<double> rep(b * (size_t)P.mgen);
    for (size_t i = 0; i < b; ++i) std::copy(h->hp.row_f.begin(), h->hp.row_f.begin() + P.mgen, rep.begin() + i * P.mgen);
    HIP_TRY(hipMemcpy(h->d_row_f_inst, rep.data(), rep.size() * sizeof(double), hipMemcpyHostToDevice));
    return COPRA_OK;
}

// A reference of cost term t given by hand or by a schedule: the cost leaves the target calculation's list, as those setters end a schedule
inline void target_drop_cost(copra_batch* h, int t)
{
    for (int k = 0; k < h->target_ncost; ++k) {
        if (h->target_cost[k] != t) continue;
        h->target_map[k].unset(); // (its copy goes to the end of the list, kept: a launch in flight may still read it)
        for (int q = k + 1; q < h->target_ncost; ++q) {
            h->target_cost[q - 1] = h->target_cost[q], h->target_rows[q - 1] = h->target_rows[q];
            std::swap(h->target_map[q - 1], h->target_map[q]); // (the view and the copy travel together)
        }
        h->target_ncost -= 1;
        return;
    }
}

// ---- copra_hip.hip ----
typedef void (*fused_kernel_t)(const FusedPlan);
FusedPlan device_plan(const copra_batch* h);
copra_status_t ensure_lds_attr(copra_batch* h);
copra_status_t prepare_riccati(copra_batch* h);
bool use_riccati(copra_batch* h);
fused_kernel_t select_fused_kernel(const FusedPlan& P);
fused_kernel_t select_tier2_kernel(const FusedPlan& P);
// ---- copra_hip_score.hip: one tick's update of the records, on `s` behind the plant step -- x [batch][nx] the true state after the tick, u
// [batch][nu] and age [batch] what the tick wrote as u_out / age_out; called only while h->score_on; no synchronisation, no allocation ----
copra_status_t launch_score(copra_batch* h, const double* x, const double* u, const int* age, hipStream_t s, const char* who);
// ---- copra_hip_trace.hip: one tick of the trace, on `s` behind the score -- x, u, age as for launch_score; est [batch][nx] the estimate of the
// same tick where the observer simulates a plant (x is then the plant's own state), else null; called only while h->trace_on; moves the trace's
// tick count, launches on a recorded tick only; no synchronisation, no allocation ----
copra_status_t launch_trace(copra_batch* h, const double* x, const double* est, const double* u, const int* age, hipStream_t s, const char* who);
// ---- copra_hip_trace_quant.hip: the quantiles of a recorded tick, on `s` behind the trace's launches -- T the tick as launch_trace handed it
// to its kernels, `slot` the slot it counted; returns at once while quantiles are off; no synchronisation, no allocation.  trace_quant_off:
// quantiles end and their buffers go ----
namespace copra_hip {
struct TraceArgs;
}
copra_status_t launch_trace_quant(copra_batch* h, const copra_hip::TraceArgs& T, long long slot, hipStream_t s, const char* who);
void trace_quant_off(copra_batch* h);
// ---- copra_hip_target.hip: the steady states and the driven costs' references from the model, the d and the setpoint's block in force, on
// `s` (behind the handle's last stream where that is another one); returns at once while targets are off; no synchronisation, no allocation ----
copra_status_t launch_target(copra_batch* h, hipStream_t s, const char* who);
// ---- copra_hip_plant.hip: the shared model of copra_batch_set_shared_system on the device, uploaded once per model ----
copra_status_t shared_model_on_device(copra_batch* h);
// ---- copra_hip_delay.hip: input delay.  launch_delay: with push the last solve's command and status go into the ring slot the plant step just
// applied and the head moves on; then the prediction from xnow, the model and d in force and the queue becomes x0 (own_x0) -- on `s` (behind
// the handle's last stream where that is another one), returns at once while delay is off; no synchronisation, no allocation.
// delay_adopt_x0: a setter brought a new state -- h->x0 is copied into xnow on `s` and the prediction takes its place ----
copra_status_t launch_delay(copra_batch* h, int push, const double* fallback_u, hipStream_t s, const char* who);
copra_status_t delay_adopt_x0(copra_batch* h, hipStream_t s, const char* who);
// ---- copra_hip_jit.hip: dense-QP kernels compiled at run time for one problem size (copra_qp_dense_specialise) ----
hipFunction_t dense_jit_lookup(int n, int lanes);
