/*
 * copra_hip.h -- C ABI of the MI355X-native batched condensed linear-MPC engine (libcopra_hip.so).
 *
 * This is the drop-in boundary BENEATH copra's C++ classes.  The reference (jrl-umi3218/copra v1.3.3) has no C
 * ABI of its own; each entry point below names the reference interface it replaces (file:line relative to the
 * reference tree).  Plain pointers and sizes only -- no torch / Eigen types.  All matrices are FP64 and
 * column-major per instance (Eigen's default layout, include/PreviewSystem.h:56-62); batched arrays are
 * batch-major: element (b, i, j) of a [batch][rows x cols] array lives at  ptr[b*rows*cols + j*rows + i].
 *
 * Error convention: every function returns a copra_status_t; COPRA_ERR_DOMAIN corresponds to the reference's
 * std::domain_error (include/debugUtils.h:32-36), COPRA_ERR_RUNTIME to std::runtime_error (:38-42).  No C++
 * exception crosses this boundary; the C++ wrappers (copra_amd/cpp) translate codes back into those exceptions.
 * copra_last_error() returns a thread-local message.
 *
 * The library REQUIRES a HIP device (gfx950).  There is no CPU fallback: without a usable device every compute
 * entry point returns COPRA_ERR_HIP.
 */
#ifndef COPRA_HIP_H
#define COPRA_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    COPRA_OK = 0,
    COPRA_ERR_DOMAIN = 1, /* std::domain_error: dimension mismatch (debugUtils.h:32-36) */
    COPRA_ERR_RUNTIME = 2, /* std::runtime_error (debugUtils.h:38-42) */
    COPRA_ERR_HIP = 3, /* HIP runtime failure / no device */
    COPRA_ERR_UNSUPPORTED = 4, /* valid copra problem that this build of the engine does not cover */
    COPRA_ERR_ARG = 5 /* NULL / negative argument */
} copra_status_t;

/* Cost kinds: include/costFunctions.h:103 (TrajectoryCost), :134 (TargetCost), :165 (ControlCost), :196 (MixedCost).
 * COPRA_COST_DENSE: a user-defined CostFunction subclass (plug-in point 2, include/costFunctions.h:22-97) whose update()
 * ran on the host: the base-class members Q_ (fullUDim x fullUDim), c_ (fullUDim), E_ (xDim x fullUDim), f_ (fullUDim)
 * as LMPC::makeQPForm (src/LMPC.cpp:252-255: Q += Q_, c += c_) and InitialStateLMPC::makeQPForm
 * (src/InitialStateLMPC.cpp:80-84: Q += Q_, E += E_, tail of c += f_) consume them. */
typedef enum {
    COPRA_COST_TRAJECTORY = 0,
    COPRA_COST_TARGET = 1,
    COPRA_COST_CONTROL = 2,
    COPRA_COST_MIXED = 3,
    COPRA_COST_DENSE = 4
} copra_cost_kind_t;

/* Constraint kinds: include/constraints.h:114, :153, :193, :234, :284 */
typedef enum {
    COPRA_CSTR_TRAJECTORY = 0,
    COPRA_CSTR_CONTROL = 1,
    COPRA_CSTR_MIXED = 2,
    COPRA_CSTR_TRAJECTORY_BOUND = 3,
    COPRA_CSTR_CONTROL_BOUND = 4,
    /* a user-defined EqIneqConstraint subclass (plug-in point 2, include/constraints.h:42-107) whose update() ran on the
     * host: A_ (rows x fullUDim), b_ (rows), Y_ (rows x xDim), z_ (rows) with b = z - Y x0.  LMPC stacks [A | b]
     * (src/LMPC.cpp:257-271), InitialStateLMPC stacks [Y, A | z] (src/InitialStateLMPC.cpp:88-102). */
    COPRA_CSTR_DENSE = 5
} copra_cstr_kind_t;

/* Per-instance solver status == SolverInterface::SI_fail() of QuadProgDenseSolver (include/QuadProgSolver.h:21-27),
 * plus one engine-specific code. */
typedef enum {
    COPRA_QP_OK = 0, /* "No problems" */
    COPRA_QP_INFEASIBLE = 1, /* "The minimization problem has no solution" */
    COPRA_QP_NOT_PD = 2, /* "Problems with the decomposition of Q" */
    COPRA_QP_ITER_LIMIT = 3 /* engine safety cap on active-set iterations (never hit by a well-posed QP) */
} copra_qp_status_t;

/* A cost function exactly as handed to LMPC::addCost (src/LMPC.cpp:118-122), i.e. the constructor arguments of
 * include/costFunctions.h:112-118 / :142-148 / :171-177 / :203-210 plus CostFunction::weights (:54-67).
 * Host pointers; copied at copra_batch_create.  The parameters are shared by every instance of the batch (references and weights can be
 * set per instance later: copra_batch_set_cost_reference, copra_batch_set_cost_weights). */
typedef struct {
    int kind; /* copra_cost_kind_t */
    int rows; /* rows of M / N / p / weights */
    int m_cols; /* cols of M: xDim (per-step entry) or fullXDim (full-size entry); 0 if unused */
    int n_cols; /* cols of N: uDim or fullUDim; 0 if unused */
    const double* M; /* rows x m_cols */
    const double* N; /* rows x n_cols */
    const double* p; /* rows */
    const double* weights; /* rows */
    /* COPRA_COST_DENSE only (column-major; rows / M / N / p / weights unused): LMPC reads Q and c, InitialStateLMPC reads
     * Q, E and f; a pointer the variant does not read may be NULL */
    const double* Q; /* fullUDim x fullUDim, symmetric */
    const double* c; /* fullUDim */
    const double* E; /* xDim x fullUDim */
    const double* f; /* fullUDim */
} copra_cost_desc_t;

/* A constraint exactly as handed to LMPC::addConstraint (src/LMPC.cpp:124-128): constructor arguments of
 * include/constraints.h:125-132 / :165-172 / :209-217 / :242-255 / :296-303. */
typedef struct {
    int kind; /* copra_cstr_kind_t */
    int rows; /* rows of E / G / f, or length of lower / upper */
    int e_cols; /* cols of E (xDim | fullXDim), 0 if unused */
    int g_cols; /* cols of G (uDim | fullUDim), 0 if unused */
    int is_inequality; /* isInequalityConstraint (constraints.h:126); ignored by the bound kinds */
    const double* E;
    const double* G;
    const double* f;
    const double* lower;
    const double* upper;
    /* COPRA_CSTR_DENSE only (column-major, `rows` rows, is_inequality as above): LMPC reads A and b, InitialStateLMPC
     * reads Y, A and z */
    const double* A; /* rows x fullUDim */
    const double* b; /* rows */
    const double* Y; /* rows x xDim */
    const double* z; /* rows */
} copra_cstr_desc_t;

/* Dimensions of the preview systems of one batch: PreviewSystem::system(state, control, bias, xInit, numberOfSteps)
 * (src/PreviewSystem.cpp:16-55). */
typedef struct {
    int nx; /* xDim */
    int nu; /* uDim */
    int N; /* nrUStep */
    int batch; /* number of independent preview systems (instances) */
} copra_dims_t;

/* InitialStateLMPC::resetInitialStateCost(R, r) (src/InitialStateLMPC.cpp:35-40): R [nx x nx] positive definite, r [nx];
 * shared by the batch. */
typedef struct {
    const double* R;
    const double* r;
} copra_initial_state_desc_t;

typedef struct copra_batch copra_batch_t; /* opaque handle == one batched LMPC controller */

/* ---- engine options: every switch the engine consults, fixed when the controller is created (no environment
 *      variable is read by the library on any path; earlier rounds steered it through ~50 COPRA_* variables).  There is no reference
 *      counterpart: copra's LMPC has no tuning surface beyond selectQPSolver.  copra_options_init fills in the process-wide defaults
 *      (all zeros / "the engine decides" unless copra_set_default_options changed them); a caller sets `struct_size =
 *      sizeof(copra_options_t)` (done by copra_options_init) so that a library built against a longer struct keeps defaults for the
 *      fields the caller does not know.  Integer switches: 0 = off / engine's choice.  Results are the same under every setting --
 *      the options choose WHICH kernels run (tests pin each tier by switching the others off), never what they compute. ---- */
typedef struct {
    int struct_size;
    /* plan builder: classification of full-size entries as per-step entries */
    int no_stage_refs; /* block-diagonal full-size costs with repeating blocks stay dense Psi'WPsi contractions */
    int no_step_rows; /* full-size constraint rows inside one step keep the full-row machinery */
    int no_selection_rows; /* one-hot TrajectoryConstraint rows are not treated like TrajectoryBound rows */
    /* tier selection of the one-wave kernels */
    int no_ric; /* never the Riccati-factor tier (lmpc_fused_ric.hpp) */
    int no_tri; /* never a factor-only tier */
    int ric_general; /* Riccati-factor tier: the general variant even where the compact one applies */
    int no_dense_layout; /* run-time shapes: the safe compact layout instead of the densest one */
    int no_q1regs; /* factor-only tier with Q1 in LDS */
    int no_ladder; /* the layout ladder behaves as exhausted */
    int no_packed; /* small problems: one wavefront per instance instead of 16 / 32 lanes */
    int ric_k; /* Riccati-factor tier: start on the LDS-Q1 layout for this many instances per CU (0: Q1 in registers) */
    /* the one-instance-per-lane pass in front of the first tier (lmpc_lane.hpp) */
    int no_lane_pass;
    int no_lane_handover; /* the pass only filters; the tier sweeps itself */
    int no_lane_spec; /* the pass does not take the first step of the active-set iteration itself (a bound on u_0 as the first pick) */
    int no_lane_axes; /* the pass treats every system as dense: decoupled axes (FusedPlan::lane_axes -- state i on axis i % nu, control c on axis c, nothing
                         between them in A, B and the costs: the CoM model) are not looked for, no product is left out */
    int lane_min_batch; /* smallest batch that runs the pass (0: 20480 in front of the Riccati-factor tier, 4096 elsewhere; -1: any) */
    /* shared-model mode */
    int no_ric_shared; /* lmpc_shared.hpp instead of the Riccati-factor tier's shared-model mode */
    /* long horizons */
    int no_riccati; /* COPRA_SOLVER_DEFAULT keeps Goldfarb-Idnani where the Riccati interior-point kernel would be picked */
    int no_ric_fast; /* the streaming interior-point kernel instead of the LDS-resident one */
    double ric_step_tol, ric_mu_tol; /* interior-point tolerances (0: defaults of stage_plan.hpp) */
    /* misc */
    int debug; /* print launch geometry and adaptation decisions to stderr */
    /* (fields are only ever APPENDED from here on: a caller built against a shorter struct keeps its meaning, struct_size says how much it knows) */
    int no_axis_solver; /* never the one-(instance, axis)-per-lane solver (lmpc_axis.hpp; round 6): controllers whose axes are decoupled keep the
                           one-instance-per-lane pass + first tier */
} copra_options_t;
void copra_options_init(copra_options_t* opts);
/* the process-wide defaults copra_options_init hands out and the entry points without an options argument use (copra_batch_create,
 * copra_batch_create_initial_state, copra_plan_check, copra_qp_solve_dense_batch); NULL restores the built-in ones */
copra_status_t copra_set_default_options(const copra_options_t* opts);

/* ---- controller life cycle (replaces LMPC::LMPC / initializeController / addCost / addConstraint,
 *      src/LMPC.cpp:56-77, 118-128; dimension checks of costFunctions.cpp:44-61,88-98,122-137,173-193 and
 *      constraints.cpp:45-64,106-135,171-195,263-282,333-357 -> COPRA_ERR_DOMAIN) ---- */
copra_status_t copra_batch_create(copra_batch_t** out, const copra_dims_t* dims, int n_costs,
    const copra_cost_desc_t* costs, int n_cstrs, const copra_cstr_desc_t* cstrs);
/* the same with explicit engine options (`is` NULL: LMPC, else InitialStateLMPC as copra_batch_create_initial_state; `opts` NULL:
 * the process-wide defaults) */
copra_status_t copra_batch_create_with_options(copra_batch_t** out, const copra_dims_t* dims, int n_costs,
    const copra_cost_desc_t* costs, int n_cstrs, const copra_cstr_desc_t* cstrs, const copra_initial_state_desc_t* is,
    const copra_options_t* opts);
void copra_batch_destroy(copra_batch_t* h);

/* ---- how the controller is mapped onto the device: lanes that work on ONE instance -- 16 or 32 (several small
 *      problems share a 64-lane wavefront), 64 (one wavefront per instance) or the workgroup size of the
 *      workgroup-per-instance kernel (64 < decision variables <= 512). ---- */
int copra_batch_lanes_per_instance(const copra_batch_t* h);

/* ---- run-time specialisation: compile the kernels for THIS controller's (xDim, uDim, nrStep, cost rows) with
 *      `hipcc --genco` from the headers next to libcopra_hip.so (about 20-40 s, once per shape: the code object is kept in
 *      cache_dir, or $COPRA_JIT_CACHE, or ~/.cache/copra_amd when NULL; the compiler is $HIPCC or /opt/rocm/bin/hipcc -- the
 *      only environment the library reads, and only here) and use them from the next solve on.  The library
 *      ships such instantiations for the BASELINE shapes only; every other shape otherwise runs on the run-time-shape
 *      kernel, which is ~2.5x slower on the same problem.  A no-op (COPRA_OK) for shapes that already have dedicated
 *      kernels (BASELINE shapes, packed small problems, InitialStateLMPC, more than 64 variables).  Results are the
 *      same either way; COPRA_ERR_RUNTIME if hipcc is not available. ---- */
copra_status_t copra_batch_specialise(copra_batch_t* h, const char* cache_dir);
/* the same with a gate between compiler and loader: `check(path, user)` is called with the code object's path (cached or freshly
 * compiled) BEFORE hipModuleLoad; a non-zero answer deletes the object, leaves the handle exactly as it was (the library's kernels)
 * and returns COPRA_ERR_RUNTIME.  copra_amd/batch.py passes the matrix-instruction hazard lint (copra_amd/hazard_lint.py) here. */
typedef int (*copra_code_object_check_t)(const char* code_object_path, void* user);
copra_status_t copra_batch_specialise_checked(copra_batch_t* h, const char* cache_dir, copra_code_object_check_t check, void* user);

/* ---- the checks of copra_batch_create / copra_batch_create_initial_state WITHOUT touching the device: what
 *      LMPC::addCost / addConstraint do when they call initializeCost / initializeConstraint (src/LMPC.cpp:118-128).
 *      `is` may be NULL.  Returns COPRA_OK, COPRA_ERR_DOMAIN, COPRA_ERR_RUNTIME or COPRA_ERR_UNSUPPORTED. ---- */
copra_status_t copra_plan_check(const copra_dims_t* dims, int n_costs, const copra_cost_desc_t* costs, int n_cstrs,
    const copra_cstr_desc_t* cstrs, const copra_initial_state_desc_t* is);

/* ---- InitialStateLMPC variant (include/InitialStateLMPC.h:18-42, src/InitialStateLMPC.cpp): the decision vector is
 *      [x0; U]; costs contribute E and f, the Hessian is [[R + E Q^-1 E', E], [E', Q]] (InitialStateLMPC.cpp:77-122).
 *      Covered on the device for xDim + fullUDim <= 512 (xDim <= 16), per-step and full-size entries; other shapes
 *      COPRA_ERR_UNSUPPORTED.
 *      Initial-state bounds (resetInitialStateBounds, :42-46) are per instance, [batch][nx]; when they are never set
 *      both default to the x0 handed to copra_batch_set_system (InitialStateLMPC.cpp:20-28).
 *      copra_batch_get_initial_state == InitialStateLMPC::initialState() (:30-33), [batch][nx]. ---- */
copra_status_t copra_batch_create_initial_state(copra_batch_t** out, const copra_dims_t* dims, int n_costs,
    const copra_cost_desc_t* costs, int n_cstrs, const copra_cstr_desc_t* cstrs, const copra_initial_state_desc_t* is);
copra_status_t copra_batch_set_initial_state_bounds(copra_batch_t* h, const double* x0lb, const double* x0ub,
    int on_device);
copra_status_t copra_batch_get_initial_state(copra_batch_t* h, double* x0_opt);

/* ---- PreviewSystem::system / xInit for every instance (src/PreviewSystem.cpp:16-55, include/PreviewSystem.h:52).
 *      A [batch][nx x nx], B [batch][nx x nu], d [batch][nx], x0 [batch][nx].
 *      on_device != 0: the pointers are device pointers and are USED IN PLACE (they must stay valid until the next
 *      call); on_device == 0: host pointers, copied H2D into engine-owned HBM buffers. ---- */
copra_status_t copra_batch_set_system(copra_batch_t* h, const double* A, const double* B, const double* d,
    const double* x0, int on_device);
copra_status_t copra_batch_set_x0(copra_batch_t* h, const double* x0, int on_device);
/* ---- the same from ROW-major per-instance matrices that are already on the device (what C arrays and numpy hold; Eigen --
 *      src/PreviewSystem.cpp:16-55 takes Eigen matrices -- and every other entry point here are column-major): the library
 *      transposes A and B into buffers of its own with a kernel on `hip_stream` (no host-side layout conversion, nothing
 *      blocks); d and x0 are used in place.  For host pipelines that stage pinned buffers asynchronously. ---- */
copra_status_t copra_batch_set_system_rowmajor_async(copra_batch_t* h, const double* A, const double* B, const double* d,
    const double* x0, void* hip_stream);

/* ---- per-instance references: p of cost `cost_index` (the order of the `costs` array given at creation) for EVERY
 *      instance, [batch][rows] with the rows of that cost as created (per-step entry: r, full-size entry: r (N+1) or
 *      r N) -- each instance of the batch tracks its own goal / reference trajectory; in the reference this is one
 *      TrajectoryCost(M, p_b) / TargetCost / ControlCost / MixedCost object per LMPC (include/costFunctions.h:103-219).
 *      p == NULL restores the controller-wide p.  on_device != 0: used in place.  Works on the shared-model fast path
 *      too (the gradient is affine in p: c = c0 + C1 x0 + C2 p, probed once -- one column of C2 per entry of p, reference
 *      trajectories included; from 10 240 instances on, on the shapes of the Riccati-factor tier, the batch-wide stage records stay
 *      and every instance adds the delta of its feed-forward terms: 193 M solves/s with per-instance goals, 327 M with per-instance
 *      reference trajectories at the headline shape, profiles/r04/shared_goals.txt, shared_tracking.txt). ---- */
copra_status_t copra_batch_set_cost_reference(copra_batch_t* h, int cost_index, const double* p, int on_device);
/* ... and ONE new reference for every instance: p[rows] (rows as above -- a reference trajectory: r (N+1) or r N), host or device.
 *      The reference's API has no setter for p (include/costFunctions.h:103-219: a constructor argument): a tracking controller
 *      replaces the cost object and the next solve evaluates the new one (src/LMPC.cpp:233-247).  Here the new reference is written
 *      once per instance into the library's buffer (a broadcast on the device) and the per-instance path above is taken: no new
 *      plan, no new handle. */
copra_status_t copra_batch_set_cost_reference_all(copra_batch_t* h, int cost_index, const double* p, int on_device);
/*      Cost of that convenience: the controller is in per-instance-reference mode afterwards (until copra_batch_set_cost_reference(h,
 *      k, NULL, 0), which restores the reference given at CREATION).  In that mode a long-horizon controller runs the streaming
 *      interior-point kernel instead of the LDS-resident one (config 5: about 0.6 x the rate), a shared-model controller leaves the
 *      Riccati-factor tier's shared mode, and every call broadcasts batch x rows doubles.  Where that matters -- InitialStateLMPC /
 *      long horizons, shared-model ticks -- create a new controller with the new reference instead; the C++ and Python mirrors do so
 *      for controllers with more than 64 decision variables. */
/* ---- per-instance cost weights: the weights of cost `cost_index` (the order of the `costs` array given at creation) for EVERY instance,
 *      [batch][rows] with the rows of that cost as created, after the tiling of CostFunction::weights (per-step entry: r, full-size
 *      entry: r (N+1) or r N).  Replaces the reference's setter CostFunction::weights / weight (include/costFunctions.h:49-76), which a
 *      user calls between solves (src/LMPC.cpp:233-247 evaluates every cost anew): each instance of the batch gets its own weights, no new
 *      plan, no new handle.  w == NULL restores the weights given at creation.  on_device != 0: used in place (it must stay valid);
 *      otherwise copied into a buffer of the library.  A dense (host-evaluated) cost: COPRA_ERR_UNSUPPORTED.  A full-size cost with
 *      repeating blocks that the controller evaluates step by step (copra_options_t::no_stage_refs unset) needs weights that repeat
 *      along the horizon too: COPRA_ERR_DOMAIN otherwise; such a cost takes host weights only (COPRA_ERR_UNSUPPORTED with on_device).
 *      While any cost has per-instance weights, the (instance, axis)-per-lane solver runs its builds that rebuild their tables from each
 *      instance's weights where it has them (the headline's shape: xDim 6, uDim 3, N <= 20, tables the same along the horizon, creation
 *      weights non-zero); every other kernel that holds the creation weights in tables of the plan is not launched: other shapes of that
 *      solver, the one-instance-per-lane pass and the Riccati-factor tier give way to the generic one-wave kernels, long horizons run the
 *      Goldfarb-Idnani kernels; a controller that only the Riccati interior-point solver covers, or one
 *      forced onto it (copra_batch_select_solver), and a controller in shared-model mode (copra_batch_set_shared_system) return
 *      COPRA_ERR_UNSUPPORTED from copra_batch_solve -- a shared model written out per instance (the (instance, axis)-per-lane solver's
 *      case) solves as a batch.  Restoring every cost's weights gives the controller its kernels back. ---- */
copra_status_t copra_batch_set_cost_weights(copra_batch_t* h, int cost_index, const double* w, int on_device);

/* ---- per-instance constraint data.  copra_batch_set_constraint_rhs: f of the Trajectory / Control / Mixed constraint
 *      `cstr_index` (position in the `cstrs` array given at creation) for every instance, [batch][rows] with the rows
 *      of that constraint as created (per-step entry: r values used at every step; full-size entry: all of them) -- in
 *      the reference one TrajectoryConstraint(E, f_b) ... object per LMPC (include/constraints.h:114-226).
 *      copra_batch_set_control_bounds: lower / upper of the ControlBoundConstraint for every instance, [batch][fullUDim]
 *      (include/constraints.h:284-308).  TrajectoryBoundConstraint stays controller-wide (its infinite components
 *      are dropped at creation, src/constraints.cpp:263-282).  Both copy their input. ---- */
copra_status_t copra_batch_set_constraint_rhs(copra_batch_t* h, int cstr_index, const double* f, int on_device);
copra_status_t copra_batch_set_control_bounds(copra_batch_t* h, const double* lower, const double* upper, int on_device);

/* ---- shared-model receding-horizon fast path: ONE preview system (A [nx x nx], B [nx x nu], d [nx], column-major) for
 *      the whole batch; only x0 differs per instance (copra_batch_set_x0, [batch][nx]).  This is the reference's own
 *      receding-horizon use: PreviewSystem::xInit between solves with isUpdated left true (include/PreviewSystem.h:
 *      52-54, src/LMPC.cpp:233), where c = E'x0 + f and b = z - Y x0 carry the whole x0-dependence
 *      (src/costFunctions.cpp:80, src/constraints.cpp:81).  The preview matrices, the Hessian, its Cholesky factor and
 *      J = R^-1 are then computed ONCE (at the first copra_batch_solve after this call) and every solve only forms the
 *      free response and the gradient, copies J and runs the active-set loop.  LMPC with at most 64 decision variables;
 *      InitialStateLMPC / larger problems: COPRA_ERR_UNSUPPORTED.  Results are those of copra_batch_set_system with the
 *      same system replicated. ---- */
copra_status_t copra_batch_set_shared_system(copra_batch_t* h, const double* A, const double* B, const double* d,
    int on_device);

/* ---- LMPC::selectQPSolver(SolverFlag) (src/LMPC.cpp:62-65, include/solverUtils.h:34-50) for the batched controller.
 *      COPRA_SOLVER_DEFAULT (SolverFlag::DEFAULT): the engine picks -- the condensed Goldfarb-Idnani kernels up to 64
 *        decision variables, and for longer horizons the stage-wise Riccati interior-point kernel when every cost /
 *        constraint of the controller is stage-wise (per-step entries, block-diagonal full-size entries, at most 32
 *        equality rows), else the condensed workgroup-per-instance Goldfarb-Idnani kernel; instances the interior-point
 *        kernel does not converge on (infeasible ones) are finished by Goldfarb-Idnani, which sets their status.
 *      COPRA_SOLVER_QUADPROG_DENSE (SolverFlag::QuadProgDense): always the Goldfarb-Idnani kernels -- the arithmetic of
 *        the reference's QuadProgDense path, same active-set iteration counts as the CPU path.
 *      COPRA_SOLVER_RICCATI_IPM: force the interior-point kernel; COPRA_ERR_UNSUPPORTED when the controller is not
 *        stage-wise.
 *      Both solvers return the unique optimum of the same strictly convex QP: controls / trajectories agree to solver
 *      accuracy; status codes agree; iter[0] counts active-set iterations or Newton steps respectively.
 *      copra_batch_solver_info: which one the next copra_batch_solve runs (a copra_solver_t). ---- */
typedef enum { COPRA_SOLVER_DEFAULT = 0, COPRA_SOLVER_QUADPROG_DENSE = 1, COPRA_SOLVER_RICCATI_IPM = 2 } copra_solver_t;
copra_status_t copra_batch_select_solver(copra_batch_t* h, int solver);
int copra_batch_solver_info(const copra_batch_t* h);

/* ---- warm start of the active set across receding-horizon ticks on the shared-model path: with
 *      enable != 0 every instance remembers the active set it ended with, moved one step towards the present (the rows of
 *      step 0 leave), and its next solve takes those rows as the first candidates of the dual active-set method: while the
 *      list lasts, the next constraint to activate is the list's next row that is violated at the current iterate (one slack
 *      evaluation instead of a scan over all rows; the method may pick ANY violated constraint, its invariants hold
 *      throughout).  Same optimum and status as a cold start.  enable == 0 forgets the stored sets. ---- */
copra_status_t copra_batch_set_warm_start(copra_batch_t* h, int enable);

/* ---- optional: let the caller own the result buffers (device pointers, e.g. torch tensors that are later handed to
 *      an RCCL gather); must be called before copra_batch_solve and stay valid.  Sizes as in the results block. ---- */
copra_status_t copra_batch_set_outputs(copra_batch_t* h, double* control, double* trajectory, int* status, int* iter);

/* ---- LMPC::solve for every instance (src/LMPC.cpp:79-101): condensed-QP build + Goldfarb-Idnani solve +
 *      updateResults, one launch on `hip_stream` (a hipStream_t, may be NULL = default stream).  Asynchronous. ---- */
copra_status_t copra_batch_solve(copra_batch_t* h, void* hip_stream);
copra_status_t copra_batch_synchronize(copra_batch_t* h);

/* ---- results: LMPC::control() / trajectory() (include/LMPC.h:108-110), SI_fail / SI_iter
 *      (src/QuadProgSolver.cpp:14-22).  control [batch][nu*N], trajectory [batch][nx*(N+1)], status [batch],
 *      iter [batch][2] (main iterations, constraint drops).  Device-resident accessors return engine-owned HBM
 *      pointers valid for the lifetime of the handle.  A failed instance keeps NaN in control/trajectory. ---- */
const double* copra_batch_control_device(const copra_batch_t* h);
const double* copra_batch_trajectory_device(const copra_batch_t* h);
const int* copra_batch_status_device(const copra_batch_t* h);
const int* copra_batch_iter_device(const copra_batch_t* h);
copra_status_t copra_batch_get_results(copra_batch_t* h, double* control, double* trajectory, int* status, int* iter);

/* ---- the receding-horizon tick.  The reference's closed loop is  ps->xInit(x); lmpc.solve(); u = lmpc.control().head(nu); x = plant(x, u)
 *      (include/PreviewSystem.h:52, include/LMPC.h:108): copra_batch_advance replaces its last two steps and the xInit of the next tick for
 *      every instance, on the device.  With status / control the buffers the LAST LAUNCHED solve wrote (copra_batch_set_outputs honoured):
 *        ok = status[b] == COPRA_QP_OK;    u = ok ? control[b][0 .. nu) : fallback_u ? fallback_u[b] : none
 *        x+ = (ok || fallback_u) ? A[b] x0[b] + B[b] u + d[b] (+ w[b]) : x0[b]       -- no fallback: a failed instance KEEPS its state, bit for bit
 *        x0[b] <- x+;   x_out[b] = x+;   u_out[b] = u (NaN where the state was kept);   status_out[b] = status[b]
 *      The NaN a failed instance holds in `control` never reaches a state: the status is looked at first.  x+ always comes from the plant,
 *      never from trajectory[:, nx .. 2 nx): one rule whether or not plant and model differ.
 *      copra_plant_step_t: A, B, d are the plant -- device arrays in the layout of copra_batch_set_system, or ONE system for the batch
 *      (`shared`), or all NULL: the model the last solve read (per instance, or the one of copra_batch_set_shared_system).  Every pointer is
 *      a device pointer, used in place.  struct_size as in copra_options_t (set by copra_plant_step_init; fields are only ever appended).
 *      copra_batch_advance is asynchronous on `hip_stream` and ordered behind the solve.  The new state goes into a buffer of the LIBRARY,
 *      which becomes the controller's x0 (copra_batch_x0_device; copra_batch_get_x0 waits and copies it to the host): a device buffer the
 *      caller handed to copra_batch_set_x0 / copra_batch_set_system is read once more and never written.  A later copra_batch_set_x0 /
 *      copra_batch_set_system replaces the state as before.  `step` NULL: the model as plant, no disturbance, failed instances keep their state.
 *      copra_batch_rollout: `ticks` x (copra_batch_solve, copra_batch_advance) enqueued on one stream -- a Monte-Carlo closed-loop run in one
 *      call, no host synchronisation of its own (what copra_batch_solve does on a controller's first solves stays).  x_hist[0] is the state
 *      the first solve read, x_hist[t + 1] / u_hist[t] / status_hist[t] are x_out / u_out / status_out of tick t (a NULL history: the step's
 *      own pointer, overwritten every tick); w_seq[t] replaces step->w.  Device pointers.
 *      COPRA_ERR_RUNTIME: copra_batch_advance before any solve into the current result buffers; COPRA_ERR_UNSUPPORTED: an InitialStateLMPC
 *      controller (its x0 is a decision variable), a plant too wide for the LDS (xDim beyond about 130); COPRA_ERR_ARG: some but not all of
 *      A, B, d, ticks < 0, a NULL handle. ---- */
typedef struct {
    int struct_size; /* sizeof(copra_plant_step_t): append-only, as copra_options_t */
    const double *A, *B, *d; /* plant, device pointers; all NULL: the controller's model */
    int shared; /* A, B, d hold ONE system for the whole batch */
    const double* w; /* additive disturbance [batch][nx], device; NULL: none */
    const double* fallback_u; /* [batch][nu] applied where the solve failed; NULL: such an instance keeps its state */
    double* x_out; /* optional copies for the caller: [batch][nx], [batch][nu], [batch] */
    double* u_out;
    int* status_out;
    int* age_out; /* optional [batch], device: where the applied control came from (backup plans below) */
    int* age_hist; /* copra_batch_rollout only: [ticks][batch], device; tick t's age_out */
    int solve_every; /* copra_batch_rollout only: 0 or 1: a solve at every tick; k > 1: a solve at the ticks t with t % k == 0 */
} copra_plant_step_t;
void copra_plant_step_init(copra_plant_step_t* step);
copra_status_t copra_batch_advance(copra_batch_t* h, const copra_plant_step_t* step, void* hip_stream);
copra_status_t copra_batch_rollout(copra_batch_t* h, const copra_plant_step_t* step, int ticks, const double* w_seq, double* x_hist,
    double* u_hist, int* status_hist, void* hip_stream);
const double* copra_batch_x0_device(const copra_batch_t* h);
copra_status_t copra_batch_get_x0(copra_batch_t* h, double* x0);

/* ---- backup plans: what the tick does without a fresh solution (ABI 10).  A receding-horizon loop whose solve fails for a few ticks -- limits
 *      that tighten (limit schedules below) make that an ordinary event -- keeps applying the tail u_1, u_2, ... of the last plan that did
 *      solve until a solve succeeds again or the tail runs out; the reference's loop (include/LMPC.h:108) leaves that to its caller.
 *      copra_batch_set_backup_steps(h, K): K = 0 (the state of a new handle): off, the store is released, the tick is the one above.
 *      1 <= K <= N - 1: the library keeps per instance plan[b][K][nu], the controls of horizon steps 1 .. K of the instance's last successful
 *      solve, and an int next[b], the step of that plan the next tick without a fresh solution applies (0: no plan yet, > K: used up).
 *      A tick is FRESH when a copra_batch_solve has been launched since the previous copra_batch_advance (a flag of the handle: set by the
 *      solve, cleared by the advance).  With K > 0 the tick's rule for instance b is
 *        fresh && status[b] == COPRA_QP_OK :  u = control[b][0 .. nu);  plan[b][j-1] = control[b][j nu .. (j+1) nu), j = 1 .. K;
 *                                             next[b] = 1;  age = 0
 *        else if 1 <= next[b] <= K         :  u = plan[b][next[b] - 1];  age = next[b];  next[b] += 1
 *        else if fallback_u                :  u = fallback_u[b];  age = COPRA_PLAN_FALLBACK  (next[b] unchanged)
 *        else                              :  the state is kept bit for bit, u_out[b] = NaN;  age = COPRA_PLAN_HELD
 *      and x+ = A[b] x0[b] + B[b] u + d[b] (+ w[b]) in the first three cases, exactly as above: the plan is applied to the PLANT, nothing is
 *      taken from the model's trajectory.  The control of an instance whose solve failed holds NaN and is still never loaded, neither its
 *      first nu entries nor its tail.  age_out[b] (optional) receives `age`.  status_out stays the content of the status buffer: on a tick
 *      without a solve that is the LAST solve's status, so it is stale -- age_out is what says where a control came from.
 *      With K = 0 age_out receives 0 / COPRA_PLAN_FALLBACK / COPRA_PLAN_HELD by the three cases of the tick above, and `fresh` is not looked
 *      at: a second copra_batch_advance without a solve applies u_0 again.
 *      EVERY call forgets all plans (next <- 0, asynchronously on the stream of the last solve / tick), also one that repeats the K in force.
 *      copra_batch_set_x0 and copra_batch_set_system do NOT touch the plans: a caller that starts a new episode calls
 *      copra_batch_set_backup_steps again.
 *      Multi-rate loops: copra_batch_rollout with copra_plant_step_t::solve_every = k > 1 launches a solve at the ticks t with t % k == 0
 *      only; the ticks in between play the plan (ages 1 .. k - 1), the plant and the tick counter of the schedules move at every tick, so the
 *      next solve reads the right window.  It needs K >= k - 1.  age_hist[t] is tick t's age_out.  copra_batch_advance ignores solve_every and
 *      age_hist.
 *      COPRA_ERR_ARG: K outside 0 .. N - 1, a NULL handle, solve_every < 0, solve_every = k > 1 with K < k - 1; COPRA_ERR_UNSUPPORTED: an
 *      InitialStateLMPC controller (as for the tick itself). ---- */
#define COPRA_PLAN_FALLBACK (-1) /* age_out: fallback_u was applied */
#define COPRA_PLAN_HELD (-2) /* age_out: the state was kept */
copra_status_t copra_batch_set_backup_steps(copra_batch_t* h, int steps);

/* ---- disturbance estimator: an offset-free tick (ABI 11).  The tick has taken a plant that differs from the model since ABI 7, but every
 *      solve predicted with the d the caller set once: under a constant load or a mismatched plant every instance settles away from its
 *      goal.  The reference leaves the correction to its caller, who changes the bias of the PreviewSystem between solves
 *      (src/PreviewSystem.cpp:16-55).  Here the tick learns the difference itself, per instance, with the full state measured.  For
 *      instance b, after the new state is formed, with dhat the d the controller's model holds for b and Am, Bm that model's A, B:
 *        x+      = what the tick stores as the next state (plant, applied control, w)                          -- unchanged
 *        pred_r  = dhat_r + sum_j Am[r,j] x_j + sum_c Bm[r,c] u_c        -- the controller's MODEL, no w; u = the control the tick applied
 *        e_r     = x+_r - pred_r
 *        dhat+_r = dhat_r + sum_j L[r,j] e_j   (dense gain)      |      dhat_r + l_r e_r   (diagonal gain)
 *      dhat+ is the d the next copra_batch_solve reads for that instance.  u is whatever the tick applied: the fresh control, a step of
 *      the backup plan, or fallback_u.  An instance whose state is HELD (no control applied) keeps dhat bit for bit, as it keeps x.  With
 *      no plant given (copra_plant_step_t::A == NULL) the plant is the model with its current dhat, so e = w up to rounding: defined
 *      behaviour, not an error.  With L = I and plant = model + a constant c, dhat = d + c after one tick, up to rounding, and the loop is
 *      the nominal loop from then on.  Nothing is clamped and nothing is forgotten.
 *      copra_batch_set_bias_estimator(h, gain, dense, per_instance, on_device): gain is [per_instance ? batch : 1][nx] with dense == 0 and
 *      [per_instance ? batch : 1][nx x nx], column-major, with dense != 0.  A host gain is copied (the call synchronises the stream of the
 *      last solve / tick once); with on_device != 0 it is used in place and must stay valid.  Turning the estimator on, the library takes
 *      a buffer of its OWN, [batch][nx], seeds it with a stream-ordered copy of the d in force and makes it the controller's d: a device
 *      buffer the caller gave to copra_batch_set_system / copra_batch_set_system_rowmajor_async is read for that copy and never written,
 *      and neither is the library's copy of a host d.  A call while the estimator is on replaces the gain and keeps the estimates.
 *      gain == NULL ends the estimator; the last estimates stay the model's d, as a schedule's last window stays.
 *      copra_batch_set_system / copra_batch_set_system_rowmajor_async while the estimator is on keep it on: the estimates restart from the
 *      new d, which is copied, not adopted.  copra_batch_set_shared_system ENDS the estimator: one d for the batch cannot hold
 *      per-instance estimates.  A fleet that shares one model and wants estimates writes the model out with copra_batch_set_system.
 *      copra_batch_set_bias(h, d, on_device): d [batch][nx] replaces the estimates -- a new episode (stream-ordered with on_device != 0).
 *      copra_batch_bias_device: the buffer the next solve reads as d (the library's while the estimates are in force).
 *      copra_batch_get_bias waits for the last tick and copies [batch][nx] to the host.
 *      The tick hands the estimates out through copra_plant_step_ex_t: copra_plant_step_t with two fields appended behind it, in memory
 *      exactly the struct of ABI 10 grown at its end (append-only, as ever) -- under a name of its own, so that copra_plant_step_t and
 *      copra_plant_step_init keep the size every caller compiled against ABI 10 has.  copra_plant_step_ex_init zeroes it and sets
 *      step.struct_size = sizeof(copra_plant_step_ex_t); copra_batch_advance / copra_batch_rollout take a pointer to it as the pointer to its
 *      first member (&ex.step), and struct_size tells them which of the two they were given.
 *      d_out, optional [batch][nx]: dhat+ of the tick (dhat of a held instance); ignored while the estimator is off.
 *      d_hist, copra_batch_rollout only: [ticks][batch][nx], tick t's d_out.  The tick neither synchronises nor allocates.
 *      COPRA_ERR_ARG: a NULL handle, copra_batch_set_bias / copra_batch_get_bias with a NULL d.  COPRA_ERR_RUNTIME: no system has been set
 *      yet; copra_batch_set_bias while the library's estimates are not the d in force (the estimator was never on, or a system was set
 *      after it ended).  COPRA_ERR_UNSUPPORTED: an InitialStateLMPC controller; a handle whose model came from
 *      copra_batch_set_shared_system, whether or not the library wrote it out per instance; an instance whose model, plant and gain do
 *      not fit the LDS. ---- */
typedef struct {
    copra_plant_step_t step; /* first: its struct_size is sizeof(copra_plant_step_ex_t) */
    double* d_out; /* optional [batch][nx], device: the disturbance estimates after the tick; ignored while the estimator is off */
    double* d_hist; /* copra_batch_rollout only: [ticks][batch][nx], device; tick t's d_out */
} copra_plant_step_ex_t;
void copra_plant_step_ex_init(copra_plant_step_ex_t* step);
copra_status_t copra_batch_set_bias_estimator(copra_batch_t* h, const double* gain, int dense, int per_instance, int on_device);
copra_status_t copra_batch_set_bias(copra_batch_t* h, const double* d, int on_device);
const double* copra_batch_bias_device(const copra_batch_t* h);
copra_status_t copra_batch_get_bias(copra_batch_t* h, double* d);

/* ---- output feedback: a state observer in the tick (ABI 12).  Everything above takes the state the plant step writes for the state the
 *      next solve reads: the full state is measured.  A machine gives y = C x + v with fewer outputs than states, and the reference's loop
 *      (include/LMPC.h:108, include/PreviewSystem.h:52) leaves the observer between measurement and xInit to its caller.  Here the tick
 *      runs it, in the same launch.  The plant gets a state of its OWN, xp [batch][nx], a buffer of the library; the controller's x0 becomes
 *      the ESTIMATE xhat.  For instance b, with dhat the controller's d, Am, Bm the controller's model, Ap, Bp, dp the plant (the step's, or
 *      the model with d = dhat when the step gives none) and u the control the tick applied -- chosen exactly as above: fresh solution,
 *      backup plan, fallback_u, or none:
 *        xp+   = Ap xp + Bp u + dp (+ w)                  the plant moves its OWN state, not xhat
 *        y     = C xp+ (+ v)                              ny outputs; v optional [batch][ny]; or y = y_meas[b] (below)
 *        xpred = Am xhat + Bm u + dhat                    the model's prediction, no w  (the `pred` of the disturbance estimator)
 *        inn   = y - C xpred                              ny innovations
 *        xhat+ = xpred + Lx inn                           Lx [nx x ny]
 *        dhat+ = dhat + Ld inn                            Ld [nx x ny], optional
 *        x0 <- xhat+ ;  d <- dhat+                        the next solve reads both
 *      An instance to which no control was applied is HELD: xp, xhat and dhat keep their bits, its y_out row is C xp (+ v) of the unchanged
 *      state.  With C = I, Lx = I, Ld = L and no v this is the disturbance estimator above, up to rounding.  All matrices column-major.
 *      copra_batch_set_observer(h, ny, C, Lx, Ld, per_instance, on_device): C is [ny x nx], Lx and Ld are [nx x ny], each given once for
 *      the batch or, with per_instance != 0, [batch] times (one flag for all three).  Host arrays are copied (the call synchronises the
 *      stream of the last solve / tick once); device arrays are used in place and must stay valid.  Ld == NULL: a state observer only -- d
 *      is not touched and no buffer is taken for it.  With Ld the library takes its buffer of estimates and seeds it exactly as
 *      copra_batch_set_bias_estimator does; copra_batch_set_bias, copra_batch_get_bias and copra_batch_bias_device work on it.  Turning the
 *      observer on seeds xp with a stream-ordered copy of the x0 in force.  A call while the observer is on replaces C and the gains and
 *      keeps xp, xhat and dhat.  C == NULL ends the observer: x0 and d stay as the last tick left them.
 *      copra_batch_set_plant_state(h, x, on_device) / copra_batch_plant_state_device / copra_batch_get_plant_state handle the true state
 *      xp, [batch][nx].  copra_batch_set_x0 keeps its meaning: it sets the controller's x0, which is now the estimate.  A new episode sets
 *      both.
 *      copra_plant_step_obs_t is copra_plant_step_ex_t as its first member with the observer's fields appended (append-only; the two
 *      smaller structs keep their fields and sizes, struct_size tells the three apart; copra_plant_step_obs_init zeroes it and sets
 *      ex.step.struct_size).  While the observer is on x_out / x_hist are the plant's state xp -- the truth, what they have always held --,
 *      x_hist[0] is xp before the first tick, xhat_out is xhat+ and xhat_hist[t] the estimate the solve of tick t + 1 reads, y_out / y_hist[t]
 *      the outputs y, v_seq[t] replaces v.  While the observer is off the new fields are ignored.
 *      y_meas (copra_batch_advance only): the caller's measurement of a REAL plant after it applied u.  No plant is simulated: xp is neither
 *      read nor written, x_out is not written, the step's plant, w and v are ignored; everything from xpred on is as above (y_out receives
 *      y_meas).  copra_batch_rollout with y_meas != NULL returns COPRA_ERR_ARG.
 *      The observer and the disturbance estimator exclude each other: whichever is asked for second gets COPRA_ERR_RUNTIME.  Backup plans,
 *      solve_every and all schedules are untouched: they decide u and the windows, not the state.  copra_batch_set_system keeps the observer
 *      on (with Ld, dhat restarts from the new d, as for the estimator); copra_batch_set_shared_system ends it.
 *      COPRA_ERR_ARG: a NULL handle, ny < 1 (ny > nx is no error: redundant sensors exist), C without Lx, a NULL x for
 *      copra_batch_set_plant_state / copra_batch_get_plant_state.  COPRA_ERR_RUNTIME: no system or no x0 set yet; the plant-state calls
 *      while the observer was never on.  COPRA_ERR_UNSUPPORTED: an InitialStateLMPC controller; a handle whose model came from
 *      copra_batch_set_shared_system; an instance whose image does not fit the LDS. ---- */
typedef struct {
    copra_plant_step_ex_t ex; /* first: ex.step.struct_size is sizeof(copra_plant_step_obs_t) */
    const double* v; /* optional sensor noise [batch][ny], device */
    const double* y_meas; /* copra_batch_advance only: measured outputs [batch][ny], device; no plant is simulated */
    double* y_out; /* optional [batch][ny], device: the outputs the observer read */
    double* xhat_out; /* optional [batch][nx], device: the estimates after the tick */
    const double* v_seq; /* copra_batch_rollout only: [ticks][batch][ny], device; tick t's replaces v */
    double* y_hist; /* copra_batch_rollout only: [ticks][batch][ny], device; tick t's y_out */
    double* xhat_hist; /* copra_batch_rollout only: [ticks][batch][nx], device; tick t's xhat_out */
} copra_plant_step_obs_t;
void copra_plant_step_obs_init(copra_plant_step_obs_t* step);
copra_status_t copra_batch_set_observer(copra_batch_t* h, int ny, const double* C, const double* Lx, const double* Ld, int per_instance, int on_device);
copra_status_t copra_batch_set_plant_state(copra_batch_t* h, const double* x, int on_device);
const double* copra_batch_plant_state_device(const copra_batch_t* h);
copra_status_t copra_batch_get_plant_state(copra_batch_t* h, double* x);

/* ---- Monte-Carlo ticks: process and sensor noise drawn on the device (ABI 13).  w and v above are arrays the caller fills; a rollout of
 *      many ticks needs [ticks][batch][nx] of them, and a C caller has no generator.  copra_batch_set_noise makes the plant step draw them
 *      itself, inside its launch, from a counter-based generator -- Philox4x32-10 -- so that the draw of instance b at noise tick t depends
 *      on (seed, first_instance + b, stream, row, t) and on nothing else: not on the batch, the launch, or the GPU a shard of a larger
 *      batch runs on, and the same seed gives the same noise to every controller variant (common random numbers).  It costs no memory.
 *      Rows 2j and 2j + 1 of instance b share one call; stream s is 0 for process noise w, 1 for sensor noise v:
 *        key     = (seed & 0xffffffff, seed >> 32)
 *        counter = ((first_instance + b) & 0xffffffff, (s << 16) | j, t & 0xffffffff, t >> 32)        -> words o0 .. o3
 *        u1 = (((o0 << 32 | o1) >> 12) + 0.5) 2^-52,  u2 likewise from (o2, o3);   rad = sqrt(-2 log u1),  ang = 6.283185307179586 u2
 *        n[2j] = rad cos ang,  n[2j + 1] = rad sin ang          (an odd number of rows drops the last sin)
 *      The noise term of row r is sigma[r] n[r], rounded once; the tick uses w = term where the step gives no w and w = w_given + term
 *      where it does (w_seq of a rollout included), and v likewise.  With y_meas no v exists and none is drawn.  An instance whose state
 *      is held shows no process noise; draws are indexed by tick, so no other draw moves.
 *      copra_batch_set_noise(h, noise): sigma_w is [nx] or, with per_instance != 0, [batch][nx]; sigma_v [ny] or [batch][ny] (one flag
 *      for both).  Host arrays are copied (the call synchronises the stream of the last solve / tick once), device arrays (on_device != 0)
 *      are used in place and must stay valid.  noise == NULL or both sigmas NULL: off.  first_instance is the global index of this
 *      handle's instance 0 where a batch is spread over several handles; first_instance + batch <= 2^32.
 *      The handle keeps a NOISE TICK of its own, apart from the schedule tick (replicas share schedules, not seeds): every plant step --
 *      copra_batch_advance, every tick of copra_batch_rollout, with or without a solve -- adds one; copra_batch_set_noise sets it to 0,
 *      copra_batch_noise_seek to `tick`; copra_batch_set_x0, copra_batch_set_system and the schedule calls leave it alone.
 *      copra_batch_draw_noise writes the terms of one tick and one stream (0: process, 1: sensor) to out_device, [batch][nx] or [batch][ny],
 *      on hip_stream: bit for bit what the plant step of that noise tick adds.  The tick neither synchronises nor allocates for the noise.
 *      Turning the observer off while sigma_v is set drops the sensor noise; turning it on again with another ny returns
 *      COPRA_ERR_RUNTIME until copra_batch_set_noise is called again.
 *      COPRA_ERR_ARG: a NULL handle; a negative or NaN sigma in a host array; first_instance + batch > 2^32; a stream outside {0, 1}; a
 *      NULL out_device.  COPRA_ERR_RUNTIME: sigma_v, or stream 1, while the observer is off; copra_batch_draw_noise for a stream whose
 *      sigma is not set.  COPRA_ERR_UNSUPPORTED: an InitialStateLMPC controller. ---- */
typedef struct {
    int struct_size; /* append-only, set by copra_noise_init */
    unsigned long long seed;
    unsigned long long first_instance; /* global index of this handle's instance 0 (shards) */
    const double* sigma_w; /* [nx] or [batch][nx]; NULL: no process noise */
    const double* sigma_v; /* [ny] or [batch][ny]; NULL: no sensor noise */
    int per_instance; /* one flag for both */
    int on_device; /* used in place, must stay valid; else copied */
} copra_noise_t;
void copra_noise_init(copra_noise_t* noise);
copra_status_t copra_batch_set_noise(copra_batch_t* h, const copra_noise_t* noise);
copra_status_t copra_batch_noise_seek(copra_batch_t* h, unsigned long long tick);
unsigned long long copra_batch_noise_tick(const copra_batch_t* h);
copra_status_t copra_batch_draw_noise(copra_batch_t* h, unsigned long long tick, int stream, double* out_device, void* hip_stream);

/* ---- closed-loop scores: the tick keeps score (ABI 14).  A closed-loop study wants a few numbers per instance -- the accumulated stage
 *      cost, how often and how badly limits were violated on the TRUE state, how many ticks were held or ran on a backup plan -- and their
 *      distribution over the batch; taken from x_hist / u_hist they cost [ticks][batch][nx + nu] doubles and a caller without an array
 *      library a loop on the host.  Here the caller hands the measure over once (copra_batch_set_score); every copra_batch_advance and every
 *      tick of copra_batch_rollout then updates one 64-byte record per instance on the device, in a kernel of its own behind the plant step
 *      on the same stream, and copra_batch_score_summary reduces the records to a few hundred bytes, reproducibly.  No history is needed.
 *      The measure, copra_score_t (append-only, struct_size set by copra_score_init):
 *        qx       weights of the state term: [nx] with dense == 0, [nx x nx] column-major with dense != 0; NULL: no state term
 *        ru       weights of the control term: [nu] or [nu x nu] likewise (dense is one flag for both); NULL: none
 *        x_ref    the reference signal of the state term, [per_instance ? batch : 1][ref_steps][nx]; NULL: zero.  ref_steps == 1: a constant
 *                 goal.  The row read for the state after a tick is min(tau, ref_steps - 1), tau the handle's schedule tick AFTER that
 *                 tick's tau += 1 (copra_batch_schedule_tick; copra_batch_schedule_seek moves it with the other schedules): a state at
 *                 schedule time tau is compared with the block a reference trajectory's window shows at its step 0 at that tau.
 *        x_lo, x_hi [nx], u_lo, u_hi [nu]   box limits, each may be NULL; infinite entries are allowed as in copra_batch_set_control_bounds
 *        tol >= 0   a tick counts as violating when its largest violation exceeds tol
 *        per_instance   one flag for every array: each is then given [batch] times
 *        on_device      the arrays are used in place and must stay valid; otherwise they are copied and the stream of the last solve /
 *                       tick is synchronised once
 *      The update, after the plant step of a tick, for instance b.  x is the true state after the tick: the plant's xp+ while the observer
 *      simulates a plant; the estimate xhat+ on a y_meas tick, where no truth exists; otherwise the new x0.  u is the control the tick
 *      applied, age what age_out reports.  Rows within an instance are taken in ASCENDING order, every sum starts from 0.0:
 *        e_r  = x_r - x_ref_r
 *        lx   = sum_r (qx_r e_r) e_r   |   sum_r e_r (sum_j Qx[r,j] e_j)            (diagonal | dense)
 *        lu   = sum_c (ru_c u_c) u_c   |   sum_c u_c (sum_j Ru[c,j] u_j)            where a control was applied, else 0
 *        v_r  = max(0, lo_r - z_r, z_r - hi_r) over the rows of x, then of u (a held instance has no u rows); comparisons with `>`: a NaN
 *               row counts 0;   vmax = max_r v_r
 *        jx += lx;  ju += lu;  viol_sum += sum_r v_r;  viol_max = max(viol_max, vmax);  peak = max(peak, lx + lu);  ticks += 1
 *        held += (age == COPRA_PLAN_HELD);  replayed += (age >= 1);  fallback += (age == COPRA_PLAN_FALLBACK)
 *        if vmax > tol:  violating += 1;  if first_violation == 0: first_violation = ticks    (the 1-based tick of the first violation
 *                                                                                               since the last reset; 0: none)
 *      A held instance is scored on its unchanged state -- time passes and the robot sits there -- and its ju keeps its bits: the NaN its
 *      u_out row holds is never added, by the discipline the tick has for a failed instance's control.  A NaN state or reference makes that
 *      instance's jx NaN: defined behaviour, the summary counts it out.  peak and viol_max ignore a NaN (`>` again).
 *      The record, copra_score_record_t: 64 bytes per instance, all-zero bytes are the initial state.
 *      Lifetime: copra_batch_set_score takes the record buffer and zeroes it (on the stream of the last solve / tick); a call while scoring is on
 *      replaces the measure and zeroes the records; copra_batch_set_score(h, NULL) ends scoring and releases the buffers;
 *      copra_batch_score_reset zeroes the records in stream order -- a new episode.  copra_batch_set_x0, copra_batch_set_system, the
 *      schedule calls, copra_batch_set_noise and copra_batch_set_backup_steps leave the records alone.  copra_batch_score_device returns the
 *      records on the device (NULL while scoring is off); copra_batch_get_score waits for the last tick and copies [batch] records.
 *      Scoring works with backup plans, solve_every, the estimator, the observer, noise and every schedule: they decide x, u and age, the
 *      score only reads them.  u and age are the tick's own u_out / age_out (u_hist[t] / age_hist[t] of a rollout); where the caller gives
 *      none the tick writes them to buffers the setter took.  The tick neither synchronises nor allocates for the score; while scoring was
 *      never enabled the tick launches exactly what it launched in ABI 13.
 *      The summary: copra_batch_score_summary waits for the last tick and reduces the records on the device.  For each of the five double
 *      fields a copra_score_stat_t over the records whose field is FINITE: n, mean, m2 (the sum of squared deviations from the mean;
 *      variance = m2 / (n - 1)), min, max, argmin, argmax (ties: the lowest index); with n == 0: mean = m2 = 0, min = +inf, max = -inf,
 *      arg = -1.  Then the batch totals of ticks, held, replayed, fallback, violating, and instances_violating / instances_held: the number
 *      of records whose counter is not zero -- the first is the Monte-Carlo estimate of the probability of a violation.
 *      No floating-point atomics: partial statistics a, b are merged with the pairwise update
 *        delta = mean_b - mean_a;  n = n_a + n_b;  mean = mean_a + delta n_b / n;  m2 = m2_a + m2_b + delta^2 n_a n_b / n
 *      (an empty side returns the other unchanged) in an order that depends on the batch size alone, never on the grid, the occupancy or
 *      the run, so that two summaries of the same records are equal bit for bit:
 *        stage 1: chunk c is records [1024 c, 1024 (c + 1)), one workgroup of 256 threads each.  Thread t merges, from the empty statistic,
 *                 records 1024 c + t, + 256, + 512, + 768 in ascending order; inside each wave of 64 lanes, for off = 32, 16, 8, 4, 2, 1,
 *                 lane l <- merge(lane l, lane l + off); thread 0 merges the four waves in ascending order, (((w0, w1), w2), w3).
 *        stage 2: one workgroup over the chunks' partials: thread t merges partials t, t + 256, ... in ascending order, then the same lane
 *                 tree and fold of the waves.
 *      COPRA_ERR_ARG: a NULL handle; ref_steps < 1 with an x_ref; a negative or NaN tol; a NaN weight or lo > hi in a host array; a NULL
 *      destination.  COPRA_ERR_RUNTIME: reset, get or summary while scoring is not on.  COPRA_ERR_UNSUPPORTED: an InitialStateLMPC
 *      controller, as for the tick itself; an instance whose image does not fit the LDS. ---- */
typedef struct {
    int struct_size; /* append-only, set by copra_score_init */
    const double* qx; /* [nx] or [nx x nx]; NULL: no state term */
    const double* ru; /* [nu] or [nu x nu]; NULL: no control term */
    int dense; /* one flag for both weights */
    const double* x_ref; /* [per_instance ? batch : 1][ref_steps][nx]; NULL: zero */
    long long ref_steps;
    const double* x_lo; /* [nx]; NULL: none */
    const double* x_hi;
    const double* u_lo; /* [nu]; NULL: none */
    const double* u_hi;
    double tol;
    int per_instance; /* one flag for every array */
    int on_device; /* used in place, must stay valid; else copied */
} copra_score_t;
typedef struct {
    double jx, ju, viol_sum, viol_max, peak;
    int ticks, held, replayed, fallback, violating, first_violation;
} copra_score_record_t;
typedef struct {
    long long n;
    double mean, m2, min, max;
    long long argmin, argmax;
} copra_score_stat_t;
typedef struct {
    copra_score_stat_t jx, ju, viol_sum, viol_max, peak;
    long long ticks, held, replayed, fallback, violating;
    long long instances_violating, instances_held;
} copra_score_summary_t;
void copra_score_init(copra_score_t* score);
copra_status_t copra_batch_set_score(copra_batch_t* h, const copra_score_t* score);
copra_status_t copra_batch_score_reset(copra_batch_t* h);
const copra_score_record_t* copra_batch_score_device(const copra_batch_t* h);
copra_status_t copra_batch_get_score(copra_batch_t* h, copra_score_record_t* host);
copra_status_t copra_batch_score_summary(copra_batch_t* h, copra_score_summary_t* out);

/* ---- steady-state targets: the references follow d and a setpoint (ABI 15).  The estimator and the observer make the model's d right; an
 *      offset-free loop also needs the target calculator, which recomputes the steady state (xs, us) that is consistent with the model, its
 *      current d and the setpoint, and makes it the reference of the costs: a TrajectoryCost towards a goal beside a ControlCost whose
 *      reference is zero pull against each other under a constant load, because the equilibrium control is not zero.  Here the caller hands
 *      the controlled outputs, the setpoint signal and the driven costs over once (copra_batch_set_target) and a kernel of its own keeps the
 *      references right on the device, in stream order.  Per instance b, with n = nx + nu and nr == nu:
 *        M = [ A - I   B ]      rhs = [ -d ]        M z = rhs,   z = [xs ; us]
 *            [   H     0 ]            [  r ]
 *        p_c[s r_c + i] = (T_c z)[i]      for every driven cost c, every block s = 0 .. S_c - 1, every row i = 0 .. r_c - 1
 *      A, B, d are the controller's model in force -- d the estimates while the estimator or the observer's Ld is on.  r is block
 *      min(tau + offset, steps - 1) of the setpoint signal, tau the schedule tick (copra_batch_schedule_tick).  T_c = cost_map[c] is
 *      [cost_rows[c] x n] column-major and shared by the batch; for the step forms of the four cost kinds it is [M_c N_c] (a missing M or N:
 *      zeros), so that p = M xs + N us.  S_c = (rows of the cost as created) / cost_rows[c], the rule of copra_batch_set_reference_schedule.
 *      The blocks are written into the per-instance references the solve reads: the driven costs go into per-instance-reference mode, as
 *      copra_batch_set_cost_reference_all puts them there, every instance starting from the reference in force.
 *      The solve: Gaussian elimination with partial pivoting on [M | rhs] -- the pivot of column k is the entry of largest magnitude among
 *      rows k .. n - 1, ties to the LOWEST row (for a double integrator A - I has a zero diagonal: without pivoting the first pivot is 0);
 *      f = M_ik / M_kk, M_ij = M_ij - f M_kj for j = k + 1 .. n ASCENDING; back substitution acc = rhs_i, acc = acc - M_ij z_j for
 *      j = i + 1 .. n - 1 ASCENDING, z_i = acc / M_ii; a reference row is ((0.0 + T[i,0] z_0) + T[i,1] z_1) + ...  (target_step.hpp).
 *      An instance is SINGULAR when a pivot has |pivot| <= n 2^-52 max|M_ij| or M or rhs holds a non-finite value: target_status[b] = 1,
 *      its references and its stored z keep their bits, nothing of its neighbours changes.  Otherwise target_status[b] = 0.
 *      The kernel is stateless -- it factorises from A, B, H every time, nothing cached can go stale -- and is launched, stream-ordered,
 *      without a synchronisation or an allocation, by: every copra_batch_advance and every tick of copra_batch_rollout, behind the plant
 *      step (which moves d), the tick counter's += 1, the score and the schedule windows; copra_batch_set_target itself, on the stream of
 *      the last solve / tick, so that the first solve is right; copra_batch_schedule_seek; copra_batch_set_bias; copra_batch_set_system
 *      and copra_batch_set_system_rowmajor_async.  Held instances are computed like any other: their r may move.  While targets were never
 *      enabled every one of these launches exactly what it launched in ABI 14.
 *      A driven cost cannot also follow a reference schedule: copra_batch_set_target on a cost with a live schedule is COPRA_ERR_RUNTIME; a
 *      later copra_batch_set_reference_schedule or copra_batch_set_cost_reference[_all] on a driven cost takes it off the target's list.
 *      copra_batch_set_target(h, NULL) ends the targets and keeps the last references; copra_batch_set_shared_system ends them too.
 *      copra_batch_target_device / _target_status_device: z [batch][nx + nu] and the status [batch] on the device (NULL while off);
 *      copra_batch_get_target waits for the last tick and copies; z or status may be NULL.  copra_batch_get_cost_reference waits likewise and
 *      copies the per-instance reference of cost `cost_index` in force, [batch][rows of the cost as created] -- what this kernel, a
 *      schedule's window or copra_batch_set_cost_reference[_all] wrote; COPRA_ERR_RUNTIME while the controller-wide reference is in force.
 *      COPRA_ERR_ARG: a NULL handle, steps < 1, offset < 0, n_costs outside 1 .. 8, no such cost (or one cost twice), a NULL array.
 *      COPRA_ERR_DOMAIN: nr != uDim; cost_rows[c] does not divide the cost's rows.  COPRA_ERR_RUNTIME: no system set yet; a driven cost
 *      with a live schedule; copra_batch_get_target while targets are off.  COPRA_ERR_UNSUPPORTED: an InitialStateLMPC controller; a model
 *      from copra_batch_set_shared_system, which has one d; a dense (host-evaluated) cost, or a full-size cost the controller does not
 *      evaluate step by step; systems of one wave (64 instances) that do not fit the LDS (xDim + uDim beyond about 16). ---- */
typedef struct {
    int struct_size; /* append-only, set by copra_target_init */
    int nr; /* must equal uDim */
    const double* H; /* [nr x nx] column-major, one for the batch */
    const double* r; /* [per_instance ? batch : 1][steps][nr] */
    long long steps;
    int offset;
    int per_instance;
    int n_costs; /* 1 .. 8 driven costs */
    const int* cost_index;
    const int* cost_rows;
    const double* const* cost_map; /* T_c [cost_rows[c] x (nx + nu)] column-major */
    int on_device; /* H, r, cost_map[*] are device arrays used in place; else copied (one synchronisation) */
} copra_target_t;
void copra_target_init(copra_target_t* target);
copra_status_t copra_batch_set_target(copra_batch_t* h, const copra_target_t* target);
const double* copra_batch_target_device(const copra_batch_t* h);
const int* copra_batch_target_status_device(const copra_batch_t* h);
copra_status_t copra_batch_get_target(copra_batch_t* h, double* z, int* status);
copra_status_t copra_batch_get_cost_reference(copra_batch_t* h, int cost_index, double* p);

/* ---- input delay in the tick: command queue and state predictor (ABI 16).  Every tick above assumes that the control computed from the state
 *      at tick t reaches the plant at tick t.  In a real loop the solve, the bus and the drive take time: the command computed at t acts at
 *      t + D.  The remedy is to queue the commands already issued and to hand the solver the state PREDICTED for the time its command will
 *      act.  The reference leaves this to its caller, like everything between control() and xInit() (include/LMPC.h:108,
 *      include/PreviewSystem.h:52); here copra_batch_set_input_delay(h, D, u_init, on_device), 0 <= D <= COPRA_DELAY_MAX, puts it into the tick.
 *      D = 0 is the state of a new handle: delay is off, the buffers are released and the tick is the one of ABI 15.
 *      With D >= 1 the library keeps per instance b
 *        q[b][D][nu]   a ring of pending commands          qs[D][batch]   the status of the solve that issued each pending command
 *        xnow[b][nx]   the state AT THE CURRENT TICK: the measured state, or with the observer the estimate xhat
 *      and one handle-wide `head`, the slot applied next: every instance pops and pushes exactly one entry per tick.
 *      What the solve reads: the controller's x0 (copra_batch_x0_device, copra_batch_get_x0) becomes the PREDICTION.  Start from xnow and
 *      walk the D pending entries, oldest first, with the controller's MODEL (the A, B, d in force, per instance or the one system of
 *      copra_batch_set_shared_system; d the estimates where the estimator or the observer's Ld is on) and no w, each entry by the plant
 *      step's own rule:
 *        status == COPRA_QP_OK          x <- Am x + Bm u + d        (the row sum in the order of the plant step)
 *        else, this step has fallback_u the same with u = fallback_u[b]
 *        else                           x is kept: the plant will hold that instance at that tick
 *      A tick (copra_batch_advance, every tick of copra_batch_rollout), for instance b:
 *        1. the plant step runs as above, reading q[b][head] and qs[head][b] in place of control[b][0 .. nu) and status[b], and xnow in place
 *           of x0 (xhat = xnow with the observer).  u_out, age_out and status_out therefore describe the command that REACHED THE PLANT,
 *           issued D ticks ago; the estimator and the observer see the applied control; x_out, x_hist and the score's truth stay the
 *           current true state (the plant's xp while the observer simulates one, else xnow).
 *        2. a kernel of its own, ordered behind it, writes the last launched solve's control[b][0 .. nu) and status[b] into slot head --
 *           the status is looked at first, a failed instance's control is never loaded and its slot holds NaN; `fresh` is not looked at,
 *           as with K = 0 -- advances head, forms the prediction from the updated xnow, d and queue and stores it as the controller's x0.
 *      u_init is [batch][nu] (NULL: zeros) and fills all D slots with status COPRA_QP_OK.  Every call of the setter resets the queue, one
 *      that repeats the D in force included.  When delay is turned on xnow is seeded by a stream-ordered copy of the x0 in force (a caller's
 *      device buffer is read once and never written); a call while it is on keeps xnow.  The setter launches the first prediction.  It
 *      synchronises the stream of the last solve / tick once; the tick neither synchronises nor allocates.
 *      copra_batch_set_x0, copra_batch_set_bias, copra_batch_set_system and copra_batch_set_system_rowmajor_async while delay is on keep
 *      the queue, set xnow / d / the model and predict again, with the same kernel and its push off (no step: failed entries count as held).
 *      copra_batch_set_shared_system keeps delay on; the prediction then reads the one system.  D = 0 makes xnow the x0 again.
 *      copra_batch_set_observer while delay is on seeds the plant's own state from xnow, the state in force, not from the prediction.
 *      copra_batch_input_delay: the D in force (-1: NULL handle).  copra_batch_delay_state_device / copra_batch_get_delay_state: xnow
 *      [batch][nx].  copra_batch_get_delay_queue waits for the last tick and copies the queue OLDEST FIRST, q [batch][D][nu] and status
 *      [batch][D] (either may be NULL); copra_batch_delay_queue_device gives the ring as it lies on the device -- q [batch][D][nu],
 *      status [D][batch] -- with the slot `head` of the oldest entry; entry j, oldest first, is slot (head + j) % D.
 *      A real plant: copra_batch_advance with y_meas works unchanged.  It needs the observer (C = I, Lx = I is full-state measurement): the
 *      caller applies u_out, the popped command, and measures.
 *      Schedules: the schedules' tick is untouched.  The solve at tick t plans from time t + D: a delayed loop passes offset + D to
 *      copra_batch_set_reference_schedule, copra_batch_set_constraint_schedule, copra_batch_set_control_bound_schedule and
 *      copra_target_t::offset.  The score's reference needs no shift: it is compared with the current true state.
 *      Not covered yet (follow-ups): delay together with backup plans (K > 0) or solve_every > 1 -- the plan store reads the tail of
 *      `control` with its stride; whichever is asked for second gets COPRA_ERR_RUNTIME --, per-instance delays, fractional delays, and
 *      fusing the push and the prediction into the plant step's launch.
 *      COPRA_ERR_ARG: a NULL handle, D outside 0 .. 8, a NULL destination.  COPRA_ERR_RUNTIME: no system or no x0 set yet, the getters
 *      while delay is off, the exclusion above.  COPRA_ERR_UNSUPPORTED: an InitialStateLMPC controller, as for the tick itself; an
 *      instance whose image does not fit the LDS. ---- */
#define COPRA_DELAY_MAX 8
copra_status_t copra_batch_set_input_delay(copra_batch_t* h, int steps, const double* u_init, int on_device);
int copra_batch_input_delay(const copra_batch_t* h);
const double* copra_batch_delay_state_device(const copra_batch_t* h);
copra_status_t copra_batch_get_delay_state(copra_batch_t* h, double* x);
copra_status_t copra_batch_delay_queue_device(const copra_batch_t* h, const double** q, const int** status, int* head);
copra_status_t copra_batch_get_delay_queue(copra_batch_t* h, double* q, int* status);

/* ---- ensemble traces: per-tick fleet statistics on the device (ABI 17).  The scores above reduce a run to one record per instance: how
 *      each robot did over the whole run.  A Monte-Carlo study also asks how the FLEET looked at tick t -- the mean, spread and extremes of
 *      every state and control, the share violating a limit, the share held or on a backup plan, the observer's ensemble error -- which
 *      otherwise takes x_hist / u_hist / age_hist / xhat_hist off the device.  A trace is a buffer of `capacity` slots on the device; every
 *      recorded tick reduces the batch into the next slot, behind the score on the tick's stream.
 *      The slot: one copra_trace_head_t (64 bytes), then `rows` copra_score_stat_t in the order x, u, err, viol -- the groups `what` names
 *      and, where any limit is given, ONE row viol: 64 + 56 rows bytes.
 *        COPRA_TRACE_X    nx rows: the true state after the tick -- the state the score reads: the plant's own while the observer
 *                         simulates one, the estimate on a y_meas tick, xnow under an input delay, otherwise the new x0
 *        COPRA_TRACE_U    nu rows: the applied control (u_out); a HELD instance has none -- its age decides, its NaN row is never read
 *        COPRA_TRACE_ERR  nx rows: estimate - plant state (one subtraction; the estimate of the same tick, xnow under delay) on ticks where
 *                         the observer simulates a plant; on every other tick the rows are empty statistics
 *        viol             vmax, the score's own rule: the largest of max(0, lo_r - z_r, z_r - hi_r) over the rows of x, then of u (held: no
 *                         u rows); comparisons with `>` from 0.0, so a NaN row counts 0
 *      A row's statistic is over the instances whose value is FINITE, as in the summary: n, mean, m2, min, max, argmin, argmax (ties: the
 *      lowest index); with n == 0: mean = m2 = 0, min = +inf, max = -inf, arg = -1.
 *      The head: tick, the trace's own tick count since the last set or reset (0 for the first); tau, the schedule tick after that tick;
 *      solved = #(age == 0), replayed = #(age >= 1), fallback = #(age == COPRA_PLAN_FALLBACK), held = #(age == COPRA_PLAN_HELD) -- they sum
 *      to the batch --; violating = #(vmax > tol), 0 without limits; reserved = 0.
 *      The reduction order is the contract.  Row r of a recorded tick is reduced exactly as copra_batch_score_summary reduces a field, with
 *      "record i" read as "instance i's value of row r":
 *        stage 1: chunk c is instances [1024 c, 1024 (c + 1)), one workgroup of 256 threads each.  Thread t merges, from the empty statistic,
 *                 instances 1024 c + t, + 256, + 512, + 768 in ascending order; inside each wave of 64 lanes, for off = 32, 16, 8, 4, 2, 1,
 *                 lane l <- merge(lane l, lane l + off); thread 0 merges the four waves in ascending order, (((w0, w1), w2), w3).
 *        stage 2: one workgroup over the chunks' partials: thread t merges partials t, t + 256, ... in ascending order, then the same lane
 *                 tree and fold of the waves.
 *      The head counts are integer sums through the same tree.  No floating-point atomics, no counter on the device: two traces of the
 *      same run are equal byte for byte, whatever the grid or the occupancy.
 *      Which ticks: with t the trace's tick count, the ticks with t % every == 0 are recorded (every == 0 means 1).  t moves at every tick
 *      while tracing is on.  A tick never fails because the trace is full: further ticks are not recorded and `missed` counts them.
 *      Lifetime: copra_batch_set_trace takes the slots, the partials and -- for ticks where neither the caller nor the score supplies u_out /
 *      age_out -- buffers for them; it waits for the handle's last stream once.  A call while tracing is on replaces the trace and restarts
 *      it; copra_batch_set_trace(h, NULL) ends tracing and releases the buffers; copra_batch_trace_reset takes the tick count back to 0 in
 *      stream order: the next recorded tick writes slot 0 behind everything launched before.  copra_batch_trace_info reports the slots
 *      recorded, the ticks missed, the rows and the bytes of a slot (each pointer may be NULL); copra_batch_trace_device returns the slots
 *      on the device (NULL while tracing is off); copra_batch_get_trace waits for the last tick and copies slots [first, first + count).
 *      The tick: two launches per recorded tick behind the score and before the schedule windows, no synchronisation, no allocation;
 *      while tracing was never enabled the tick launches exactly what it launched in ABI 16.  Tracing works with backup plans, solve_every,
 *      the estimator, the observer and y_meas, noise, scores, targets, input delay, every schedule and the shared model: it only reads what
 *      they decided.  Limits on the device (on_device) are used in place and must stay valid; host limits are copied.
 *      Not covered yet (follow-ups): per-instance limits or a reference signal in the trace, and a one-launch variant in which the last
 *      workgroup does stage 2.
 *      COPRA_ERR_ARG: a NULL handle, capacity < 1, no (or an unknown) `what` bit, every < 0, a negative or NaN tol, lo > hi or a NaN limit
 *      in a host array, a NULL destination, first / count outside the recorded slots.  COPRA_ERR_RUNTIME: reset, info or get while tracing
 *      is off.  COPRA_ERR_UNSUPPORTED: an InitialStateLMPC controller, as for the tick itself. ---- */
#define COPRA_TRACE_X 1
#define COPRA_TRACE_U 2
#define COPRA_TRACE_ERR 4
typedef struct {
    int struct_size; /* append-only, set by copra_trace_init */
    long long capacity; /* recorded ticks the trace holds, >= 1 */
    int what; /* COPRA_TRACE_* bits, at least one */
    int every; /* record the ticks t with t % every == 0 (0 means 1) */
    const double* x_lo; /* [nx], one for the batch; NULL: none */
    const double* x_hi;
    const double* u_lo; /* [nu] likewise; any limit given adds ONE row viol and the count violating */
    const double* u_hi;
    double tol; /* >= 0 */
    int on_device; /* limits used in place, must stay valid; else copied */
} copra_trace_t;
typedef struct {
    long long tick, tau, solved, replayed, fallback, held, violating, reserved;
} copra_trace_head_t;
void copra_trace_init(copra_trace_t* trace);
copra_status_t copra_batch_set_trace(copra_batch_t* h, const copra_trace_t* trace);
copra_status_t copra_batch_trace_reset(copra_batch_t* h);
copra_status_t copra_batch_trace_info(const copra_batch_t* h, long long* recorded, long long* missed, int* rows, long long* slot_bytes);
const void* copra_batch_trace_device(const copra_batch_t* h);
copra_status_t copra_batch_get_trace(copra_batch_t* h, long long first, long long count, void* host);

/* ---- trace quantiles: exact per-tick fleet percentiles on the device (ABI 18).  A slot's mean and spread are a band for a Gaussian row; a
 *      velocity against its bound or the violation row, zero for most of the fleet, is none, and the extremes are one robot each.  With
 *      copra_batch_set_trace_quantiles every recorded tick also selects, for every row of the slot and each of `count` levels, an order
 *      statistic of the row -- where 5 %, 50 % and 95 % of the fleet lie -- without x_hist / u_hist leaving the device.
 *      The rule.  For a recorded tick and row r of the slot -- the same rows in the same order x | u | err | viol, the same values the slot's
 *      statistic is made of: a held instance has no u rows, no instance has err rows off an observer tick, viol is vmax --
 *        V    the instances whose value is finite; n = |V| is the n of the row's statistic in the slot
 *        key  V is ordered ascending by the key of the value's 64 bits b:  key = b ^ (b >> 63 ? ~0ull : 1ull << 63)  -- numeric order, with
 *             -0.0 before +0.0
 *        k    for a level p:  c = ceil(p * (double)n), one FP64 multiply, then ceil;  k = min(n - 1, max(0, c - 1));  the quantile is the
 *             k-th element, 0-based.  p = 0 gives the minimum, p = 1 the maximum, p = 0.5 with n even the lower median (numpy's
 *             method="inverted_cdf")
 *        n == 0: the quiet NaN with bits 0x7FF8000000000000
 *      An order statistic is an element of the data: the result has one right set of bytes, whatever the grid or the occupancy.
 *      Levels: at most COPRA_TRACE_QUANT_MAX, each finite in [0, 1]; they need not be sorted and may repeat.  `levels` is a host array.
 *      The buffer: [capacity][rows][count] doubles beside the slots; slot k of one belongs to slot k of the other.
 *      Lifetime: copra_batch_set_trace_quantiles needs tracing on; it waits for the handle's last stream once, takes the buffer and the key
 *      buffer the kernel works in ([rows][batch] 64-bit keys) and RESTARTS the trace -- tick count, recorded and missed go to 0 --, so every
 *      recorded slot has its quantiles.  levels == NULL or count == 0 ends quantiles and keeps the trace and its slots.  Quantiles belong to
 *      the trace in force: copra_batch_set_trace, whether it replaces the trace or ends it with NULL, ends them too;
 *      copra_batch_trace_reset keeps them.  copra_batch_trace_quantile_info reports the levels (`levels` has room for
 *      COPRA_TRACE_QUANT_MAX, entries past count are 0; each pointer may be NULL); copra_batch_trace_quantiles_device returns the buffer
 *      (NULL while quantiles are off); copra_batch_get_trace_quantiles waits for the last tick and copies slots [first, first + count),
 *      checked against the recorded slots as copra_batch_get_trace checks them.
 *      The tick: a recorded tick launches ONE kernel more behind the trace's two, on the tick's stream, into the slot the host counted: one
 *      workgroup per row, a radix select on the key, eight passes of eight bits over histograms in LDS (integer atomics).  No
 *      synchronisation, no allocation, no counter on the device, no floating-point atomics.  A full trace records nothing further, a tick
 *      that `every` skips launches nothing, and while quantiles were never enabled the tick launches what it launched in ABI 17.
 *      Exact quantiles of shards do not merge: there is no counterpart of merging two slots.
 *      COPRA_ERR_ARG: a NULL handle, count outside 0 .. COPRA_TRACE_QUANT_MAX, a level that is NaN or outside [0, 1], a NULL destination,
 *      first / count outside the recorded slots.  COPRA_ERR_RUNTIME: tracing off; info or get while quantiles are off. ---- */
#define COPRA_TRACE_QUANT_MAX 8
copra_status_t copra_batch_set_trace_quantiles(copra_batch_t* h, const double* levels, int count);
copra_status_t copra_batch_trace_quantile_info(const copra_batch_t* h, int* count, double* levels /* [COPRA_TRACE_QUANT_MAX], may be NULL */);
const double* copra_batch_trace_quantiles_device(const copra_batch_t* h);
copra_status_t copra_batch_get_trace_quantiles(copra_batch_t* h, long long first, long long count, double* host);

/* ---- reference schedules: tracking inside the tick.  The reference's API has no setter for a cost's p (include/costFunctions.h:103-219: a
 *      constructor argument); a tracking loop replaces the cost object every tick and the next solve evaluates the new one
 *      (src/LMPC.cpp:233-247).  Here the caller hands the whole reference SIGNAL of cost `cost_index` over once,
 *      sched [per_instance ? batch : 1][steps][r] doubles, and the library moves the window the horizon sees by one step per tick, on the
 *      device, in stream order.  With S = (rows of that cost as created) / r and tau the controller's tick counter, the next solve reads for
 *      instance b
 *        p[b][s r + i] = sched[b or 0][min(tau + offset + s, steps - 1)][i],   s = 0 .. S-1
 *      (the last block is held beyond the end of the schedule).  A reference trajectory -- a full-size TrajectoryCost -- has r = xDim,
 *      S = N + 1, offset 0; a full-size ControlCost / MixedCost S = N; a per-step cost (a goal that moves) S = 1; a TargetCost S = 1 and
 *      offset = N (the goal of the horizon's end).
 *      The window is written into the library's per-instance reference buffer, which becomes the cost's reference: the state
 *      copra_batch_set_cost_reference_all leaves (same remarks on the per-instance-reference mode), every kernel reads it unchanged.
 *      copra_batch_set_reference_schedule writes the window of the current tau at once, on the stream of the last solve / tick; it
 *      synchronises that stream once when it copies a host schedule, never with on_device != 0 (the schedule is then used in place and
 *      must stay valid).  sched == NULL ends the schedule and keeps the last window; copra_batch_set_cost_reference and
 *      copra_batch_set_cost_reference_all on that cost end it too (p == NULL: back to the creation reference).
 *      The tick: copra_batch_advance does tau += 1 for the controller -- all instances share tau; a failed instance keeps its state, but
 *      time moves on -- and writes, behind the plant step on the same stream, the new windows of all scheduled costs with ONE launch: no
 *      host synchronisation, no allocation.  copra_batch_rollout therefore tracks.  copra_batch_schedule_seek: tau <- tick and the windows
 *      rewritten, ordered on the stream of the last solve / tick, no synchronisation.  copra_batch_schedule_tick: tau (-1: NULL handle).
 *      COPRA_ERR_DOMAIN: r does not divide the cost's rows, or the controller evaluates a full-size cost step by step and r is not the rows
 *      of one step; COPRA_ERR_ARG: steps < 1, offset < 0, no such cost, a NULL handle, a negative tick; COPRA_ERR_UNSUPPORTED: a dense
 *      (host-evaluated) cost, more than 8 scheduled costs. ---- */
copra_status_t copra_batch_set_reference_schedule(copra_batch_t* h, int cost_index, const double* sched, long long steps, int r, int offset,
    int per_instance, int on_device);
copra_status_t copra_batch_schedule_seek(copra_batch_t* h, long long tick);
long long copra_batch_schedule_tick(const copra_batch_t* h);

/* ---- limit schedules: moving limits inside the tick (ABI 9).  The reference has no setter for a constraint's limits either
 *      (include/constraints.h:114-308: constructor arguments; ControlBoundConstraint: :272-308): a loop whose actuator derates, whose speed
 *      limit tightens or whose corridor moves replaces the constraint object between solves, and the next solve evaluates the new one
 *      (src/LMPC.cpp:233-247).  Here the caller hands the limit SIGNAL over once and the library moves the window the horizon sees by one
 *      step per tick, on the device, in stream order, with the tick counter tau of the reference schedules (copra_batch_advance: tau += 1;
 *      copra_batch_schedule_seek: tau <- tick, reference AND limit windows rewritten; copra_batch_schedule_tick unchanged).
 *      copra_batch_set_constraint_schedule: sched [per_instance ? batch : 1][steps][r] are the right-hand sides f of the Trajectory / Control /
 *      Mixed constraint `cstr_index` (position in the array given at creation).  A per-step entry (E with xDim / G with uDim columns) has
 *      r = its rows and S = its steps (N + 1 with a state part, else N); a full-size entry any r that divides its rows, S = rows / r.  With
 *      first = min(tau + offset, steps - 1) the next solve reads for instance b, for s = 0 .. S-1,
 *        f[b][s r + i] = sched[b or 0][preview ? min(tau + offset + s, steps - 1) : first][i]
 *      preview != 0: the horizon sees the future limits (the last block is held beyond the end of the schedule); preview == 0: the limit of
 *      the present tick at every step -- the case the (instance, axis)-per-lane solver keeps in registers; with preview an instance whose
 *      window varies along the horizon is solved by the tier behind it.
 *      copra_batch_set_control_bound_schedule: lower and upper, each [per_instance ? batch : 1][steps][uDim], become the bounds of the
 *      controller's ControlBoundConstraint by the same formula with r = uDim, S = N; both are needed; infinite entries are allowed as in
 *      copra_batch_set_control_bounds.
 *      The windows are written into the per-instance limits copra_batch_set_constraint_rhs / copra_batch_set_control_bounds write (on first
 *      use every instance starts from the controller-wide right-hand sides; rows of other constraints are never touched) -- every kernel
 *      reads them unchanged.  Both setters write the window of the current tau at once, on the stream of the last solve / tick; they
 *      synchronise that stream once when they copy a host schedule, never with on_device != 0 (the schedule is then used in place and must
 *      stay valid).  sched == NULL (lower == NULL and upper == NULL) ends the schedule and keeps the last window (where one was live it waits
 *      for that stream first: the schedule may be freed on return);
 *      copra_batch_set_constraint_rhs on that constraint and copra_batch_set_control_bounds end it too (they wait for the stream first where
 *      a schedule was live).  The tick writes all live limit windows with ONE launch behind the reference windows: no host synchronisation,
 *      no allocation.  Reference schedules and limit schedules coexist.
 *      Once a limit schedule has been set (live, or ended with its last window kept) the (instance, axis)-per-lane solver runs only where
 *      both of its builds read per-instance limits.
 *      COPRA_ERR_DOMAIN: r does not fit as above; COPRA_ERR_ARG: steps < 1, offset < 0, no such constraint, a NULL handle, exactly one of
 *      lower / upper; COPRA_ERR_UNSUPPORTED: a bound constraint or a dense constraint as `cstr_index`, a controller without a
 *      ControlBoundConstraint, more than 8 live limit windows (lower and upper count as one each). ---- */
copra_status_t copra_batch_set_constraint_schedule(copra_batch_t* h, int cstr_index, const double* sched, long long steps, int r, int offset,
    int preview, int per_instance, int on_device);
copra_status_t copra_batch_set_control_bound_schedule(copra_batch_t* h, const double* lower, const double* upper, long long steps, int offset,
    int preview, int per_instance, int on_device);

/* ---- parity hooks: the dense QP of one instance as LMPC exposes it (include/LMPC.h:112-127: Q c Aineq bineq Aeq
 *      beq lb ub), rebuilt ON THE DEVICE by the same condense code the solver runs.  Any pointer may be NULL.
 *      Q [n x n], c [n], Aeq [neq x n], beq [neq], Aineq [nineq x n], bineq [nineq], lb [n], ub [n]. ---- */
copra_status_t copra_batch_qp_sizes(const copra_batch_t* h, int* nvar, int* neq, int* nineq);
copra_status_t copra_batch_dump_qp(copra_batch_t* h, int instance, double* Q, double* c, double* Aeq, double* beq,
    double* Aineq, double* bineq, double* lb, double* ub);

/* ---- how the next copra_batch_solve maps instances to the GPU (no reference counterpart; for tests and tuning):
 *      LDS bytes per instance of the first launch, number of active constraints that launch has room for (instances
 *      that need more finish in a second launch), 1 if it keeps only the Cholesky factor (no inverse factor),
 *      1 if a second launch exists.  The first solves of a controller may step to a roomier layout. ---- */
copra_status_t copra_batch_layout_info(const copra_batch_t* h, int* lds_bytes, int* active_capacity, int* factor_only,
    int* two_tier);

/* ---- timing contract of LMPC::solveTime()/solveAndBuildTime() (src/LMPC.cpp:82-99, 108-116): device time of the
 *      last copra_batch_solve in seconds (hipEvent pair on the launch stream); whole batch, EVERY launch of the solve (the
 *      second launch, which only sees the instances whose active set outgrew the first one's layout, included).  For the
 *      one-wave kernels the events ride in the dispatch packets of the launches themselves; copra_options_t::recorded_events
 *      brackets the solve with recorded events instead. ---- */
copra_status_t copra_batch_last_solve_seconds(copra_batch_t* h, double* seconds);
/* ---- the first launch of that solve alone (no reference counterpart: the figure a kernel profile -- rocprofv3 -- of the
 *      dominant kernel is compared with); equals copra_batch_last_solve_seconds where the solve is not timed per launch. ---- */
copra_status_t copra_batch_last_first_tier_seconds(copra_batch_t* h, double* seconds);
/* ---- the one-instance-per-lane pass of the last solve (no reference counterpart; for tests, tuning and the bench line).  For a
 *      controller whose costs are all per-step entries (src/costFunctions.cpp:63-215) the unconstrained minimiser qpgen2 starts from
 *      is the LQ roll-out of one Riccati sweep; a pass in front of the first tier does that sweep and roll-out for the whole batch
 *      with one instance per LANE, finishes every instance whose minimiser violates no constraint (what QuadProgDense::solve returns
 *      after its first scan, src/QuadProgSolver.cpp:45-72) and hands the factor of the others to the first tier.
 *      ran: 1 if the last solve ran it, 2 if it ran the one-(instance, axis)-per-lane solver instead (lmpc_axis.hpp, round 6: controllers whose
 *      axes are decoupled -- the WHOLE solve per lane; what it cannot finish goes to the first tier the same way); finished: the instances that
 *      ended in it (waits for the solve; NULL: not asked for). ---- */
copra_status_t copra_batch_lane_pass_info(copra_batch_t* h, int* ran, int* finished);
/*      Whether the pass runs is decided per controller from the batch size (from 20480 instances on in front of the Riccati-factor
 *      tier, 4096 elsewhere) and, where it only filters, from the share of instances that ended in it in the first two solves --
 *      sampled again every 256 solves.  Which instances the pass or the tier finish does not change statuses or iteration counts,
 *      but the two evaluate the unconstrained minimiser in different orders of summation: results are reproducible to rounding
 *      (1e-11 relative), not bit for bit, across batch sizes and across the solves around such a decision. */

/* ---- device-side split of that time: per-instance shader-clock cycles of the 7 phases of the fused kernel
 *      (preview, costs, norms, cholesky, inverse+x0, active set, result stores) + total; 8 values per instance.
 *      enable != 0 turns the stamps on for subsequent solves; cycles_out (host, [batch][8]) may be NULL. ---- */
copra_status_t copra_batch_phase_profile(copra_batch_t* h, int enable, long long* cycles_out);

/* ---- plug-in point 1, batched: QuadProgDenseSolver::SI_problem + SI_solve (src/QuadProgSolver.cpp:45-72) for
 *      `batch` independent dense QPs  min 1/2 x'Qx + c'x  s.t. Aeq x = beq, Aineq x <= bineq, XL <= x <= XU.
 *      Q [batch][n x n] (upper triangle read), c [batch][n], Aeq [batch][neq x n], beq [batch][neq],
 *      Aineq [batch][nineq x n], bineq [batch][nineq], XL/XU [batch][n]; outputs x [batch][n], fail [batch]
 *      (SI_fail), iter [batch][2].  on_device selects host or device pointers for ALL arrays.
 *      n <= 64: one QP per wavefront, Q/J/R in LDS; 64 < n <= 512: one QP per workgroup, J/R in an HBM workspace
 *      (the call then allocates that workspace and synchronises the stream); n > 512: COPRA_ERR_UNSUPPORTED. ---- */
copra_status_t copra_qp_solve_dense_batch(int batch, int n, int neq, int nineq, const double* Q, const double* c,
    const double* Aeq, const double* beq, const double* Aineq, const double* bineq, const double* XL,
    const double* XU, double* x, int* fail, int* iter, int on_device, void* hip_stream);

/* ---- PreviewSystem::updateSystem (src/PreviewSystem.cpp:57-74) for ONE system, on the device: Phi [fullXDim x xDim],
 *      Psi [fullXDim x fullUDim], xi [fullXDim], column-major host buffers.  The solve path never materialises them (they
 *      only exist block-wise in LDS); this entry point serves host-evaluated user subclasses of Constraint / CostFunction,
 *      whose update(const PreviewSystem&) reads ps.Phi / ps.Psi / ps.xi. ---- */
copra_status_t copra_preview_update(int nx, int nu, int N, const double* A, const double* B, const double* d, double* Phi,
    double* Psi, double* xi);

/* ---- misc ---- */
/* ---- run-time specialisation of the dense-QP kernel for problems with `n` variables (n <= 64): as
 *      copra_batch_specialise; later copra_qp_solve_dense_batch calls with that n use the compiled kernels. ---- */
copra_status_t copra_qp_dense_specialise(int n, const char* cache_dir);

const char* copra_last_error(void);
copra_status_t copra_device_info(int* n_devices, int* cu_count, char* arch_name, int arch_name_len);
int copra_abi_version(void);
/* sha1 over the sources this library was built from (copra_amd/csrc/Makefile: COPRA_SRC_HASH; the same value keys the cache of run-time-
 * compiled kernels): what a committed profile records so that a benchmark can tell whether the counters it quotes were taken on THIS build */
const char* copra_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* COPRA_HIP_H */
