// Ensemble traces from a C / C++ caller that has no array library and touches no device memory: the fleet of double integrators of
// tests/cpp/test_score.cpp through include/copra_hip.h alone.  One handle runs copra_batch_rollout WITHOUT any history with a trace of x, u and
// the viol row and reads copra_batch_get_trace; a twin runs the same ticks one by one (solve, get_results, advance, get_x0) and forms the same
// statistics of every tick on the host.  n, the head counts and the args must agree exactly, min / max and the means to 1e-8 relative -- a rollout
// and the same loop with read-outs in between agree to 1e-9 in their states (tests/test_closed_loop_gpu.py).  Prints one slot.  Built and run by
// tests/test_trace_gpu.py.
#include <copra_hip.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#define CHECK(expr)                                                                          \
    do {                                                                                     \
        const copra_status_t rc_ = (expr);                                                   \
        if (rc_ != COPRA_OK) {                                                               \
            std::printf("%s: %d (%s)\n", #expr, (int)rc_, copra_last_error());               \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

static_assert(sizeof(copra_trace_head_t) == 64 && sizeof(copra_score_stat_t) == 56, "a slot is 64 + 56 rows bytes");

int main()
{
    const int batch = 70, N = 8, ticks = 6, nx = 2, nu = 1, stuck = 3, rows = nx + nu + 1;
    const double dt = 0.1, inf = std::numeric_limits<double>::infinity();
    std::vector<double> A((size_t)batch * 4), B((size_t)batch * 2), d((size_t)batch * 2, 0.0), x0((size_t)batch * 2);
    for (int b = 0; b < batch; ++b) {
        double* a = &A[(size_t)b * 4]; // column-major [[1, dt], [0, 1]]
        a[0] = 1.0, a[1] = 0.0, a[2] = dt, a[3] = 1.0;
        B[(size_t)b * 2] = 0.5 * dt * dt * (1.0 + 0.01 * b), B[(size_t)b * 2 + 1] = dt * (1.0 + 0.01 * b);
        x0[(size_t)b * 2] = 0.2 + 0.01 * b, x0[(size_t)b * 2 + 1] = 0.0;
    }
    x0[(size_t)stuck * 2 + 1] = 50.0; // far outside the velocity bound: infeasible at every tick, its state is held
    double I2[4] = { 1, 0, 0, 1 }, I1[1] = { 1 }, goal[2] = { 1.0, 0.0 }, wx[2] = { 10.0, 1.0 }, zero1[1] = { 0 }, wu[1] = { 1e-2 };
    double xlow[2] = { -inf, -inf }, xup[2] = { inf, 1.0 }, ulow[1] = { -5.0 }, uup[1] = { 5.0 };
    copra_cost_desc_t costs[2] = {};
    costs[0].kind = COPRA_COST_TRAJECTORY, costs[0].rows = 2, costs[0].m_cols = 2, costs[0].M = I2, costs[0].p = goal, costs[0].weights = wx;
    costs[1].kind = COPRA_COST_CONTROL, costs[1].rows = 1, costs[1].n_cols = 1, costs[1].N = I1, costs[1].p = zero1, costs[1].weights = wu;
    copra_cstr_desc_t cstrs[2] = {};
    cstrs[0].kind = COPRA_CSTR_TRAJECTORY_BOUND, cstrs[0].rows = 2, cstrs[0].lower = xlow, cstrs[0].upper = xup;
    cstrs[1].kind = COPRA_CSTR_CONTROL_BOUND, cstrs[1].rows = 1, cstrs[1].lower = ulow, cstrs[1].upper = uup;
    const copra_dims_t dims = { nx, nu, N, batch };
    copra_batch_t *h = nullptr, *twin = nullptr;
    CHECK(copra_batch_create(&h, &dims, 2, costs, 2, cstrs));
    CHECK(copra_batch_create(&twin, &dims, 2, costs, 2, cstrs));
    CHECK(copra_batch_set_system(h, A.data(), B.data(), d.data(), x0.data(), 0));
    CHECK(copra_batch_set_system(twin, A.data(), B.data(), d.data(), x0.data(), 0));

    // the trace: x, u and the viol row of the velocity bound and a control box the loop does exceed at its start
    double slo[2] = { -inf, -1.0 }, shi[2] = { inf, 1.0 }, tlo[1] = { -0.5 }, thi[1] = { 0.5 };
    copra_trace_t m;
    copra_trace_init(&m);
    if (m.struct_size != (int)sizeof m) return 1;
    m.capacity = ticks, m.what = COPRA_TRACE_X | COPRA_TRACE_U, m.x_lo = slo, m.x_hi = shi, m.u_lo = tlo, m.u_hi = thi, m.tol = 1e-9;
    long long recorded = -1, missed = -1, slot_bytes = 0;
    int got_rows = 0;
    if (copra_batch_trace_info(h, &recorded, &missed, &got_rows, &slot_bytes) != COPRA_ERR_RUNTIME || copra_batch_trace_device(h)) return 1; // (not on yet)
    CHECK(copra_batch_set_trace(h, &m));
    CHECK(copra_batch_trace_info(h, &recorded, &missed, &got_rows, &slot_bytes));
    if (recorded != 0 || missed != 0 || got_rows != rows || slot_bytes != 64 + 56 * rows || !copra_batch_trace_device(h) || copra_batch_trace_device(twin)) return 1;

    copra_plant_step_t step;
    copra_plant_step_init(&step);
    CHECK(copra_batch_rollout(h, &step, ticks + 1, nullptr, nullptr, nullptr, nullptr, nullptr)); // no history at all; one tick more than the trace holds
    CHECK(copra_batch_trace_info(h, &recorded, &missed, nullptr, nullptr));
    if (recorded != ticks || missed != 1) return 1;
    std::vector<unsigned char> trace((size_t)ticks * (size_t)slot_bytes);
    if (copra_batch_get_trace(h, 1, ticks, trace.data()) != COPRA_ERR_ARG || copra_batch_get_trace(h, 0, ticks, nullptr) != COPRA_ERR_ARG) return 1;
    CHECK(copra_batch_get_trace(h, 0, ticks, trace.data()));

    // the twin: the same ticks one by one, every tick's statistics on the host
    std::vector<double> x((size_t)batch * nx), control((size_t)batch * nu * N), traj((size_t)batch * nx * (N + 1));
    std::vector<int> status((size_t)batch), iter((size_t)batch * 2);
    const auto close = [](double a, double b) { return std::fabs(a - b) <= 1e-8 * std::fmax(std::fabs(a), std::fabs(b)) + 1e-300; };
    int bad = 0;
    for (int t = 0; t < ticks; ++t) {
        CHECK(copra_batch_solve(twin, nullptr));
        CHECK(copra_batch_get_results(twin, control.data(), traj.data(), status.data(), iter.data()));
        CHECK(copra_batch_advance(twin, &step, nullptr));
        CHECK(copra_batch_get_x0(twin, x.data()));
        copra_trace_head_t head;
        copra_score_stat_t stat[rows];
        std::memcpy(&head, &trace[(size_t)t * (size_t)slot_bytes], sizeof head);
        std::memcpy(stat, &trace[(size_t)t * (size_t)slot_bytes + sizeof head], sizeof stat);
        long long held = 0, violating = 0, n[3] = { 0, 0, 0 }, argmax[3] = { -1, -1, -1 };
        double sum[3] = { 0, 0, 0 }, top[3] = { -inf, -inf, -inf }, low[3] = { inf, inf, inf }, vtop = 0.0;
        for (int b = 0; b < batch; ++b) {
            const bool ok = status[(size_t)b] == COPRA_QP_OK;
            const double z[3] = { x[(size_t)b * nx], x[(size_t)b * nx + 1], control[(size_t)b * nu * N] };
            double v = 0.0;
            for (int r = 0; r < nx + (ok ? nu : 0); ++r) { // (a held instance has no u row)
                n[r] += 1, sum[r] += z[r];
                if (z[r] > top[r]) top[r] = z[r], argmax[r] = b;
                low[r] = std::fmin(low[r], z[r]);
                v = std::fmax(v, r < nx ? std::fmax(slo[r] - z[r], z[r] - shi[r]) : std::fmax(tlo[0] - z[r], z[r] - thi[0]));
            }
            held += !ok, violating += v > m.tol, vtop = std::fmax(vtop, v);
        }
        bool same = head.tick == t && head.tau == t + 1 && head.solved == batch - held && head.held == held && head.replayed == 0 && head.fallback == 0
            && head.violating == violating && head.reserved == 0 && stat[3].n == batch && std::fabs(stat[3].max - vtop) <= 1e-9;
        for (int r = 0; r < 3; ++r)
            same = same && stat[r].n == n[r] && close(stat[r].mean, sum[r] / (double)n[r]) && close(stat[r].max, top[r]) && close(stat[r].min, low[r])
                && stat[r].argmax == argmax[r] && stat[r].m2 >= 0.0;
        if (!same) {
            std::printf("tick %d: solved %lld held %lld / %lld violating %lld / %lld; position n %lld mean %.17g / %.17g max %.17g / %.17g argmax %lld / %lld\n", t, head.solved,
                head.held, held, head.violating, violating, stat[0].n, stat[0].mean, sum[0] / (double)n[0], stat[0].max, top[0], stat[0].argmax, argmax[0]);
            ++bad;
        }
        if (t == ticks - 1)
            std::printf("tick %lld of %d instances: position %.6g +- %.3g in [%.6g (instance %lld), %.6g (instance %lld)], control mean %.4g over %lld, "
                        "%lld held, %lld beyond a limit (largest violation %.4g)\n",
                head.tick, batch, stat[0].mean, std::sqrt(stat[0].m2 / (double)(stat[0].n - 1)), stat[0].min, stat[0].argmin, stat[0].max, stat[0].argmax, stat[2].mean,
                stat[2].n, head.held, head.violating, stat[3].max);
        if (stat[1].argmax != stuck || stat[2].n != batch - 1 || head.held != 1) ++bad; // the stuck instance: the fastest, held, without a control
    }
    CHECK(copra_batch_trace_reset(h));
    CHECK(copra_batch_trace_info(h, &recorded, &missed, nullptr, nullptr));
    if (recorded != 0 || missed != 0 || copra_batch_get_trace(h, 0, 1, trace.data()) != COPRA_ERR_ARG) ++bad;
    CHECK(copra_batch_set_trace(h, nullptr));
    if (copra_batch_trace_device(h) || copra_batch_trace_reset(h) != COPRA_ERR_RUNTIME) ++bad;
    copra_batch_destroy(h);
    copra_batch_destroy(twin);
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
