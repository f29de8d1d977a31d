// Closed-loop scores from a C / C++ caller that has no array library and touches no device memory: a fleet of double integrators through
// include/copra_hip.h alone.  One handle runs copra_batch_rollout WITHOUT any history and reads copra_batch_get_score and
// copra_batch_score_summary; a twin runs the same ticks one by one (solve, get_results, advance, get_x0) and accumulates the same measure on
// the host.  The sums must agree to 1e-8 relative -- a rollout and the same loop with read-outs in between agree to 1e-9 in their states
// (tests/test_closed_loop_gpu.py) --, the largest violation to 1e-9 absolute, the counters exactly (tol = 1e-9 keeps a velocity that sits ON
// its bound from counting).  Built and run by tests/test_score_gpu.py.
#include <copra_hip.h>

#include <cmath>
#include <cstdio>
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

static_assert(sizeof(copra_score_record_t) == 64, "one record is 64 bytes");

int main()
{
    const int batch = 70, N = 8, ticks = 6, nx = 2, nu = 1, stuck = 3;
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
    double xlow[2] = { -inf, -inf }, xup[2] = { inf, 1.0 }, ulow[1] = { -5.0 }, uup[1] = { 5.0 }; // (upper-only, as copra_amd/workloads.py::com_preview)
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

    // the measure: |x - goal|^2 with weights (1, 0.1), 1e-3 u^2, the velocity bound, a control box the loop does exceed at its start
    double qx[2] = { 1.0, 0.1 }, ru[1] = { 1e-3 }, slo[2] = { -inf, -1.0 }, shi[2] = { inf, 1.0 }, tlo[1] = { -0.5 }, thi[1] = { 0.5 };
    copra_score_t m;
    copra_score_init(&m);
    if (m.struct_size != (int)sizeof m) return 1;
    m.qx = qx, m.ru = ru, m.x_ref = goal, m.ref_steps = 1, m.x_lo = slo, m.x_hi = shi, m.u_lo = tlo, m.u_hi = thi, m.tol = 1e-9;
    std::vector<copra_score_record_t> rec((size_t)batch);
    copra_score_summary_t sum;
    if (copra_batch_get_score(h, rec.data()) != COPRA_ERR_RUNTIME || copra_batch_score_summary(h, &sum) != COPRA_ERR_RUNTIME) return 1; // (not on yet)
    CHECK(copra_batch_set_score(h, &m));
    if (!copra_batch_score_device(h) || copra_batch_score_device(twin)) return 1;

    copra_plant_step_t step;
    copra_plant_step_init(&step);
    CHECK(copra_batch_rollout(h, &step, ticks, nullptr, nullptr, nullptr, nullptr, nullptr)); // no history at all
    CHECK(copra_batch_get_score(h, rec.data()));
    CHECK(copra_batch_score_summary(h, &sum));

    // the twin: the same ticks one by one, the measure accumulated on the host
    std::vector<double> jx((size_t)batch, 0.0), ju((size_t)batch, 0.0), vmax((size_t)batch, 0.0), x((size_t)batch * nx);
    std::vector<int> held((size_t)batch, 0), violating((size_t)batch, 0), first((size_t)batch, 0), status((size_t)batch), iter((size_t)batch * 2);
    std::vector<double> control((size_t)batch * nu * N), traj((size_t)batch * nx * (N + 1));
    for (int t = 0; t < ticks; ++t) {
        CHECK(copra_batch_solve(twin, nullptr));
        CHECK(copra_batch_get_results(twin, control.data(), traj.data(), status.data(), iter.data()));
        CHECK(copra_batch_advance(twin, &step, nullptr));
        CHECK(copra_batch_get_x0(twin, x.data()));
        for (int b = 0; b < batch; ++b) {
            const bool ok = status[(size_t)b] == COPRA_QP_OK;
            double lx = 0.0, v = 0.0;
            for (int r = 0; r < nx; ++r) {
                const double z = x[(size_t)b * nx + r], e = z - goal[r];
                lx += qx[r] * e * e;
                v = std::fmax(v, std::fmax(slo[r] - z, z - shi[r]));
            }
            jx[(size_t)b] += lx;
            if (ok) {
                const double u = control[(size_t)b * nu * N];
                ju[(size_t)b] += ru[0] * u * u;
                v = std::fmax(v, std::fmax(tlo[0] - u, u - thi[0]));
            }
            held[(size_t)b] += !ok;
            vmax[(size_t)b] = std::fmax(vmax[(size_t)b], v);
            if (v > m.tol) {
                violating[(size_t)b] += 1;
                if (!first[(size_t)b]) first[(size_t)b] = t + 1;
            }
        }
    }
    int bad = 0;
    long long n_held = 0, n_viol = 0, inst_viol = 0;
    double mean = 0.0, top = -inf;
    long long argtop = -1;
    const auto close = [](double a, double b) { return std::fabs(a - b) <= 1e-8 * std::fmax(std::fabs(a), std::fabs(b)); };
    for (int b = 0; b < batch; ++b) {
        const copra_score_record_t& r = rec[(size_t)b];
        const bool same = close(r.jx, jx[(size_t)b]) && close(r.ju, ju[(size_t)b]) && std::fabs(r.viol_max - vmax[(size_t)b]) <= 1e-9 && r.ticks == ticks && r.held == held[(size_t)b]
            && r.replayed == 0 && r.fallback == 0 && r.violating == violating[(size_t)b] && r.first_violation == first[(size_t)b];
        if (!same) {
            std::printf("instance %d: jx %.17g / %.17g, ju %.17g / %.17g, held %d / %d, violating %d / %d, first %d / %d\n", b, r.jx, jx[(size_t)b], r.ju, ju[(size_t)b],
                r.held, held[(size_t)b], r.violating, violating[(size_t)b], r.first_violation, first[(size_t)b]);
            ++bad;
        }
        n_held += r.held, n_viol += r.violating, inst_viol += r.violating != 0, mean += r.jx / batch;
        if (r.jx > top) top = r.jx, argtop = b;
    }
    if (rec[stuck].held != ticks || rec[stuck].ju != 0.0 || rec[stuck].first_violation != 1 || rec[0].held != 0 || rec[0].ju <= 0.0) ++bad;
    if (sum.jx.n != batch || !close(sum.jx.mean, mean) || !close(sum.jx.max, top) || sum.jx.argmax != argtop || sum.ticks != (long long)batch * ticks || sum.held != n_held
        || sum.violating != n_viol || sum.instances_violating != inst_viol || sum.instances_held != 1 || sum.jx.m2 <= 0.0) {
        std::printf("summary: n %lld mean %.17g / %.17g max %.17g / %.17g argmax %lld / %lld held %lld / %lld\n", sum.jx.n, sum.jx.mean, mean, sum.jx.max, top,
            sum.jx.argmax, argtop, sum.held, n_held);
        ++bad;
    }
    std::printf("scores of %d instances after %d ticks: mean cost %.6g, std %.3g, worst %.6g (instance %lld), %lld instances violated a limit, %lld ticks held\n", batch,
        ticks, sum.jx.mean, std::sqrt(sum.jx.m2 / (double)(sum.jx.n - 1)), sum.jx.max, sum.jx.argmax, sum.instances_violating, sum.held);
    CHECK(copra_batch_score_reset(h));
    CHECK(copra_batch_get_score(h, rec.data()));
    for (const copra_score_record_t& r : rec) bad += r.ticks != 0 || r.jx != 0.0;
    CHECK(copra_batch_set_score(h, nullptr));
    if (copra_batch_score_device(h) || copra_batch_score_reset(h) != COPRA_ERR_RUNTIME) ++bad;
    copra_batch_destroy(h);
    copra_batch_destroy(twin);
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
