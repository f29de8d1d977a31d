// Trace quantiles from a C / C++ caller that has no array library and touches no device memory: the fleet of double integrators of
// tests/cpp/test_trace.cpp through include/copra_hip.h alone.  The handle traces x, u and the viol row with the levels 0, 5 %, 50 %, 95 %, 1,
// runs copra_batch_rollout WITHOUT any history and reads the slots and their quantiles.  Of every recorded tick, level 0 and level 1 must be the
// slot's min and max and the levels must ascend; of the last tick, whose state copra_batch_get_x0 returns, the position and velocity rows must
// be, bit for bit, the order statistics a sort on the host picks by the rule of the header.  Prints the band of the position row.  Built and run
// by tests/test_trace_quant_gpu.py.
#include <copra_hip.h>

#include <algorithm>
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

static unsigned long long bits_of(double v)
{
    unsigned long long b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

// the rule of the header, by sorting
static unsigned long long by_sort(const std::vector<double>& v, double p)
{
    std::vector<unsigned long long> keys;
    for (double x : v)
        if (std::isfinite(x)) {
            const unsigned long long b = bits_of(x);
            keys.push_back(b ^ ((b >> 63) ? ~0ull : 1ull << 63));
        }
    if (keys.empty()) return 0x7FF8000000000000ull;
    std::sort(keys.begin(), keys.end());
    const long long n = (long long)keys.size(), c = (long long)std::ceil(p * (double)n);
    const unsigned long long key = keys[(size_t)std::min(n - 1, std::max(0ll, c - 1))];
    return key ^ ((key >> 63) ? 1ull << 63 : ~0ull);
}

int main()
{
    const int batch = 70, N = 8, ticks = 6, nx = 2, nu = 1, stuck = 3, rows = nx + nu + 1, nq = 5;
    const double dt = 0.1, inf = std::numeric_limits<double>::infinity();
    const double levels[nq] = { 0.0, 0.05, 0.5, 0.95, 1.0 };
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
    copra_batch_t* h = nullptr;
    CHECK(copra_batch_create(&h, &dims, 2, costs, 2, cstrs));
    CHECK(copra_batch_set_system(h, A.data(), B.data(), d.data(), x0.data(), 0));

    int bad = 0, count = -1;
    double back[COPRA_TRACE_QUANT_MAX];
    if (copra_batch_set_trace_quantiles(h, levels, nq) != COPRA_ERR_RUNTIME) ++bad; // (tracing is not on yet)
    double slo[2] = { -inf, -1.0 }, shi[2] = { inf, 1.0 }, tlo[1] = { -0.5 }, thi[1] = { 0.5 };
    copra_trace_t m;
    copra_trace_init(&m);
    m.capacity = ticks, m.what = COPRA_TRACE_X | COPRA_TRACE_U, m.x_lo = slo, m.x_hi = shi, m.u_lo = tlo, m.u_hi = thi, m.tol = 1e-9;
    CHECK(copra_batch_set_trace(h, &m));
    if (copra_batch_trace_quantile_info(h, &count, back) != COPRA_ERR_RUNTIME || copra_batch_trace_quantiles_device(h)) ++bad; // (quantiles are not on yet)
    const double beyond[2] = { 0.5, 1.5 }, nan_level[1] = { std::nan("") };
    if (copra_batch_set_trace_quantiles(h, beyond, 2) != COPRA_ERR_ARG || copra_batch_set_trace_quantiles(h, nan_level, 1) != COPRA_ERR_ARG
        || copra_batch_set_trace_quantiles(h, levels, COPRA_TRACE_QUANT_MAX + 1) != COPRA_ERR_ARG)
        ++bad;
    CHECK(copra_batch_set_trace_quantiles(h, levels, nq));
    CHECK(copra_batch_trace_quantile_info(h, &count, back));
    if (count != nq || std::memcmp(back, levels, sizeof levels) != 0 || !copra_batch_trace_quantiles_device(h)) ++bad;

    copra_plant_step_t step;
    copra_plant_step_init(&step);
    CHECK(copra_batch_rollout(h, &step, ticks, nullptr, nullptr, nullptr, nullptr, nullptr)); // no history at all
    long long recorded = -1, missed = -1, slot_bytes = 0;
    CHECK(copra_batch_trace_info(h, &recorded, &missed, nullptr, &slot_bytes));
    if (recorded != ticks || missed != 0) ++bad;
    std::vector<unsigned char> trace((size_t)ticks * (size_t)slot_bytes);
    std::vector<double> quant((size_t)ticks * rows * nq), x((size_t)batch * nx);
    CHECK(copra_batch_get_trace(h, 0, ticks, trace.data()));
    if (copra_batch_get_trace_quantiles(h, 1, ticks, quant.data()) != COPRA_ERR_ARG || copra_batch_get_trace_quantiles(h, 0, ticks, nullptr) != COPRA_ERR_ARG) ++bad;
    CHECK(copra_batch_get_trace_quantiles(h, 0, ticks, quant.data()));
    CHECK(copra_batch_get_x0(h, x.data()));

    for (int t = 0; t < ticks; ++t) {
        copra_score_stat_t stat[rows];
        std::memcpy(stat, &trace[(size_t)t * (size_t)slot_bytes + sizeof(copra_trace_head_t)], sizeof stat);
        for (int r = 0; r < rows; ++r) {
            const double* q = &quant[((size_t)t * rows + r) * nq];
            bool ok = q[0] == stat[r].min && q[nq - 1] == stat[r].max;
            for (int k = 1; k < nq; ++k) ok = ok && q[k - 1] <= q[k];
            if (!ok) {
                std::printf("tick %d row %d: %.17g %.17g %.17g %.17g %.17g against min %.17g max %.17g\n", t, r, q[0], q[1], q[2], q[3], q[4], stat[r].min, stat[r].max);
                ++bad;
            }
        }
    }
    for (int r = 0; r < nx; ++r) { // the last tick's state is the handle's x0: bit for bit the sort's
        std::vector<double> col((size_t)batch);
        for (int b = 0; b < batch; ++b) col[(size_t)b] = x[(size_t)b * nx + r];
        for (int k = 0; k < nq; ++k)
            if (bits_of(quant[((size_t)(ticks - 1) * rows + r) * nq + k]) != by_sort(col, levels[k])) {
                std::printf("row %d level %g: %.17g is not the sort's\n", r, levels[k], quant[((size_t)(ticks - 1) * rows + r) * nq + k]);
                ++bad;
            }
    }
    const double* pos = &quant[(size_t)(ticks - 1) * rows * nq];
    const double* viol = &quant[((size_t)(ticks - 1) * rows + rows - 1) * nq];
    std::printf("tick %d of %d instances: position 5 %% %.6g, median %.6g, 95 %% %.6g in [%.6g, %.6g]; violation median %.4g, 95 %% %.4g, largest %.4g\n", ticks - 1, batch,
        pos[1], pos[2], pos[3], pos[0], pos[4], viol[2], viol[3], viol[4]);
    if (quant[((size_t)(ticks - 1) * rows + 1) * nq + nq - 1] != 50.0) ++bad; // the stuck instance is the fastest

    CHECK(copra_batch_trace_reset(h)); // keeps the levels
    CHECK(copra_batch_trace_quantile_info(h, &count, nullptr));
    if (count != nq || copra_batch_get_trace_quantiles(h, 0, 1, quant.data()) != COPRA_ERR_ARG) ++bad;
    CHECK(copra_batch_set_trace_quantiles(h, nullptr, 0)); // quantiles end, the trace stays
    if (copra_batch_trace_quantiles_device(h) || !copra_batch_trace_device(h) || copra_batch_get_trace_quantiles(h, 0, 0, quant.data()) != COPRA_ERR_RUNTIME) ++bad;
    CHECK(copra_batch_set_trace_quantiles(h, levels, 2));
    CHECK(copra_batch_set_trace(h, nullptr)); // the trace ends, and its quantiles with it
    if (copra_batch_trace_quantiles_device(h) || copra_batch_trace_quantile_info(h, &count, nullptr) != COPRA_ERR_RUNTIME) ++bad;
    copra_batch_destroy(h);
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
