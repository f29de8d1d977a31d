// emu_plant_bias_main.cpp -- the five-tick script of tests/test_backup_plan_abi.py with the disturbance estimator on, as a stand-alone program
// around tests/emu/emu_plant_bias.cpp, for a build with -fsanitize=address,undefined: (nx, nu, N) = (6, 3, 4), K = 3, batch 5, group 4 (a
// partial last group), and one dense per-instance case at (9, 3), batch 7, group 2.  Every array is allocated with exactly the elements the
// kernel may touch.  Exit status 0 and nothing on stderr is what the test asserts; the ages are compared with the script's table, a held
// instance's estimate with its old bits, and nothing may turn NaN.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

extern "C" int emu_plant_bias_step(int batch, int nx, int nu, int N, int group, int threads, int shared, const double* A, const double* B, const double* d,
    const double* x0, const double* w, const double* fallback_u, const int* status, const double* control, double* x0_next, double* x_out, double* u_out,
    int* status_out, int* vec2_used, int backup_steps, int fresh, double* plan, int* next, int* age_out, int est, int gain_dense, int gain_shared,
    const double* Am, const double* Bm, const double* gain, double* dhat, double* d_out, int vec2_mode);

namespace {

constexpr int kTicks = 5, kScriptBatch = 5;
// instance 0 solves at every tick; 1 never; 2 once, then fails until its plan is used up; 3 fails two ticks, then solves again; 4 starts
// without a plan.  Tick 4 has no solve: status and control are those of tick 3.
const int kStatus[4][kScriptBatch] = { { 0, 1, 0, 0, 1 }, { 0, 1, 1, 1, 0 }, { 0, 1, 2, 1, 3 }, { 0, 1, 3, 0, 0 } };
const int kFresh[kTicks] = { 1, 1, 1, 1, 0 };
const int kAge[kTicks][kScriptBatch] = { { 0, -2, 0, 0, -2 }, { 0, -2, 1, 1, 0 }, { 0, -2, 2, 2, 1 }, { 0, -2, 3, 0, 0 }, { 1, -2, -2, 1, 1 } };

double value(unsigned& seed) // a small deterministic generator: values in (-1, 1)
{
    seed = seed * 1664525u + 1013904223u;
    return (double)(seed >> 8) / (double)(1u << 23) - 1.0;
}

struct Shape {
    int batch, nx, nu, N, K, group;
    bool script; // the statuses of the table above (batch 5); otherwise everything solves at every tick
};

// plant: 0 none (the model with its estimates), 1 one per instance, 2 one for the batch
int run(const Shape& S, int threads, int plant, bool dense, bool per, bool with_w, bool with_fb, bool in_place)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int b = S.batch, nx = S.nx, nu = S.nu, N = S.N, K = S.K;
    unsigned seed = 4321u + (unsigned)threads + 7u * (unsigned)plant;
    const int ps = plant == 2 ? 1 : b, g1 = dense ? nx * nx : nx, gs = per ? b : 1;
    std::unique_ptr<double[]> Am(new double[b * nx * nx]), Bm(new double[b * nx * nu]), dhat(new double[b * nx]), d_out(new double[b * nx]), old(new double[b * nx]);
    std::unique_ptr<double[]> A, B, d;
    if (plant) A.reset(new double[ps * nx * nx]), B.reset(new double[ps * nx * nu]), d.reset(new double[ps * nx]);
    std::unique_ptr<double[]> gain(new double[gs * g1]);
    std::unique_ptr<double[]> x(new double[b * nx]), xn(new double[b * nx]), w(new double[b * nx]), fb(new double[b * nu]);
    std::unique_ptr<double[]> control(new double[b * nu * N]), plan(new double[b * K * nu]);
    std::unique_ptr<double[]> x_out(new double[b * nx]), u_out(new double[b * nu]);
    std::unique_ptr<int[]> status(new int[b]), next(new int[b]), status_out(new int[b]), age(new int[b]);
    for (int i = 0; i < b * nx * nx; ++i) Am[i] = 0.3 * value(seed);
    for (int i = 0; i < b * nx * nu; ++i) Bm[i] = value(seed);
    for (int i = 0; i < b * nx; ++i) dhat[i] = value(seed);
    if (plant) {
        for (int i = 0; i < ps * nx * nx; ++i) A[i] = 0.3 * value(seed);
        for (int i = 0; i < ps * nx * nu; ++i) B[i] = value(seed);
        for (int i = 0; i < ps * nx; ++i) d[i] = value(seed);
    }
    for (int i = 0; i < gs * g1; ++i) gain[i] = 0.5 * value(seed);
    for (int i = 0; i < b * nx; ++i) x[i] = value(seed), w[i] = 0.01 * value(seed);
    for (int i = 0; i < b * nu; ++i) fb[i] = value(seed);
    for (int i = 0; i < b * K * nu; ++i) plan[i] = nan; // (a plan is read only after it has been stored)
    for (int i = 0; i < b; ++i) next[i] = 0;
    for (int t = 0; t < kTicks; ++t) {
        if (kFresh[t])
            for (int i = 0; i < b; ++i) {
                status[i] = S.script ? kStatus[t][i] : 0;
                for (int e = 0; e < nu * N; ++e) control[i * nu * N + e] = status[i] == 0 ? value(seed) : nan;
            }
        std::memcpy(old.get(), dhat.get(), sizeof(double) * (size_t)(b * nx));
        double* out = in_place ? x.get() : xn.get();
        const int rc = emu_plant_bias_step(b, nx, nu, N, S.group, threads, plant == 2, A.get(), B.get(), d.get(), x.get(), with_w ? w.get() : nullptr,
            with_fb ? fb.get() : nullptr, status.get(), control.get(), out, x_out.get(), u_out.get(), status_out.get(), nullptr, K, kFresh[t], plan.get(),
            next.get(), age.get(), 1, dense, !per, Am.get(), Bm.get(), gain.get(), dhat.get(), d_out.get(), -1);
        if (rc != 0) return 2;
        if (!in_place) x.swap(xn);
        for (int i = 0; i < b; ++i) {
            const int script_age = S.script ? kAge[t][i] : (kFresh[t] ? 0 : 1);
            const int want = (script_age == -2 && with_fb) ? -1 : script_age;
            if (age[i] != want) {
                std::printf("tick %d instance %d: age %d, expected %d\n", t, i, age[i], want);
                return 1;
            }
            for (int r = 0; r < nx; ++r)
                if (std::isnan(x[i * nx + r]) || std::isnan(dhat[i * nx + r])) {
                    std::printf("tick %d instance %d: NaN in the state or the estimate\n", t, i);
                    return 1;
                }
            if (std::memcmp(d_out.get() + i * nx, dhat.get() + i * nx, sizeof(double) * (size_t)nx) != 0) {
                std::printf("tick %d instance %d: d_out is not the estimate\n", t, i);
                return 1;
            }
            if (want == -2 && std::memcmp(old.get() + i * nx, dhat.get() + i * nx, sizeof(double) * (size_t)nx) != 0) {
                std::printf("tick %d instance %d: a held instance's estimate moved\n", t, i);
                return 1;
            }
        }
    }
    return 0;
}

} // namespace

int main()
{
    const Shape script { kScriptBatch, 6, 3, 4, 3, 4, true };
    for (int threads : { 3, 64 })
        for (int m = 0; m < 64; ++m) {
            const int rc = run(script, threads, m % 3, m & 4, m & 8, m & 16, m & 32, m & 1);
            if (rc != 0) return rc;
        }
    const Shape dense { 7, 9, 3, 4, 3, 2, false }; // a dense gain per instance, an odd xDim, a partial last group
    for (int threads : { 5, 256 })
        for (int plant = 0; plant < 3; ++plant) {
            const int rc = run(dense, threads, plant, true, true, plant != 1, false, true);
            if (rc != 0) return rc;
        }
    return 0;
}
