// emu_plant_backup_main.cpp -- the five-tick script of tests/test_backup_plan_abi.py as a stand-alone program around
// tests/emu/emu_plant_backup.cpp, for a build with -fsanitize=address,undefined: (nx, nu, N) = (6, 3, 4), K = 3, batch 5, group 4 (a partial
// last group), every array allocated with exactly the elements the kernel may touch -- `control` with nu N doubles per instance, NaN where the
// instance's solve failed.  Exit status 0 and nothing on stderr is what the test asserts; the ages are compared with the script's table too.
#include <cmath>
#include <cstdio>
#include <limits>
#include <memory>

extern "C" int emu_plant_backup_step(int batch, int nx, int nu, int N, int group, int threads, int shared, const double* A, const double* B,
    const double* d, const double* x0, const double* w, const double* fallback_u, const int* status, const double* control, double* x0_next, double* x_out,
    double* u_out, int* status_out, int* vec2_used, int backup_steps, int fresh, double* plan, int* next, int* age_out);

namespace {

constexpr int kBatch = 5, kNx = 6, kNu = 3, kN = 4, kK = 3, kGroup = 4, kTicks = 5;
// instance 0 solves at every tick; 1 never; 2 once, then fails until its plan is used up; 3 fails two ticks, then solves again; 4 starts
// without a plan.  Tick 4 has no solve: status and control are those of tick 3.
const int kStatus[4][kBatch] = { { 0, 1, 0, 0, 1 }, { 0, 1, 1, 1, 0 }, { 0, 1, 2, 1, 3 }, { 0, 1, 3, 0, 0 } };
const int kFresh[kTicks] = { 1, 1, 1, 1, 0 };
const int kAge[kTicks][kBatch] = { { 0, -2, 0, 0, -2 }, { 0, -2, 1, 1, 0 }, { 0, -2, 2, 2, 1 }, { 0, -2, 3, 0, 0 }, { 1, -2, -2, 1, 1 } };

double value(unsigned& seed) // a small deterministic generator: values in (-1, 1)
{
    seed = seed * 1664525u + 1013904223u;
    return (double)(seed >> 8) / (double)(1u << 23) - 1.0;
}

int run(int threads, bool shared, bool with_w, bool with_fb, bool in_place)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    unsigned seed = 12345u + (unsigned)threads;
    const int gs = shared ? 1 : kBatch;
    std::unique_ptr<double[]> A(new double[gs * kNx * kNx]), B(new double[gs * kNx * kNu]), d(new double[gs * kNx]);
    std::unique_ptr<double[]> x(new double[kBatch * kNx]), xn(new double[kBatch * kNx]), w(new double[kBatch * kNx]), fb(new double[kBatch * kNu]);
    std::unique_ptr<double[]> control(new double[kBatch * kNu * kN]), plan(new double[kBatch * kK * kNu]);
    std::unique_ptr<double[]> x_out(new double[kBatch * kNx]), u_out(new double[kBatch * kNu]);
    std::unique_ptr<int[]> status(new int[kBatch]), next(new int[kBatch]), status_out(new int[kBatch]), age(new int[kBatch]);
    for (int i = 0; i < gs * kNx * kNx; ++i) A[i] = 0.3 * value(seed);
    for (int i = 0; i < gs * kNx * kNu; ++i) B[i] = value(seed);
    for (int i = 0; i < gs * kNx; ++i) d[i] = value(seed);
    for (int i = 0; i < kBatch * kNx; ++i) x[i] = value(seed), w[i] = 0.01 * value(seed);
    for (int i = 0; i < kBatch * kNu; ++i) fb[i] = value(seed);
    for (int i = 0; i < kBatch * kK * kNu; ++i) plan[i] = nan; // (a plan is read only after it has been stored)
    for (int b = 0; b < kBatch; ++b) next[b] = 0;
    for (int t = 0; t < kTicks; ++t) {
        if (kFresh[t])
            for (int b = 0; b < kBatch; ++b) {
                status[b] = kStatus[t][b];
                for (int e = 0; e < kNu * kN; ++e) control[b * kNu * kN + e] = status[b] == 0 ? value(seed) : nan;
            }
        double* out = in_place ? x.get() : xn.get();
        const int rc = emu_plant_backup_step(kBatch, kNx, kNu, kN, kGroup, threads, shared, A.get(), B.get(), d.get(), x.get(), with_w ? w.get() : nullptr,
            with_fb ? fb.get() : nullptr, status.get(), control.get(), out, x_out.get(), u_out.get(), status_out.get(), nullptr, kK, kFresh[t], plan.get(),
            next.get(), age.get());
        if (rc != 0) return 2;
        if (!in_place) x.swap(xn);
        for (int b = 0; b < kBatch; ++b) {
            const int want = (kAge[t][b] == -2 && with_fb) ? -1 : kAge[t][b];
            if (age[b] != want) {
                std::printf("tick %d instance %d: age %d, expected %d\n", t, b, age[b], want);
                return 1;
            }
            for (int r = 0; r < kNx; ++r)
                if (std::isnan(x[b * kNx + r])) {
                    std::printf("tick %d instance %d: NaN in the state\n", t, b);
                    return 1;
                }
            if (std::isnan(u_out[b * kNu]) != (want == -2)) {
                std::printf("tick %d instance %d: u_out and the age disagree\n", t, b);
                return 1;
            }
        }
    }
    return 0;
}

} // namespace

int main()
{
    for (int threads : { 3, 64 })
        for (int m = 0; m < 16; ++m) {
            const int rc = run(threads, m & 1, m & 2, m & 4, m & 8);
            if (rc != 0) return rc;
        }
    return 0;
}
