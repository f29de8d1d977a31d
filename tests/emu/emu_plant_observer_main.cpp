// emu_plant_observer_main.cpp -- the five-tick script of tests/test_backup_plan_abi.py with the state observer on, as a stand-alone program
// around tests/emu/emu_plant_observer.cpp, for a build with -fsanitize=address,undefined: (nx, nu, ny, N) = (6, 3, 3, 4), K = 3, batch 5,
// group 4 (a partial last group), and per-instance matrices at (2, 1, 3) (ny > nx, odd counts) and (9, 3, 3), batch 7, group 2.  Every array
// is allocated with exactly the elements the kernel may touch.  Exit status 0 and nothing on stderr is what the test asserts; the ages are
// compared with the script's table, a held instance's plant state, estimate and dhat with their old bits, and nothing may turn NaN.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

extern "C" {
struct EmuObserverTick {
    int batch, nx, nu, ny, N, group, threads, shared;
    const double *A, *B, *d;
    double* xp;
    const double *w, *fallback_u;
    const int* status;
    const double* control;
    double *x_out, *u_out;
    int* status_out;
    int backup_steps, fresh;
    double* plan;
    int* next;
    int* age_out;
    int gain_shared;
    const double *Am, *Bm;
    double* dhat;
    const double* xhat;
    double* xhat_next;
    const double *C, *Lx, *Ld, *v, *y_meas;
    double *y_out, *xhat_out, *d_out;
    int vec2_mode, vec2_used;
};
int emu_plant_observer_step(EmuObserverTick* t);
}

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
    int batch, nx, nu, ny, N, K, group;
    bool script; // the statuses of the table above (batch 5); otherwise everything solves at every tick
};

std::unique_ptr<double[]> filled(int n, double scale, unsigned& seed)
{
    std::unique_ptr<double[]> a(new double[n > 0 ? n : 1]);
    for (int i = 0; i < n; ++i) a[i] = scale * value(seed);
    return a;
}

bool same(const double* a, const double* b, int n) { return std::memcmp(a, b, sizeof(double) * (size_t)n) == 0; }

// plant: 0 none (the model with its estimates), 1 one per instance, 2 one for the batch
int run(const Shape& S, int threads, int plant, bool per, bool with_Ld, bool with_w, bool with_v, bool with_fb, bool meas, bool in_place)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int b = S.batch, nx = S.nx, nu = S.nu, ny = S.ny, N = S.N, K = S.K;
    unsigned seed = 97u + (unsigned)threads + 7u * (unsigned)plant;
    const int ps = plant == 2 ? 1 : b, gs = per ? b : 1;
    auto Am = filled(b * nx * nx, 0.3, seed), Bm = filled(b * nx * nu, 1.0, seed), dhat = filled(b * nx, 1.0, seed);
    auto A = filled(plant ? ps * nx * nx : 0, 0.3, seed), B = filled(plant ? ps * nx * nu : 0, 1.0, seed), d = filled(plant ? ps * nx : 0, 1.0, seed);
    auto Cm = filled(gs * ny * nx, 1.0, seed), Lx = filled(gs * nx * ny, 0.5, seed), Ld = filled(gs * nx * ny, 0.2, seed);
    auto xp = filled(b * nx, 1.0, seed), xhat = filled(b * nx, 1.0, seed), w = filled(b * nx, 0.01, seed), v = filled(b * ny, 0.01, seed);
    auto ym = filled(b * ny, 1.0, seed), fb = filled(b * nu, 1.0, seed);
    std::unique_ptr<double[]> xhat2(new double[b * nx]), control(new double[b * nu * N]), plan(new double[b * K * nu]);
    std::unique_ptr<double[]> x_out(new double[b * nx]), u_out(new double[b * nu]), y_out(new double[b * ny]), xhat_out(new double[b * nx]), d_out(new double[b * nx]);
    std::unique_ptr<double[]> old_xp(new double[b * nx]), old_xh(new double[b * nx]), old_dh(new double[b * nx]);
    std::unique_ptr<int[]> status(new int[b]), next(new int[b]), status_out(new int[b]), age(new int[b]);
    for (int i = 0; i < b * K * nu; ++i) plan[i] = nan; // (a plan is read only after it has been stored)
    for (int i = 0; i < b; ++i) next[i] = 0;
    for (int t = 0; t < kTicks; ++t) {
        if (kFresh[t])
            for (int i = 0; i < b; ++i) {
                status[i] = S.script ? kStatus[t][i] : 0;
                for (int e = 0; e < nu * N; ++e) control[i * nu * N + e] = status[i] == 0 ? value(seed) : nan;
            }
        std::memcpy(old_xp.get(), xp.get(), sizeof(double) * (size_t)(b * nx));
        std::memcpy(old_xh.get(), xhat.get(), sizeof(double) * (size_t)(b * nx));
        std::memcpy(old_dh.get(), dhat.get(), sizeof(double) * (size_t)(b * nx));
        EmuObserverTick T {};
        T.batch = b, T.nx = nx, T.nu = nu, T.ny = ny, T.N = N, T.group = S.group, T.threads = threads, T.shared = plant == 2;
        if (plant) T.A = A.get(), T.B = B.get(), T.d = d.get();
        T.xp = meas ? nullptr : xp.get(); // (measured outputs: the plant's state is not looked at)
        T.w = with_w ? w.get() : nullptr, T.fallback_u = with_fb ? fb.get() : nullptr;
        T.status = status.get(), T.control = control.get();
        T.x_out = meas ? nullptr : x_out.get(), T.u_out = u_out.get(), T.status_out = status_out.get();
        T.backup_steps = K, T.fresh = kFresh[t], T.plan = plan.get(), T.next = next.get(), T.age_out = age.get();
        T.gain_shared = !per;
        T.Am = Am.get(), T.Bm = Bm.get(), T.dhat = dhat.get();
        T.xhat = xhat.get(), T.xhat_next = in_place ? xhat.get() : xhat2.get();
        T.C = Cm.get(), T.Lx = Lx.get(), T.Ld = with_Ld ? Ld.get() : nullptr;
        T.v = with_v ? v.get() : nullptr, T.y_meas = meas ? ym.get() : nullptr;
        T.y_out = y_out.get(), T.xhat_out = xhat_out.get(), T.d_out = with_Ld ? d_out.get() : nullptr;
        T.vec2_mode = -1;
        if (emu_plant_observer_step(&T) != 0) return 2;
        if (!in_place) xhat.swap(xhat2);
        for (int i = 0; i < b; ++i) {
            const int script_age = S.script ? kAge[t][i] : (kFresh[t] ? 0 : 1);
            const int want = (script_age == -2 && with_fb) ? -1 : script_age;
            if (age[i] != want) {
                std::printf("tick %d instance %d: age %d, expected %d\n", t, i, age[i], want);
                return 1;
            }
            for (int r = 0; r < nx; ++r)
                if (std::isnan(xp[i * nx + r]) || std::isnan(xhat[i * nx + r]) || std::isnan(dhat[i * nx + r])) {
                    std::printf("tick %d instance %d: NaN in a state or an estimate\n", t, i);
                    return 1;
                }
            for (int o = 0; o < ny; ++o)
                if (std::isnan(y_out[i * ny + o])) {
                    std::printf("tick %d instance %d: NaN in y_out\n", t, i);
                    return 1;
                }
            if (!same(xhat_out.get() + i * nx, xhat.get() + i * nx, nx) || (with_Ld && !same(d_out.get() + i * nx, dhat.get() + i * nx, nx))
                || (!meas && !same(x_out.get() + i * nx, xp.get() + i * nx, nx))) {
                std::printf("tick %d instance %d: a copy differs from what it copies\n", t, i);
                return 1;
            }
            const bool kept_d = same(old_dh.get() + i * nx, dhat.get() + i * nx, nx);
            if ((want == -2 || !with_Ld) && !kept_d) {
                std::printf("tick %d instance %d: dhat moved where it must not\n", t, i);
                return 1;
            }
            if ((want == -2 || meas) && !same(old_xp.get() + i * nx, xp.get() + i * nx, nx)) {
                std::printf("tick %d instance %d: the plant's state moved where it must not\n", t, i);
                return 1;
            }
            if (want == -2 && !same(old_xh.get() + i * nx, xhat.get() + i * nx, nx)) {
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
    const Shape script { kScriptBatch, 6, 3, 3, 4, 3, 4, true };
    for (int threads : { 3, 64 })
        for (int m = 0; m < 256; ++m) {
            const int rc = run(script, threads, m % 3, m & 2, m & 4, m & 8, m & 16, m & 32, m & 64, m & 128);
            if (rc != 0) return rc;
        }
    const Shape wide { 7, 2, 1, 3, 4, 3, 2, false }, odd { 7, 9, 3, 3, 4, 3, 2, false }; // per-instance matrices, odd counts, a partial last group
    for (const Shape& S : { wide, odd })
        for (int threads : { 5, 256 })
            for (int plant = 0; plant < 3; ++plant)
                for (int meas = 0; meas < 2; ++meas) {
                    const int rc = run(S, threads, plant, true, plant != 2, plant != 1, plant != 0, false, meas != 0, true);
                    if (rc != 0) return rc;
                }
    return 0;
}
