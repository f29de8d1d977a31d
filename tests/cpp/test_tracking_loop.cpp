// A closed-loop TRACKING run from a C / C++ caller: the controller of examples/tracking.py -- the CoM controller with a full-size TrajectoryCost whose
// reference follows a signal -- through include/copra_hip.h alone: copra_batch_set_reference_schedule hands the signal over once, ONE
// copra_batch_rollout tracks it.  Driven by tests/test_reference_schedule_gpu.py, which writes the systems, the disturbances, the signal and the
// histories it expects; the histories found are compared with those here (statuses equal, states and controls within 1e-9) and written out.
// Usage: test_tracking_loop <in> <out>
//   in:  int32 batch, N, ticks, steps, per_instance; doubles wx[6], wu[3], xupper[6], uupper[3], A[batch][6x6], B[batch][6x3], d[batch][6],
//        x0[batch][6], w_seq[ticks][batch][6], sched[per_instance ? batch : 1][steps][6], x_hist[ticks+1][batch][6], u_hist[ticks][batch][3];
//        int32 status_hist[ticks][batch]  (A, B column-major per instance)
//   out: doubles x_hist, u_hist; int32 status_hist
#include <copra_hip.h>
#include <hip/hip_runtime_api.h>

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
#define HIP(expr)                                                                            \
    do {                                                                                     \
        const hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess) {                                                              \
            std::printf("%s: %s\n", #expr, hipGetErrorString(e_));                           \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int head[5];
    if (std::fread(head, sizeof(int), 5, in) != 5) return 2;
    const int batch = head[0], N = head[1], ticks = head[2], steps = head[3], per_instance = head[4], nx = 6, nu = 3;
    const auto read = [&](size_t count) {
        std::vector<double> v(count);
        if (std::fread(v.data(), sizeof(double), count, in) != count) v.clear();
        return v;
    };
    const size_t nxh = (size_t)(ticks + 1) * batch * nx, nuh = (size_t)ticks * batch * nu, nsh = (size_t)ticks * batch;
    const std::vector<double> wx = read(6), wu = read(3), xup = read(6), uup = read(3);
    const std::vector<double> A = read((size_t)batch * 36), B = read((size_t)batch * 18), d = read((size_t)batch * 6), x0 = read((size_t)batch * 6);
    const std::vector<double> w_seq = read((size_t)ticks * batch * 6), sched = read((size_t)(per_instance ? batch : 1) * steps * nx);
    const std::vector<double> x_want = read(nxh), u_want = read(nuh);
    std::vector<int> s_want(nsh);
    const bool all_read = std::fread(s_want.data(), sizeof(int), nsh, in) == nsh;
    std::fclose(in);
    if (!all_read || u_want.empty()) return 2;

    // the full-size TrajectoryCost: M = blkdiag(I6 .. I6) over the N + 1 states, the weights of one step tiled, p the window of tick 0
    const int X = nx * (N + 1);
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> M((size_t)X * X, 0.0), wfull((size_t)X), p0((size_t)X);
    for (int i = 0; i < X; ++i) M[(size_t)i * X + i] = 1.0, wfull[i] = wx[i % nx];
    for (int s = 0; s <= N; ++s)
        for (int i = 0; i < nx; ++i) p0[(size_t)s * nx + i] = sched[(size_t)(s < steps ? s : steps - 1) * nx + i];
    double I3[9] = {}, zero3[3] = {}, xlow[6], ulow[3];
    for (int i = 0; i < 6; ++i) xlow[i] = -inf;
    for (int i = 0; i < 3; ++i) I3[4 * i] = 1.0, ulow[i] = -uup[i];
    copra_cost_desc_t costs[2] = {};
    costs[0].kind = COPRA_COST_TRAJECTORY, costs[0].rows = X, costs[0].m_cols = X, costs[0].M = M.data(), costs[0].p = p0.data(), costs[0].weights = wfull.data();
    costs[1].kind = COPRA_COST_CONTROL, costs[1].rows = 3, costs[1].n_cols = 3, costs[1].N = I3, costs[1].p = zero3, costs[1].weights = wu.data();
    copra_cstr_desc_t cstrs[2] = {};
    cstrs[0].kind = COPRA_CSTR_TRAJECTORY_BOUND, cstrs[0].rows = 6, cstrs[0].lower = xlow, cstrs[0].upper = xup.data();
    cstrs[1].kind = COPRA_CSTR_CONTROL_BOUND, cstrs[1].rows = 3, cstrs[1].lower = ulow, cstrs[1].upper = uup.data();
    const copra_dims_t dims = { nx, nu, N, batch };
    copra_batch_t* h = nullptr;
    CHECK(copra_batch_create(&h, &dims, 2, costs, 2, cstrs));
    CHECK(copra_batch_set_system(h, A.data(), B.data(), d.data(), x0.data(), 0));
    if (copra_batch_set_reference_schedule(h, 0, sched.data(), steps, nx + 1, 0, per_instance, 0) != COPRA_ERR_DOMAIN) {
        std::printf("copra_batch_set_reference_schedule: r = %d was not refused\n", nx + 1);
        return 1;
    }
    CHECK(copra_batch_set_reference_schedule(h, 0, sched.data(), steps, nx, 0, per_instance, 0)); // (a host schedule: copied)

    double *dw = nullptr, *dxh = nullptr, *duh = nullptr;
    int* dsh = nullptr;
    HIP(hipMalloc((void**)&dw, w_seq.size() * sizeof(double)));
    HIP(hipMalloc((void**)&dxh, nxh * sizeof(double)));
    HIP(hipMalloc((void**)&duh, nuh * sizeof(double)));
    HIP(hipMalloc((void**)&dsh, nsh * sizeof(int)));
    HIP(hipMemcpy(dw, w_seq.data(), w_seq.size() * sizeof(double), hipMemcpyHostToDevice));
    hipStream_t stream;
    HIP(hipStreamCreate(&stream));
    CHECK(copra_batch_rollout(h, nullptr, ticks, dw, dxh, duh, dsh, stream));
    CHECK(copra_batch_synchronize(h));
    if (copra_batch_schedule_tick(h) != ticks) {
        std::printf("copra_batch_schedule_tick: %lld after %d ticks\n", copra_batch_schedule_tick(h), ticks);
        return 1;
    }
    std::vector<double> xh(nxh), uh(nuh);
    std::vector<int> sh(nsh);
    HIP(hipMemcpy(xh.data(), dxh, nxh * sizeof(double), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(uh.data(), duh, nuh * sizeof(double), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(sh.data(), dsh, nsh * sizeof(int), hipMemcpyDeviceToHost));
    double dx = 0.0, du = 0.0;
    int ds = 0, bad = 0;
    for (size_t i = 0; i < nxh; ++i) {
        const double e = std::fabs(xh[i] - x_want[i]);
        if (!(e <= dx)) dx = e; // (a NaN sticks)
    }
    for (size_t i = 0; i < nuh; ++i) {
        const double e = std::fabs(uh[i] - u_want[i]);
        if (!(e <= du)) du = e;
    }
    for (size_t i = 0; i < nsh; ++i) ds += sh[i] != s_want[i], bad += sh[i] != COPRA_QP_OK;
    std::printf("tracking rollout: %d ticks x %d instances, %d solves failed, %d statuses differ, max difference of the states %.2e, of the controls %.2e\n", ticks,
        batch, bad, ds, dx, du);
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    std::fwrite(xh.data(), sizeof(double), nxh, out);
    std::fwrite(uh.data(), sizeof(double), nuh, out);
    std::fwrite(sh.data(), sizeof(int), nsh, out);
    std::fclose(out);
    copra_batch_destroy(h);
    (void)hipStreamDestroy(stream);
    for (void* q : { (void*)dw, (void*)dxh, (void*)duh, (void*)dsh }) (void)hipFree(q);
    return (ds == 0 && dx <= 1e-9 && du <= 1e-9) ? 0 : 1;
}
