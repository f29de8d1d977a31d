// A Monte-Carlo closed-loop run from a C / C++ caller: the CoM controller of copra_amd/workloads.py::com_preview through include/copra_hip.h alone,
// copra_batch_rollout with per-tick disturbances, the histories written to a file.  Driven by tests/test_closed_loop_gpu.py, which writes the
// systems and the disturbances and checks every tick of the histories against the CPU oracle.  Usage: test_closed_loop <in> <out>
//   in:  int32 batch, N, ticks; doubles goal[6], wx[6], wu[3], xupper[6], uupper[3], A[batch][6x6], B[batch][6x3], d[batch][6], x0[batch][6],
//        w_seq[ticks][batch][6]  (A, B column-major per instance)
//   out: doubles x_hist[ticks+1][batch][6], u_hist[ticks][batch][3]; int32 status_hist[ticks][batch]
#include <copra_hip.h>
#include <hip/hip_runtime_api.h>

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
    int head[3];
    if (std::fread(head, sizeof(int), 3, in) != 3) return 2;
    const int batch = head[0], N = head[1], ticks = head[2], nx = 6, nu = 3;
    const auto read = [&](size_t count) {
        std::vector<double> v(count);
        if (std::fread(v.data(), sizeof(double), count, in) != count) v.clear();
        return v;
    };
    const std::vector<double> goal = read(6), wx = read(6), wu = read(3), xup = read(6), uup = read(3);
    const std::vector<double> A = read((size_t)batch * 36), B = read((size_t)batch * 18), d = read((size_t)batch * 6), x0 = read((size_t)batch * 6);
    const std::vector<double> w_seq = read((size_t)ticks * batch * 6);
    std::fclose(in);
    if (w_seq.empty()) return 2;

    const double inf = std::numeric_limits<double>::infinity();
    double I6[36] = {}, I3[9] = {}, zero3[3] = {}, xlow[6], ulow[3];
    for (int i = 0; i < 6; ++i) I6[7 * i] = 1.0, xlow[i] = -inf;
    for (int i = 0; i < 3; ++i) I3[4 * i] = 1.0, ulow[i] = -uup[i];
    copra_cost_desc_t costs[2] = {};
    costs[0].kind = COPRA_COST_TRAJECTORY, costs[0].rows = 6, costs[0].m_cols = 6, costs[0].M = I6, costs[0].p = goal.data(), costs[0].weights = wx.data();
    costs[1].kind = COPRA_COST_CONTROL, costs[1].rows = 3, costs[1].n_cols = 3, costs[1].N = I3, costs[1].p = zero3, costs[1].weights = wu.data();
    copra_cstr_desc_t cstrs[2] = {};
    cstrs[0].kind = COPRA_CSTR_TRAJECTORY_BOUND, cstrs[0].rows = 6, cstrs[0].lower = xlow, cstrs[0].upper = xup.data();
    cstrs[1].kind = COPRA_CSTR_CONTROL_BOUND, cstrs[1].rows = 3, cstrs[1].lower = ulow, cstrs[1].upper = uup.data();
    const copra_dims_t dims = { nx, nu, N, batch };
    copra_batch_t* h = nullptr;
    CHECK(copra_batch_create(&h, &dims, 2, costs, 2, cstrs));
    CHECK(copra_batch_set_system(h, A.data(), B.data(), d.data(), x0.data(), 0));

    const size_t nxh = (size_t)(ticks + 1) * batch * nx, nuh = (size_t)ticks * batch * nu, nsh = (size_t)ticks * batch;
    double *dw = nullptr, *dxh = nullptr, *duh = nullptr;
    int* dsh = nullptr;
    HIP(hipMalloc((void**)&dw, w_seq.size() * sizeof(double)));
    HIP(hipMalloc((void**)&dxh, nxh * sizeof(double)));
    HIP(hipMalloc((void**)&duh, nuh * sizeof(double)));
    HIP(hipMalloc((void**)&dsh, nsh * sizeof(int)));
    HIP(hipMemcpy(dw, w_seq.data(), w_seq.size() * sizeof(double), hipMemcpyHostToDevice));
    hipStream_t stream;
    HIP(hipStreamCreate(&stream));

    copra_plant_step_t step;
    copra_plant_step_init(&step); // the controller's model as plant, failed instances keep their state
    if (step.struct_size != (int)sizeof step) {
        std::printf("copra_plant_step_init: struct_size %d, sizeof %d\n", step.struct_size, (int)sizeof step);
        return 1;
    }
    CHECK(copra_batch_rollout(h, &step, ticks, dw, dxh, duh, dsh, stream));
    CHECK(copra_batch_synchronize(h));
    std::vector<double> xh(nxh), uh(nuh), xlast((size_t)batch * nx);
    std::vector<int> sh(nsh);
    HIP(hipMemcpy(xh.data(), dxh, nxh * sizeof(double), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(uh.data(), duh, nuh * sizeof(double), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(sh.data(), dsh, nsh * sizeof(int), hipMemcpyDeviceToHost));
    CHECK(copra_batch_get_x0(h, xlast.data()));
    int differ = 0, solved = 0;
    for (size_t i = 0; i < xlast.size(); ++i) differ += xlast[i] != xh[(size_t)ticks * batch * nx + i];
    for (size_t i = 0; i < nsh; ++i) solved += sh[i] == COPRA_QP_OK;
    std::printf("rollout: %d ticks x %d instances, %d solves ok, state of the handle differs from x_hist[ticks] in %d entries\n", ticks, batch, solved, differ);
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    std::fwrite(xh.data(), sizeof(double), nxh, out);
    std::fwrite(uh.data(), sizeof(double), nuh, out);
    std::fwrite(sh.data(), sizeof(int), nsh, out);
    std::fclose(out);
    copra_batch_destroy(h);
    (void)hipStreamDestroy(stream);
    for (void* q : { (void*)dw, (void*)dxh, (void*)duh, (void*)dsh }) (void)hipFree(q);
    return differ ? 1 : 0;
}
