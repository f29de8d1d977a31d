// emu_target_main.cpp -- tests/emu/emu_target.cpp as a stand-alone program for the address and undefined-behaviour sanitizers
// (tests/test_target_abi.py builds and runs it): (6, 3), (9, 3) and (2, 1); batches 1, group - 1, group + 1 and 2 group + 1 at the launch's own
// group; a shared and a per-instance setpoint signal read below and past its end; one, two and eight driven costs with odd rows and
// S = 1, 2, 5; a zero column of B and a NaN in d among good instances; three walk orders.  Every array has exactly the elements the kernel
// may touch.  Exit status 0: every walk ran, the walk orders agree bit for bit, a good instance satisfies its equations and a singular
// one kept its bits.
#include "emu_target.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Lcg {
    unsigned long long s;
    double next()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) / 9007199254740992.0 - 0.5;
    }
};

std::vector<double> rnd(Lcg& g, size_t n, double scale = 1.0)
{
    std::vector<double> v(n);
    for (double& x : v) x = scale * g.next();
    return v;
}

int even(int v) { return (v + 1) & ~1; }

int run_shape(int nx, int nu, int ncost)
{
    const int n = nx + nu, threads = emu_target_threads();
    const int rows_of[8] = { nx, nu, 5, 1, 3, 2, 7, 4 }, blocks_of[8] = { 1, 2, 5, 1, 2, 1, 1, 5 };
    int maps = 0;
    for (int k = 0; k < ncost; ++k) maps += even(rows_of[k] * n);
    const int group = emu_target_launch_group(nx, nu, maps);
    Lcg g { (unsigned long long)(1000 * nx + 10 * nu + ncost) };
    int bad = 0;
    for (int batch : { 1, group - 1, group + 1, 2 * group + 1 })
        for (int per = 0; per < 2; ++per) {
            const size_t b = (size_t)batch, steps = 3;
            // a double integrator per axis where the shape allows it (a zero diagonal of A - I), a random system otherwise
            std::vector<double> A(b * nx * nx, 0.0), B = rnd(g, b * nx * nu, 2.0), d = rnd(g, b * nx, 0.1), H((size_t)nu * nx, 0.0);
            for (size_t i = 0; i < b; ++i)
                for (int r = 0; r < nx; ++r)
                    for (int j = 0; j < nx; ++j) A[i * nx * nx + r + (size_t)nx * j] = (r == j ? 1.0 : 0.0) + (j == r + nu ? 0.1 : 0.0) + (nx < 2 * nu ? 0.3 * g.next() : 0.0);
            for (int a = 0; a < nu; ++a) H[a + (size_t)nu * a] = 1.0;
            const size_t zero_col = b > 2 ? 2 : b, nan_d = b > 4 ? b - 2 : b; // (b: none)
            if (zero_col < b)
                for (int r = 0; r < nx; ++r) B[zero_col * nx * nu + r + (size_t)nx * (nu - 1)] = 0.0;
            if (nan_d < b) d[nan_d * nx] = NAN;
            const std::vector<double> sig = rnd(g, (per ? b : 1) * steps * nu);
            std::vector<std::vector<double>> map((size_t)ncost);
            std::vector<int> rows((size_t)ncost), blocks((size_t)ncost);
            for (int k = 0; k < ncost; ++k) rows[(size_t)k] = rows_of[k], blocks[(size_t)k] = blocks_of[k], map[(size_t)k] = rnd(g, (size_t)rows_of[k] * n);
            for (long long tau : { 0LL, 1LL, 5LL }) {
                std::vector<double> z0[3];
                std::vector<int> st0[3];
                std::vector<std::vector<double>> out0[3];
                for (int order = 0; order < 3; ++order) {
                    std::vector<double> z(b * n, -3.5);
                    std::vector<int> st(b, -9);
                    std::vector<std::vector<double>> out((size_t)ncost);
                    std::vector<const double*> mp((size_t)ncost);
                    std::vector<double*> op((size_t)ncost);
                    for (int k = 0; k < ncost; ++k) {
                        out[(size_t)k].assign(b * (size_t)(rows_of[k] * blocks_of[k]), -4.5);
                        mp[(size_t)k] = map[(size_t)k].data(), op[(size_t)k] = out[(size_t)k].data();
                    }
                    EmuTarget t;
                    std::memset(&t, 0, sizeof t);
                    t.batch = batch, t.nx = nx, t.nu = nu, t.group = group, t.threads = order == 2 ? 3 : threads, t.per_instance = per;
                    t.order = order, t.vec2_mode = -1, t.seed = 7;
                    t.A = A.data(), t.B = B.data(), t.d = d.data(), t.H = H.data(), t.r = sig.data();
                    t.steps = (long long)steps, t.tau = tau, t.ncost = ncost;
                    t.cost_rows = rows.data(), t.cost_blocks = blocks.data(), t.cost_map = mp.data(), t.cost_out = op.data();
                    t.z = z.data(), t.status = st.data();
                    if (emu_target_run(&t) != 0 || t.nan_left) return 1;
                    z0[order] = z, st0[order] = st, out0[order] = out;
                }
                for (int order = 1; order < 3; ++order)
                    if (z0[0].size() != z0[order].size() || std::memcmp(z0[0].data(), z0[order].data(), z0[0].size() * sizeof(double)) != 0 || st0[0] != st0[order]
                        || out0[0] != out0[order]) {
                        std::printf("nx %d nu %d costs %d batch %d per %d: walk order %d disagrees\n", nx, nu, ncost, batch, per, order);
                        ++bad;
                    }
                const size_t row = (size_t)(tau < (long long)steps - 1 ? tau : (long long)steps - 1);
                for (size_t i = 0; i < b; ++i) {
                    const bool singular = i == zero_col || i == nan_d;
                    const double* z = z0[0].data() + i * n;
                    bool ok = st0[0][i] == (singular ? 1 : 0);
                    if (singular) {
                        for (int j = 0; j < n; ++j) ok = ok && z[j] == -3.5;
                        for (int k = 0; k < ncost; ++k)
                            for (int e = 0; e < rows_of[k] * blocks_of[k]; ++e) ok = ok && out0[0][(size_t)k][i * (size_t)(rows_of[k] * blocks_of[k]) + e] == -4.5;
                    } else { // the equations, to a tolerance far above the rounding of a system this small and far below a wrong entry
                        double zmax = 1.0;
                        for (int j = 0; j < n; ++j) zmax = std::fmax(zmax, std::fabs(z[j]));
                        for (int r = 0; r < nx; ++r) {
                            double acc = d[i * nx + r] - z[r];
                            for (int j = 0; j < nx; ++j) acc += A[i * nx * nx + r + (size_t)nx * j] * z[j];
                            for (int c = 0; c < nu; ++c) acc += B[i * nx * nu + r + (size_t)nx * c] * z[nx + c];
                            ok = ok && std::fabs(acc) <= 1e-9 * zmax;
                        }
                        for (int a = 0; a < nu; ++a) ok = ok && std::fabs(z[a] - sig[((per ? i : 0) * steps + row) * nu + a]) <= 1e-9 * zmax;
                        for (int k = 0; k < ncost; ++k)
                            for (int e = 0; e < rows_of[k] * blocks_of[k]; ++e) {
                                double acc = 0.0;
                                for (int j = 0; j < n; ++j) acc += map[(size_t)k][(size_t)(e % rows_of[k]) + (size_t)rows_of[k] * j] * z[j];
                                ok = ok && out0[0][(size_t)k][i * (size_t)(rows_of[k] * blocks_of[k]) + e] == acc;
                            }
                    }
                    if (!ok) {
                        std::printf("nx %d nu %d costs %d batch %d per %d tau %lld: instance %zu is wrong\n", nx, nu, ncost, batch, per, tau, i);
                        ++bad;
                    }
                }
            }
        }
    return bad;
}

} // namespace

int main()
{
    int bad = (emu_target_max_costs() != 8);
    bad += run_shape(6, 3, 2) + run_shape(6, 3, 8) + run_shape(9, 3, 1) + run_shape(2, 1, 2);
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
