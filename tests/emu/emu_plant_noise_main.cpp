// emu_plant_noise_main.cpp -- tests/emu/emu_plant_noise.cpp as a stand-alone program for the address and undefined-behaviour sanitizers
// (tests/test_noise_abi.py builds and runs it): (6, 3, 3) and (3, 1, 1), batch 5, group 4 -- a partial last group, an odd row count -- all
// three builds of the tick with process (and, for the observer, sensor) noise on, sigma shared and per instance, w / v given and not, and the
// fill kernel's body.  Every array has exactly the elements the kernel may touch.  Exit status 0: every walk ran and the tick drew what the
// fill gives.
#include "emu_plant_noise.h"

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

std::vector<double> rnd(Lcg& g, size_t n, double scale = 1.0, double shift = 0.0)
{
    std::vector<double> v(n);
    for (double& x : v) x = shift + scale * g.next();
    return v;
}

int run_shape(int nx, int nu, int ny)
{
    const int batch = 5, group = 4, N = 3, threads = 64;
    Lcg g { (unsigned long long)(1000 * nx + ny) };
    const size_t b = batch;
    int bad = 0;
    for (int build = 0; build < 3; ++build)
        for (int per = 0; per < 2; ++per)
            for (int given = 0; given < 2; ++given) {
                auto A = rnd(g, b * nx * nx), B = rnd(g, b * nx * nu), d = rnd(g, b * nx), Am = rnd(g, b * nx * nx), Bm = rnd(g, b * nx * nu);
                auto gain = rnd(g, b * nx), C = rnd(g, (size_t)ny * nx), Lx = rnd(g, (size_t)nx * ny), Ld = rnd(g, (size_t)nx * ny);
                auto w = rnd(g, b * nx, 0.01), v = rnd(g, b * ny, 0.01), control = rnd(g, b * nu * N), fb = rnd(g, b * nu);
                auto sw = rnd(g, (per ? b : 1) * nx, 1.0, 1.0), sv = rnd(g, (per ? b : 1) * ny, 1.0, 1.0);
                const auto x0 = rnd(g, b * nx), dh0 = rnd(g, b * nx), xh0 = rnd(g, b * nx);
                std::vector<int> status(b, 0);
                status[3] = 2; // (a failed instance: its control is never read)
                for (int c = 0; c < nu * N; ++c) control[3 * nu * N + c] = NAN;
                std::vector<double> tw(b * nx), tv(b * ny);
                emu_noise_fill(batch, nx, 0, per, 2, threads, 99, 4294967291ull, (1ull << 32) + build, sw.data(), tw.data());
                emu_noise_fill(batch, ny, 1, per, 3, threads, 99, 4294967291ull, (1ull << 32) + build, sv.data(), tv.data());
                std::vector<double> res[2];
                for (int explicit_terms = 0; explicit_terms < 2; ++explicit_terms) {
                    auto x = x0, dhat = dh0, xhat = xh0;
                    std::vector<double> x_out(b * nx), u_out(b * nu), d_out(b * nx), y_out(b * ny), xhat_out(b * nx);
                    std::vector<int> s_out(b), a_out(b);
                    std::vector<double> we(b * nx), ve(b * ny);
                    for (size_t i = 0; i < we.size(); ++i) we[i] = given ? w[i] + tw[i] : tw[i];
                    for (size_t i = 0; i < ve.size(); ++i) ve[i] = given ? v[i] + tv[i] : tv[i];
                    EmuNoiseTick t;
                    std::memset(&t, 0, sizeof t);
                    t.build = build, t.knoise = !explicit_terms, t.batch = batch, t.nx = nx, t.nu = nu, t.ny = ny, t.N = N, t.group = group, t.threads = threads;
                    t.A = A.data(), t.B = B.data(), t.d = d.data(), t.x = x.data(), t.fallback_u = fb.data(), t.status = status.data(), t.control = control.data();
                    t.x_out = x_out.data(), t.u_out = u_out.data(), t.status_out = s_out.data(), t.age_out = a_out.data(), t.fresh = 1;
                    t.gain_shared = build == 2;
                    t.Am = Am.data(), t.Bm = Bm.data(), t.gain = gain.data(), t.dhat = dhat.data(), t.d_out = d_out.data();
                    t.xhat = xhat.data(), t.C = C.data(), t.Lx = Lx.data(), t.Ld = Ld.data(), t.y_out = y_out.data(), t.xhat_out = xhat_out.data();
                    if (explicit_terms) {
                        t.w = we.data(), t.v = build == 2 ? ve.data() : nullptr;
                    } else {
                        t.w = given ? w.data() : nullptr, t.v = given && build == 2 ? v.data() : nullptr;
                        t.seed = 99, t.first = 4294967291ull, t.tick = (1ull << 32) + build; // (first + batch == 2^32)
                        t.sigma_w = sw.data(), t.sigma_v = build == 2 ? sv.data() : nullptr, t.per_instance = per;
                    }
                    if (emu_plant_noise_tick(&t) != 0) return 1;
                    res[explicit_terms] = x;
                    res[explicit_terms].insert(res[explicit_terms].end(), dhat.begin(), dhat.end());
                    res[explicit_terms].insert(res[explicit_terms].end(), xhat.begin(), xhat.end());
                    res[explicit_terms].insert(res[explicit_terms].end(), y_out.begin(), build == 2 ? y_out.end() : y_out.begin());
                }
                if (res[0].size() != res[1].size() || std::memcmp(res[0].data(), res[1].data(), res[0].size() * sizeof(double)) != 0) {
                    std::printf("nx %d ny %d build %d per %d given %d: the tick and the fill disagree\n", nx, ny, build, per, given);
                    ++bad;
                }
            }
    return bad;
}

} // namespace

int main()
{
    const int bad = run_shape(6, 3, 3) + run_shape(3, 1, 1);
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
