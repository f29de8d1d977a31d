// emu_delay_main.cpp -- tests/emu/emu_delay.cpp as a stand-alone program for the address and undefined-behaviour sanitizers
// (tests/test_delay_abi.py builds and runs it): (6, 3) and (3, 1), batch 5, group 4 -- a partial last group -- and group 1; D = 1, 2, 8;
// a model per instance and one for the batch; with and without fallback controls; failed entries at the head, in the middle and as the
// newest; 2 D + 3 launches with the push on, so that the head wraps, then one with it off.  Every array has exactly the elements the kernel
// may touch.  Exit status 0: every walk ran, the three walk orders agree bit for bit, the ring holds what was pushed and a prediction over
// nothing but held entries is the state itself.
#include "emu_delay.h"

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

struct State {
    std::vector<double> q, x0;
    std::vector<int> qs;
};

int run_shape(int nx, int nu)
{
    const int batch = 5, threads = 64, N = 4;
    const size_t b = batch;
    int bad = 0;
    for (int D : { 1, 2, 8 })
        for (int group : { 4, 1 })
            for (int shared = 0; shared < 2; ++shared)
                for (int fb = 0; fb < 2; ++fb) {
                    State res[3];
                    for (int order = 0; order < 3; ++order) {
                        Lcg g { (unsigned long long)(1000 * nx + 100 * nu + 10 * D + group) };
                        const size_t lead = shared ? 1 : b;
                        auto A = rnd(g, lead * nx * nx), B = rnd(g, lead * nx * nu), d = rnd(g, lead * nx, 0.1);
                        auto xnow = rnd(g, b * nx, 2.0), fu = rnd(g, b * nu);
                        State s { std::vector<double>(b * D * nu, 0.25), std::vector<double>(b * nx, NAN), std::vector<int>(b * D, 0) };
                        int head = 0;
                        const int ticks = 2 * D + 3;
                        for (int t = 0; t <= ticks; ++t) {
                            const int push = t < ticks;
                            auto control = rnd(g, b * nu * N);
                            std::vector<int> status(b, 0);
                            status[(size_t)(t % batch)] = 2; // a failed solve walks through the batch: newest, middle, head of its ring
                            for (int c = 0; c < nu * N; ++c) control[(size_t)(t % batch) * nu * N + c] = NAN;
                            if (push) head = (head + 1) % D;
                            EmuDelayRun r;
                            std::memset(&r, 0, sizeof r);
                            r.batch = batch, r.nx = nx, r.nu = nu, r.D = D, r.head = head, r.push = push, r.ctrl_stride = nu * N;
                            r.group = group, r.threads = threads, r.shared = shared, r.order = order, r.vec2_mode = -1, r.seed = 7;
                            r.A = A.data(), r.B = B.data(), r.d = d.data(), r.xnow = xnow.data();
                            r.q = s.q.data(), r.qs = s.qs.data(), r.fallback_u = fb ? fu.data() : nullptr;
                            r.status = push ? status.data() : nullptr, r.control = push ? control.data() : nullptr;
                            r.x0 = s.x0.data();
                            if (emu_delay_run(&r) != 0) return 1;
                            const int newest = (head + D - 1) % D;
                            for (size_t i = 0; push && i < b; ++i) { // the ring holds what was pushed: the status, and the control unless it failed
                                bool ok = s.qs[(size_t)newest * b + i] == status[i];
                                for (int c = 0; c < nu; ++c) {
                                    const double got = s.q[(i * D + newest) * nu + c];
                                    ok = ok && (status[i] == 0 ? got == control[i * nu * N + c] : std::isnan(got));
                                }
                                bad += !ok;
                            }
                            for (size_t i = 0; i < b; ++i) { // with fallback controls nothing is held and every prediction is finite
                                bool all_failed = true;
                                for (int j = 0; j < D; ++j) all_failed = all_failed && s.qs[(size_t)j * b + i] != 0;
                                for (int k = 0; k < nx; ++k) {
                                    const double got = s.x0[i * nx + k];
                                    if (!std::isfinite(got) || (!fb && all_failed && got != xnow[i * nx + k])) ++bad;
                                }
                            }
                        }
                        res[order] = s;
                    }
                    for (int order = 1; order < 3; ++order) {
                        const bool same = std::memcmp(res[0].x0.data(), res[order].x0.data(), b * nx * sizeof(double)) == 0
                            && std::memcmp(res[0].q.data(), res[order].q.data(), b * D * nu * sizeof(double)) == 0
                            && std::memcmp(res[0].qs.data(), res[order].qs.data(), b * D * sizeof(int)) == 0;
                        if (!same) {
                            std::printf("nx %d nu %d D %d group %d shared %d fb %d: walk order %d disagrees\n", nx, nu, D, group, shared, fb, order);
                            ++bad;
                        }
                    }
                }
    return bad;
}

} // namespace

int main()
{
    int bad = emu_delay_max() != 8;
    bad += run_shape(6, 3) + run_shape(3, 1);
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
