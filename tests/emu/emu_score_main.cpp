// emu_score_main.cpp -- tests/emu/emu_score.cpp as a stand-alone program for the address and undefined-behaviour sanitizers
// (tests/test_score_abi.py builds and runs it): (6, 3) and (3, 1), batch 5, group 4 -- a partial last group, odd row counts -- and group 1;
// diagonal and dense weights, shared and per-instance measures, every optional array given and not, ref_steps 1 and 4, held instances with
// NaN controls; then the reduction at record counts around a chunk.  Every array has exactly the elements the kernel may touch.  Exit
// status 0: every walk ran, the walk orders agree bit for bit and the counters are what the ages say.
#include "emu_score.h"

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

std::vector<double> rnd(Lcg& g, size_t n, double scale = 1.0, double shift = 0.0)
{
    std::vector<double> v(n);
    for (double& x : v) x = shift + scale * g.next();
    return v;
}

struct Rec { // copra_score_record_t
    double jx, ju, viol_sum, viol_max, peak;
    int ticks, held, replayed, fallback, violating, first_violation;
};

int run_shape(int nx, int nu)
{
    const int batch = 5, threads = 64;
    const size_t b = batch;
    Lcg g { (unsigned long long)(1000 * nx + nu) };
    int bad = 0;
    for (int group : { 4, 1 })
        for (int dense = 0; dense < 2; ++dense)
            for (int per = 0; per < 2; ++per)
                for (int opt = 0; opt < 3; ++opt) // 0: every array, ref_steps 4; 1: every array, a constant goal; 2: weights only
                {
                    const size_t lead = per ? b : 1, steps = opt == 0 ? 4 : 1;
                    auto x = rnd(g, b * nx, 4.0), u = rnd(g, b * nu, 4.0);
                    auto qx = rnd(g, lead * (dense ? nx * nx : nx), 1.0, 1.0), ru = rnd(g, lead * (dense ? nu * nu : nu), 1.0, 1.0);
                    auto ref = rnd(g, lead * steps * nx), xlo = rnd(g, lead * nx, 0.5, -1.0), xhi = rnd(g, lead * nx, 0.5, 1.0);
                    auto ulo = rnd(g, lead * nu, 0.5, -1.0), uhi = rnd(g, lead * nu, 0.5, 1.0);
                    xhi[0] = INFINITY, ulo[0] = -INFINITY;
                    std::vector<int> age = { 0, 2, -1, -2, -2 };
                    for (int c = 0; c < nu; ++c) u[3 * nu + c] = u[4 * nu + c] = NAN; // (held: their control is never used)
                    std::vector<Rec> res[3];
                    for (int order = 0; order < 3; ++order) {
                        std::vector<Rec> rec(b);
                        std::memset(rec.data(), 0, b * sizeof(Rec));
                        for (long long tau = 2; tau < 5; ++tau) { // below, at and beyond the end of a signal of 4 steps
                            EmuScoreTick t;
                            std::memset(&t, 0, sizeof t);
                            t.batch = batch, t.nx = nx, t.nu = nu, t.group = group, t.threads = threads, t.dense = dense, t.per_instance = per;
                            t.order = order, t.vec2_mode = -1, t.seed = 7;
                            t.x = x.data(), t.u = u.data(), t.age = age.data(), t.qx = qx.data(), t.ru = ru.data();
                            if (opt < 2) {
                                t.x_ref = ref.data(), t.ref_steps = (long long)steps;
                                t.x_lo = xlo.data(), t.x_hi = xhi.data(), t.u_lo = ulo.data(), t.u_hi = uhi.data();
                            }
                            t.tau = tau, t.tol = 0.25, t.rec = rec.data();
                            if (emu_score_tick(&t) != 0) return 1;
                        }
                        res[order] = rec;
                    }
                    for (int order = 1; order < 3; ++order)
                        if (std::memcmp(res[0].data(), res[order].data(), b * sizeof(Rec)) != 0) {
                            std::printf("nx %d nu %d group %d dense %d per %d opt %d: walk order %d disagrees\n", nx, nu, group, dense, per, opt, order);
                            ++bad;
                        }
                    for (size_t i = 0; i < b; ++i) {
                        const Rec& r = res[0][i];
                        const bool ok = r.ticks == 3 && r.held == 3 * (age[i] == -2) && r.replayed == 3 * (age[i] >= 1) && r.fallback == 3 * (age[i] == -1)
                            && std::isfinite(r.jx) && std::isfinite(r.ju) && std::isfinite(r.viol_sum) && (age[i] != -2 || r.ju == 0.0);
                        if (!ok) {
                            std::printf("nx %d nu %d group %d dense %d per %d opt %d: record %zu is wrong\n", nx, nu, group, dense, per, opt, i);
                            ++bad;
                        }
                    }
                }
    return bad;
}

int run_reduce()
{
    int chunk = emu_score_chunk(), bad = 0;
    Lcg g { 5 };
    for (long long count : { 1LL, 63LL, 64LL, 65LL, (long long)chunk - 1, (long long)chunk, (long long)chunk + 1, 2LL * chunk + 1 }) {
        std::vector<Rec> rec((size_t)count);
        for (Rec& r : rec) {
            r.jx = 10.0 + g.next(), r.ju = g.next(), r.viol_sum = g.next() + 0.5, r.viol_max = g.next() + 0.5, r.peak = NAN;
            r.ticks = 3, r.held = g.next() > 0.4, r.replayed = 1, r.fallback = 0, r.violating = g.next() > 0.0, r.first_violation = r.violating;
        }
        rec[(size_t)(count / 2)].jx = NAN;
        long long out[42];
        if (emu_score_reduce(count, rec.data(), out) != 0) return 1;
        long long held = 0;
        for (const Rec& r : rec) held += r.held != 0;
        // (n of jx, n of peak, the total of ticks, instances_held: words 0, 28, 35, 41 of the summary)
        if (out[0] != count - 1 || out[28] != 0 || out[35] != 3 * count || out[41] != held) {
            std::printf("reduce %lld: wrong counts\n", count);
            ++bad;
        }
    }
    return bad;
}

} // namespace

int main()
{
    int record = 0, stat = 0, summary = 0;
    emu_score_sizes(&record, &stat, &summary);
    int bad = (record != 64) + (stat != 56) + (summary != 336);
    bad += run_shape(6, 3) + run_shape(3, 1) + run_reduce();
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
