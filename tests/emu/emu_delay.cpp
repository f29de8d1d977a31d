// emu_delay.cpp -- the delay kernel's phase bodies (copra_amd/csrc/delay_step.hpp) on the host: a walker over the stage and the D prediction
// steps with a NaN-filled image, the guard words and the walk orders of emu_walk.h.
// Compile with -ffp-contract=off: the expectation (tests/delay_ref.py) rounds every product and every sum.
#include "emu_delay.h"

#include "../../copra_amd/csrc/delay_step.hpp"
#include "emu_walk.h"

using namespace copra_hip;

extern "C" {

int emu_delay_run(EmuDelayRun* t)
{
    DelayArgs P {};
    P.batch = t->batch, P.nx = t->nx, P.nu = t->nu, P.D = t->D;
    P.head = t->head, P.push = t->push, P.ctrl_stride = t->ctrl_stride;
    P.group = t->group, P.shared = t->shared;
    P.A = t->A, P.B = t->B, P.d = t->d;
    P.xnow = t->xnow, P.q = t->q, P.qs = t->qs;
    P.fallback_u = t->fallback_u, P.status = t->status, P.control = t->control;
    P.x0 = t->x0;
    P.vec2 = t->vec2_mode < 0 ? delay_vec2_ok(P) : 0;
    t->vec2_used = P.vec2;
    const DelayLds L = delay_lds(P);
    t->lds_doubles = L.total;
    emu::Image img((size_t)L.total);
    if (!img.lds) return emu::kEmuNoMemory;
    const int grid = (P.batch + P.group - 1) / P.group;
    return emu::walk(img, grid, 1 + P.D, t->threads, t->order, t->seed, [&](int wg, int ph, int tid) {
        if (ph == 0) delay_stage(P, wg, tid, t->threads, img.lds);
        else delay_predict(P, wg, tid, t->threads, img.lds, ph - 1);
    });
}

long long emu_delay_image_bytes(int nx, int nu, int D) { return (long long)delay_image_bytes(nx, nu, D); }
int emu_delay_launch_group(int nx, int nu, int D) { return delay_group(nx, nu, D); }
int emu_delay_layout(int nx, int nu, int D, int group, int shared, int has_fb, int* out)
{
    const DelayLds L = delay_lds(nx, nu, D, group, shared, has_fb);
    const int v[10] = { L.oA, L.oB, L.od, L.oxa, L.oxb, L.oq, L.ofb, L.oun, L.ost, L.total };
    for (int i = 0; i < 10; ++i) out[i] = v[i];
    return 10;
}
int emu_delay_max(void) { return kDelayMax; }
}
