// emu_limit_window.cpp -- the limit-window kernel's body (copra_amd/csrc/limit_window.hpp) on the host: every workgroup's threads are walked one
// after the other, with the launch shaped by the function the library shapes it with (limit_window_prepare).  Compiled by
// tests/test_limit_schedule_abi.py itself (g++ -shared into its tmp_path); no part of the emulator's Makefile.
#include "../../copra_amd/csrc/limit_window.hpp"

using namespace copra_hip;

extern "C" {

// One launch for `nwin` windows (at most kLimitWindowMax): sched[k] is the schedule of window k, out[k] the buffer it is written into
// ([batch][stride[k]], the window at row0[k]); steps / first / r / S / per_instance / preview its descriptor.  vec2_used[k] (may be null) says
// whether window k was copied two doubles per lane.  Returns 0; -1: too many windows or threads not a power of two; -2: a window that does not
// fit its stride.
int emu_limit_window(int batch, int nwin, int group, int threads, const double* const* sched, double* const* out, const long long* steps,
    const long long* first, const int* stride, const int* row0, const int* r, const int* S, const int* per_instance, const int* preview, int* vec2_used)
{
    if (nwin < 0 || nwin > kLimitWindowMax || threads < 1 || (threads & (threads - 1))) return -1;
    LimitWindowArgs P {};
    P.batch = batch, P.nwin = nwin, P.group = group;
    for (int k = 0; k < nwin; ++k) {
        LimitWindow& c = P.w[k];
        if (row0[k] < 0 || row0[k] + r[k] * S[k] > stride[k]) return -2;
        c.sched = sched[k], c.out = out[k], c.steps = steps[k], c.first = first[k], c.stride = stride[k], c.row0 = row0[k], c.r = r[k], c.S = S[k];
        c.per_instance = per_instance[k], c.preview = preview[k];
    }
    limit_window_prepare(P, threads);
    if (vec2_used)
        for (int k = 0; k < nwin; ++k) vec2_used[k] = P.w[k].vec2;
    const int grid = (batch + group - 1) / group;
    for (int wg = 0; wg < grid; ++wg)
        for (int tid = 0; tid < threads; ++tid) limit_window_body(P, wg, tid, threads);
    return 0;
}

int emu_limit_window_group(void) { return kLimitWindowGroup; }
int emu_limit_window_max(void) { return kLimitWindowMax; }

} // extern "C"
