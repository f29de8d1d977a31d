// emu_ref_window.cpp -- the reference-window kernel's body (copra_amd/csrc/ref_window.hpp) on the host: every workgroup's threads are walked one
// after the other, with the launch shaped by the function the library shapes it with (ref_window_prepare).  Compiled by
// tests/test_reference_schedule_abi.py itself (g++ -shared into its tmp_path); no part of the emulator's Makefile.
#include "../../copra_amd/csrc/ref_window.hpp"

using namespace copra_hip;

extern "C" {

// One launch for `ncost` costs (at most kRefWindowMax): sched[k] / out[k] are the arrays of cost k, steps / first / r / S / per_instance its
// descriptor.  vec2_used[k] (may be null) says whether cost k was copied two doubles per lane.  Returns 0; -1: too many costs or threads not a
// power of two.
int emu_ref_window(int batch, int ncost, int group, int threads, const double* const* sched, double* const* out, const long long* steps,
    const long long* first, const int* r, const int* S, const int* per_instance, int* vec2_used)
{
    if (ncost < 0 || ncost > kRefWindowMax || threads < 1 || (threads & (threads - 1))) return -1;
    RefWindowArgs P {};
    P.batch = batch, P.ncost = ncost, P.group = group;
    for (int k = 0; k < ncost; ++k) {
        RefWindowCost& c = P.c[k];
        c.sched = sched[k], c.out = out[k], c.steps = steps[k], c.first = first[k], c.r = r[k], c.S = S[k], c.per_instance = per_instance[k];
    }
    ref_window_prepare(P, threads);
    if (vec2_used)
        for (int k = 0; k < ncost; ++k) vec2_used[k] = P.c[k].vec2;
    const int grid = (batch + group - 1) / group;
    for (int wg = 0; wg < grid; ++wg)
        for (int tid = 0; tid < threads; ++tid) ref_window_body(P, wg, tid, threads);
    return 0;
}

int emu_ref_window_group(void) { return kRefWindowGroup; }

} // extern "C"
