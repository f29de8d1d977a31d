// emu_delay.h -- the C interface of tests/emu/emu_delay.cpp: the phase bodies of copra_amd/csrc/delay_step.hpp (input delay, ABI 16) walked
// thread by thread on the host.  tests/test_delay_abi.py mirrors EmuDelayRun with ctypes; tests/emu/emu_delay_main.cpp is the same code as a
// program for the sanitizers.
#pragma once

extern "C" {

struct EmuDelayRun {
    int batch, nx, nu, D;
    int head; // the slot of the OLDEST entry as the kernel sees it: after the push's advance
    int push;
    int ctrl_stride;
    int group, threads;
    int shared;
    int order; // of the walk (emu_walk.h): 0 ascending, 1 descending, 2 a permutation drawn from seed
    int vec2_mode; // -1: the launch's rule (delay_vec2_ok); 0: off
    unsigned long long seed;
    const double *A, *B, *d; // column-major blocks, [batch] of them or one (shared)
    const double* xnow; // [batch][nx]
    double* q; // [batch][D][nu]: the ring
    int* qs; // [D][batch]
    const double* fallback_u; // [batch][nu] or null
    const int* status; // [batch] (push)
    const double* control; // [batch][ctrl_stride] (push)
    double* x0; // [batch][nx]
    int lds_doubles, vec2_used; // out: the image's size, whether pairs were copied
};

// one launch of the kernel: stage, then D prediction steps; 0, or kEmuNoMemory / kEmuGuardTouched of emu_walk.h
int emu_delay_run(EmuDelayRun* t);

// the geometry of delay_step.hpp
long long emu_delay_image_bytes(int nx, int nu, int D);
int emu_delay_launch_group(int nx, int nu, int D);
// offsets in the order of the image, then the total (10 values): A, B, d, xa, xb, q, fb, unew, status, total
int emu_delay_layout(int nx, int nu, int D, int group, int shared, int has_fb, int* out);
int emu_delay_max(void);
}
