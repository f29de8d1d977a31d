// emu_score.h -- the C interface of tests/emu/emu_score.cpp: the phase bodies of copra_amd/csrc/score_step.hpp (closed-loop scores, ABI 14)
// walked thread by thread on the host, and the summary's reduction applied lane by lane in the order that header writes down.
// tests/test_score_abi.py mirrors EmuScoreTick with ctypes; tests/emu/emu_score_main.cpp is the same code as a program for the sanitizers.
#pragma once

extern "C" {

struct EmuScoreTick {
    int batch, nx, nu, group, threads;
    int dense, per_instance;
    int order; // of the walk (emu_walk.h): 0 ascending, 1 descending, 2 a permutation drawn from seed
    int vec2_mode; // -1: the launch's rule (score_vec2_ok); 0: off
    unsigned long long seed;
    const double* x; // [batch][nx]
    const double* u; // [batch][nu]
    const int* age; // [batch]
    const double *qx, *ru, *x_ref;
    long long ref_steps, tau; // the row read is min(tau, ref_steps - 1)
    const double *x_lo, *x_hi, *u_lo, *u_hi;
    double tol;
    void* rec; // [batch] records of 64 bytes, updated in place
    int lds_doubles, vec2_used; // out: the image's size, whether pairs were copied
};

// one tick's update of every record; 0, or kEmuNoMemory / kEmuGuardTouched of emu_walk.h
int emu_score_tick(EmuScoreTick* t);

// the summary of `count` records: stage 1 and stage 2 as the kernel runs them; out is a copra_score_summary_t.  0 or kEmuNoMemory
int emu_score_reduce(long long count, const void* rec, void* out);

// the geometry of score_step.hpp
long long emu_score_image_bytes(int nx, int nu, int dense);
int emu_score_launch_group(int nx, int nu, int dense);
// offsets in the order of the image, then the total (14 values); flags: dense, per_instance, has qx, ru, x_ref, x_lo, x_hi, u_lo, u_hi
int emu_score_layout(int nx, int nu, int group, const int* flags, int* out);
int emu_score_chunk(void);
int emu_score_threads(void);
int emu_score_sizes(int* record, int* stat, int* summary);
}
