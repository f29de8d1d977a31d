// emu_trace.h -- the C interface of tests/emu/emu_trace.cpp: the bodies of copra_amd/csrc/trace_step.hpp (ensemble traces, ABI 17) walked on the
// host at the launch's own workgroup and thread counts -- stage 1's copy into a NaN-filled image with a guard behind it, every thread's fold of
// every row, the lane tree and the fold of the waves applied lane by lane, stage 2 over the partials -- and the host's rule for which tick
// takes which slot.  tests/test_trace_abi.py mirrors the structs with ctypes; tests/emu/emu_trace_main.cpp is the same code as a program for
// the sanitizers.
#pragma once

extern "C" {

struct EmuTraceTick {
    int batch, nx, nu, what;
    int order; // of the walk (emu_walk.h): 0 ascending, 1 descending, 2 a permutation drawn from seed
    int lds_mode; // -1: the launch's rule (trace_in_lds); 0: direct loads; 1: the image
    int vec2_mode; // -1: the launch's rule (trace_vec2_ok); 0: off
    unsigned long long seed;
    const double* x; // [batch][nx]
    const double* u; // [batch][nu]
    const double* est; // [batch][nx] or null: the err rows are empty on this tick
    const int* age; // [batch]
    const double *x_lo, *x_hi, *u_lo, *u_hi;
    double tol;
    long long tick, tau; // what the head reports
    void* slot; // 64 + 56 rows bytes, written
    int rows, lds_doubles, lds_used, vec2_used; // out: the slot's rows, the image's size, whether it was used, whether pairs were copied
};

struct EmuTraceClock { // TraceClock of trace_step.hpp
    long long tick, recorded, missed, capacity;
    int every;
};

// one recorded tick into t->slot: stage 1 over every chunk, stage 2 over the partials; 0, or kEmuNoMemory / kEmuGuardTouched of emu_walk.h
int emu_trace_tick(EmuTraceTick* t);

// one tick of a trace whose slots lie in `buffer`: the clock moves (trace_next_slot); on a recorded tick t->tick and t->slot are set and the
// tick is walked.  Returns the slot written, -1 where the tick writes none, or -10 + an error of emu_trace_tick
long long emu_trace_record(EmuTraceTick* t, EmuTraceClock* clock, void* buffer);

// stage 2 alone: `chunks` slot-shaped partials of `rows` rows -> slot.  0
int emu_trace_stage2(int rows, long long chunks, const void* partials, long long tick, long long tau, void* slot);

int emu_trace_rows(int what, int nx, int nu, int limits);
long long emu_trace_slot_bytes(int rows);
int emu_trace_in_lds(int nx, int nu, int what, int x_limits, int u_limits);
int emu_trace_sizes(int* head, int* stat);
}
