// emu_trace_quant.h -- the C interface of tests/emu/emu_trace_quant.cpp: the bodies of copra_amd/csrc/trace_quant_step.hpp (trace quantiles, ABI
// 18) walked on the host at the launch's own workgroup and thread counts -- one workgroup per row, every pass thread by thread in the walk
// orders of emu_walk.h over an LDS block and a key buffer that start out as garbage, the scan lane by lane -- and the host's rule for which
// tick takes which slot.  tests/test_trace_quant_abi.py mirrors the structs with ctypes; tests/emu/emu_trace_quant_main.cpp is the same code
// as a program for the sanitizers.
#pragma once

extern "C" {

struct EmuQuantTick {
    int batch, nx, nu, what;
    int order; // of the walk (emu_walk.h): 0 ascending, 1 descending, 2 a permutation drawn from seed
    int nq;
    unsigned long long seed;
    const double* x; // [batch][nx]
    const double* u; // [batch][nu]
    const double* est; // [batch][nx] or null: the err rows are empty on this tick
    const int* age; // [batch]
    const double *x_lo, *x_hi, *u_lo, *u_hi;
    double level[8];
    double* out; // [rows][nq], written
    int rows; // out: the slot's rows
};

struct EmuQuantClock { // TraceClock of trace_step.hpp
    long long tick, recorded, missed, capacity;
    int every;
};

// one recorded tick into t->out; 0, or kEmuNoMemory / kEmuGuardTouched of emu_walk.h (the guard: behind the key buffer)
int emu_trace_quant_tick(EmuQuantTick* t);

// one tick of a trace whose quantile slots lie in `buffer` ([capacity][rows][nq]): the clock moves (trace_next_slot); on a recorded tick
// t->out is set and the tick is walked.  Returns the slot written, -1 where the tick writes none, or -10 + an error of emu_trace_quant_tick
long long emu_trace_quant_record(EmuQuantTick* t, EmuQuantClock* clock, double* buffer);

unsigned long long emu_trace_quant_key(double v);
long long emu_trace_quant_rank(double p, long long n);
int emu_trace_quant_sizes(int* max_levels, int* threads, int* lds_bytes);
}
