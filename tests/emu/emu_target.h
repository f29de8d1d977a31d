// emu_target.h -- the C interface of tests/emu/emu_target.cpp: the phase bodies of copra_amd/csrc/target_step.hpp (steady-state targets, ABI 15)
// walked thread by thread on the host.  tests/test_target_abi.py mirrors EmuTarget with ctypes; tests/emu/emu_target_main.cpp is the same
// code as a program for the sanitizers.
#pragma once

extern "C" {

struct EmuTarget {
    int batch, nx, nu, group, threads;
    int per_instance;
    int order; // of the walk (emu_walk.h): 0 ascending, 1 descending, 2 a permutation drawn from seed
    int vec2_mode; // -1: the launch's rule (target_prepare); 0: 8-byte accesses everywhere
    unsigned long long seed;
    const double *A, *B, *d; // [batch][nx x nx], [batch][nx x nu] column-major, [batch][nx]
    const double* H; // [nu x nx] column-major
    const double* r; // [per_instance ? batch : 1][steps][nu]
    long long steps, tau; // the block read is min(tau, steps - 1): tau is the schedule tick plus the offset
    int ncost;
    const int* cost_rows; // [ncost] r_c
    const int* cost_blocks; // [ncost] S_c
    const double* const* cost_map; // [ncost] T_c [r_c x (nx + nu)] column-major
    double* const* cost_out; // [ncost] [batch][S_c r_c], written in place
    double* z; // [batch][nx + nu], written in place
    int* status; // [batch]
    int lds_doubles, vec2_used; // out: the image's size; bit 0: pairs loaded, bit 1: z stored in pairs, bit 2 + c: cost c stored in pairs
    int nan_left; // out: a good instance left a NaN in its z column of the image
};

// one launch; 0, or kEmuNoMemory / kEmuGuardTouched of emu_walk.h
int emu_target_run(EmuTarget* t);

// the geometry of target_step.hpp: one wave's image in bytes, the group of the launch, the image's parts (oM, oH, oT, ost, total), the
// limits; map_doubles is the sum over the driven costs of even(r_c (nx + nu))
long long emu_target_image_bytes(int nx, int nu, int map_doubles);
int emu_target_launch_group(int nx, int nu, int map_doubles);
int emu_target_layout(int nx, int nu, int group, int map_doubles, int* out);
int emu_target_threads(void);
int emu_target_max_costs(void);
long long emu_target_lds_max(void);
}
