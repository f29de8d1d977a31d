// emu_plant_noise.h -- the arguments of tests/emu/emu_plant_noise.cpp, shared with its stand-alone program
#pragma once
#include "../../copra_amd/csrc/plant_step.hpp"

extern "C" {

// One tick; every pointer as the library's launch would pass it.  build: 0 the plain tick, 1 with the disturbance estimator, 2 with the state
// observer.  knoise: walk the phase-1 bodies built with kNoise (the others never look at the sigmas).  x is the state the plant moves, in
// place (the observer's xp); xhat and dhat are updated in place.  A == NULL with build 1 or 2: no plant of its own.  sigma_w / sigma_v NULL:
// that stream is off.  lds_doubles returns the image the walk used.
struct EmuNoiseTick {
    int build, knoise, batch, nx, nu, ny, N, group, threads, shared;
    const double *A, *B, *d;
    double* x;
    const double *w, *fallback_u;
    const int* status;
    const double* control;
    double *x_out, *u_out;
    int* status_out;
    int backup_steps, fresh;
    double* plan;
    int* next;
    int* age_out;
    int gain_dense, gain_shared;
    const double *Am, *Bm, *gain;
    double *dhat, *d_out;
    double* xhat;
    const double *C, *Lx, *Ld, *v, *y_meas;
    double *y_out, *xhat_out;
    unsigned long long seed, first, tick;
    const double *sigma_w, *sigma_v;
    int per_instance, lds_doubles;
};

int emu_plant_noise_tick(EmuNoiseTick* t);
void emu_noise_fill(int batch, int rows, int stream, int per_instance, int group, int threads, unsigned long long seed, unsigned long long first,
    unsigned long long tick, const double* sigma, double* out);
void emu_philox(const unsigned* counter, const unsigned* key, unsigned* out);
void emu_noise_words(int count, const unsigned long long* seed, const unsigned long long* gi, const int* s, const int* j, const unsigned long long* t, unsigned* out);
}
