// What the factorisation kernel (pde_adi.hip) shares with the kernel that differentiates its coefficient stage
// (pde_adi_tangent_dev.h): the argument structure, the clamp and the half-row store.  One definition of each, so that
// the expression base + slope*t, its contraction and the clamp's comparison are the same code in both.
#pragma once
#include "pde_common.h"

namespace pde {
namespace {

struct FactorArgs {
    SweepTab* tab;
    int* varying;           // [C] 1 when a clamp mask of the channel differs between sweeps; followed in memory by the
                            // per-(sweep, channel) partials this kernel writes: int dpart[S][C], float kpart[S][C]
    float t_first[2];       // time of the earliest sweep of each axis
    const float* ab;
    const float* bb;
    const float* as;
    const float* bs;
    float* coef;            // [S][C][kRecAll]
    float* wide;            // optional [S][C][kWideRec]: lane-major copy of the records (pde_common.h), may be null
    float* kmax;            // optional [S] (atomic max of coeff), may be null
    int C, N, S;
    int win;                // sweeps per launch window: tab[w] describes sweeps w*win .. w*win+win-1 as ONE launch
    int smooth3, has_max;
    float cmax, eps;
    PdeSweep sweep[PDE_MAX_SWEEPS];
};

// One thread per (sweep, channel, HALF line): the two-sided factorisation makes the halves of a line
// independent up to the junction factor (one lane exchange), so a wave is 32 lines x 2 halves of one
// channel — the sweep kernels' own layout — and each thread's serial chain (divisions!) is N/2 long.
// A thread writes its half of every image row as 16-byte stores.  No LDS.  The row-layout images
// (KAPX, MASKX) of a y sweep are NOT transposed through memory: thread (h, hf) recomputes the
// coefficients of its half of row h directly from the parameters (three rows for the smoothed variants).
template <int N>
__device__ __forceinline__ void store_half_row(float* row, int hf, const float (&v)[N / 2]) {
    // image row = [16 floats: half seen from the low end][16: half seen from the high end][4 pad]
    float h[kHalfPad];
#pragma unroll
    for (int k = 0; k < kHalfPad; ++k) h[k] = 0.f;
#pragma unroll
    for (int k = 0; k < N / 2; ++k) h[k] = v[k];
    float4* dst = reinterpret_cast<float4*>(row + hf * kHalfPad);
#pragma unroll
    for (int q = 0; q < kHalfPad / 4; ++q) dst[q] = make_float4(h[4 * q], h[4 * q + 1], h[4 * q + 2], h[4 * q + 3]);
    if (hf) *reinterpret_cast<float4*>(row + 2 * kHalfPad) = make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ float clamp_theta(float th, const FactorArgs& a, bool& pass) {
    pass = (th >= a.eps) && (!a.has_max || th <= a.cmax);                  // clamp passes the gradient
    th = fmaxf(th, a.eps);
    if (a.has_max) th = fminf(th, a.cmax);
    return th;
}

constexpr int kFacLd = PDE_MAX_N + 1;     // LDS row stride of the staged parameter planes
}  // namespace
}  // namespace pde
