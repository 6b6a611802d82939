// K1 for ANY plane (2 <= H, W <= 128): the implicit sweeps of mnist_test.py:50-198 / cifar10.py:86-211 with one THREAD per
// line and the plane in LDS.  The fused kernels of pde_adi_dev.h hold a line in the registers of two lanes and exist for
// N = 8, 12, ..., 32 — the sizes the reference's own call sites use; its classes take any `size` (mnist_test.py:12,
// cifar10.py:25, SVHN.py:13), and this file is what serves the others: the reference's plain Thomas recurrences
// (mnist_test.py:151-198) per line, the adjoint as the transposed recurrences, the state rebuilt backwards or read from
// checkpoints exactly as the fused backward does, the clamp mask and the transposed 3-tap smoothing applied per sweep.
// Correct and deterministic, not tuned: a plane of 64 x 64 keeps 64 threads busy.
// The kernels take a plane of H rows and W columns: an x sweep is H lines of W unknowns, a y sweep W lines of H unknowns
// (the reference's sweeps read B, C, H, W = u.shape and transpose for y: mnist_test.py:72,105, cifar10.py:126,152).  The
// square entry points (PdeAdiDesc / PdeAdiDescF64, one N) call them with H = W = N; the pde_adi_rect_* entry points at the
// end of this file (PdeAdiRectDesc / PdeAdiRectDescF64) with any H, W in [2, PDE_MAX_N_GENERIC].
// The family is generic over the arithmetic type T: float (the PdeAdiDesc entry points of pde_adi.hip) and double (the
// pde_adi_f64_* / pde_adi_rect_f64_* entry points at the end of this file: schedule, clamp bounds and eps in double too).
#include "pde_common.h"
#include "pde_adi_gen.h"

#include <type_traits>

namespace pde {
namespace {

constexpr int kGenArr = 4;                  // per (sweep, channel): coeff | c* | 1/den | clamp pass-through, each [k][line]

template <typename T> struct GenSweep { int axis; T t, scale, pad; };   // device copy of the schedule: scale = delta/h2 in T

__device__ __forceinline__ float gen_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double gen_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float gen_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double gen_min(double a, double b) { return fmin(a, b); }

// SW: PdeSweep (T = float) | PdeSweepF64 (T = double)
template <typename T, typename SW>
struct GenFactorArgs {
    const T *ab, *bb, *as, *bs;
    T* fac;                                  // [S][C][kGenArr][H*W]: x sweeps [k < W][line < H], y sweeps [k < H][line < W]
    GenSweep<T>* tab;                        // [S]
    T* kmax;                                 // nullptr | [S], zeroed before the launch
    int C, H, W, S, smooth3, has_max;
    T cmax, eps;
    SW sweep[PDE_MAX_SWEEPS];
};

template <typename T>
__device__ __forceinline__ T block_max(T v, T* red) {
    for (int o = 32; o > 0; o >>= 1) v = gen_max(v, __shfl_xor(v, o));
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    T m = red[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) m = gen_max(m, red[i]);
    return m;
}

// coefficients are positive: their bit patterns order like the values
__device__ __forceinline__ void gen_atomic_max(float* p, float m) { atomicMax(reinterpret_cast<int*>(p), __float_as_int(m)); }
__device__ __forceinline__ void gen_atomic_max(double* p, double m) {
    atomicMax(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(m));
}

// one workgroup per (sweep, channel), one thread per line
template <typename T, typename SW>
__global__ void gen_factor_kernel(GenFactorArgs<T, SW> a) {
    __shared__ T red[4];
    const int s = blockIdx.x / a.C, c = blockIdx.x % a.C, ln = threadIdx.x;
    const SW sw = a.sweep[s];
    const int ax = sw.axis;
    const int N = (ax == PDE_AXIS_X) ? a.W : a.H, L = (ax == PDE_AXIS_X) ? a.H : a.W;   // unknowns per line, lines
    const size_t HW = (size_t)a.H * a.W;
    if (a.tab && c == 0 && ln == 0) a.tab[s] = GenSweep<T>{ax, sw.t, sw.delta / sw.h2, T(0)};
    T kmx = T(0);
    if (ln < L) {
        const T* base = (ax == PDE_AXIS_X ? a.ab : a.bb) + (size_t)c * HW;
        const T* slope = (ax == PDE_AXIS_X ? a.as : a.bs) + (size_t)c * HW;
        const int lstride = (ax == PDE_AXIS_X) ? a.W : 1, kstride = (ax == PDE_AXIS_X) ? 1 : a.W;
        T* f = a.fac ? a.fac + ((size_t)s * a.C + c) * kGenArr * HW : nullptr;   // nullptr: the maxima alone
        auto raw = [&](int k) { const int i = ln * lstride + k * kstride; return base[i] + slope[i] * sw.t; };
        auto theta = [&](int k) {
            T th = gen_max(raw(k), a.eps);
            if (a.has_max) th = gen_min(th, a.cmax);
            return th;
        };
        const T third = T(1) / T(3);
        T cs_prev = T(0);
        for (int k = 0; k < N; ++k) {
            const T r = raw(k);
            const bool pass = (r >= a.eps) && (!a.has_max || r <= a.cmax);
            T th = theta(k);
            if (a.smooth3) th = (theta(k > 0 ? k - 1 : 0) * third + th * third) + theta(k + 1 < N ? k + 1 : N - 1) * third;
            const T co = th * sw.delta / sw.h2;
            const T b = (k == 0 || k == N - 1) ? T(1) + co : T(1) + T(2) * co;
            const T den = (k ? b + co * cs_prev : b) + a.eps;
            const T cs = (k < N - 1) ? -co / den : T(0);
            if (f) {
                const size_t o = (size_t)k * L + ln;
                f[o] = co;
                f[HW + o] = cs;
                f[2 * HW + o] = T(1) / den;
                f[3 * HW + o] = pass ? T(1) : T(0);
            }
            cs_prev = cs;
            kmx = gen_max(kmx, co);
        }
    }
    if (a.kmax) {
        const T m = block_max(kmx, red);
        if (threadIdx.x == 0) gen_atomic_max(a.kmax + s, m);
    }
}

template <typename IO> struct GenIo;
template <> struct GenIo<double> {
    __device__ static double ld(const void* p, size_t i) { return static_cast<const double*>(p)[i]; }
    __device__ static void st(void* p, size_t i, double v) { static_cast<double*>(p)[i] = v; }
};
template <> struct GenIo<float> {
    __device__ static float ld(const void* p, size_t i) { return static_cast<const float*>(p)[i]; }
    __device__ static void st(void* p, size_t i, float v) { static_cast<float*>(p)[i] = v; }
};
struct gen_bf16 { unsigned short v; };
template <> struct GenIo<gen_bf16> {
    __device__ static float ld(const void* p, size_t i) {
        return __uint_as_float((unsigned)static_cast<const unsigned short*>(p)[i] << 16);
    }
    __device__ static void st(void* p, size_t i, float v) { static_cast<unsigned short*>(p)[i] = f32_to_bf16_hw(v); }
};
struct gen_f16 { unsigned short v; };
template <> struct GenIo<gen_f16> {
    __device__ static float ld(const void* p, size_t i) { return f16_to_f32(static_cast<const unsigned short*>(p)[i]); }
    __device__ static void st(void* p, size_t i, float v) { static_cast<unsigned short*>(p)[i] = f32_to_f16_hw(v); }
};

template <typename T>
struct GenSweepArgs {
    const void *in0, *in1;                   // forward: u, -; backward: gy, y
    void* out;                               // forward: y (nullptr: checkpoint pre-pass); backward: gu
    const T* fac;
    const GenSweep<T>* tab;
    T* ckpt;                                 // [nck][B][C][H*W] in T | nullptr
    T* part;                                 // backward: [G][C][4][H*W]
    unsigned long long ck[2];
    int B, C, H, W, S, G;
    T eps;
    T* xg;                                   // backward with the state plane in global memory: [G*C][H][W+1] | nullptr
};
// The emitting variants (EMIT = true) take their own argument structure, so the plain kernels keep theirs to the byte.
// Bit s of em = the state after sweep s leaves the launch; forward: written to states[slot][B][C][H*W] in the I/O type;
// backward: the same layout holds dL/d(state).
template <typename T>
struct GenEmitArgs : GenSweepArgs<T> {
    void* states;
    unsigned long long em[2];
};
template <typename T, bool EMIT>
using GenArgs = typename std::conditional<EMIT, GenEmitArgs<T>, GenSweepArgs<T>>::type;

__device__ __forceinline__ int gen_ck_bit(const unsigned long long (&ck)[2], int s) { return (int)((ck[s >> 6] >> (s & 63)) & 1ull); }
__device__ __forceinline__ int gen_ck_slot(const unsigned long long (&ck)[2], int s) {
    const unsigned long long below = (s & 63) ? (ck[s >> 6] & ((1ull << (s & 63)) - 1ull)) : 0ull;
    return __popcll(below) + ((s >> 6) ? __popcll(ck[0]) : 0);
}

// The per-line recurrences are serial, so what a thread waits for is latency: the loops below work in batches of kGenBatch
// elements — all LDS reads of the plane and all coefficient reads (global memory, L2-resident) of a batch are issued
// together, then the dependent arithmetic runs on registers, then the batch is written back.  (Written one element at a
// time the compiler must keep every LDS read behind the previous element's LDS write — it cannot know the stride is not
// zero — and a thread pays a full LDS or L2 round trip per element.)
constexpr int kGenBatch = 8;

// forward: one workgroup per plane; sweeps 0..S-1 on the plane in LDS ([row < H][W+1])
// EMIT (the *_forward_states entry points): the plane also goes to a.states after every sweep whose bit is set in a.em
template <typename TT, typename IO, bool EMIT = false>
__global__ void gen_fwd_kernel(GenArgs<TT, EMIT> a) {
    extern __shared__ float gen_fsmem[];
    TT* X = reinterpret_cast<TT*>(gen_fsmem);
    const int W = a.W, ld = W + 1, tid = threadIdx.x, T = blockDim.x, NN = a.H * W;
    const size_t plane = (size_t)NN, pb = (size_t)blockIdx.x * plane;         // blockIdx = b*C + c
    const int c = blockIdx.x % a.C;
    for (int e = tid; e < NN; e += T) X[(e / W) * ld + (e % W)] = GenIo<IO>::ld(a.in0, pb + e);
    __syncthreads();
    for (int s = 0; s < a.S; ++s) {
        const GenSweep<TT> sw = a.tab[s];
        const int N = (sw.axis == PDE_AXIS_X) ? W : a.H, L = (sw.axis == PDE_AXIS_X) ? a.H : W;   // unknowns per line, lines
        if (tid < L) {
            const TT* __restrict__ f = a.fac + ((size_t)s * a.C + c) * kGenArr * plane + tid;   // [arr][k][line = tid]
            TT* v = X + (sw.axis == PDE_AXIS_X ? tid * ld : tid);
            const int st = (sw.axis == PDE_AXIS_X) ? 1 : ld;
            // d*_0 = d_0/den_0, d*_i = (d_i - a_i d*_{i-1})/den_i with a_i = -coeff_i   (mnist_test.py:167-185)
            TT prev = v[0] * f[2 * plane];
            v[0] = prev;
            for (int k0 = 1; k0 < N; k0 += kGenBatch) {
                TT t[kGenBatch], co[kGenBatch], iv[kGenBatch];
#pragma unroll
                for (int j = 0; j < kGenBatch; ++j) {
                    const int k = k0 + j < N ? k0 + j : N - 1;
                    t[j] = v[k * st];
                    co[j] = f[(size_t)k * L];
                    iv[j] = f[2 * plane + (size_t)k * L];
                }
#pragma unroll
                for (int j = 0; j < kGenBatch; ++j)
                    if (k0 + j < N) { prev = (t[j] + co[j] * prev) * iv[j]; t[j] = prev; }
#pragma unroll
                for (int j = 0; j < kGenBatch; ++j)
                    if (k0 + j < N) v[(k0 + j) * st] = t[j];
            }
            // x_{N-1} = d*_{N-1}, x_i = d*_i - c*_i x_{i+1}                                (mnist_test.py:187-196)
            for (int k0 = N - 2; k0 >= 0; k0 -= kGenBatch) {
                TT t[kGenBatch], cs[kGenBatch];
#pragma unroll
                for (int j = 0; j < kGenBatch; ++j) {
                    const int k = k0 - j >= 0 ? k0 - j : 0;
                    t[j] = v[k * st];
                    cs[j] = f[plane + (size_t)k * L];
                }
#pragma unroll
                for (int j = 0; j < kGenBatch; ++j)
                    if (k0 - j >= 0) { prev = t[j] - cs[j] * prev; t[j] = prev; }
#pragma unroll
                for (int j = 0; j < kGenBatch; ++j)
                    if (k0 - j >= 0) v[(k0 - j) * st] = t[j];
            }
        }
        __syncthreads();
        if (a.ckpt && gen_ck_bit(a.ck, s)) {
            TT* dst = a.ckpt + (size_t)gen_ck_slot(a.ck, s) * a.B * a.C * plane + pb;
            for (int e = tid; e < NN; e += T) dst[e] = X[(e / W) * ld + (e % W)];
            __syncthreads();                 // as below: a wave that is done copying must not start the next sweep on lines
                                             // another wave is still reading
        }
        if constexpr (EMIT) {
            if (gen_ck_bit(a.em, s)) {
                const size_t o = (size_t)gen_ck_slot(a.em, s) * a.B * a.C * plane + pb;
                for (int e = tid; e < NN; e += T) GenIo<IO>::st(a.states, o + e, X[(e / W) * ld + (e % W)]);
                __syncthreads();             // the copy reads other threads' lines: all of it before the next sweep writes them
            }
        }
    }
    if (a.out)
        for (int e = tid; e < NN; e += T) GenIo<IO>::st(a.out, pb + e, X[(e / W) * ld + (e % W)]);
}

// backward: workgroup (c, g) walks the planes b = g, g+G, ... of channel c; adjoint in R, state in X (both LDS);
// parameter-gradient partial sums in part[g][c][arr][H*W], every entry owned by one thread of this workgroup.
// ALDS: the four partial-sum images live in LDS beside the two planes and go to `part` once, at the end (chosen while four
// workgroups still fit on a CU, see the launch); otherwise every update is a read-modify-write of global memory by the
// owning thread.
// XG (two planes beyond the LDS limit: T = double at 128 x 128): the state plane X lives in a global scratch slice the workgroup owns,
// the adjoint plane R stays in LDS.
// EMIT (the *_backward_states entry points): a.states holds dL/d(state after sweep s) for every bit s of a.em; the plane is
// added to the adjoint once sweep s+1 has been undone (state and adjoint are the true ones here: no scale).
template <typename TT, typename IO, bool ALDS, bool XG, bool EMIT = false>
__global__ void gen_bwd_kernel(GenArgs<TT, EMIT> a, int smooth3) {
    extern __shared__ float gen_smem[];
    const int H = a.H, W = a.W, ld = W + 1, tid = threadIdx.x, T = blockDim.x, NN = H * W;
    TT* X = XG ? a.xg + (size_t)blockIdx.x * H * ld : reinterpret_cast<TT*>(gen_smem);
    TT* R = XG ? reinterpret_cast<TT*>(gen_smem) : X + (size_t)H * ld;
    TT* ACC = R + (size_t)H * ld;                         // ALDS: [4][H][ld], indexed like the planes
    const size_t plane = (size_t)NN;
    const int c = blockIdx.x % a.C, g = blockIdx.x / a.C;
    TT* part = a.part + ((size_t)g * a.C + c) * 4 * plane;
    if constexpr (ALDS) {
        for (int e = tid; e < 4 * H * ld; e += T) ACC[e] = TT(0);
    } else {
        for (size_t e = tid; e < 4 * plane; e += T) part[e] = TT(0);
    }
    const TT one_eps = TT(1) + a.eps, third = TT(1) / TT(3);
    for (int b = g; b < a.B; b += a.G) {
        const size_t pb = ((size_t)b * a.C + c) * plane;
        __syncthreads();
        for (int e = tid; e < NN; e += T) {
            R[(e / W) * ld + (e % W)] = GenIo<IO>::ld(a.in0, pb + e);
            X[(e / W) * ld + (e % W)] = GenIo<IO>::ld(a.in1, pb + e);
        }
        __syncthreads();
        for (int s = a.S - 1; s >= 0; --s) {
            const GenSweep<TT> sw = a.tab[s];
            const bool xs = sw.axis == PDE_AXIS_X;
            const int N = xs ? W : H, L = xs ? H : W;             // unknowns per line, lines
            if (tid < L) {
                const TT* __restrict__ f = a.fac + ((size_t)s * a.C + c) * kGenArr * plane + tid;   // [arr][k][line = tid]
                TT* r = R + (xs ? tid * ld : tid);
                TT* x = X + (xs ? tid * ld : tid);
                const int st = xs ? 1 : ld;
                // transposed recurrences: U^T w = r (unit lower, sub-diagonal c*), L^T lam = w (diagonal den, super-diagonal a)
                TT prev = r[0];
                for (int k0 = 1; k0 < N; k0 += kGenBatch) {
                    TT t[kGenBatch], cs[kGenBatch];
#pragma unroll
                    for (int j = 0; j < kGenBatch; ++j) {
                        const int k = k0 + j < N ? k0 + j : N - 1;
                        t[j] = r[k * st];
                        cs[j] = f[plane + (size_t)(k - 1) * L];
                    }
#pragma unroll
                    for (int j = 0; j < kGenBatch; ++j)
                        if (k0 + j < N) { prev = t[j] - cs[j] * prev; t[j] = prev; }
#pragma unroll
                    for (int j = 0; j < kGenBatch; ++j)
                        if (k0 + j < N) r[(k0 + j) * st] = t[j];
                }
                prev = prev * f[2 * plane + (size_t)(N - 1) * L];
                r[(N - 1) * st] = prev;
                for (int k0 = N - 2; k0 >= 0; k0 -= kGenBatch) {
                    TT t[kGenBatch], co[kGenBatch], iv[kGenBatch];
#pragma unroll
                    for (int j = 0; j < kGenBatch; ++j) {
                        const int k = k0 - j >= 0 ? k0 - j : 0;
                        t[j] = r[k * st];
                        co[j] = f[(size_t)(k + 1) * L];
                        iv[j] = f[2 * plane + (size_t)k * L];
                    }
#pragma unroll
                    for (int j = 0; j < kGenBatch; ++j)
                        if (k0 - j >= 0) { prev = (t[j] + co[j] * prev) * iv[j]; t[j] = prev; }
#pragma unroll
                    for (int j = 0; j < kGenBatch; ++j)
                        if (k0 - j >= 0) r[(k0 - j) * st] = t[j];
                }
                // coefficient gradient -lam.q with the sweep's OUTPUT state, q = (Neumann second difference, sign flipped);
                // x_old = (1+eps) x + coeff q; then the transposed smoothing (entry j is complete once k = j+1 is known),
                // the clamp mask, and the two parameters: d/d base, d/d slope = t * d/d base
                TT* __restrict__ pbase = part + (xs ? 0 : 2) * plane;
                TT* __restrict__ pslope = pbase + plane;
                // partial sums in global memory are kept [k][line] for BOTH axes (threads of a wave then touch consecutive
                // words; [line][k] made every x-sweep update a cache line of its own): the alpha images are stored
                // transposed ([k < W][line < H]) and gen_reduce_kernel turns them back
                const int pl = tid, pk = L;
                TT* lbase = ACC + (xs ? 0 : 2) * H * ld + (xs ? tid * ld : tid);
                auto add = [&](int j, TT gv) __attribute__((always_inline)) {
                    if constexpr (ALDS) {
                        lbase[j * st] += gv;
                        lbase[H * ld + j * st] += sw.t * gv;
                    } else {
                        pbase[pl + j * pk] += gv;
                        pslope[pl + j * pk] += sw.t * gv;
                    }
                };
                TT xm = TT(0), xc = x[0], g2 = TT(0), g1 = TT(0);         // x_{k-1}, x_k; gsm_{k-2}, gsm_{k-1}
                for (int k0 = 0; k0 < N; k0 += kGenBatch) {
                    TT xn[kGenBatch], lam[kGenBatch], co[kGenBatch], ps[kGenBatch], gout[kGenBatch];
#pragma unroll
                    for (int j = 0; j < kGenBatch; ++j) {
                        const int k = k0 + j < N ? k0 + j : N - 1;
                        xn[j] = (k0 + j + 1 < N) ? x[(k0 + j + 1) * st] : TT(0);    // x_{k+1}
                        lam[j] = r[k * st];
                        co[j] = f[(size_t)k * L];
                        ps[j] = f[3 * plane + (size_t)k * L];
                    }
                    const TT ps_before = k0 > 0 ? f[3 * plane + (size_t)(k0 - 1) * L] : TT(0);   // mask of entry k0-1 (smoothing)
#pragma unroll
                    for (int j = 0; j < kGenBatch; ++j) {
                        const int k = k0 + j;
                        gout[j] = TT(0);
                        if (k < N) {
                            const TT xp = xn[j];
                            const TT q = ((k == 0 || k == N - 1) ? xc : TT(2) * xc) - xm - xp;
                            const TT g0 = -lam[j] * q * sw.scale;
                            xn[j] = one_eps * xc + co[j] * q;                       // becomes x_old[k]
                            xm = xc;
                            xc = xp;
                            if (!smooth3) {
                                gout[j] = g0 * ps[j];                               // entry k
                            } else if (k >= 1) {                                    // finishes entry k-1
                                TT gv = (g2 * third + g1 * third) + g0 * third;
                                if (k == 1) gv += g1 * third;                       // replicate end: theta_0 is used twice by sm_0
                                gout[j] = gv * (j > 0 ? ps[j - 1] : ps_before);
                            }
                            g2 = g1;
                            g1 = g0;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < kGenBatch; ++j) {
                        const int k = k0 + j;
                        if (k < N) {
                            x[k * st] = xn[j];
                            if (!smooth3) add(k, gout[j]);
                            else if (k >= 1) add(k - 1, gout[j]);
                        }
                    }
                }
                if (smooth3) {                                             // entry N-1: (gsm_{N-2} + 2 gsm_{N-1}) / 3
                    const TT gv = (g2 * third + g1 * third) + g1 * third;
                    add(N - 1, gv * f[3 * plane + (size_t)(N - 1) * L]);
                }
            }
            __syncthreads();
            if (s > 0 && a.ckpt && gen_ck_bit(a.ck, s - 1)) {             // the parked state instead of the rebuilt one
                const TT* src = a.ckpt + (size_t)gen_ck_slot(a.ck, s - 1) * a.B * a.C * plane + pb;
                for (int e = tid; e < NN; e += T) X[(e / W) * ld + (e % W)] = src[e];
                __syncthreads();
            }
            if constexpr (EMIT) {
                if (s > 0 && gen_ck_bit(a.em, s - 1)) {
                    const size_t o = (size_t)gen_ck_slot(a.em, s - 1) * a.B * a.C * plane + pb;
                    for (int e = tid; e < NN; e += T) R[(e / W) * ld + (e % W)] += GenIo<IO>::ld(a.states, o + e);
                    __syncthreads();
                }
            }
        }
        for (int e = tid; e < NN; e += T) GenIo<IO>::st(a.out, pb + e, R[(e / W) * ld + (e % W)]);
    }
    if constexpr (ALDS) {
        __syncthreads();
        for (int arr = 0; arr < 4; ++arr)
            for (int e = tid; e < NN; e += T)              // alpha images transposed, as above
                part[arr * plane + e] = ACC[arr * H * ld + (arr < 2 ? (e % H) * ld + (e / H) : (e / W) * ld + (e % W))];
    }
}

// backward for the input alone (the *_backward_input entry points): gu = F^T gy.  One workgroup per plane like
// gen_fwd_kernel, the adjoint plane in LDS, sweeps S-1 .. 0 with the transposed recurrences of gen_bwd_kernel — the same
// operations in the same order on every plane, so gu is that kernel's bit for bit — and nothing of what the parameter
// gradients need: no y, no rebuilt state, no sums.  Adjoints are the true ones (no scale), as there.
// EMIT: a.states holds dL/d(state after sweep s) for every bit s of a.em; the plane joins once sweep s+1 has been undone.
template <typename T>
struct GenInputArgs {
    const void* gy;
    void* gu;
    const void* states;                      // EMIT only
    const T* fac;
    const GenSweep<T>* tab;
    unsigned long long em[2];
    int B, C, H, W, S;
};
template <typename TT, typename IO, bool EMIT>
__global__ void gen_bwd_input_kernel(GenInputArgs<TT> a) {
    extern __shared__ float gen_ismem[];
    TT* R = reinterpret_cast<TT*>(gen_ismem);
    const int W = a.W, ld = W + 1, tid = threadIdx.x, T = blockDim.x, NN = a.H * W;
    const size_t plane = (size_t)NN, pb = (size_t)blockIdx.x * plane;         // blockIdx = b*C + c
    const int c = blockIdx.x % a.C;
    for (int e = tid; e < NN; e += T) R[(e / W) * ld + (e % W)] = GenIo<IO>::ld(a.gy, pb + e);
    __syncthreads();
    for (int s = a.S - 1; s >= 0; --s) {
        const GenSweep<TT> sw = a.tab[s];
        const bool xs = sw.axis == PDE_AXIS_X;
        const int N = xs ? W : a.H, L = xs ? a.H : W;                         // unknowns per line, lines
        if (tid < L) {
            const TT* __restrict__ f = a.fac + ((size_t)s * a.C + c) * kGenArr * plane + tid;   // [arr][k][line = tid]
            TT* r = R + (xs ? tid * ld : tid);
            const int st = xs ? 1 : ld;
            // transposed recurrences: U^T w = r (unit lower, sub-diagonal c*), L^T lam = w (diagonal den, super-diagonal a)
            TT prev = r[0];
            for (int k0 = 1; k0 < N; k0 += kGenBatch) {
                TT t[kGenBatch], cs[kGenBatch];
#pragma unroll
                for (int j = 0; j < kGenBatch; ++j) {
                    const int k = k0 + j < N ? k0 + j : N - 1;
                    t[j] = r[k * st];
                    cs[j] = f[plane + (size_t)(k - 1) * L];
                }
#pragma unroll
                for (int j = 0; j < kGenBatch; ++j)
                    if (k0 + j < N) { prev = t[j] - cs[j] * prev; t[j] = prev; }
#pragma unroll
                for (int j = 0; j < kGenBatch; ++j)
                    if (k0 + j < N) r[(k0 + j) * st] = t[j];
            }
            prev = prev * f[2 * plane + (size_t)(N - 1) * L];
            r[(N - 1) * st] = prev;
            for (int k0 = N - 2; k0 >= 0; k0 -= kGenBatch) {
                TT t[kGenBatch], co[kGenBatch], iv[kGenBatch];
#pragma unroll
                for (int j = 0; j < kGenBatch; ++j) {
                    const int k = k0 - j >= 0 ? k0 - j : 0;
                    t[j] = r[k * st];
                    co[j] = f[(size_t)(k + 1) * L];
                    iv[j] = f[2 * plane + (size_t)k * L];
                }
#pragma unroll
                for (int j = 0; j < kGenBatch; ++j)
                    if (k0 - j >= 0) { prev = (t[j] + co[j] * prev) * iv[j]; t[j] = prev; }
#pragma unroll
                for (int j = 0; j < kGenBatch; ++j)
                    if (k0 - j >= 0) r[(k0 - j) * st] = t[j];
            }
        }
        __syncthreads();                     // the next sweep (or the copy below) reads lines other threads wrote
        if constexpr (EMIT) {
            if (s > 0 && gen_ck_bit(a.em, s - 1)) {
                const size_t o = (size_t)gen_ck_slot(a.em, s - 1) * a.B * a.C * plane + pb;
                for (int e = tid; e < NN; e += T) R[(e / W) * ld + (e % W)] += GenIo<IO>::ld(a.states, o + e);
                __syncthreads();
            }
        }
    }
    for (int e = tid; e < NN; e += T) GenIo<IO>::st(a.gu, pb + e, R[(e / W) * ld + (e % W)]);
}

// the four parameter gradients: partial sums added over the groups in a fixed order
template <typename T>
__global__ void gen_reduce_kernel(const T* part, int G, int C, int H, int W, T* g_ab, T* g_as, T* g_bb, T* g_bs) {
    const int NN = H * W, e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= C * NN) return;
    const int c = e / NN, p = e % NN, pt = (p % W) * H + p / W;        // the alpha images are stored transposed: [W][H]
    T s[4] = {T(0), T(0), T(0), T(0)};
    for (int g = 0; g < G; ++g)
        for (int arr = 0; arr < 4; ++arr) s[arr] += part[(((size_t)g * C + c) * 4 + arr) * NN + (arr < 2 ? pt : p)];
    g_ab[e] = s[0]; g_as[e] = s[1]; g_bb[e] = s[2]; g_bs[e] = s[3];
}

// ---- the tangent-linear pass (include/pdecnn_tangent.h) ---------------------------------------------------------------
// d(coeff) of every sweep from the four parameter tangents: dco = (delta/h2) * smooth3(pass . (dbase + dslope t)) with the
// clamp mask gen_factor_kernel stored (fac's fourth array) and its 3-tap association.  Grid and thread mapping are that
// kernel's: one workgroup per (sweep, channel), one thread per line.  A null tangent is zero.
template <typename T, typename SW>
struct GenFactorTangentArgs {
    const T *dab, *dbb, *das, *dbs;          // each nullptr | [C][H*W]
    const T* fac;                            // the factorisation of the same call (the pass mask is read)
    T* dco;                                  // [S][C][H*W], laid out [k][line] like fac's arrays
    int C, H, W, S, smooth3;
    SW sweep[PDE_MAX_SWEEPS];
};

template <typename T, typename SW>
__global__ void gen_factor_tangent_kernel(GenFactorTangentArgs<T, SW> a) {
    const int s = blockIdx.x / a.C, c = blockIdx.x % a.C, ln = threadIdx.x;
    const SW sw = a.sweep[s];
    const int ax = sw.axis;
    const int N = (ax == PDE_AXIS_X) ? a.W : a.H, L = (ax == PDE_AXIS_X) ? a.H : a.W;   // unknowns per line, lines
    if (ln >= L) return;
    const size_t HW = (size_t)a.H * a.W;
    const T* db = (ax == PDE_AXIS_X) ? a.dab : a.dbb;
    const T* ds = (ax == PDE_AXIS_X) ? a.das : a.dbs;
    if (db) db += (size_t)c * HW;
    if (ds) ds += (size_t)c * HW;
    const int lstride = (ax == PDE_AXIS_X) ? a.W : 1, kstride = (ax == PDE_AXIS_X) ? 1 : a.W;
    const T* pass = a.fac + (((size_t)s * a.C + c) * kGenArr + 3) * HW + ln;             // [k][line = ln]
    T* out = a.dco + ((size_t)s * a.C + c) * HW + ln;
    auto p = [&](int k) {
        const int i = ln * lstride + k * kstride;
        const T r = (db ? db[i] : T(0)) + (ds ? ds[i] : T(0)) * sw.t;
        return pass[(size_t)k * L] != T(0) ? r : T(0);
    };
    const T third = T(1) / T(3);
    for (int k = 0; k < N; ++k) {
        T v = p(k);
        if (a.smooth3) v = (p(k > 0 ? k - 1 : 0) * third + v * third) + p(k + 1 < N ? k + 1 : N - 1) * third;
        out[(size_t)k * L] = v * sw.delta / sw.h2;
    }
}

template <typename T>
struct GenTangentArgs {
    const void *u, *du;                      // du nullptr: a zero input tangent
    void *y, *dy;                            // y nullptr: not written
    const T* fac;
    const T* dco;                            // read only when has_param
    const GenSweep<T>* tab;
    T* xg;                                   // XG: [G*C][H][W+1], the primal plane of each workgroup
    int B, C, H, W, S, G, has_param;
};

// the two recurrences of one line, operation for operation those of gen_fwd_kernel (v: the line, st: its stride)
template <typename TT>
__device__ __forceinline__ void gen_tan_solve(TT* v, int st, const TT* __restrict__ f, size_t plane, int L, int N) {
    TT prev = v[0] * f[2 * plane];
    v[0] = prev;
    for (int k0 = 1; k0 < N; k0 += kGenBatch) {
        TT t[kGenBatch], co[kGenBatch], iv[kGenBatch];
#pragma unroll
        for (int j = 0; j < kGenBatch; ++j) {
            const int k = k0 + j < N ? k0 + j : N - 1;
            t[j] = v[k * st];
            co[j] = f[(size_t)k * L];
            iv[j] = f[2 * plane + (size_t)k * L];
        }
#pragma unroll
        for (int j = 0; j < kGenBatch; ++j)
            if (k0 + j < N) { prev = (t[j] + co[j] * prev) * iv[j]; t[j] = prev; }
#pragma unroll
        for (int j = 0; j < kGenBatch; ++j)
            if (k0 + j < N) v[(k0 + j) * st] = t[j];
    }
    for (int k0 = N - 2; k0 >= 0; k0 -= kGenBatch) {
        TT t[kGenBatch], cs[kGenBatch];
#pragma unroll
        for (int j = 0; j < kGenBatch; ++j) {
            const int k = k0 - j >= 0 ? k0 - j : 0;
            t[j] = v[k * st];
            cs[j] = f[plane + (size_t)k * L];
        }
#pragma unroll
        for (int j = 0; j < kGenBatch; ++j)
            if (k0 - j >= 0) { prev = t[j] - cs[j] * prev; t[j] = prev; }
#pragma unroll
        for (int j = 0; j < kGenBatch; ++j)
            if (k0 - j >= 0) v[(k0 - j) * st] = t[j];
    }
}

// tangent-linear pass: workgroup (g, c) walks the planes b = g, g+G, ... of channel c (G = B unless XG: one plane per
// workgroup, blockIdx = b*C + c as in gen_fwd_kernel); the primal plane X and the tangent plane D side by side in LDS, both
// [row < H][W+1].  Per sweep a thread owns line tid of BOTH planes: it solves the primal line, adds dco_k (x_{k-1} - m_k x_k
// + x_{k+1}) of the SOLVED line to the tangent line (m = 1 at the two ends, 2 inside, a missing neighbour dropped; skipped
// when no parameter carries a tangent), then solves the tangent line with the same rows.  Nothing crosses threads inside a
// sweep, so the barriers are gen_fwd_kernel's: one after every sweep.
// XG (two planes beyond the LDS limit, as gen_bwd_kernel): X lives in a global scratch slice the workgroup owns.
template <typename TT, typename IO, bool XG>
__global__ void gen_tangent_kernel(GenTangentArgs<TT> a) {
    extern __shared__ float gen_tsmem[];
    const int H = a.H, W = a.W, ld = W + 1, tid = threadIdx.x, T = blockDim.x, NN = H * W;
    TT* D = reinterpret_cast<TT*>(gen_tsmem);
    TT* X = XG ? a.xg + (size_t)blockIdx.x * H * ld : D + (size_t)H * ld;
    const size_t plane = (size_t)NN;
    const int c = blockIdx.x % a.C, g = blockIdx.x / a.C;
    for (int b = g; b < a.B; b += a.G) {
        const size_t pb = ((size_t)b * a.C + c) * plane;
        if (b != g) __syncthreads();         // the stores of the previous plane read other threads' lines
        for (int e = tid; e < NN; e += T) {
            X[(e / W) * ld + (e % W)] = GenIo<IO>::ld(a.u, pb + e);
            D[(e / W) * ld + (e % W)] = a.du ? TT(GenIo<IO>::ld(a.du, pb + e)) : TT(0);
        }
        __syncthreads();
        for (int s = 0; s < a.S; ++s) {
            const GenSweep<TT> sw = a.tab[s];
            const bool xs = sw.axis == PDE_AXIS_X;
            const int N = xs ? W : H, L = xs ? H : W;                            // unknowns per line, lines
            if (tid < L) {
                const TT* __restrict__ f = a.fac + ((size_t)s * a.C + c) * kGenArr * plane + tid;   // [arr][k][line = tid]
                TT* x = X + (xs ? tid * ld : tid);
                TT* dl = D + (xs ? tid * ld : tid);
                const int st = xs ? 1 : ld;
                gen_tan_solve<TT>(x, st, f, plane, L, N);
                if (a.has_param) {
                    const TT* __restrict__ dc = a.dco + ((size_t)s * a.C + c) * plane + tid;        // [k][line = tid]
                    TT xm = TT(0), xc = x[0];                                    // x_{k-1}, x_k
                    for (int k0 = 0; k0 < N; k0 += kGenBatch) {
                        TT xn[kGenBatch], co[kGenBatch], dv[kGenBatch];
#pragma unroll
                        for (int j = 0; j < kGenBatch; ++j) {
                            const int k = k0 + j < N ? k0 + j : N - 1;
                            xn[j] = (k0 + j + 1 < N) ? x[(k0 + j + 1) * st] : TT(0);                // x_{k+1}
                            co[j] = dc[(size_t)k * L];
                            dv[j] = dl[k * st];
                        }
#pragma unroll
                        for (int j = 0; j < kGenBatch; ++j) {
                            const int k = k0 + j;
                            if (k < N) {
                                const TT xp = xn[j];
                                const TT lap = (xm + xp) - ((k == 0 || k == N - 1) ? xc : TT(2) * xc);
                                dv[j] += co[j] * lap;
                                xm = xc;
                                xc = xp;
                            }
                        }
#pragma unroll
                        for (int j = 0; j < kGenBatch; ++j)
                            if (k0 + j < N) dl[(k0 + j) * st] = dv[j];
                    }
                }
                gen_tan_solve<TT>(dl, st, f, plane, L, N);
            }
            __syncthreads();                 // the next sweep (or the stores below) reads lines other threads wrote
        }
        for (int e = tid; e < NN; e += T) {
            if (a.y) GenIo<IO>::st(a.y, pb + e, X[(e / W) * ld + (e % W)]);
            GenIo<IO>::st(a.dy, pb + e, D[(e / W) * ld + (e % W)]);
        }
    }
}

size_t up256(size_t x) { return (x + 255) / 256 * 256; }
// rows and columns of a descriptor's plane: the square descriptors have one N, the rectangle ones H and W
template <typename D> int rows_of(const D* d) { return d->N; }
template <typename D> int cols_of(const D* d) { return d->N; }
int rows_of(const PdeAdiRectDesc* d) { return d->H; }
int cols_of(const PdeAdiRectDesc* d) { return d->W; }
int rows_of(const PdeAdiRectDescF64* d) { return d->H; }
int cols_of(const PdeAdiRectDescF64* d) { return d->W; }
template <typename D> size_t plane_of(const D* d) { return (size_t)rows_of(d) * cols_of(d); }
template <typename T, typename D>
size_t fac_bytes(const D* d) { return up256((size_t)d->num_sweeps * d->C * kGenArr * plane_of(d) * sizeof(T)); }
template <typename T>
size_t tab_bytes_gen() { return up256(sizeof(GenSweep<T>) * PDE_MAX_SWEEPS); }
template <typename D>
int gen_groups(const D* d) {
    int G = (1024 + d->C - 1) / d->C;
    return G > d->B ? d->B : (G < 1 ? 1 : G);
}
// one thread per line of the longer axis' count: max(H, W) lines, whole waves
template <typename D> int gen_threads(const D* d) {
    const int n = rows_of(d) > cols_of(d) ? rows_of(d) : cols_of(d);
    return (n + 63) / 64 * 64;
}

constexpr int kGenLdsMax = 160 * 1024;        // the CU's LDS (two fp32 128 x 129 planes are 132 KB)
// one plane image [H][W+1] in T; the backward keeps two of them in LDS while their bytes fit (fp32: every plane; fp64 squares:
// N <= 100), else the state plane goes to a global scratch slice per workgroup (bwd_xg)
template <typename T, typename D>
size_t gen_img(const D* d) { return (size_t)rows_of(d) * (cols_of(d) + 1) * sizeof(T); }
template <typename T, typename D>
bool bwd_xg(const D* d) { return 2 * gen_img<T>(d) > (size_t)kGenLdsMax; }
// workgroups of the backward: with the state in global memory (one workgroup per CU by its LDS) about one per CU
template <typename T, typename D>
int bwd_groups(const D* d) {
    if (!bwd_xg<T>(d)) return gen_groups(d);
    int G = (256 + d->C - 1) / d->C;
    return G > d->B ? d->B : (G < 1 ? 1 : G);
}

template <typename T, typename D>
int launch_gen_factor(const D* d, const T* ab, const T* bb, const T* as, const T* bs, T* fac, GenSweep<T>* tab, T* kmax,
                      hipStream_t st) {
    using SW = typename std::remove_cv<typename std::remove_reference<decltype(d->sweep[0])>::type>::type;
    GenFactorArgs<T, SW> fa;
    fa.ab = ab; fa.bb = bb; fa.as = as; fa.bs = bs; fa.fac = fac; fa.tab = tab; fa.kmax = kmax;
    fa.C = d->C; fa.H = rows_of(d); fa.W = cols_of(d); fa.S = d->num_sweeps; fa.smooth3 = d->smooth3; fa.has_max = d->has_clamp_max;
    fa.cmax = d->clamp_max; fa.eps = d->eps;
    for (int s = 0; s < d->num_sweeps; ++s) fa.sweep[s] = d->sweep[s];
    if (kmax && hipMemsetAsync(kmax, 0, sizeof(T) * d->num_sweeps, st) != hipSuccess) return PDE_E_LAUNCH;
    hipLaunchKernelGGL((gen_factor_kernel<T, SW>), dim3(d->num_sweeps * d->C), dim3(gen_threads(d)), 0, st, fa);
    return check_launch();
}

template <typename K>
int gen_lds(K kernel, unsigned long long& done) { return ensure_dynamic_lds((const void*)kernel, kGenLdsMax, done); }

template <typename T, typename D>
int launch_gen_fwd(const D* d, const void* u, void* y, const T* fac, const GenSweep<T>* tab, int S, T* ckpt,
                   const uint64_t ck[2], hipStream_t st, void* states = nullptr, const uint64_t* emit = nullptr) {
    GenSweepArgs<T> sa{};
    sa.in0 = u; sa.out = y; sa.fac = fac; sa.tab = tab; sa.ckpt = ckpt;
    sa.ck[0] = ck ? ck[0] : 0ull; sa.ck[1] = ck ? ck[1] : 0ull;
    sa.B = d->B; sa.C = d->C; sa.H = rows_of(d); sa.W = cols_of(d); sa.S = S; sa.eps = d->eps;
    const size_t lds = gen_img<T>(d);
    static unsigned long long done_f = 0, done_b = 0, done_h = 0;
    int rc;
    if (emit) {
        GenEmitArgs<T> ea{};
        static_cast<GenSweepArgs<T>&>(ea) = sa;
        ea.states = states; ea.em[0] = emit[0]; ea.em[1] = emit[1];
        static unsigned long long done_e[3] = {0, 0, 0};
#define PDE_GEN_FWD_EMIT(TY, IO, SLOT)                                                                                  \
    do {                                                                                                                \
        if ((rc = gen_lds(gen_fwd_kernel<TY, IO, true>, done_e[SLOT])) != PDE_OK) return rc;                            \
        hipLaunchKernelGGL((gen_fwd_kernel<TY, IO, true>), dim3(d->B * d->C), dim3(gen_threads(d)), lds, st, ea);      \
    } while (0)
        if constexpr (std::is_same<T, double>::value) PDE_GEN_FWD_EMIT(double, double, 0);
        else if (d->io_dtype == PDE_IO_F32) PDE_GEN_FWD_EMIT(float, float, 0);
        else if (d->io_dtype == PDE_IO_F16) PDE_GEN_FWD_EMIT(float, gen_f16, 1);
        else PDE_GEN_FWD_EMIT(float, gen_bf16, 2);
#undef PDE_GEN_FWD_EMIT
        return check_launch();
    }
    if constexpr (std::is_same<T, double>::value) {
        if ((rc = gen_lds(gen_fwd_kernel<double, double>, done_f)) != PDE_OK) return rc;
        hipLaunchKernelGGL((gen_fwd_kernel<double, double>), dim3(d->B * d->C), dim3(gen_threads(d)), lds, st, sa);
    } else if (d->io_dtype == PDE_IO_F32) {
        if ((rc = gen_lds(gen_fwd_kernel<float, float>, done_f)) != PDE_OK) return rc;
        hipLaunchKernelGGL((gen_fwd_kernel<float, float>), dim3(d->B * d->C), dim3(gen_threads(d)), lds, st, sa);
    } else if (d->io_dtype == PDE_IO_F16) {
        if ((rc = gen_lds(gen_fwd_kernel<float, gen_f16>, done_h)) != PDE_OK) return rc;
        hipLaunchKernelGGL((gen_fwd_kernel<float, gen_f16>), dim3(d->B * d->C), dim3(gen_threads(d)), lds, st, sa);
    } else {
        if ((rc = gen_lds(gen_fwd_kernel<float, gen_bf16>, done_b)) != PDE_OK) return rc;
        hipLaunchKernelGGL((gen_fwd_kernel<float, gen_bf16>), dim3(d->B * d->C), dim3(gen_threads(d)), lds, st, sa);
    }
    return check_launch();
}

template <typename T, typename D>
size_t fwd_ws_bytes(const D* d) { return fac_bytes<T>(d) + tab_bytes_gen<T>(); }

template <typename T, typename D>
size_t bwd_ws_bytes(const D* d, int nck) {
    const int G = bwd_groups<T>(d);
    return fac_bytes<T>(d) + tab_bytes_gen<T>() + up256((size_t)G * d->C * 4 * plane_of(d) * sizeof(T)) +
           up256((size_t)nck * d->B * d->C * plane_of(d) * sizeof(T)) +
           (bwd_xg<T>(d) ? up256((size_t)G * d->C * gen_img<T>(d)) : 0);
}

template <typename T, typename D>
int factor_impl(const D* d, const T* ab, const T* bb, const T* as, const T* bs, T* kmax, void* workspace, hipStream_t st) {
    char* ws = static_cast<char*>(workspace);
    return launch_gen_factor<T>(d, ab, bb, as, bs, reinterpret_cast<T*>(ws), reinterpret_cast<GenSweep<T>*>(ws + fac_bytes<T>(d)),
                                kmax, st);
}

template <typename T, typename D>
int forward_sweeps_impl(const D* d, const void* u, void* y, const void* workspace, hipStream_t st, void* states = nullptr,
                        const uint64_t* emit = nullptr) {
    const char* ws = static_cast<const char*>(workspace);
    return launch_gen_fwd<T>(d, u, y, reinterpret_cast<const T*>(ws), reinterpret_cast<const GenSweep<T>*>(ws + fac_bytes<T>(d)),
                             d->num_sweeps, (T*)nullptr, nullptr, st, states, emit);
}

template <typename T, typename D>
int backward_impl(const D* d, const void* gy, const void* y, const void* u, const uint64_t ckpt_mask[2], int nck, int Sf,
                  void* gu, const T* ab, const T* bb, const T* as, const T* bs, T* g_ab, T* g_bb, T* g_as, T* g_bs,
                  const void* fwd_workspace, void* workspace, hipStream_t st, const void* gstates = nullptr,
                  const uint64_t* emit = nullptr) {
    char* ws = static_cast<char*>(workspace);
    const T* fac = reinterpret_cast<const T*>(ws);
    const GenSweep<T>* tab = reinterpret_cast<const GenSweep<T>*>(ws + fac_bytes<T>(d));
    ws += fac_bytes<T>(d) + tab_bytes_gen<T>();
    const int G = bwd_groups<T>(d);
    T* part = reinterpret_cast<T*>(ws);
    ws += up256((size_t)G * d->C * 4 * plane_of(d) * sizeof(T));
    T* ckpt = nck ? reinterpret_cast<T*>(ws) : nullptr;
    ws += up256((size_t)nck * d->B * d->C * plane_of(d) * sizeof(T));
    const bool xg = bwd_xg<T>(d);
    T* xplanes = xg ? reinterpret_cast<T*>(ws) : nullptr;
    int rc;
    if (fwd_workspace) {
        const char* fw = static_cast<const char*>(fwd_workspace);
        fac = reinterpret_cast<const T*>(fw);
        tab = reinterpret_cast<const GenSweep<T>*>(fw + fac_bytes<T>(d));
    } else {
        rc = launch_gen_factor<T>(d, ab, bb, as, bs, const_cast<T*>(fac), const_cast<GenSweep<T>*>(tab), (T*)nullptr, st);
        if (rc != PDE_OK) return rc;
    }
    if (nck) {
        rc = launch_gen_fwd<T>(d, u, nullptr, fac, tab, Sf, ckpt, ckpt_mask, st);
        if (rc != PDE_OK) return rc;
    }
    GenSweepArgs<T> sa{};
    sa.in0 = gy; sa.in1 = y; sa.out = gu; sa.fac = fac; sa.tab = tab; sa.ckpt = ckpt; sa.part = part; sa.xg = xplanes;
    sa.ck[0] = nck ? ckpt_mask[0] : 0ull; sa.ck[1] = nck ? ckpt_mask[1] : 0ull;
    sa.B = d->B; sa.C = d->C; sa.H = rows_of(d); sa.W = cols_of(d); sa.S = d->num_sweeps; sa.G = G; sa.eps = d->eps;
    GenEmitArgs<T> ea{};
    static_cast<GenSweepArgs<T>&>(ea) = sa;
    if (emit) { ea.states = const_cast<void*>(gstates); ea.em[0] = emit[0]; ea.em[1] = emit[1]; }
    const size_t img = gen_img<T>(d);
    // the partial sums beside the planes while four workgroups still fit on a CU (squares: fp32 N <= 40, fp64 N <= 28)
    const bool alds = !xg && 4 * 6 * img <= (size_t)kGenLdsMax;
    const size_t lds = xg ? img : (alds ? 6 : 2) * img;
    static unsigned long long done[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, done_e[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const dim3 grid(G * d->C), block(gen_threads(d));
#define PDE_GEN_BWD(TY, IO, AL, XG, SLOT)                                                                          \
    do {                                                                                                           \
        if (emit) {                                                                                                \
            if ((rc = gen_lds(gen_bwd_kernel<TY, IO, AL, XG, true>, done_e[SLOT])) != PDE_OK) return rc;           \
            hipLaunchKernelGGL((gen_bwd_kernel<TY, IO, AL, XG, true>), grid, block, lds, st, ea, (int)d->smooth3); \
        } else {                                                                                                   \
            if ((rc = gen_lds(gen_bwd_kernel<TY, IO, AL, XG>, done[SLOT])) != PDE_OK) return rc;                   \
            hipLaunchKernelGGL((gen_bwd_kernel<TY, IO, AL, XG>), grid, block, lds, st, sa, (int)d->smooth3);       \
        }                                                                                                          \
    } while (0)
    if constexpr (std::is_same<T, double>::value) {
        if (xg) PDE_GEN_BWD(double, double, false, true, 4);
        else if (alds) PDE_GEN_BWD(double, double, true, false, 5);
        else PDE_GEN_BWD(double, double, false, false, 6);
    } else if (d->io_dtype == PDE_IO_F32) {
        if (alds) PDE_GEN_BWD(float, float, true, false, 0); else PDE_GEN_BWD(float, float, false, false, 1);
    } else if (d->io_dtype == PDE_IO_F16) {
        if (alds) PDE_GEN_BWD(float, gen_f16, true, false, 7); else PDE_GEN_BWD(float, gen_f16, false, false, 8);
    } else {
        if (alds) PDE_GEN_BWD(float, gen_bf16, true, false, 2); else PDE_GEN_BWD(float, gen_bf16, false, false, 3);
    }
#undef PDE_GEN_BWD
    if ((rc = check_launch()) != PDE_OK) return rc;
    const int total = d->C * (int)plane_of(d);
    hipLaunchKernelGGL((gen_reduce_kernel<T>), dim3((total + 255) / 256), dim3(256), 0, st, part, G, d->C, rows_of(d),
                       cols_of(d), g_ab, g_as, g_bb, g_bs);
    return check_launch();
}

// the input backward: the factorisation of the forward call, or one made here, then one launch
template <typename T, typename D>
int backward_input_impl(const D* d, const void* gy, void* gu, const T* ab, const T* bb, const T* as, const T* bs,
                        const void* fwd_workspace, void* workspace, hipStream_t st, const void* gstates,
                        const uint64_t* emit) {
    const char* ws = static_cast<const char*>(fwd_workspace ? fwd_workspace : workspace);
    const T* fac = reinterpret_cast<const T*>(ws);
    const GenSweep<T>* tab = reinterpret_cast<const GenSweep<T>*>(ws + fac_bytes<T>(d));
    int rc;
    if (!fwd_workspace) {
        rc = launch_gen_factor<T>(d, ab, bb, as, bs, const_cast<T*>(fac), const_cast<GenSweep<T>*>(tab), (T*)nullptr, st);
        if (rc != PDE_OK) return rc;
    }
    GenInputArgs<T> ia{};
    ia.gy = gy; ia.gu = gu; ia.states = emit ? gstates : nullptr; ia.fac = fac; ia.tab = tab;
    ia.em[0] = emit ? emit[0] : 0ull; ia.em[1] = emit ? emit[1] : 0ull;
    ia.B = d->B; ia.C = d->C; ia.H = rows_of(d); ia.W = cols_of(d); ia.S = d->num_sweeps;
    const size_t lds = gen_img<T>(d);
    const dim3 grid(d->B * d->C), block(gen_threads(d));
    static unsigned long long done[4] = {0, 0, 0, 0}, done_e[4] = {0, 0, 0, 0};
#define PDE_GEN_BWD_INPUT(TY, IO, SLOT)                                                                    \
    do {                                                                                                   \
        if (emit) {                                                                                        \
            if ((rc = gen_lds(gen_bwd_input_kernel<TY, IO, true>, done_e[SLOT])) != PDE_OK) return rc;     \
            hipLaunchKernelGGL((gen_bwd_input_kernel<TY, IO, true>), grid, block, lds, st, ia);            \
        } else {                                                                                           \
            if ((rc = gen_lds(gen_bwd_input_kernel<TY, IO, false>, done[SLOT])) != PDE_OK) return rc;      \
            hipLaunchKernelGGL((gen_bwd_input_kernel<TY, IO, false>), grid, block, lds, st, ia);           \
        }                                                                                                  \
    } while (0)
    if constexpr (std::is_same<T, double>::value) PDE_GEN_BWD_INPUT(double, double, 0);
    else if (d->io_dtype == PDE_IO_F32) PDE_GEN_BWD_INPUT(float, float, 1);
    else if (d->io_dtype == PDE_IO_F16) PDE_GEN_BWD_INPUT(float, gen_f16, 2);
    else PDE_GEN_BWD_INPUT(float, gen_bf16, 3);
#undef PDE_GEN_BWD_INPUT
    return check_launch();
}

// the tangent-linear pass: workspace = factorisation | schedule | dco | (XG) one primal plane per workgroup
template <typename T, typename D>
size_t dco_bytes(const D* d) { return up256((size_t)d->num_sweeps * d->C * plane_of(d) * sizeof(T)); }
template <typename T, typename D>
int tan_groups(const D* d) { return bwd_xg<T>(d) ? bwd_groups<T>(d) : d->B; }
template <typename T, typename D>
size_t tan_ws_bytes(const D* d) {
    return fwd_ws_bytes<T>(d) + dco_bytes<T>(d) +
           (bwd_xg<T>(d) ? up256((size_t)tan_groups<T>(d) * d->C * gen_img<T>(d)) : 0);
}

// factorisation, d(coeff) when a parameter carries a tangent, then one launch for all sweeps
template <typename T, typename D>
int tangent_impl(const D* d, const void* u, const void* du, const T* ab, const T* bb, const T* as, const T* bs, const T* dab,
                 const T* dbb, const T* das, const T* dbs, void* y, void* dy, void* workspace, hipStream_t st) {
    using SW = typename std::remove_cv<typename std::remove_reference<decltype(d->sweep[0])>::type>::type;
    char* ws = static_cast<char*>(workspace);
    T* fac = reinterpret_cast<T*>(ws);
    GenSweep<T>* tab = reinterpret_cast<GenSweep<T>*>(ws + fac_bytes<T>(d));
    T* dco = reinterpret_cast<T*>(ws + fwd_ws_bytes<T>(d));
    const bool xg = bwd_xg<T>(d);
    T* xplanes = xg ? reinterpret_cast<T*>(ws + fwd_ws_bytes<T>(d) + dco_bytes<T>(d)) : nullptr;
    const int has_param = (dab || dbb || das || dbs) ? 1 : 0;
    int rc = launch_gen_factor<T>(d, ab, bb, as, bs, fac, tab, (T*)nullptr, st);
    if (rc != PDE_OK) return rc;
    if (has_param) {
        GenFactorTangentArgs<T, SW> fa;
        fa.dab = dab; fa.dbb = dbb; fa.das = das; fa.dbs = dbs; fa.fac = fac; fa.dco = dco;
        fa.C = d->C; fa.H = rows_of(d); fa.W = cols_of(d); fa.S = d->num_sweeps; fa.smooth3 = d->smooth3;
        for (int s = 0; s < d->num_sweeps; ++s) fa.sweep[s] = d->sweep[s];
        hipLaunchKernelGGL((gen_factor_tangent_kernel<T, SW>), dim3(d->num_sweeps * d->C), dim3(gen_threads(d)), 0, st, fa);
        if ((rc = check_launch()) != PDE_OK) return rc;
    }
    const int G = tan_groups<T>(d);
    GenTangentArgs<T> ta{};
    ta.u = u; ta.du = du; ta.y = y; ta.dy = dy; ta.fac = fac; ta.dco = dco; ta.tab = tab; ta.xg = xplanes;
    ta.B = d->B; ta.C = d->C; ta.H = rows_of(d); ta.W = cols_of(d); ta.S = d->num_sweeps; ta.G = G; ta.has_param = has_param;
    const size_t lds = (xg ? 1 : 2) * gen_img<T>(d);
    const dim3 grid(G * d->C), block(gen_threads(d));
    static unsigned long long done[5] = {0, 0, 0, 0, 0};
#define PDE_GEN_TANGENT(TY, IO, XG, SLOT)                                                          \
    do {                                                                                           \
        if ((rc = gen_lds(gen_tangent_kernel<TY, IO, XG>, done[SLOT])) != PDE_OK) return rc;       \
        hipLaunchKernelGGL((gen_tangent_kernel<TY, IO, XG>), grid, block, lds, st, ta);            \
    } while (0)
    if constexpr (std::is_same<T, double>::value) {
        if (xg) PDE_GEN_TANGENT(double, double, true, 0); else PDE_GEN_TANGENT(double, double, false, 1);
    } else if (d->io_dtype == PDE_IO_F32) PDE_GEN_TANGENT(float, float, false, 2);
    else if (d->io_dtype == PDE_IO_F16) PDE_GEN_TANGENT(float, gen_f16, false, 3);
    else PDE_GEN_TANGENT(float, gen_bf16, false, 4);
#undef PDE_GEN_TANGENT
    return check_launch();
}

}  // namespace

bool gen_n_ok(int N) { return N >= 2 && N <= PDE_MAX_N_GENERIC; }

size_t gen_forward_workspace_bytes(const PdeAdiDesc* d) { return fwd_ws_bytes<float>(d); }

size_t gen_backward_workspace_bytes(const PdeAdiDesc* d, int nck) { return bwd_ws_bytes<float>(d, nck); }

int gen_kappa_max(const PdeAdiDesc* d, const float* ab, const float* bb, const float* as, const float* bs, float* kmax,
                  hipStream_t st) {
    return launch_gen_factor<float>(d, ab, bb, as, bs, nullptr, nullptr, kmax, st);
}

int gen_factor(const PdeAdiDesc* d, const float* ab, const float* bb, const float* as, const float* bs, float* kmax,
               void* workspace, hipStream_t st) {
    return factor_impl<float>(d, ab, bb, as, bs, kmax, workspace, st);
}

int gen_forward_sweeps(const PdeAdiDesc* d, const void* u, void* y, const void* workspace, hipStream_t st, void* states,
                       const uint64_t* emit) {
    return forward_sweeps_impl<float>(d, u, y, workspace, st, states, emit);
}

int gen_backward(const PdeAdiDesc* d, const void* gy, const void* y, const void* u, const uint64_t ckpt_mask[2], int nck,
                 int Sf, void* gu, const float* ab, const float* bb, const float* as, const float* bs, float* g_ab,
                 float* g_bb, float* g_as, float* g_bs, const void* fwd_workspace, void* workspace, hipStream_t st,
                 const void* gstates, const uint64_t* emit) {
    return backward_impl<float>(d, gy, y, u, ckpt_mask, nck, Sf, gu, ab, bb, as, bs, g_ab, g_bb, g_as, g_bs, fwd_workspace,
                                workspace, st, gstates, emit);
}

int gen_backward_input(const PdeAdiDesc* d, const void* gy, void* gu, const float* ab, const float* bb, const float* as,
                       const float* bs, const void* fwd_workspace, void* workspace, hipStream_t st, const void* gstates,
                       const uint64_t* emit) {
    return backward_input_impl<float>(d, gy, gu, ab, bb, as, bs, fwd_workspace, workspace, st, gstates, emit);
}

}  // namespace pde

// ---- float64 entry points (include/pdecnn.h): the same kernels instantiated for double ------------------------------
using namespace pde;

namespace {

int check_desc_f64(const PdeAdiDescF64* d) {
    if (!d) return PDE_E_BADARG;
    if (d->B <= 0 || d->C <= 0 || d->num_sweeps <= 0) return PDE_E_BADARG;
    if (!gen_n_ok(d->N)) return PDE_E_UNSUPPORTED_N;
    if (d->num_sweeps > PDE_MAX_SWEEPS) return PDE_E_TOO_MANY_SWEEPS;
    if (d->io_dtype != PDE_IO_F64) return PDE_E_BADARG;
    for (int s = 0; s < d->num_sweeps; ++s)
        if (d->sweep[s].axis != PDE_AXIS_X && d->sweep[s].axis != PDE_AXIS_Y) return PDE_E_BADARG;
    return PDE_OK;
}

// checkpoint mask -> (count, number of forward sweeps to recompute); PDE_E_BADARG when inconsistent
template <typename D>
int ckpt_plan(const D* d, const uint64_t ckpt_mask[2], const void* u, int& nck, int& Sf) {
    nck = ckpt_mask ? __builtin_popcountll(ckpt_mask[0]) + __builtin_popcountll(ckpt_mask[1]) : 0;
    Sf = 0;
    if (nck) {
        if (!u) return PDE_E_BADARG;
        for (int s = 0; s < 128; ++s)
            if ((ckpt_mask[s >> 6] >> (s & 63)) & 1ull) {
                if (s >= d->num_sweeps - 1) return PDE_E_BADARG;   // beyond the schedule, or the last state (y itself)
                Sf = s + 1;
            }
    }
    return PDE_OK;
}

// emission mask -> the mask to launch with (nullptr: empty, the plain call); PDE_E_BADARG for a bit at or above S-1 (the
// last state is y itself) or a missing tensor
int emit_plan(int num_sweeps, const uint64_t emit_mask[2], const void* states, const uint64_t*& emit) {
    emit = nullptr;
    if (!emit_mask || !(emit_mask[0] | emit_mask[1])) return PDE_OK;
    if (!states) return PDE_E_BADARG;
    for (int s = num_sweeps > 0 ? num_sweeps - 1 : 0; s < 128; ++s)
        if ((emit_mask[s >> 6] >> (s & 63)) & 1ull) return PDE_E_BADARG;
    emit = emit_mask;
    return PDE_OK;
}

// rectangle descriptors: both sides on the any-size path's range, io_dtype of the family (T = double: PDE_IO_F64 alone)
template <typename T, typename D>
int check_desc_rect(const D* d) {
    constexpr bool f64 = std::is_same<T, double>::value;
    if (!d) return PDE_E_BADARG;
    if (d->B <= 0 || d->C <= 0 || d->num_sweeps <= 0) return PDE_E_BADARG;
    if (!gen_n_ok(d->H) || !gen_n_ok(d->W)) return PDE_E_UNSUPPORTED_N;
    if (d->num_sweeps > PDE_MAX_SWEEPS) return PDE_E_TOO_MANY_SWEEPS;
    if (f64 ? d->io_dtype != PDE_IO_F64
            : (d->io_dtype != PDE_IO_F32 && d->io_dtype != PDE_IO_BF16 && d->io_dtype != PDE_IO_F16))
        return PDE_E_BADARG;
    for (int s = 0; s < d->num_sweeps; ++s)
        if (d->sweep[s].axis != PDE_AXIS_X && d->sweep[s].axis != PDE_AXIS_Y) return PDE_E_BADARG;
    return PDE_OK;
}

template <typename T, typename D>
size_t rect_fwd_bytes(const D* d) { return check_desc_rect<T>(d) != PDE_OK ? 0 : fwd_ws_bytes<T>(d); }

template <typename T, typename D>
size_t rect_bwd_bytes(const D* d, int nck) {
    if (check_desc_rect<T>(d) != PDE_OK || nck < 0 || nck >= d->num_sweeps) return 0;
    return bwd_ws_bytes<T>(d, nck);
}

template <typename T, typename D>
int rect_kappa_max(const D* d, const T* ab, const T* bb, const T* as, const T* bs, T* kmax, void* stream) {
    const int rc = check_desc_rect<T>(d);
    if (rc != PDE_OK) return rc;
    if (!ab || !bb || !as || !bs || !kmax || misaligned(sizeof(T), ab, bb, as, bs, kmax)) return PDE_E_BADARG;
    return launch_gen_factor<T>(d, ab, bb, as, bs, (T*)nullptr, (GenSweep<T>*)nullptr, kmax, static_cast<hipStream_t>(stream));
}

// factorisation (+ maxima), the maxima's way to the host, the sweeps
template <typename T, typename D>
int rect_forward(const D* d, const void* u, void* y, const T* ab, const T* bb, const T* as, const T* bs, T* kmax,
                 T* kmax_host, void* kappa_event, void* workspace, size_t workspace_bytes, void* stream,
                 void* states = nullptr, const uint64_t* emit_mask = nullptr) {
    int rc = check_desc_rect<T>(d);
    if (rc != PDE_OK) return rc;
    if (!u || !y || !ab || !bb || !as || !bs || !workspace) return PDE_E_BADARG;
    // one element at a time in every kernel of this path (pdecnn.h, "Alignment"): the element's own alignment is all it asks
    if (misaligned(io_elem_bytes(d->io_dtype), u, y, states) || misaligned(sizeof(T), ab, bb, as, bs, kmax, kmax_host))
        return PDE_E_BADARG;
    const uint64_t* emit;
    if ((rc = emit_plan(d->num_sweeps, emit_mask, states, emit)) != PDE_OK) return rc;
    if (kmax_host && !kmax) return PDE_E_BADARG;
    if (workspace_bytes < fwd_ws_bytes<T>(d) || ((uintptr_t)workspace & 15)) return PDE_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = factor_impl<T>(d, ab, bb, as, bs, kmax, workspace, st);
    if (rc != PDE_OK) return rc;
    // the maxima leave for the host right behind the factorisation kernel, before the sweep launch (as pde_adi_forward)
    if (kmax_host && hipMemcpyAsync(kmax_host, kmax, (size_t)d->num_sweeps * sizeof(T), hipMemcpyDeviceToHost, st) != hipSuccess)
        return PDE_E_LAUNCH;
    if (kappa_event && hipEventRecord(static_cast<hipEvent_t>(kappa_event), st) != hipSuccess) return PDE_E_LAUNCH;
    return forward_sweeps_impl<T>(d, u, y, workspace, st, states, emit);
}

template <typename T, typename D>
int rect_backward(const D* d, const void* gy, const void* y, const void* u, const uint64_t ckpt_mask[2], void* gu,
                  const T* ab, const T* bb, const T* as, const T* bs, T* g_ab, T* g_bb, T* g_as, T* g_bs,
                  const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream,
                  const void* gstates = nullptr, const uint64_t* emit_mask = nullptr) {
    int rc = check_desc_rect<T>(d);
    if (rc != PDE_OK) return rc;
    if (!gy || !y || !gu || !ab || !bb || !as || !bs || !g_ab || !g_bb || !g_as || !g_bs || !workspace) return PDE_E_BADARG;
    if (misaligned(io_elem_bytes(d->io_dtype), gy, gstates, y, u, gu) || misaligned(sizeof(T), ab, bb, as, bs, g_ab, g_bb, g_as, g_bs))
        return PDE_E_BADARG;
    if (misaligned(kVecAlign, fwd_workspace)) return PDE_E_WORKSPACE;
    const uint64_t* emit;
    if ((rc = emit_plan(d->num_sweeps, emit_mask, gstates, emit)) != PDE_OK) return rc;
    int nck, Sf;
    rc = ckpt_plan(d, ckpt_mask, u, nck, Sf);
    if (rc != PDE_OK) return rc;
    if (workspace_bytes < bwd_ws_bytes<T>(d, nck) || ((uintptr_t)workspace & 15)) return PDE_E_WORKSPACE;
    return backward_impl<T>(d, gy, y, u, ckpt_mask, nck, Sf, gu, ab, bb, as, bs, g_ab, g_bb, g_as, g_bs, fwd_workspace,
                            workspace, static_cast<hipStream_t>(stream), gstates, emit);
}

// the input backward of the rectangle families and of float64 squares (CHECK: the family's descriptor check)
template <typename T, typename D, typename CHECK>
int any_backward_input(const D* d, CHECK&& check, const void* gy, const void* gstates, const uint64_t* emit_mask, void* gu,
                       const T* ab, const T* bb, const T* as, const T* bs, const void* fwd_workspace, void* workspace,
                       size_t workspace_bytes, void* stream) {
    int rc = check(d);
    if (rc != PDE_OK) return rc;
    if (!gy || !gu || !ab || !bb || !as || !bs || !workspace) return PDE_E_BADARG;
    if (misaligned(io_elem_bytes(d->io_dtype), gy, gstates, gu) || misaligned(sizeof(T), ab, bb, as, bs)) return PDE_E_BADARG;
    if (misaligned(kVecAlign, fwd_workspace)) return PDE_E_WORKSPACE;
    const uint64_t* emit;
    if ((rc = emit_plan(d->num_sweeps, emit_mask, gstates, emit)) != PDE_OK) return rc;
    if (workspace_bytes < fwd_ws_bytes<T>(d) || ((uintptr_t)workspace & 15)) return PDE_E_WORKSPACE;
    return backward_input_impl<T>(d, gy, gu, ab, bb, as, bs, fwd_workspace, workspace, static_cast<hipStream_t>(stream),
                                  gstates, emit);
}

// fp32-family squares on the any-size kernels: every N in 2 .. PDE_MAX_N_GENERIC (checks and codes of pde_adi_forward)
int check_desc_sq(const PdeAdiDesc* d) {
    if (!d) return PDE_E_BADARG;
    if (d->B <= 0 || d->C <= 0 || d->num_sweeps <= 0) return PDE_E_BADARG;
    if (!gen_n_ok(d->N)) return PDE_E_UNSUPPORTED_N;
    if (d->num_sweeps > PDE_MAX_SWEEPS) return PDE_E_TOO_MANY_SWEEPS;
    if (d->io_dtype != PDE_IO_F32 && d->io_dtype != PDE_IO_BF16 && d->io_dtype != PDE_IO_F16) return PDE_E_BADARG;
    for (int s = 0; s < d->num_sweeps; ++s)
        if (d->sweep[s].axis != PDE_AXIS_X && d->sweep[s].axis != PDE_AXIS_Y) return PDE_E_BADARG;
    return PDE_OK;
}

// the tangent-linear pass of all four families (CHECK: the family's descriptor check)
template <typename T, typename D, typename CHECK>
size_t any_tangent_bytes(const D* d, CHECK&& check) { return check(d) != PDE_OK ? 0 : tan_ws_bytes<T>(d); }

template <typename T, typename D, typename CHECK>
int any_tangent(const D* d, CHECK&& check, const void* u, const void* du, const T* ab, const T* bb, const T* as, const T* bs,
                const T* dab, const T* dbb, const T* das, const T* dbs, void* y, void* dy, void* workspace,
                size_t workspace_bytes, void* stream) {
    const int rc = check(d);
    if (rc != PDE_OK) return rc;
    if (!u || !dy || !ab || !bb || !as || !bs || !workspace) return PDE_E_BADARG;
    if (!du && !dab && !dbb && !das && !dbs) return PDE_E_BADARG;
    if (misaligned(io_elem_bytes(d->io_dtype), u, du, y, dy) || misaligned(sizeof(T), ab, bb, as, bs, dab, dbb, das, dbs))
        return PDE_E_BADARG;
    if (workspace_bytes < tan_ws_bytes<T>(d) || ((uintptr_t)workspace & 15)) return PDE_E_WORKSPACE;
    return tangent_impl<T>(d, u, du, ab, bb, as, bs, dab, dbb, das, dbs, y, dy, workspace, static_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" {

// ---- the tangent-linear pass (include/pdecnn_tangent.h): (y, dy) from (u, du) and the four parameter tangents ----------
size_t pde_adi_tangent_workspace_bytes(const PdeAdiDesc* d) { return any_tangent_bytes<float>(d, check_desc_sq); }
int pde_adi_tangent(const PdeAdiDesc* d, const void* u, const void* du, const float* alpha_base, const float* beta_base,
                    const float* alpha_slope, const float* beta_slope, const float* d_alpha_base, const float* d_beta_base,
                    const float* d_alpha_slope, const float* d_beta_slope, void* y, void* dy, void* workspace,
                    size_t workspace_bytes, void* stream) {
    return any_tangent<float>(d, check_desc_sq, u, du, alpha_base, beta_base, alpha_slope, beta_slope, d_alpha_base,
                              d_beta_base, d_alpha_slope, d_beta_slope, y, dy, workspace, workspace_bytes, stream);
}
size_t pde_adi_f64_tangent_workspace_bytes(const PdeAdiDescF64* d) { return any_tangent_bytes<double>(d, check_desc_f64); }
int pde_adi_f64_tangent(const PdeAdiDescF64* d, const double* u, const double* du, const double* alpha_base,
                        const double* beta_base, const double* alpha_slope, const double* beta_slope,
                        const double* d_alpha_base, const double* d_beta_base, const double* d_alpha_slope,
                        const double* d_beta_slope, double* y, double* dy, void* workspace, size_t workspace_bytes,
                        void* stream) {
    return any_tangent<double>(d, check_desc_f64, u, du, alpha_base, beta_base, alpha_slope, beta_slope, d_alpha_base,
                               d_beta_base, d_alpha_slope, d_beta_slope, y, dy, workspace, workspace_bytes, stream);
}
size_t pde_adi_rect_tangent_workspace_bytes(const PdeAdiRectDesc* d) {
    return any_tangent_bytes<float>(d, check_desc_rect<float, PdeAdiRectDesc>);
}
int pde_adi_rect_tangent(const PdeAdiRectDesc* d, const void* u, const void* du, const float* alpha_base,
                         const float* beta_base, const float* alpha_slope, const float* beta_slope,
                         const float* d_alpha_base, const float* d_beta_base, const float* d_alpha_slope,
                         const float* d_beta_slope, void* y, void* dy, void* workspace, size_t workspace_bytes,
                         void* stream) {
    return any_tangent<float>(d, check_desc_rect<float, PdeAdiRectDesc>, u, du, alpha_base, beta_base, alpha_slope,
                              beta_slope, d_alpha_base, d_beta_base, d_alpha_slope, d_beta_slope, y, dy, workspace,
                              workspace_bytes, stream);
}
size_t pde_adi_rect_f64_tangent_workspace_bytes(const PdeAdiRectDescF64* d) {
    return any_tangent_bytes<double>(d, check_desc_rect<double, PdeAdiRectDescF64>);
}
int pde_adi_rect_f64_tangent(const PdeAdiRectDescF64* d, const double* u, const double* du, const double* alpha_base,
                             const double* beta_base, const double* alpha_slope, const double* beta_slope,
                             const double* d_alpha_base, const double* d_beta_base, const double* d_alpha_slope,
                             const double* d_beta_slope, double* y, double* dy, void* workspace, size_t workspace_bytes,
                             void* stream) {
    return any_tangent<double>(d, check_desc_rect<double, PdeAdiRectDescF64>, u, du, alpha_base, beta_base, alpha_slope,
                               beta_slope, d_alpha_base, d_beta_base, d_alpha_slope, d_beta_slope, y, dy, workspace,
                               workspace_bytes, stream);
}

// ---- the backward of a layer whose coefficients take no gradient (gu = F^T gy): float64 squares and rectangles ----
size_t pde_adi_f64_backward_input_workspace_bytes(const PdeAdiDescF64* d) {
    return check_desc_f64(d) != PDE_OK ? 0 : fwd_ws_bytes<double>(d);
}
int pde_adi_f64_backward_input_states(const PdeAdiDescF64* d, const double* gy, const double* gstates,
                                      const uint64_t emit_mask[2], double* gu, const double* alpha_base,
                                      const double* beta_base, const double* alpha_slope, const double* beta_slope,
                                      const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream) {
    return any_backward_input<double>(d, check_desc_f64, gy, gstates, emit_mask, gu, alpha_base, beta_base, alpha_slope,
                                      beta_slope, fwd_workspace, workspace, workspace_bytes, stream);
}
int pde_adi_f64_backward_input(const PdeAdiDescF64* d, const double* gy, double* gu, const double* alpha_base,
                               const double* beta_base, const double* alpha_slope, const double* beta_slope,
                               const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream) {
    return pde_adi_f64_backward_input_states(d, gy, nullptr, nullptr, gu, alpha_base, beta_base, alpha_slope, beta_slope,
                                             fwd_workspace, workspace, workspace_bytes, stream);
}
size_t pde_adi_rect_backward_input_workspace_bytes(const PdeAdiRectDesc* d) { return rect_fwd_bytes<float>(d); }
int pde_adi_rect_backward_input_states(const PdeAdiRectDesc* d, const void* gy, const void* gstates,
                                       const uint64_t emit_mask[2], void* gu, const float* alpha_base,
                                       const float* beta_base, const float* alpha_slope, const float* beta_slope,
                                       const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream) {
    return any_backward_input<float>(d, check_desc_rect<float, PdeAdiRectDesc>, gy, gstates, emit_mask, gu, alpha_base,
                                     beta_base, alpha_slope, beta_slope, fwd_workspace, workspace, workspace_bytes, stream);
}
int pde_adi_rect_backward_input(const PdeAdiRectDesc* d, const void* gy, void* gu, const float* alpha_base,
                                const float* beta_base, const float* alpha_slope, const float* beta_slope,
                                const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream) {
    return pde_adi_rect_backward_input_states(d, gy, nullptr, nullptr, gu, alpha_base, beta_base, alpha_slope, beta_slope,
                                              fwd_workspace, workspace, workspace_bytes, stream);
}
size_t pde_adi_rect_f64_backward_input_workspace_bytes(const PdeAdiRectDescF64* d) { return rect_fwd_bytes<double>(d); }
int pde_adi_rect_f64_backward_input_states(const PdeAdiRectDescF64* d, const double* gy, const double* gstates,
                                           const uint64_t emit_mask[2], double* gu, const double* alpha_base,
                                           const double* beta_base, const double* alpha_slope, const double* beta_slope,
                                           const void* fwd_workspace, void* workspace, size_t workspace_bytes,
                                           void* stream) {
    return any_backward_input<double>(d, check_desc_rect<double, PdeAdiRectDescF64>, gy, gstates, emit_mask, gu, alpha_base,
                                      beta_base, alpha_slope, beta_slope, fwd_workspace, workspace, workspace_bytes, stream);
}
int pde_adi_rect_f64_backward_input(const PdeAdiRectDescF64* d, const double* gy, double* gu, const double* alpha_base,
                                    const double* beta_base, const double* alpha_slope, const double* beta_slope,
                                    const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream) {
    return pde_adi_rect_f64_backward_input_states(d, gy, nullptr, nullptr, gu, alpha_base, beta_base, alpha_slope,
                                                  beta_slope, fwd_workspace, workspace, workspace_bytes, stream);
}

size_t pde_adi_f64_forward_workspace_bytes(const PdeAdiDescF64* d) {
    if (check_desc_f64(d) != PDE_OK) return 0;
    return fwd_ws_bytes<double>(d);
}

size_t pde_adi_f64_backward_workspace_bytes(const PdeAdiDescF64* d, int32_t num_checkpoints) {
    if (check_desc_f64(d) != PDE_OK || num_checkpoints < 0 || num_checkpoints >= d->num_sweeps) return 0;
    return bwd_ws_bytes<double>(d, num_checkpoints);
}

int pde_adi_f64_forward_states(const PdeAdiDescF64* d, const double* u, double* y, double* states, const uint64_t emit_mask[2],
                               const double* alpha_base, const double* beta_base, const double* alpha_slope,
                               const double* beta_slope, double* kappa_max, void* workspace, size_t workspace_bytes,
                               void* stream) {
    int rc = check_desc_f64(d);
    if (rc != PDE_OK) return rc;
    if (!u || !y || !alpha_base || !beta_base || !alpha_slope || !beta_slope || !workspace) return PDE_E_BADARG;
    if (misaligned(8, u, y, states, alpha_base, beta_base, alpha_slope, beta_slope, kappa_max)) return PDE_E_BADARG;
    const uint64_t* emit;
    if ((rc = emit_plan(d->num_sweeps, emit_mask, states, emit)) != PDE_OK) return rc;
    if (workspace_bytes < pde_adi_f64_forward_workspace_bytes(d) || ((uintptr_t)workspace & 15)) return PDE_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = factor_impl<double>(d, alpha_base, beta_base, alpha_slope, beta_slope, kappa_max, workspace, st);
    if (rc != PDE_OK) return rc;
    return forward_sweeps_impl<double>(d, u, y, workspace, st, states, emit);
}

int pde_adi_f64_forward(const PdeAdiDescF64* d, const double* u, double* y, const double* alpha_base, const double* beta_base,
                        const double* alpha_slope, const double* beta_slope, double* kappa_max, void* workspace,
                        size_t workspace_bytes, void* stream) {
    return pde_adi_f64_forward_states(d, u, y, nullptr, nullptr, alpha_base, beta_base, alpha_slope, beta_slope, kappa_max,
                                      workspace, workspace_bytes, stream);
}

int pde_adi_f64_backward_states(const PdeAdiDescF64* d, const double* gy, const double* gstates, const uint64_t emit_mask[2],
                                const double* y, const double* u, const uint64_t ckpt_mask[2], double* gu,
                                const double* alpha_base, const double* beta_base, const double* alpha_slope,
                                const double* beta_slope, double* g_alpha_base, double* g_beta_base, double* g_alpha_slope,
                                double* g_beta_slope, const void* fwd_workspace, void* workspace, size_t workspace_bytes,
                                void* stream) {
    int rc = check_desc_f64(d);
    if (rc != PDE_OK) return rc;
    if (!gy || !y || !gu || !alpha_base || !beta_base || !alpha_slope || !beta_slope || !g_alpha_base || !g_beta_base ||
        !g_alpha_slope || !g_beta_slope || !workspace)
        return PDE_E_BADARG;
    if (misaligned(8, gy, gstates, y, u, gu, alpha_base, beta_base, alpha_slope, beta_slope, g_alpha_base, g_beta_base, g_alpha_slope,
                   g_beta_slope))
        return PDE_E_BADARG;
    if (misaligned(kVecAlign, fwd_workspace)) return PDE_E_WORKSPACE;
    const uint64_t* emit;
    if ((rc = emit_plan(d->num_sweeps, emit_mask, gstates, emit)) != PDE_OK) return rc;
    int nck, Sf;
    rc = ckpt_plan(d, ckpt_mask, u, nck, Sf);
    if (rc != PDE_OK) return rc;
    if (workspace_bytes < pde_adi_f64_backward_workspace_bytes(d, nck) || ((uintptr_t)workspace & 15)) return PDE_E_WORKSPACE;
    return backward_impl<double>(d, gy, y, u, ckpt_mask, nck, Sf, gu, alpha_base, beta_base, alpha_slope, beta_slope,
                                 g_alpha_base, g_beta_base, g_alpha_slope, g_beta_slope, fwd_workspace, workspace,
                                 static_cast<hipStream_t>(stream), gstates, emit);
}

int pde_adi_f64_backward(const PdeAdiDescF64* d, const double* gy, const double* y, const double* u,
                         const uint64_t ckpt_mask[2], double* gu, const double* alpha_base, const double* beta_base,
                         const double* alpha_slope, const double* beta_slope, double* g_alpha_base, double* g_beta_base,
                         double* g_alpha_slope, double* g_beta_slope, const void* fwd_workspace, void* workspace,
                         size_t workspace_bytes, void* stream) {
    return pde_adi_f64_backward_states(d, gy, nullptr, nullptr, y, u, ckpt_mask, gu, alpha_base, beta_base, alpha_slope,
                                       beta_slope, g_alpha_base, g_beta_base, g_alpha_slope, g_beta_slope, fwd_workspace,
                                       workspace, workspace_bytes, stream);
}

// ---- rectangular planes (include/pdecnn.h): the same kernels with H != W, fp32 / bf16 / fp16 tensors and float64 -----
int pde_adi_rect_supported(int32_t H, int32_t W) { return (gen_n_ok(H) && gen_n_ok(W)) ? 1 : 0; }

size_t pde_adi_rect_forward_workspace_bytes(const PdeAdiRectDesc* d) { return rect_fwd_bytes<float>(d); }

size_t pde_adi_rect_backward_workspace_bytes(const PdeAdiRectDesc* d, int32_t num_checkpoints) {
    return rect_bwd_bytes<float>(d, num_checkpoints);
}

int pde_adi_rect_kappa_max(const PdeAdiRectDesc* d, const float* alpha_base, const float* beta_base, const float* alpha_slope,
                           const float* beta_slope, float* kappa_max, void* stream) {
    return rect_kappa_max<float>(d, alpha_base, beta_base, alpha_slope, beta_slope, kappa_max, stream);
}

int pde_adi_rect_forward(const PdeAdiRectDesc* d, const void* u, void* y, const float* alpha_base, const float* beta_base,
                         const float* alpha_slope, const float* beta_slope, float* kappa_max, float* kappa_max_host,
                         void* kappa_event, void* workspace, size_t workspace_bytes, void* stream) {
    return rect_forward<float>(d, u, y, alpha_base, beta_base, alpha_slope, beta_slope, kappa_max, kappa_max_host,
                               kappa_event, workspace, workspace_bytes, stream);
}

int pde_adi_rect_backward(const PdeAdiRectDesc* d, const void* gy, const void* y, const void* u, const uint64_t ckpt_mask[2],
                          void* gu, const float* alpha_base, const float* beta_base, const float* alpha_slope,
                          const float* beta_slope, float* g_alpha_base, float* g_beta_base, float* g_alpha_slope,
                          float* g_beta_slope, const void* fwd_workspace, void* workspace, size_t workspace_bytes,
                          void* stream) {
    return rect_backward<float>(d, gy, y, u, ckpt_mask, gu, alpha_base, beta_base, alpha_slope, beta_slope, g_alpha_base,
                                g_beta_base, g_alpha_slope, g_beta_slope, fwd_workspace, workspace, workspace_bytes, stream);
}

int pde_adi_rect_forward_states(const PdeAdiRectDesc* d, const void* u, void* y, void* states, const uint64_t emit_mask[2],
                                const float* alpha_base, const float* beta_base, const float* alpha_slope,
                                const float* beta_slope, float* kappa_max, float* kappa_max_host, void* kappa_event,
                                void* workspace, size_t workspace_bytes, void* stream) {
    return rect_forward<float>(d, u, y, alpha_base, beta_base, alpha_slope, beta_slope, kappa_max, kappa_max_host,
                               kappa_event, workspace, workspace_bytes, stream, states, emit_mask);
}

int pde_adi_rect_backward_states(const PdeAdiRectDesc* d, const void* gy, const void* gstates, const uint64_t emit_mask[2],
                                 const void* y, const void* u, const uint64_t ckpt_mask[2], void* gu,
                                 const float* alpha_base, const float* beta_base, const float* alpha_slope,
                                 const float* beta_slope, float* g_alpha_base, float* g_beta_base, float* g_alpha_slope,
                                 float* g_beta_slope, const void* fwd_workspace, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    return rect_backward<float>(d, gy, y, u, ckpt_mask, gu, alpha_base, beta_base, alpha_slope, beta_slope, g_alpha_base,
                                g_beta_base, g_alpha_slope, g_beta_slope, fwd_workspace, workspace, workspace_bytes, stream,
                                gstates, emit_mask);
}

size_t pde_adi_rect_f64_forward_workspace_bytes(const PdeAdiRectDescF64* d) { return rect_fwd_bytes<double>(d); }

size_t pde_adi_rect_f64_backward_workspace_bytes(const PdeAdiRectDescF64* d, int32_t num_checkpoints) {
    return rect_bwd_bytes<double>(d, num_checkpoints);
}

int pde_adi_rect_f64_kappa_max(const PdeAdiRectDescF64* d, const double* alpha_base, const double* beta_base,
                               const double* alpha_slope, const double* beta_slope, double* kappa_max, void* stream) {
    return rect_kappa_max<double>(d, alpha_base, beta_base, alpha_slope, beta_slope, kappa_max, stream);
}

int pde_adi_rect_f64_forward(const PdeAdiRectDescF64* d, const double* u, double* y, const double* alpha_base,
                             const double* beta_base, const double* alpha_slope, const double* beta_slope, double* kappa_max,
                             void* workspace, size_t workspace_bytes, void* stream) {
    return rect_forward<double>(d, u, y, alpha_base, beta_base, alpha_slope, beta_slope, kappa_max, (double*)nullptr,
                                nullptr, workspace, workspace_bytes, stream);
}

int pde_adi_rect_f64_backward(const PdeAdiRectDescF64* d, const double* gy, const double* y, const double* u,
                              const uint64_t ckpt_mask[2], double* gu, const double* alpha_base, const double* beta_base,
                              const double* alpha_slope, const double* beta_slope, double* g_alpha_base, double* g_beta_base,
                              double* g_alpha_slope, double* g_beta_slope, const void* fwd_workspace, void* workspace,
                              size_t workspace_bytes, void* stream) {
    return rect_backward<double>(d, gy, y, u, ckpt_mask, gu, alpha_base, beta_base, alpha_slope, beta_slope,
                                 g_alpha_base, g_beta_base, g_alpha_slope, g_beta_slope, fwd_workspace, workspace,
                                 workspace_bytes, stream);
}

int pde_adi_rect_f64_forward_states(const PdeAdiRectDescF64* d, const double* u, double* y, double* states,
                                    const uint64_t emit_mask[2], const double* alpha_base, const double* beta_base,
                                    const double* alpha_slope, const double* beta_slope, double* kappa_max, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    return rect_forward<double>(d, u, y, alpha_base, beta_base, alpha_slope, beta_slope, kappa_max, (double*)nullptr,
                                nullptr, workspace, workspace_bytes, stream, states, emit_mask);
}

int pde_adi_rect_f64_backward_states(const PdeAdiRectDescF64* d, const double* gy, const double* gstates,
                                     const uint64_t emit_mask[2], const double* y, const double* u,
                                     const uint64_t ckpt_mask[2], double* gu, const double* alpha_base,
                                     const double* beta_base, const double* alpha_slope, const double* beta_slope,
                                     double* g_alpha_base, double* g_beta_base, double* g_alpha_slope, double* g_beta_slope,
                                     const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream) {
    return rect_backward<double>(d, gy, y, u, ckpt_mask, gu, alpha_base, beta_base, alpha_slope, beta_slope,
                                 g_alpha_base, g_beta_base, g_alpha_slope, g_beta_slope, fwd_workspace, workspace,
                                 workspace_bytes, stream, gstates, emit_mask);
}

}  // extern "C"
