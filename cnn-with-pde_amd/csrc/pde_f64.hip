// float64 versions of the layer pieces around the implicit sweeps: the channel operator (cifar10.py:65-72, SVHN.py:78-86),
// the SVHN skip blend (SVHN.py:73-74), the explicit 5-point layer (tiny_imagenet.py:34-72) and the Jacobi layer
// (emotion_recognition.py:82-97).  Plain double arithmetic (v_fma_f64 and friends), one simple kernel per pass; every sum
// that feeds a parameter gradient runs in a fixed order, so two calls give the same bits.  The implicit sweeps themselves
// are the any-size family of pde_adi_gen.hip instantiated for double.  The explicit and the Jacobi kernels have an emitting
// variant each (template flag EMIT: pde_explicit5_f64_*_states, pde_jacobi_f64_*_states — the trajectory, as in
// pde_explicit.hip); the plain entry points are those calls with a NULL mask and run the plain instantiations.
#include "pde_common.h"

namespace pde {
namespace {

size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// fixed-order tree sum of one value per thread over a workgroup of 256 threads; the result is valid in thread 0
__device__ double block_sum256(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// ---- channel operator -----------------------------------------------------------------------------------------------
// out[b,i,p] = sum_j M[i,j] u[b,j,p]  (trans = 0),  out[b,j,p] = sum_i M[i,j] u[b,i,p]  (trans = 1)
__global__ __launch_bounds__(256) void mix64_apply_kernel(int C, int HW, const double* __restrict__ u,
                                                          const double* __restrict__ M, double* __restrict__ out, int trans) {
    const int p = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y, b = blockIdx.z;
    if (p >= HW) return;
    const double* ub = u + (size_t)b * C * HW + p;
    double acc = 0.0;
    for (int j = 0; j < C; ++j) acc = fma(trans ? M[(size_t)j * C + i] : M[(size_t)i * C + j], ub[(size_t)j * HW], acc);
    out[((size_t)b * C + i) * HW + p] = acc;
}

constexpr int kMixT = 16, kMixK = 32;
// gM partial sums: part[z][i][j] = sum over the samples of split z and all p of g[b,i,p] u[b,j,p]; 16 x 16 tiles of gM,
// the contraction in chunks of 32 through LDS, every sum in a fixed order
__global__ __launch_bounds__(256) void mix64_gm_kernel(int B, int C, int HW, int nsplit, const double* __restrict__ g,
                                                       const double* __restrict__ u, double* __restrict__ part) {
    __shared__ double As[kMixT][kMixK + 1], Bs[kMixT][kMixK + 1];
    const int ti = threadIdx.x / kMixT, tj = threadIdx.x % kMixT;
    const int i0 = blockIdx.y * kMixT, j0 = blockIdx.x * kMixT, z = blockIdx.z;
    const int bper = (B + nsplit - 1) / nsplit, b0 = z * bper, b1 = min(B, b0 + bper);
    double acc = 0.0;
    for (int b = b0; b < b1; ++b) {
        for (int p0 = 0; p0 < HW; p0 += kMixK) {
            for (int e = threadIdx.x; e < kMixT * kMixK; e += 256) {
                const int r = e / kMixK, k = e % kMixK, p = p0 + k;
                As[r][k] = (i0 + r < C && p < HW) ? g[((size_t)b * C + i0 + r) * HW + p] : 0.0;
                Bs[r][k] = (j0 + r < C && p < HW) ? u[((size_t)b * C + j0 + r) * HW + p] : 0.0;
            }
            __syncthreads();
#pragma unroll 8
            for (int k = 0; k < kMixK; ++k) acc = fma(As[ti][k], Bs[tj][k], acc);
            __syncthreads();
        }
    }
    if (i0 + ti < C && j0 + tj < C) part[((size_t)z * C + i0 + ti) * C + j0 + tj] = acc;
}

// acc = (accumulate ? acc : 0) + sum_z part[z] (in order of z); finalize: gM = acc
__global__ __launch_bounds__(256) void mix64_gm_reduce_kernel(int CC, int nsplit, const double* __restrict__ part, double* acc,
                                                              int accumulate, double* gM) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= CC) return;
    double s = 0.0;
    for (int z = 0; z < nsplit; ++z) s += part[(size_t)z * CC + e];
    const double v = accumulate ? acc[e] + s : s;
    acc[e] = v;
    if (gM) gM[e] = v;
}

int mix64_nsplit(int B, int C) {
    const int tiles = ((C + kMixT - 1) / kMixT) * ((C + kMixT - 1) / kMixT);
    int s = (512 + tiles - 1) / tiles;
    return s > B ? B : (s < 1 ? 1 : s);
}

bool mix64_ok(int B, int C, int HW) { return B > 0 && B <= 65535 && C >= 1 && C <= 128 && HW > 0; }

// ---- skip blend -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ double sigmoid64(double w) { return 1.0 / (1.0 + exp(-w)); }

__global__ __launch_bounds__(256) void blend64_fwd_kernel(long long n, const double* __restrict__ u0, const double* __restrict__ u,
                                                          const double* __restrict__ w, double* __restrict__ out) {
    const double s = sigmoid64(*w);
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256)
        out[e] = s * u0[e] + (1.0 - s) * u[e];
}

constexpr int kBlendParts = 512;
int blend64_parts(long long n) {
    const long long b = (n + 255) / 256;
    return (int)(b < kBlendParts ? (b < 1 ? 1 : b) : kBlendParts);
}

__global__ __launch_bounds__(256) void blend64_bwd_kernel(long long n, const double* __restrict__ g, const double* __restrict__ u0,
                                                          const double* __restrict__ u, const double* __restrict__ w,
                                                          double* __restrict__ g_u0, double* __restrict__ g_u,
                                                          double* __restrict__ part) {
    __shared__ double red[256];
    const double s = sigmoid64(*w), t = 1.0 - s;
    double acc = 0.0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const double ge = g[e];
        g_u0[e] = s * ge;
        g_u[e] = t * ge;
        acc = fma(ge, u0[e] - u[e], acc);
    }
    const double r = block_sum256(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// skip_weight takes no gradient (pde_skip_blend_f64_backward_input): the two products alone
__global__ __launch_bounds__(256) void blend64_bwd_input_kernel(long long n, const double* __restrict__ g,
                                                                const double* __restrict__ w, double* __restrict__ g_u0,
                                                                double* __restrict__ g_u) {
    const double s = sigmoid64(*w), t = 1.0 - s;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const double ge = g[e];
        g_u0[e] = s * ge;
        g_u[e] = t * ge;
    }
}

__global__ __launch_bounds__(256) void blend64_reduce_kernel(int nparts, const double* __restrict__ part,
                                                             const double* __restrict__ w, double* __restrict__ gw) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) acc += part[i];
    const double r = block_sum256(acc, red);
    if (threadIdx.x == 0) {
        const double s = sigmoid64(*w);
        *gw = s * (1.0 - s) * r;
    }
}

// ---- explicit 5-point layer -----------------------------------------------------------------------------------------
// v = s_c u;  out = u + relax*((v + a_c dt Lap0(v)) - u),  a_c = clamp(alpha_base_c, eps, max_coeff)
__device__ __forceinline__ double clamp64(double a, double lo, double hi) { return fmin(fmax(a, lo), hi); }

// EMIT: the step's output goes to `emit` (a slot of the trajectory tensor) too
template <bool EMIT = false>
__global__ __launch_bounds__(256) void expl64_fwd_kernel(int C, int H, int W, const double* __restrict__ x,
                                                         const double* __restrict__ ab, const double* __restrict__ sc,
                                                         double dt, double eps, double maxc, double relax,
                                                         double* __restrict__ out, double* __restrict__ emit) {
    const int HW = H * W, p = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (p >= HW) return;
    const int i = p / W, j = p % W;
    const double* xp = x + ((size_t)b * C + c) * HW;
    const double s = sc[c], k = clamp64(ab[c], eps, maxc) * dt;
    const double v = s * xp[p];
    const double up = i > 0 ? s * xp[p - W] : 0.0, dn = i + 1 < H ? s * xp[p + W] : 0.0;
    const double lf = j > 0 ? s * xp[p - 1] : 0.0, rt = j + 1 < W ? s * xp[p + 1] : 0.0;
    const double lap = (((up + dn) + lf) + rt) - 4.0 * v;
    const double nw = v + k * lap;
    const double o = xp[p] + relax * (nw - xp[p]);
    out[((size_t)b * C + c) * HW + p] = o;
    if constexpr (EMIT) emit[((size_t)b * C + c) * HW + p] = o;
}

// adjoint of one step for plane (b, c): gx = (1-relax) g + s (r + k Lap0(r)), r = relax g; partial sums of the two
// parameter gradients, added to part[b][c][0..1] (the steps in reverse order: a fixed order)
// EMIT: gx, the adjoint of an emitted state, gets += ginj (that state's upstream gradient)
template <bool EMIT = false>
__global__ __launch_bounds__(256) void expl64_bwd_kernel(int C, int H, int W, const double* __restrict__ x,
                                                         const double* __restrict__ g, const double* __restrict__ ab,
                                                         const double* __restrict__ sc, double dt, double eps, double maxc,
                                                         double relax, double* __restrict__ gx, double* __restrict__ part,
                                                         int accumulate, const double* __restrict__ ginj) {
    __shared__ double red[256];
    const int HW = H * W, c = blockIdx.x % C, b = blockIdx.x / C;
    const size_t off = ((size_t)b * C + c) * HW;
    const double* xp = x + off;
    const double* gp = g + off;
    const double s = sc[c], k = clamp64(ab[c], eps, maxc) * dt;
    double acc_s = 0.0, acc_k = 0.0;
    for (int p = threadIdx.x; p < HW; p += 256) {
        const int i = p / W, j = p % W;
        const double r = relax * gp[p];
        const double rup = i > 0 ? relax * gp[p - W] : 0.0, rdn = i + 1 < H ? relax * gp[p + W] : 0.0;
        const double rlf = j > 0 ? relax * gp[p - 1] : 0.0, rrt = j + 1 < W ? relax * gp[p + 1] : 0.0;
        const double gv = r + k * ((((rup + rdn) + rlf) + rrt) - 4.0 * r);
        const double v = s * xp[p];
        const double up = i > 0 ? s * xp[p - W] : 0.0, dn = i + 1 < H ? s * xp[p + W] : 0.0;
        const double lf = j > 0 ? s * xp[p - 1] : 0.0, rt = j + 1 < W ? s * xp[p + 1] : 0.0;
        const double lap = (((up + dn) + lf) + rt) - 4.0 * v;
        double o = (1.0 - relax) * gp[p] + s * gv;
        if constexpr (EMIT) o += ginj[off + p];
        gx[off + p] = o;
        acc_s = fma(gv, xp[p], acc_s);
        acc_k = fma(r, lap, acc_k);
    }
    const double ss = block_sum256(acc_s, red);
    const double sk = block_sum256(acc_k, red);
    if (threadIdx.x == 0) {
        double* q = part + ((size_t)b * C + c) * 2;
        q[0] = accumulate ? q[0] + ss : ss;
        q[1] = accumulate ? q[1] + sk : sk;
    }
}

// the adjoint of one step alone (pde_explicit5_f64_backward_input[_states]: the parameters take no gradient):
// expl64_bwd_kernel without x, the two sums and `part`; gx is formed as it is there
template <bool EMIT = false>
__global__ __launch_bounds__(256) void expl64_bwd_input_kernel(int C, int H, int W, const double* __restrict__ g,
                                                               const double* __restrict__ ab, const double* __restrict__ sc,
                                                               double dt, double eps, double maxc, double relax,
                                                               double* __restrict__ gx, const double* __restrict__ ginj) {
    const int HW = H * W, c = blockIdx.x % C, b = blockIdx.x / C;
    const size_t off = ((size_t)b * C + c) * HW;
    const double* gp = g + off;
    const double s = sc[c], k = clamp64(ab[c], eps, maxc) * dt;
    for (int p = threadIdx.x; p < HW; p += 256) {
        const int i = p / W, j = p % W;
        const double r = relax * gp[p];
        const double rup = i > 0 ? relax * gp[p - W] : 0.0, rdn = i + 1 < H ? relax * gp[p + W] : 0.0;
        const double rlf = j > 0 ? relax * gp[p - 1] : 0.0, rrt = j + 1 < W ? relax * gp[p + 1] : 0.0;
        const double gv = r + k * ((((rup + rdn) + rlf) + rrt) - 4.0 * r);
        double o = (1.0 - relax) * gp[p] + s * gv;
        if constexpr (EMIT) o += ginj[off + p];
        gx[off + p] = o;
    }
}

// the tangent-linear pass of one step (pde_explicit5_f64_tangent): expl64_fwd_kernel with a second state.  dx' is the same
// expressions on dx, then + relax*(ds*(x + k*Lap0 x) + dk*(s*Lap0 x)) with x the step's input,
// dk = [eps <= alpha_c <= max_coeff] * dalpha_c * dt; src == 0 (both parameter tangents NULL): the source is not added.
// dx NULL (first step only): a zero tangent; out NULL (last step only): y is not wanted.
__global__ __launch_bounds__(256) void expl64_tangent_kernel(int C, int H, int W, const double* __restrict__ x,
                                                             const double* __restrict__ dx, const double* __restrict__ ab,
                                                             const double* __restrict__ sc, const double* __restrict__ dab,
                                                             const double* __restrict__ dsc, double dt, double eps,
                                                             double maxc, double relax, double* __restrict__ out,
                                                             double* __restrict__ dout, int src) {
#pragma clang fp contract(off)
    // contraction off, the forward's fused operations spelled out (expl64_fwd_kernel compiles to lap = fma(-4, v, sum),
    // nw = fma(k, lap, v), o = fma(relax, nw - x, x)): y keeps the forward's bits whatever else this kernel computes
    const int HW = H * W, p = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (p >= HW) return;
    const int i = p / W, j = p % W;
    const size_t po = ((size_t)b * C + c) * HW;
    const double* xp = x + po;
    const double s = sc[c], k = clamp64(ab[c], eps, maxc) * dt;
    const double v = s * xp[p];
    const double up = i > 0 ? s * xp[p - W] : 0.0, dn = i + 1 < H ? s * xp[p + W] : 0.0;
    const double lf = j > 0 ? s * xp[p - 1] : 0.0, rt = j + 1 < W ? s * xp[p + 1] : 0.0;
    const double lap = fma(-4.0, v, ((up + dn) + lf) + rt);
    const double nw = fma(k, lap, v);
    const double o = fma(relax, nw - xp[p], xp[p]);
    double od = 0.0;
    if (dx) {
        const double* dp = dx + po;
        const double dv = s * dp[p];
        const double dup = i > 0 ? s * dp[p - W] : 0.0, ddn = i + 1 < H ? s * dp[p + W] : 0.0;
        const double dlf = j > 0 ? s * dp[p - 1] : 0.0, drt = j + 1 < W ? s * dp[p + 1] : 0.0;
        const double dlap = fma(-4.0, dv, ((dup + ddn) + dlf) + drt);
        const double dnw = fma(k, dlap, dv);
        od = fma(relax, dnw - dp[p], dp[p]);
    }
    if (src) {
        const double xu = i > 0 ? xp[p - W] : 0.0, xd = i + 1 < H ? xp[p + W] : 0.0;
        const double xl = j > 0 ? xp[p - 1] : 0.0, xr = j + 1 < W ? xp[p + 1] : 0.0;
        const double lx = fma(-4.0, xp[p], ((xu + xd) + xl) + xr);         // Lap0 x, unscaled
        const double ds = dsc ? dsc[c] : 0.0;
        const double dk = (dab && ab[c] >= eps && ab[c] <= maxc) ? dab[c] * dt : 0.0;
        od = fma(relax, fma(ds, fma(k, lx, xp[p]), dk * lap), od);
    }
    if (out) out[po + p] = o;
    dout[po + p] = od;
}

__global__ void expl64_reduce_kernel(int B, int C, const double* __restrict__ part, const double* __restrict__ ab,
                                     double dt, double eps, double maxc, double* __restrict__ ga, double* __restrict__ gs) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s0 = 0.0, s1 = 0.0;
    for (int b = 0; b < B; ++b) {
        s0 += part[((size_t)b * C + c) * 2];
        s1 += part[((size_t)b * C + c) * 2 + 1];
    }
    gs[c] = s0;
    ga[c] = (ab[c] >= eps && ab[c] <= maxc) ? s1 * dt : 0.0;     // clamp passes the gradient inside [eps, max_coeff]
}

// ---- Jacobi layer ---------------------------------------------------------------------------------------------------
// one workgroup per sample, the padded plane (H+2) x (W+2) in LDS.  P_0 = reflect-pad(u); P_{k+1} = P_k with the interior
// replaced by inner + a_i d1 + b_j d2.  states: nullptr | nt padded planes per sample (P_0 .. P_{nt-1}, the backward's)
__device__ __forceinline__ int refl(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// EMIT: the interior of the state after every step of `em` also goes to traj[slot][B][H][W]
template <bool EMIT = false>
__global__ __launch_bounds__(256) void jac64_fwd_kernel(int H, int W, int nt, const double* __restrict__ u,
                                                        const double* __restrict__ a, const double* __restrict__ bc,
                                                        double* __restrict__ out, double* __restrict__ states,
                                                        double* __restrict__ traj, EmitMask em) {
    extern __shared__ double jsm[];
    const int Hp = H + 2, Wp = W + 2, PP = Hp * Wp, b = blockIdx.x;
    double* P = jsm;
    double* Q = jsm + PP;
    const double* ub = u + (size_t)b * H * W;
    for (int e = threadIdx.x; e < PP; e += blockDim.x) {
        const int i = e / Wp, j = e % Wp;
        Q[e] = P[e] = ub[refl(i - 1, H) * W + refl(j - 1, W)];
    }
    __syncthreads();
    for (int k = 0; k < nt; ++k) {
        if (states) {
            double* st = states + ((size_t)b * nt + k) * PP;
            for (int e = threadIdx.x; e < PP; e += blockDim.x) st[e] = P[e];
        }
        for (int e = threadIdx.x; e < H * W; e += blockDim.x) {
            const int i = e / W + 1, j = e % W + 1, q = i * Wp + j;
            const double in = P[q];
            const double d1 = (P[q + Wp] - 2.0 * in) + P[q - Wp];
            const double d2 = (P[q + 1] - 2.0 * in) + P[q - 1];
            Q[q] = (in + a[i - 1] * d1) + bc[j - 1] * d2;
        }
        __syncthreads();
        double* t = P; P = Q; Q = t;        // the ring is the same in both
        if constexpr (EMIT) {
            const int slot = emit_slot(em, k + 1);
            if (slot >= 0) {
                double* tb = traj + ((size_t)slot * gridDim.x + b) * H * W;
                for (int e = threadIdx.x; e < H * W; e += blockDim.x) tb[e] = P[(e / W + 1) * Wp + e % W + 1];
            }
        }
    }
    for (int e = threadIdx.x; e < H * W; e += blockDim.x) out[(size_t)b * H * W + e] = P[(e / W + 1) * Wp + e % W + 1];
}

// adjoint, one workgroup per sample: G over the padded plane (ring entries accumulate, interior entries are replaced);
// per-sample partial sums of the coefficient gradients: threads < H own a row, threads 64..64+W-1 a column
// EMIT: once G is the adjoint of an emitted state its interior gets += gtraj[slot]
template <bool EMIT = false>
__global__ __launch_bounds__(256) void jac64_bwd_kernel(int H, int W, int nt, const double* __restrict__ gout,
                                                        const double* __restrict__ a, const double* __restrict__ bc,
                                                        const double* __restrict__ states, double* __restrict__ gu,
                                                        double* __restrict__ pa, double* __restrict__ pb,
                                                        const double* __restrict__ gtraj, EmitMask em) {
    extern __shared__ double jsm[];
    const int Hp = H + 2, Wp = W + 2, PP = Hp * Wp, b = blockIdx.x, tid = threadIdx.x;
    double* G = jsm;
    double* G2 = jsm + PP;
    for (int e = tid; e < PP; e += blockDim.x) {
        const int i = e / Wp, j = e % Wp;
        G[e] = (i >= 1 && i <= H && j >= 1 && j <= W) ? gout[(size_t)b * H * W + (i - 1) * W + (j - 1)] : 0.0;
    }
    __syncthreads();
    double acc = 0.0;
    for (int k = nt - 1; k >= 0; --k) {
        const double* P = states + ((size_t)b * nt + k) * PP;
        if (tid < H) {                                        // row tid+1: sum_j G d1
            const int i = tid + 1;
            for (int j = 1; j <= W; ++j) {
                const int q = i * Wp + j;
                acc = fma(G[q], (P[q + Wp] - 2.0 * P[q]) + P[q - Wp], acc);
            }
        } else if (tid >= 64 && tid < 64 + W) {               // column tid-63: sum_i G d2
            const int j = tid - 63;
            for (int i = 1; i <= H; ++i) {
                const int q = i * Wp + j;
                acc = fma(G[q], (P[q + 1] - 2.0 * P[q]) + P[q - 1], acc);
            }
        }
        const double* gt = nullptr;                           // dL/d(state after step k), where that state was emitted
        if constexpr (EMIT) {
            const int slot = emit_slot(em, k);
            if (slot >= 0) gt = gtraj + ((size_t)slot * gridDim.x + b) * H * W;
        }
        for (int e = tid; e < PP; e += blockDim.x) {
            const int i = e / Wp, j = e % Wp;
            const bool inner = i >= 1 && i <= H && j >= 1 && j <= W;
            double v = inner ? G[e] * ((1.0 - 2.0 * a[i - 1]) - 2.0 * bc[j - 1]) : G[e];
            if (i - 1 >= 1 && i - 1 <= H && j >= 1 && j <= W) v += a[i - 2] * G[e - Wp];
            if (i + 1 >= 1 && i + 1 <= H && j >= 1 && j <= W) v += a[i] * G[e + Wp];
            if (j - 1 >= 1 && j - 1 <= W && i >= 1 && i <= H) v += bc[j - 2] * G[e - 1];
            if (j + 1 >= 1 && j + 1 <= W && i >= 1 && i <= H) v += bc[j] * G[e + 1];
            if constexpr (EMIT) {
                if (gt && inner) v += gt[(i - 1) * W + (j - 1)];
            }
            G2[e] = v;
        }
        __syncthreads();
        double* t = G; G = G2; G2 = t;
        __syncthreads();
    }
    if (tid < H) pa[(size_t)b * H + tid] = acc;
    else if (tid >= 64 && tid < 64 + W) pb[(size_t)b * W + tid - 64] = acc;
    // reflect padding transposed: every padded entry goes to the input element it was copied from (fixed order)
    for (int e = tid; e < H * W; e += blockDim.x) {
        const int r = e / W, c = e % W;
        int rows[3], cols[3], nr = 0, nc = 0;
        rows[nr++] = r + 1;
        if (r == 1) rows[nr++] = 0;
        if (r == H - 2) rows[nr++] = H + 1;
        cols[nc++] = c + 1;
        if (c == 1) cols[nc++] = 0;
        if (c == W - 2) cols[nc++] = W + 1;
        double s = 0.0;
        for (int x = 0; x < nr; ++x)
            for (int y = 0; y < nc; ++y) s += G[rows[x] * Wp + cols[y]];
        gu[(size_t)b * H * W + e] = s;
    }
}

// the adjoint alone (pde_jacobi_f64_backward_input[_states]: a_row and b_col take no gradient): jac64_bwd_kernel without
// the parked states and the row / column sums; G is updated and folded as it is there
template <bool EMIT = false>
__global__ __launch_bounds__(256) void jac64_bwd_input_kernel(int H, int W, int nt, const double* __restrict__ gout,
                                                              const double* __restrict__ a, const double* __restrict__ bc,
                                                              double* __restrict__ gu, const double* __restrict__ gtraj,
                                                              EmitMask em) {
    extern __shared__ double jsm[];
    const int Hp = H + 2, Wp = W + 2, PP = Hp * Wp, b = blockIdx.x, tid = threadIdx.x;
    double* G = jsm;
    double* G2 = jsm + PP;
    for (int e = tid; e < PP; e += blockDim.x) {
        const int i = e / Wp, j = e % Wp;
        G[e] = (i >= 1 && i <= H && j >= 1 && j <= W) ? gout[(size_t)b * H * W + (i - 1) * W + (j - 1)] : 0.0;
    }
    __syncthreads();
    for (int k = nt - 1; k >= 0; --k) {
        const double* gt = nullptr;                           // dL/d(state after step k), where that state was emitted
        if constexpr (EMIT) {
            const int slot = emit_slot(em, k);
            if (slot >= 0) gt = gtraj + ((size_t)slot * gridDim.x + b) * H * W;
        }
        for (int e = tid; e < PP; e += blockDim.x) {
            const int i = e / Wp, j = e % Wp;
            const bool inner = i >= 1 && i <= H && j >= 1 && j <= W;
            double v = inner ? G[e] * ((1.0 - 2.0 * a[i - 1]) - 2.0 * bc[j - 1]) : G[e];
            if (i - 1 >= 1 && i - 1 <= H && j >= 1 && j <= W) v += a[i - 2] * G[e - Wp];
            if (i + 1 >= 1 && i + 1 <= H && j >= 1 && j <= W) v += a[i] * G[e + Wp];
            if (j - 1 >= 1 && j - 1 <= W && i >= 1 && i <= H) v += bc[j - 2] * G[e - 1];
            if (j + 1 >= 1 && j + 1 <= W && i >= 1 && i <= H) v += bc[j] * G[e + 1];
            if constexpr (EMIT) {
                if (gt && inner) v += gt[(i - 1) * W + (j - 1)];
            }
            G2[e] = v;
        }
        __syncthreads();
        double* t = G; G = G2; G2 = t;
    }
    // reflect padding transposed: every padded entry goes to the input element it was copied from (fixed order)
    for (int e = tid; e < H * W; e += blockDim.x) {
        const int r = e / W, c = e % W;
        int rows[3], cols[3], nr = 0, nc = 0;
        rows[nr++] = r + 1;
        if (r == 1) rows[nr++] = 0;
        if (r == H - 2) rows[nr++] = H + 1;
        cols[nc++] = c + 1;
        if (c == 1) cols[nc++] = 0;
        if (c == W - 2) cols[nc++] = W + 1;
        double s = 0.0;
        for (int x = 0; x < nr; ++x)
            for (int y = 0; y < nc; ++y) s += G[rows[x] * Wp + cols[y]];
        gu[(size_t)b * H * W + e] = s;
    }
}

// the tangent-linear pass (pde_jacobi_f64_tangent): jac64_fwd_kernel with a second state.  dP is the reflect-padded du
// (zeros when du is NULL), both rings frozen; interior dP' = the forward's expressions on dP, then
// + da_i d1(P) + db_j d2(P) with P the step's input (not added at all when src == 0).  LDS: P, Q, dP, dQ.
__global__ __launch_bounds__(256) void jac64_tangent_kernel(int H, int W, int nt, const double* __restrict__ u,
                                                            const double* __restrict__ du, const double* __restrict__ a,
                                                            const double* __restrict__ bc, const double* __restrict__ da,
                                                            const double* __restrict__ dbc, double* __restrict__ out,
                                                            double* __restrict__ dout, int src) {
    extern __shared__ double jsm[];
    const int Hp = H + 2, Wp = W + 2, PP = Hp * Wp, b = blockIdx.x;
    double* P = jsm;
    double* Q = jsm + PP;
    double* dP = jsm + 2 * PP;
    double* dQ = jsm + 3 * PP;
    const double* ub = u + (size_t)b * H * W;
    const double* dub = du ? du + (size_t)b * H * W : nullptr;
    for (int e = threadIdx.x; e < PP; e += blockDim.x) {
        const int i = e / Wp, j = e % Wp;
        const int o = refl(i - 1, H) * W + refl(j - 1, W);
        Q[e] = P[e] = ub[o];
        dQ[e] = dP[e] = dub ? dub[o] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < nt; ++k) {
        for (int e = threadIdx.x; e < H * W; e += blockDim.x) {
            const int i = e / W + 1, j = e % W + 1, q = i * Wp + j;
            const double in = P[q];
            const double d1 = (P[q + Wp] - 2.0 * in) + P[q - Wp];
            const double d2 = (P[q + 1] - 2.0 * in) + P[q - 1];
            Q[q] = (in + a[i - 1] * d1) + bc[j - 1] * d2;
            const double din = dP[q];
            const double dd1 = (dP[q + Wp] - 2.0 * din) + dP[q - Wp];
            const double dd2 = (dP[q + 1] - 2.0 * din) + dP[q - 1];
            double dn = (din + a[i - 1] * dd1) + bc[j - 1] * dd2;
            if (src) dn = (dn + (da ? da[i - 1] : 0.0) * d1) + (dbc ? dbc[j - 1] : 0.0) * d2;
            dQ[q] = dn;
        }
        __syncthreads();
        double* t = P; P = Q; Q = t;        // the rings are the same in both
        t = dP; dP = dQ; dQ = t;
    }
    for (int e = threadIdx.x; e < H * W; e += blockDim.x) {
        const int l = (e / W + 1) * Wp + e % W + 1;
        if (out) out[(size_t)b * H * W + e] = P[l];
        dout[(size_t)b * H * W + e] = dP[l];
    }
}

__global__ void jac64_reduce_kernel(int B, int H, int W, const double* __restrict__ pa, const double* __restrict__ pb,
                                    double* __restrict__ ga, double* __restrict__ gb) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < H) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += pa[(size_t)b * H + t];
        ga[t] = s;
    } else if (t < H + W) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += pb[(size_t)b * W + t - H];
        gb[t - H] = s;
    }
}

constexpr int kJacMax = 64;
bool jac64_ok(int B, int H, int W, int nt) { return B > 0 && H >= 2 && W >= 2 && H <= kJacMax && W <= kJacMax && nt >= 0; }
size_t jac64_lds(int H, int W) { return 2 * (size_t)(H + 2) * (W + 2) * sizeof(double); }

}  // namespace
}  // namespace pde

using namespace pde;

extern "C" {

int pde_channel_mix_f64_forward(int32_t B, int32_t C, int32_t HW, const double* u, const double* M, double* out, void* stream) {
    if (!mix64_ok(B, C, HW) || !u || !M || !out || misaligned(8, u, M, out)) return PDE_E_BADARG;
    hipLaunchKernelGGL(mix64_apply_kernel, dim3((HW + 255) / 256, C, B), dim3(256), 0, static_cast<hipStream_t>(stream), C, HW,
                       u, M, out, 0);
    return check_launch();
}

size_t pde_channel_mix_f64_backward_workspace_bytes(int32_t B, int32_t C, int32_t HW) {
    if (!mix64_ok(B, C, HW)) return 0;
    return up256((size_t)C * C * sizeof(double)) + up256((size_t)mix64_nsplit(B, C) * C * C * sizeof(double));
}

int pde_channel_mix_f64_backward_steps(int32_t B, int32_t C, int32_t HW, const double* u, const double* gout, const double* M,
                                       double* gu, double* gM, void* workspace, size_t workspace_bytes, int32_t accumulate,
                                       int32_t finalize, void* stream) {
    if (!mix64_ok(B, C, HW) || !u || !gout || !M || !gu || !workspace || (finalize && !gM)) return PDE_E_BADARG;
    if (misaligned(8, u, gout, M, gu, gM)) return PDE_E_BADARG;
    if (workspace_bytes < pde_channel_mix_f64_backward_workspace_bytes(B, C, HW) || ((uintptr_t)workspace & 15))
        return PDE_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* acc = static_cast<double*>(workspace);
    double* part = reinterpret_cast<double*>(static_cast<char*>(workspace) + up256((size_t)C * C * sizeof(double)));
    const int ns = mix64_nsplit(B, C), nt = (C + kMixT - 1) / kMixT;
    hipLaunchKernelGGL(mix64_apply_kernel, dim3((HW + 255) / 256, C, B), dim3(256), 0, st, C, HW, gout, M, gu, 1);
    hipLaunchKernelGGL(mix64_gm_kernel, dim3(nt, nt, ns), dim3(256), 0, st, B, C, HW, ns, gout, u, part);
    hipLaunchKernelGGL(mix64_gm_reduce_kernel, dim3((C * C + 255) / 256), dim3(256), 0, st, C * C, ns, part, acc,
                       (int)(accumulate != 0), finalize ? gM : nullptr);
    return check_launch();
}

int pde_channel_mix_f64_backward(int32_t B, int32_t C, int32_t HW, const double* u, const double* gout, const double* M,
                                 double* gu, double* gM, void* workspace, size_t workspace_bytes, void* stream) {
    if (!gM) return PDE_E_BADARG;
    return pde_channel_mix_f64_backward_steps(B, C, HW, u, gout, M, gu, gM, workspace, workspace_bytes, 0, 1, stream);
}

// gu = M^T gout alone (M takes no gradient): the first launch of pde_channel_mix_f64_backward_steps
int pde_channel_mix_f64_backward_input(int32_t B, int32_t C, int32_t HW, const double* gout, const double* M, double* gu,
                                       void* stream) {
    if (!mix64_ok(B, C, HW) || !gout || !M || !gu || misaligned(8, gout, M, gu)) return PDE_E_BADARG;
    hipLaunchKernelGGL(mix64_apply_kernel, dim3((HW + 255) / 256, C, B), dim3(256), 0, static_cast<hipStream_t>(stream), C, HW,
                       gout, M, gu, 1);
    return check_launch();
}

int pde_skip_blend_f64_forward(int64_t n, const double* u0, const double* u, const double* skip_weight, double* out,
                               void* stream) {
    if (n <= 0 || !u0 || !u || !skip_weight || !out || misaligned(8, u0, u, skip_weight, out)) return PDE_E_BADARG;
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(blend64_fwd_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), (long long)n, u0, u, skip_weight, out);
    return check_launch();
}

size_t pde_skip_blend_f64_backward_workspace_bytes(int64_t n) {
    if (n <= 0) return 0;
    return up256((size_t)blend64_parts(n) * sizeof(double));
}

int pde_skip_blend_f64_backward(int64_t n, const double* g, const double* u0, const double* u, const double* skip_weight,
                                double* g_u0, double* g_u, double* g_skip_weight, void* workspace, size_t workspace_bytes,
                                void* stream) {
    if (n <= 0 || !g || !u0 || !u || !skip_weight || !g_u0 || !g_u || !g_skip_weight || !workspace) return PDE_E_BADARG;
    if (misaligned(8, g, u0, u, skip_weight, g_u0, g_u, g_skip_weight)) return PDE_E_BADARG;
    if (workspace_bytes < pde_skip_blend_f64_backward_workspace_bytes(n) || ((uintptr_t)workspace & 15)) return PDE_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int np = blend64_parts(n);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(blend64_bwd_kernel, dim3(np), dim3(256), 0, st, (long long)n, g, u0, u, skip_weight, g_u0, g_u, part);
    hipLaunchKernelGGL(blend64_reduce_kernel, dim3(1), dim3(256), 0, st, np, part, skip_weight, g_skip_weight);
    return check_launch();
}

// skip_weight takes no gradient: g_u0 = s g, g_u = (1 - s) g, bit for bit those of pde_skip_blend_f64_backward
int pde_skip_blend_f64_backward_input(int64_t n, const double* g, const double* skip_weight, double* g_u0, double* g_u,
                                      void* stream) {
    if (n <= 0 || !g || !skip_weight || !g_u0 || !g_u || misaligned(8, g, skip_weight, g_u0, g_u)) return PDE_E_BADARG;
    hipLaunchKernelGGL(blend64_bwd_input_kernel, dim3(blend64_parts(n)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       (long long)n, g, skip_weight, g_u0, g_u);
    return check_launch();
}

int pde_explicit5_f64_forward(int32_t B, int32_t C, int32_t H, int32_t W, const double* u, const double* alpha_base,
                              const double* channel_scaling, double dt, double eps, double max_coeff, double relax,
                              int32_t num_steps, double* states, double* out, void* stream) {
    return pde_explicit5_f64_forward_states(B, C, H, W, u, alpha_base, channel_scaling, dt, eps, max_coeff, relax, num_steps,
                                            states, out, nullptr, nullptr, stream);
}

int pde_explicit5_f64_forward_states(int32_t B, int32_t C, int32_t H, int32_t W, const double* u, const double* alpha_base,
                                     const double* channel_scaling, double dt, double eps, double max_coeff, double relax,
                                     int32_t num_steps, double* states, double* out, double* traj,
                                     const uint64_t emit_mask[2], void* stream) {
    if (B <= 0 || B > 65535 || C <= 0 || C > 65535 || H <= 0 || W <= 0 || num_steps < 1 || !u || !alpha_base ||
        !channel_scaling || !out ||
        (num_steps > 1 && !states))
        return PDE_E_BADARG;
    if (misaligned(8, u, alpha_base, channel_scaling, states, out, traj)) return PDE_E_BADARG;
    EmitMask em;
    const int erc = emit_check(emit_mask, num_steps, traj, em);
    if (erc != PDE_OK) return erc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)B * C * H * W;
    const dim3 grid((H * W + 255) / 256, C, B);
    for (int k = 0; k < num_steps; ++k) {
        const double* x = k == 0 ? u : states + (k - 1) * n;
        double* y = k == num_steps - 1 ? out : states + k * n;
        const int slot = emit_slot(em, k + 1);
        if (slot >= 0)
            hipLaunchKernelGGL(expl64_fwd_kernel<true>, grid, dim3(256), 0, st, C, H, W, x, alpha_base, channel_scaling, dt,
                               eps, max_coeff, relax, y, traj + (size_t)slot * n);
        else
            hipLaunchKernelGGL(expl64_fwd_kernel<false>, grid, dim3(256), 0, st, C, H, W, x, alpha_base, channel_scaling, dt,
                               eps, max_coeff, relax, y, (double*)nullptr);
    }
    return check_launch();
}

size_t pde_explicit5_f64_backward_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_steps) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_steps < 1) return 0;
    const size_t n = (size_t)B * C * H * W;
    return up256((size_t)B * C * 2 * sizeof(double)) + (num_steps > 1 ? 2 * up256(n * sizeof(double)) : 0);
}

int pde_explicit5_f64_backward(int32_t B, int32_t C, int32_t H, int32_t W, const double* u, const double* states,
                               const double* gout, const double* alpha_base, const double* channel_scaling, double dt,
                               double eps, double max_coeff, double relax, int32_t num_steps, double* gu,
                               double* g_alpha_base, double* g_channel_scaling, void* workspace, size_t workspace_bytes,
                               void* stream) {
    return pde_explicit5_f64_backward_states(B, C, H, W, u, states, gout, nullptr, nullptr, alpha_base, channel_scaling, dt,
                                             eps, max_coeff, relax, num_steps, gu, g_alpha_base, g_channel_scaling, workspace,
                                             workspace_bytes, stream);
}

int pde_explicit5_f64_backward_states(int32_t B, int32_t C, int32_t H, int32_t W, const double* u, const double* states,
                                      const double* gout, const double* gtraj, const uint64_t emit_mask[2],
                                      const double* alpha_base, const double* channel_scaling, double dt, double eps,
                                      double max_coeff, double relax, int32_t num_steps, double* gu, double* g_alpha_base,
                                      double* g_channel_scaling, void* workspace, size_t workspace_bytes, void* stream) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_steps < 1 || !u || !gout || !alpha_base || !channel_scaling || !gu ||
        !g_alpha_base || !g_channel_scaling || !workspace || (num_steps > 1 && !states))
        return PDE_E_BADARG;
    if (misaligned(8, u, states, gout, gtraj, alpha_base, channel_scaling, gu, g_alpha_base, g_channel_scaling)) return PDE_E_BADARG;
    EmitMask em;
    const int erc = emit_check(emit_mask, num_steps, gtraj, em);
    if (erc != PDE_OK) return erc;
    if (workspace_bytes < pde_explicit5_f64_backward_workspace_bytes(B, C, H, W, num_steps) || ((uintptr_t)workspace & 15))
        return PDE_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)B * C * H * W;
    char* ws = static_cast<char*>(workspace);
    double* part = reinterpret_cast<double*>(ws);
    ws += up256((size_t)B * C * 2 * sizeof(double));
    double* buf[2] = {reinterpret_cast<double*>(ws), reinterpret_cast<double*>(ws + up256(n * sizeof(double)))};
    const double* g = gout;
    for (int k = num_steps - 1; k >= 0; --k) {
        const double* x = k == 0 ? u : states + (size_t)(k - 1) * n;
        double* gx = k == 0 ? gu : buf[k & 1];
        const int slot = emit_slot(em, k);                 // gx is the adjoint of the state after step k
        if (slot >= 0)
            hipLaunchKernelGGL(expl64_bwd_kernel<true>, dim3(B * C), dim3(256), 0, st, C, H, W, x, g, alpha_base,
                               channel_scaling, dt, eps, max_coeff, relax, gx, part, (int)(k != num_steps - 1),
                               gtraj + (size_t)slot * n);
        else
            hipLaunchKernelGGL(expl64_bwd_kernel<false>, dim3(B * C), dim3(256), 0, st, C, H, W, x, g, alpha_base,
                               channel_scaling, dt, eps, max_coeff, relax, gx, part, (int)(k != num_steps - 1),
                               (const double*)nullptr);
        g = gx;
    }
    hipLaunchKernelGGL(expl64_reduce_kernel, dim3((C + 63) / 64), dim3(64), 0, st, B, C, part, alpha_base, dt, eps, max_coeff,
                       g_alpha_base, g_channel_scaling);
    return check_launch();
}

int pde_jacobi_f64_forward(int32_t B, int32_t H, int32_t W, int32_t nt, const double* u, const double* a_row,
                           const double* b_col, double* out, void* stream) {
    return pde_jacobi_f64_forward_states(B, H, W, nt, u, a_row, b_col, out, nullptr, nullptr, stream);
}

int pde_jacobi_f64_forward_states(int32_t B, int32_t H, int32_t W, int32_t nt, const double* u, const double* a_row,
                                  const double* b_col, double* out, double* states, const uint64_t emit_mask[2],
                                  void* stream) {
    if (!jac64_ok(B, H, W, nt) || !u || !a_row || !b_col || !out) return PDE_E_BADARG;
    if (misaligned(8, u, a_row, b_col, out, states)) return PDE_E_BADARG;
    EmitMask em;
    int rc = emit_check(emit_mask, nt, states, em);
    if (rc != PDE_OK) return rc;
    static unsigned long long done = 0, done_e = 0;
    if (em.any()) {
        rc = ensure_dynamic_lds((const void*)jac64_fwd_kernel<true>, (int)jac64_lds(kJacMax, kJacMax), done_e);
        if (rc != PDE_OK) return rc;
        hipLaunchKernelGGL(jac64_fwd_kernel<true>, dim3(B), dim3(256), jac64_lds(H, W), static_cast<hipStream_t>(stream), H, W,
                           nt, u, a_row, b_col, out, (double*)nullptr, states, em);
        return check_launch();
    }
    rc = ensure_dynamic_lds((const void*)jac64_fwd_kernel<false>, (int)jac64_lds(kJacMax, kJacMax), done);
    if (rc != PDE_OK) return rc;
    hipLaunchKernelGGL(jac64_fwd_kernel<false>, dim3(B), dim3(256), jac64_lds(H, W), static_cast<hipStream_t>(stream), H, W, nt,
                       u, a_row, b_col, out, (double*)nullptr, (double*)nullptr, em);
    return check_launch();
}

size_t pde_jacobi_f64_backward_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t nt) {
    if (!jac64_ok(B, H, W, nt)) return 0;
    return up256((size_t)B * nt * (H + 2) * (W + 2) * sizeof(double)) + up256((size_t)B * (H + W) * sizeof(double)) +
           up256((size_t)B * H * W * sizeof(double));
}

int pde_jacobi_f64_backward(int32_t B, int32_t H, int32_t W, int32_t nt, const double* u, const double* gout,
                            const double* a_row, const double* b_col, double* gu, double* g_a_row, double* g_b_col,
                            void* workspace, size_t workspace_bytes, void* stream) {
    return pde_jacobi_f64_backward_states(B, H, W, nt, u, gout, nullptr, nullptr, a_row, b_col, gu, g_a_row, g_b_col, workspace,
                                          workspace_bytes, stream);
}

int pde_jacobi_f64_backward_states(int32_t B, int32_t H, int32_t W, int32_t nt, const double* u, const double* gout,
                                   const double* gstates, const uint64_t emit_mask[2], const double* a_row,
                                   const double* b_col, double* gu, double* g_a_row, double* g_b_col, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    if (!jac64_ok(B, H, W, nt) || !u || !gout || !a_row || !b_col || !gu || !g_a_row || !g_b_col || !workspace)
        return PDE_E_BADARG;
    if (misaligned(8, u, gout, gstates, a_row, b_col, gu, g_a_row, g_b_col)) return PDE_E_BADARG;
    EmitMask em;
    int rc = emit_check(emit_mask, nt, gstates, em);
    if (rc != PDE_OK) return rc;
    if (workspace_bytes < pde_jacobi_f64_backward_workspace_bytes(B, H, W, nt) || ((uintptr_t)workspace & 15))
        return PDE_E_WORKSPACE;
    static unsigned long long done_f = 0, done_b = 0, done_e = 0;
    rc = ensure_dynamic_lds((const void*)jac64_fwd_kernel<false>, (int)jac64_lds(kJacMax, kJacMax), done_f);
    if (rc != PDE_OK) return rc;
    rc = em.any() ? ensure_dynamic_lds((const void*)jac64_bwd_kernel<true>, (int)jac64_lds(kJacMax, kJacMax), done_e)
                  : ensure_dynamic_lds((const void*)jac64_bwd_kernel<false>, (int)jac64_lds(kJacMax, kJacMax), done_b);
    if (rc != PDE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    double* states = reinterpret_cast<double*>(ws);
    ws += up256((size_t)B * nt * (H + 2) * (W + 2) * sizeof(double));
    double* pa = reinterpret_cast<double*>(ws);
    double* pb = pa + (size_t)B * H;
    ws += up256((size_t)B * (H + W) * sizeof(double));
    double* scratch = reinterpret_cast<double*>(ws);          // the forward's output, not needed
    hipLaunchKernelGGL(jac64_fwd_kernel<false>, dim3(B), dim3(256), jac64_lds(H, W), st, H, W, nt, u, a_row, b_col, scratch,
                       states, (double*)nullptr, EmitMask{0, 0});
    if (em.any())
        hipLaunchKernelGGL(jac64_bwd_kernel<true>, dim3(B), dim3(256), jac64_lds(H, W), st, H, W, nt, gout, a_row, b_col,
                           states, gu, pa, pb, gstates, em);
    else
        hipLaunchKernelGGL(jac64_bwd_kernel<false>, dim3(B), dim3(256), jac64_lds(H, W), st, H, W, nt, gout, a_row, b_col,
                           states, gu, pa, pb, (const double*)nullptr, em);
    hipLaunchKernelGGL(jac64_reduce_kernel, dim3((H + W + 127) / 128), dim3(128), 0, st, B, H, W, pa, pb, g_a_row, g_b_col);
    return check_launch();
}

// ---- the backward for the input alone (pdecnn_explicit_input.h): the parameters take no gradient -----------------------
size_t pde_explicit5_f64_backward_input_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_steps) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_steps < 2) return 0;
    return 2 * up256((size_t)B * C * H * W * sizeof(double));
}

int pde_explicit5_f64_backward_input(int32_t B, int32_t C, int32_t H, int32_t W, const double* gout, const double* alpha_base,
                                     const double* channel_scaling, double dt, double eps, double max_coeff, double relax,
                                     int32_t num_steps, double* gu, void* workspace, size_t workspace_bytes, void* stream) {
    return pde_explicit5_f64_backward_input_states(B, C, H, W, gout, nullptr, nullptr, alpha_base, channel_scaling, dt, eps,
                                                   max_coeff, relax, num_steps, gu, workspace, workspace_bytes, stream);
}

int pde_explicit5_f64_backward_input_states(int32_t B, int32_t C, int32_t H, int32_t W, const double* gout,
                                            const double* gtraj, const uint64_t emit_mask[2], const double* alpha_base,
                                            const double* channel_scaling, double dt, double eps, double max_coeff,
                                            double relax, int32_t num_steps, double* gu, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_steps < 1 || !gout || !alpha_base || !channel_scaling || !gu)
        return PDE_E_BADARG;
    if (misaligned(8, gout, gtraj, alpha_base, channel_scaling, gu)) return PDE_E_BADARG;
    EmitMask em;
    const int erc = emit_check(emit_mask, num_steps, gtraj, em);
    if (erc != PDE_OK) return erc;
    const size_t need = pde_explicit5_f64_backward_input_workspace_bytes(B, C, H, W, num_steps);
    if ((need && (!workspace || workspace_bytes < need)) || ((uintptr_t)workspace & 15)) return PDE_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)B * C * H * W;
    char* ws = static_cast<char*>(workspace);
    double* buf[2] = {reinterpret_cast<double*>(ws), need ? reinterpret_cast<double*>(ws + up256(n * sizeof(double))) : nullptr};
    const double* g = gout;
    for (int k = num_steps - 1; k >= 0; --k) {
        double* gx = k == 0 ? gu : buf[k & 1];
        const int slot = emit_slot(em, k);                 // gx is the adjoint of the state after step k
        if (slot >= 0)
            hipLaunchKernelGGL(expl64_bwd_input_kernel<true>, dim3(B * C), dim3(256), 0, st, C, H, W, g, alpha_base,
                               channel_scaling, dt, eps, max_coeff, relax, gx, gtraj + (size_t)slot * n);
        else
            hipLaunchKernelGGL(expl64_bwd_input_kernel<false>, dim3(B * C), dim3(256), 0, st, C, H, W, g, alpha_base,
                               channel_scaling, dt, eps, max_coeff, relax, gx, (const double*)nullptr);
        g = gx;
    }
    return check_launch();
}

int pde_jacobi_f64_backward_input(int32_t B, int32_t H, int32_t W, int32_t nt, const double* gout, const double* a_row,
                                  const double* b_col, double* gu, void* stream) {
    return pde_jacobi_f64_backward_input_states(B, H, W, nt, gout, nullptr, nullptr, a_row, b_col, gu, stream);
}

int pde_jacobi_f64_backward_input_states(int32_t B, int32_t H, int32_t W, int32_t nt, const double* gout,
                                         const double* gstates, const uint64_t emit_mask[2], const double* a_row,
                                         const double* b_col, double* gu, void* stream) {
    if (!jac64_ok(B, H, W, nt) || !gout || !a_row || !b_col || !gu) return PDE_E_BADARG;
    if (misaligned(8, gout, gstates, a_row, b_col, gu)) return PDE_E_BADARG;
    EmitMask em;
    int rc = emit_check(emit_mask, nt, gstates, em);
    if (rc != PDE_OK) return rc;
    static unsigned long long done_b = 0, done_e = 0;
    rc = em.any() ? ensure_dynamic_lds((const void*)jac64_bwd_input_kernel<true>, (int)jac64_lds(kJacMax, kJacMax), done_e)
                  : ensure_dynamic_lds((const void*)jac64_bwd_input_kernel<false>, (int)jac64_lds(kJacMax, kJacMax), done_b);
    if (rc != PDE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (em.any())
        hipLaunchKernelGGL(jac64_bwd_input_kernel<true>, dim3(B), dim3(256), jac64_lds(H, W), st, H, W, nt, gout, a_row, b_col,
                           gu, gstates, em);
    else
        hipLaunchKernelGGL(jac64_bwd_input_kernel<false>, dim3(B), dim3(256), jac64_lds(H, W), st, H, W, nt, gout, a_row, b_col,
                           gu, (const double*)nullptr, em);
    return check_launch();
}

}  // extern "C"

// ---- the tangent-linear pass (pdecnn_explicit_tangent.h): (y, dy) from (u, du) and the parameter tangents ---------------
extern "C" {

size_t pde_explicit5_f64_tangent_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_steps) {
    if (B <= 0 || B > 65535 || C <= 0 || C > 65535 || H <= 0 || W <= 0 || num_steps < 2) return 0;
    return 4 * up256((size_t)B * C * H * W * sizeof(double));       // u and du ping-pong through two images each
}

int pde_explicit5_f64_tangent(int32_t B, int32_t C, int32_t H, int32_t W, const double* u, const double* du,
                              const double* alpha_base, const double* channel_scaling, const double* d_alpha_base,
                              const double* d_channel_scaling, double dt, double eps, double max_coeff, double relax,
                              int32_t num_steps, double* y, double* dy, void* workspace, size_t workspace_bytes,
                              void* stream) {
    if (B <= 0 || B > 65535 || C <= 0 || C > 65535 || H <= 0 || W <= 0 || num_steps < 1 || !u || !alpha_base ||
        !channel_scaling || !dy)
        return PDE_E_BADARG;
    if (!du && !d_alpha_base && !d_channel_scaling) return PDE_E_BADARG;       // nothing to differentiate: call the forward
    if (misaligned(8, u, du, alpha_base, channel_scaling, d_alpha_base, d_channel_scaling, y, dy)) return PDE_E_BADARG;
    const size_t need = pde_explicit5_f64_tangent_workspace_bytes(B, C, H, W, num_steps);
    if ((need && (!workspace || workspace_bytes < need)) || ((uintptr_t)workspace & 15)) return PDE_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t ib = up256((size_t)B * C * H * W * sizeof(double));
    char* ws = static_cast<char*>(workspace);
    double* img[2] = {need ? reinterpret_cast<double*>(ws) : nullptr, need ? reinterpret_cast<double*>(ws + ib) : nullptr};
    double* dimg[2] = {need ? reinterpret_cast<double*>(ws + 2 * ib) : nullptr,
                       need ? reinterpret_cast<double*>(ws + 3 * ib) : nullptr};
    const int src = (d_alpha_base || d_channel_scaling) ? 1 : 0;
    const dim3 grid((H * W + 255) / 256, C, B);
    for (int k = 0; k < num_steps; ++k) {
        const bool first = k == 0, last = k == num_steps - 1;
        hipLaunchKernelGGL(expl64_tangent_kernel, grid, dim3(256), 0, st, C, H, W, first ? u : (const double*)img[(k - 1) & 1],
                           first ? du : (const double*)dimg[(k - 1) & 1], alpha_base, channel_scaling, d_alpha_base,
                           d_channel_scaling, dt, eps, max_coeff, relax, last ? y : img[k & 1], last ? dy : dimg[k & 1], src);
    }
    return check_launch();
}

int pde_jacobi_f64_tangent(int32_t B, int32_t H, int32_t W, int32_t nt, const double* u, const double* du,
                           const double* a_row, const double* b_col, const double* d_a_row, const double* d_b_col,
                           double* y, double* dy, void* stream) {
    if (!jac64_ok(B, H, W, nt) || !u || !a_row || !b_col || !dy) return PDE_E_BADARG;
    if (!du && !d_a_row && !d_b_col) return PDE_E_BADARG;                     // nothing to differentiate: call the forward
    if (misaligned(8, u, du, a_row, b_col, d_a_row, d_b_col, y, dy)) return PDE_E_BADARG;
    static unsigned long long done = 0;
    const int rc = ensure_dynamic_lds((const void*)jac64_tangent_kernel, (int)(2 * jac64_lds(kJacMax, kJacMax)), done);
    if (rc != PDE_OK) return rc;
    hipLaunchKernelGGL(jac64_tangent_kernel, dim3(B), dim3(256), 2 * jac64_lds(H, W), static_cast<hipStream_t>(stream), H, W,
                       nt, u, du, a_row, b_col, d_a_row, d_b_col, y, dy, (d_a_row || d_b_col) ? 1 : 0);
    return check_launch();
}

}  // extern "C"
