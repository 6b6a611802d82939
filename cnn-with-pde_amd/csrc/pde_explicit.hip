// K2 — explicit 5-point layers.
//
// explicit5: tiny_imagenet.py:34-72, one relaxed step
//     a_c = clamp(alpha_base_c, eps, max_coeff);  v = s_c u
//     out = u + relax*(v + a_c*dt*Lap0(v) - u)            Lap0: zero ghost cells (conv2d padding=1)
//   HBM-bound: 4 B read + 4 B written per element.  Planes of 64x64, 32x32 and 16x16 take the wave-per-plane
//   kernels below: a wave keeps its whole plane in registers (lane = (row group, 4-column group), R consecutive
//   rows of one float4 each), so every element is loaded from memory exactly once; east/west neighbours come
//   from the neighbouring lane by DPP wave shifts, north/south from the lane's own registers, the two halo rows
//   of a row group from the lanes W/4 away (__shfl); num_steps > 1 stay in registers between the steps.  Other
//   plane sizes (any H, W >= 1) take the generic kernel (neighbours through L1/L2), one launch per step: in float4
//   columns when W is a multiple of 4, in single columns otherwise.
//   Backward (Lap0 is self-adjoint):
//     gu   = (1-relax) g + relax*s_c*(g + a_c dt Lap0 g)
//     gs_c = relax * sum (g + a_c dt Lap0 g) u
//     ga_c = [eps <= alpha_base_c <= max_coeff] * relax*dt*s_c * sum (Lap0 g) u
//   one workgroup per (b,c) plane writes its two partial sums; a second kernel adds
//   them over b in a fixed order (no float atomics).
//
// jacobi: emotion_recognition.py:82-97, P = reflect_pad(u); nt times
//     P_int += A_i (P[i+1,j]-2P[i,j]+P[i-1,j]) + B_j (P[i,j+1]-2P[i,j]+P[i,j-1]); ring frozen.
//   H, W <= 64: one workgroup per sample, the padded plane lives in LDS for the whole time loop.
//   Backward recomputes the forward, parking each state in the workspace, then walks the
//   adjoint back, accumulating dA_i, dB_j per sample; a second kernel sums over samples.
//   Larger planes (up to PDE_JACOBI_MAX_HW): the tiled kernels of pde_jacobi_tiled.h.
//
// trajectory (pde_explicit5_*_states, pde_jacobi_io_*_states): every forward / backward kernel above has an emitting
//   variant — a template flag (EMIT; TE for the generic explicit kernels): the plain instantiations run the instructions
//   they ran, with two more (unread) kernel arguments.
//   Forward: after a time step whose bit is set in the 128-bit mask (EmitMask, pde_common.h) the state is also written to
//   its slot of the trajectory tensor in the tensors' own type, rounded once, while the time loop goes on in fp32.
//   Backward: once the walk holds the adjoint of an emitted state, that state's upstream gradient is added to it (interior
//   cells only for Jacobi).  No launch is added: an empty mask runs the plain instantiations, and the plain entry points
//   are the *_states ones with a NULL mask.
//
// input-only backward (pdecnn_explicit_input.h: pde_explicit5_backward_input[_states], pde_jacobi_io_backward_input[_states]):
//   both layers are linear in u, so with frozen parameters gu is the adjoint walk alone.  Every backward kernel above has a
//   twin of its own (explicit5_bwd_input_wave, explicit5_bwd_input[_col]_kernel, jacobi_bwd_input_kernel,
//   jacobi_tiled_bwd_input_kernel) that is the reverse walk with everything but the adjoint removed — no u, no states, no
//   dots, no partial sums, no pgrad launch; the Jacobi twins re-run no forward and park nothing.  What happens to the adjoint
//   is written as it is in the full kernel, in its order, so gu has the same bits; the full kernels stay as they are.
#include <type_traits>

#include "pde_common.h"

namespace pde {
namespace {

struct bf16e { unsigned short v; };
__device__ __forceinline__ float bf2f(unsigned short h) { return __uint_as_float((unsigned int)h << 16); }
__device__ __forceinline__ unsigned short f2bf(float f) { return f32_to_bf16_hw(f); }
template <typename IO> struct V4;
template <> struct V4<float> {
    __device__ static __forceinline__ float4 ld(const float* p) { return *reinterpret_cast<const float4*>(p); }
    __device__ static __forceinline__ void st(float* p, float4 v) {       // written once, never re-read here
        typedef float f4 __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(f4{v.x, v.y, v.z, v.w}, reinterpret_cast<f4*>(p));
    }
    __device__ static __forceinline__ float ld1(const float* p) { return *p; }
    __device__ static __forceinline__ float4 ld_once(const float* p) {    // no neighbour re-reads this one
        typedef float f4 __attribute__((ext_vector_type(4)));
        const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p));
        return make_float4(v.x, v.y, v.z, v.w);
    }
    __device__ static __forceinline__ float4 round(float4 v) { return v; }
};
template <> struct V4<bf16e> {
    __device__ static __forceinline__ float4 ld(const bf16e* p) {
        const ushort4 q = *reinterpret_cast<const ushort4*>(p);
        return make_float4(bf2f(q.x), bf2f(q.y), bf2f(q.z), bf2f(q.w));
    }
    __device__ static __forceinline__ void st(bf16e* p, float4 v) {
        ushort4 q; q.x = f2bf(v.x); q.y = f2bf(v.y); q.z = f2bf(v.z); q.w = f2bf(v.w);
        *reinterpret_cast<ushort4*>(p) = q;
    }
    __device__ static __forceinline__ float ld1(const bf16e* p) { return bf2f(p->v); }
    __device__ static __forceinline__ float4 ld_once(const bf16e* p) { return ld(p); }
    __device__ static __forceinline__ float4 round(float4 v) {
        return make_float4(bf2f(f2bf(v.x)), bf2f(f2bf(v.y)), bf2f(f2bf(v.z)), bf2f(f2bf(v.w)));
    }
};
struct f16e { unsigned short v; };
template <> struct V4<f16e> {
    __device__ static __forceinline__ float4 ld(const f16e* p) {
        const ushort4 q = *reinterpret_cast<const ushort4*>(p);
        return make_float4(f16_to_f32(q.x), f16_to_f32(q.y), f16_to_f32(q.z), f16_to_f32(q.w));
    }
    __device__ static __forceinline__ void st(f16e* p, float4 v) {
        ushort4 q; q.x = f32_to_f16_hw(v.x); q.y = f32_to_f16_hw(v.y); q.z = f32_to_f16_hw(v.z); q.w = f32_to_f16_hw(v.w);
        *reinterpret_cast<ushort4*>(p) = q;
    }
    __device__ static __forceinline__ float ld1(const f16e* p) { return f16_to_f32(p->v); }
    __device__ static __forceinline__ float4 ld_once(const f16e* p) { return ld(p); }
    __device__ static __forceinline__ float4 round(float4 v) {
        return make_float4(f16_to_f32(f32_to_f16_hw(v.x)), f16_to_f32(f32_to_f16_hw(v.y)), f16_to_f32(f32_to_f16_hw(v.z)),
                           f16_to_f32(f32_to_f16_hw(v.w)));
    }
};
// one element of a tensor of the layer's own type (the Jacobi kernels: the time loop itself is fp32 in LDS)
template <typename IO> struct S1;
template <> struct S1<float> {
    __device__ static __forceinline__ float ld(const float* p) { return *p; }
    __device__ static __forceinline__ void st(float* p, float v) { *p = v; }
};
template <> struct S1<bf16e> {
    __device__ static __forceinline__ float ld(const bf16e* p) { return bf2f(p->v); }
    __device__ static __forceinline__ void st(bf16e* p, float v) { p->v = f2bf(v); }
};
template <> struct S1<f16e> {
    __device__ static __forceinline__ float ld(const f16e* p) { return f16_to_f32(p->v); }
    __device__ static __forceinline__ void st(f16e* p, float v) { p->v = f32_to_f16_hw(v); }
};

// 5-point Laplacian with zero ghost cells of 4 consecutive columns (h, w0..w0+3) of one plane
template <typename IO>
__device__ __forceinline__ float4 lap0_4(const IO* plane, int H, int W, int h, int w0, const float4& c) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 n = (h > 0) ? V4<IO>::ld(plane + (size_t)(h - 1) * W + w0) : z;
    const float4 s = (h + 1 < H) ? V4<IO>::ld(plane + (size_t)(h + 1) * W + w0) : z;
    const float l = (w0 > 0) ? V4<IO>::ld1(plane + (size_t)h * W + w0 - 1) : 0.f;
    const float r = (w0 + 4 < W) ? V4<IO>::ld1(plane + (size_t)h * W + w0 + 4) : 0.f;
    float4 o;
    o.x = n.x + s.x + l + c.y - 4.f * c.x;
    o.y = n.y + s.y + c.x + c.z - 4.f * c.y;
    o.z = n.z + s.z + c.y + c.w - 4.f * c.z;
    o.w = n.w + s.w + c.z + r - 4.f * c.w;
    return o;
}

// (TI / TO: the step's input and output types — a call with bf16 tensors reads bf16 in its first step and writes bf16 in
//  its last; what passes between the steps is fp32.  TE: void, or the type of the trajectory tensor `emit`, which then
//  receives this step's output too, rounded once — the emitting variants of pde_explicit5_forward_states)
struct NoEmit {};
template <typename TE> struct EmitPtr { typedef TE* type; };
template <> struct EmitPtr<void> { typedef NoEmit type; };
template <> struct EmitPtr<const void> { typedef NoEmit type; };
template <typename TI, typename TO, typename TE = void>
__global__ __launch_bounds__(256) void explicit5_fwd_kernel(const TI* __restrict__ u, const float* __restrict__ alpha,
                                                            const float* __restrict__ scale, TO* __restrict__ out,
                                                            int C, int H, int W, float dt, float eps, float maxc,
                                                            float relax, typename EmitPtr<TE>::type emit) {
    const int pc = blockIdx.x;                         // plane index b*C + c
    const int c = pc % C;
    const float a = fminf(fmaxf(alpha[c], eps), maxc) * dt;
    const float s = scale[c];
    const TI* plane = u + (size_t)pc * H * W;
    TO* oplane = out + (size_t)pc * H * W;
    const int W4 = W / 4;
    for (int f = threadIdx.x; f < H * W4; f += 256) {
        const int h = f / W4, w0 = 4 * (f % W4);
        const float4 cu = V4<TI>::ld(plane + (size_t)h * W + w0);
        const float4 lp = lap0_4<TI>(plane, H, W, h, w0, cu);          // Lap0(u); Lap0(v) = s*Lap0(u)
        float4 o;
        // v = s u; new = v + a*(s*lap); out = u + relax*(new - u)
        { const float v = s * cu.x; const float nw = v + a * (s * lp.x); o.x = cu.x + relax * (nw - cu.x); }
        { const float v = s * cu.y; const float nw = v + a * (s * lp.y); o.y = cu.y + relax * (nw - cu.y); }
        { const float v = s * cu.z; const float nw = v + a * (s * lp.z); o.z = cu.z + relax * (nw - cu.z); }
        { const float v = s * cu.w; const float nw = v + a * (s * lp.w); o.w = cu.w + relax * (nw - cu.w); }
        V4<TO>::st(oplane + (size_t)h * W + w0, o);
        if constexpr (!std::is_void<TE>::value) V4<TE>::st(emit + (size_t)pc * H * W + (size_t)h * W + w0, o);
    }
}

__device__ __forceinline__ float block_sum_256(float v, float* sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// (TE: void, or the type of `ginj`, the gradient of the emitted state this step's output is the adjoint of: added to gu)
template <typename TU, typename TG, typename TO, typename TE = void>
__global__ __launch_bounds__(256) void explicit5_bwd_kernel(const TU* __restrict__ u, const TG* __restrict__ g,
                                                            const float* __restrict__ alpha,
                                                            const float* __restrict__ scale, TO* __restrict__ gu,
                                                            float* __restrict__ part, int C, int H, int W, float dt,
                                                            float eps, float maxc, float relax, int accumulate,
                                                            typename EmitPtr<const TE>::type ginj) {
    __shared__ float sh[4];
    const int pc = blockIdx.x;
    const int c = pc % C;
    const float a = fminf(fmaxf(alpha[c], eps), maxc) * dt;
    const float s = scale[c];
    const TU* up = u + (size_t)pc * H * W;
    const TG* gp = g + (size_t)pc * H * W;
    TO* op = gu + (size_t)pc * H * W;
    const int W4 = W / 4;
    float p1 = 0.f, p2 = 0.f;                          // sum g*u, sum Lap0(g)*u
    for (int f = threadIdx.x; f < H * W4; f += 256) {
        const int h = f / W4, w0 = 4 * (f % W4);
        const float4 cg = V4<TG>::ld(gp + (size_t)h * W + w0);
        const float4 cu = V4<TU>::ld_once(up + (size_t)h * W + w0);
        const float4 lg = lap0_4<TG>(gp, H, W, h, w0, cg);
        float4 o;
        o.x = (1.f - relax) * cg.x + relax * s * (cg.x + a * lg.x);
        o.y = (1.f - relax) * cg.y + relax * s * (cg.y + a * lg.y);
        o.z = (1.f - relax) * cg.z + relax * s * (cg.z + a * lg.z);
        o.w = (1.f - relax) * cg.w + relax * s * (cg.w + a * lg.w);
        if constexpr (!std::is_void<TE>::value) {
            const float4 gi = V4<TE>::ld_once(ginj + (size_t)pc * H * W + (size_t)h * W + w0);
            o.x += gi.x; o.y += gi.y; o.z += gi.z; o.w += gi.w;
        }
        V4<TO>::st(op + (size_t)h * W + w0, o);
        p1 += cg.x * cu.x + cg.y * cu.y + cg.z * cu.z + cg.w * cu.w;
        p2 += lg.x * cu.x + lg.y * cu.y + lg.z * cu.z + lg.w * cu.w;
    }
    const float s1 = block_sum_256(p1, sh);
    const float s2 = block_sum_256(p2, sh);
    if (threadIdx.x == 0) {
        part[2 * (size_t)pc] = accumulate ? part[2 * (size_t)pc] + s1 : s1;
        part[2 * (size_t)pc + 1] = accumulate ? part[2 * (size_t)pc + 1] + s2 : s2;
    }
}

// Scalar-column variants for widths that are not a multiple of 4: a row then starts at any element, not on a 16-byte
// boundary, so the float4 body above cannot simply get a tail.  One element per thread and pass, the same expressions
// in the same order as lap0_4 and the kernels above.
template <typename IO>
__device__ __forceinline__ float lap0_1(const IO* plane, int H, int W, int h, int w, float c) {
    const float n = (h > 0) ? S1<IO>::ld(plane + (size_t)(h - 1) * W + w) : 0.f;
    const float s = (h + 1 < H) ? S1<IO>::ld(plane + (size_t)(h + 1) * W + w) : 0.f;
    const float l = (w > 0) ? S1<IO>::ld(plane + (size_t)h * W + w - 1) : 0.f;
    const float r = (w + 1 < W) ? S1<IO>::ld(plane + (size_t)h * W + w + 1) : 0.f;
    return n + s + l + r - 4.f * c;
}

template <typename TI, typename TO, typename TE = void>
__global__ __launch_bounds__(256) void explicit5_fwd_col_kernel(const TI* __restrict__ u, const float* __restrict__ alpha,
                                                                const float* __restrict__ scale, TO* __restrict__ out,
                                                                int C, int H, int W, float dt, float eps, float maxc,
                                                                float relax, typename EmitPtr<TE>::type emit) {
    const int pc = blockIdx.x;
    const int c = pc % C;
    const float a = fminf(fmaxf(alpha[c], eps), maxc) * dt;
    const float s = scale[c];
    const TI* plane = u + (size_t)pc * H * W;
    TO* oplane = out + (size_t)pc * H * W;
    for (int f = threadIdx.x; f < H * W; f += 256) {
        const int h = f / W, w = f % W;
        const float cu = S1<TI>::ld(plane + f);
        const float lp = lap0_1<TI>(plane, H, W, h, w, cu);
        const float v = s * cu;
        const float nw = v + a * (s * lp);
        const float o = cu + relax * (nw - cu);
        S1<TO>::st(oplane + f, o);
        if constexpr (!std::is_void<TE>::value) S1<TE>::st(emit + (size_t)pc * H * W + f, o);
    }
}

template <typename TU, typename TG, typename TO, typename TE = void>
__global__ __launch_bounds__(256) void explicit5_bwd_col_kernel(const TU* __restrict__ u, const TG* __restrict__ g,
                                                                const float* __restrict__ alpha,
                                                                const float* __restrict__ scale, TO* __restrict__ gu,
                                                                float* __restrict__ part, int C, int H, int W, float dt,
                                                                float eps, float maxc, float relax, int accumulate,
                                                                typename EmitPtr<const TE>::type ginj) {
    __shared__ float sh[4];
    const int pc = blockIdx.x;
    const int c = pc % C;
    const float a = fminf(fmaxf(alpha[c], eps), maxc) * dt;
    const float s = scale[c];
    const TU* up = u + (size_t)pc * H * W;
    const TG* gp = g + (size_t)pc * H * W;
    TO* op = gu + (size_t)pc * H * W;
    float p1 = 0.f, p2 = 0.f;                          // sum g*u, sum Lap0(g)*u
    for (int f = threadIdx.x; f < H * W; f += 256) {
        const int h = f / W, w = f % W;
        const float cg = S1<TG>::ld(gp + f);
        const float cu = S1<TU>::ld(up + f);
        const float lg = lap0_1<TG>(gp, H, W, h, w, cg);
        float o = (1.f - relax) * cg + relax * s * (cg + a * lg);
        if constexpr (!std::is_void<TE>::value) o += S1<TE>::ld(ginj + (size_t)pc * H * W + f);
        S1<TO>::st(op + f, o);
        p1 += cg * cu;
        p2 += lg * cu;
    }
    const float s1 = block_sum_256(p1, sh);
    const float s2 = block_sum_256(p2, sh);
    if (threadIdx.x == 0) {
        part[2 * (size_t)pc] = accumulate ? part[2 * (size_t)pc] + s1 : s1;
        part[2 * (size_t)pc + 1] = accumulate ? part[2 * (size_t)pc + 1] + s2 : s2;
    }
}

// The adjoint of one step alone (pde_explicit5_backward_input[_states]: alpha_base and channel_scaling take no gradient):
// explicit5_bwd_kernel / explicit5_bwd_col_kernel without the u loads, the two dots and `part`.  What happens to g is
// written as it is there, in the same order, so gu has the same bits.
template <typename TG, typename TO, typename TE = void>
__global__ __launch_bounds__(256) void explicit5_bwd_input_kernel(const TG* __restrict__ g, const float* __restrict__ alpha,
                                                                  const float* __restrict__ scale, TO* __restrict__ gu,
                                                                  int C, int H, int W, float dt, float eps, float maxc,
                                                                  float relax, typename EmitPtr<const TE>::type ginj) {
    const int pc = blockIdx.x;
    const int c = pc % C;
    const float a = fminf(fmaxf(alpha[c], eps), maxc) * dt;
    const float s = scale[c];
    const TG* gp = g + (size_t)pc * H * W;
    TO* op = gu + (size_t)pc * H * W;
    const int W4 = W / 4;
    for (int f = threadIdx.x; f < H * W4; f += 256) {
        const int h = f / W4, w0 = 4 * (f % W4);
        const float4 cg = V4<TG>::ld(gp + (size_t)h * W + w0);
        const float4 lg = lap0_4<TG>(gp, H, W, h, w0, cg);
        float4 o;
        o.x = (1.f - relax) * cg.x + relax * s * (cg.x + a * lg.x);
        o.y = (1.f - relax) * cg.y + relax * s * (cg.y + a * lg.y);
        o.z = (1.f - relax) * cg.z + relax * s * (cg.z + a * lg.z);
        o.w = (1.f - relax) * cg.w + relax * s * (cg.w + a * lg.w);
        if constexpr (!std::is_void<TE>::value) {
            const float4 gi = V4<TE>::ld_once(ginj + (size_t)pc * H * W + (size_t)h * W + w0);
            o.x += gi.x; o.y += gi.y; o.z += gi.z; o.w += gi.w;
        }
        V4<TO>::st(op + (size_t)h * W + w0, o);
    }
}

template <typename TG, typename TO, typename TE = void>
__global__ __launch_bounds__(256) void explicit5_bwd_input_col_kernel(const TG* __restrict__ g, const float* __restrict__ alpha,
                                                                      const float* __restrict__ scale, TO* __restrict__ gu,
                                                                      int C, int H, int W, float dt, float eps, float maxc,
                                                                      float relax, typename EmitPtr<const TE>::type ginj) {
    const int pc = blockIdx.x;
    const int c = pc % C;
    const float a = fminf(fmaxf(alpha[c], eps), maxc) * dt;
    const float s = scale[c];
    const TG* gp = g + (size_t)pc * H * W;
    TO* op = gu + (size_t)pc * H * W;
    for (int f = threadIdx.x; f < H * W; f += 256) {
        const int h = f / W, w = f % W;
        const float cg = S1<TG>::ld(gp + f);
        const float lg = lap0_1<TG>(gp, H, W, h, w, cg);
        float o = (1.f - relax) * cg + relax * s * (cg + a * lg);
        if constexpr (!std::is_void<TE>::value) o += S1<TE>::ld(ginj + (size_t)pc * H * W + f);
        S1<TO>::st(op + f, o);
    }
}

// one workgroup per channel: 256 threads add the per-plane partial sums of their samples, then a
// fixed-order block reduction (a single 64-thread block looping over all samples took 84 us at B=256)
__global__ __launch_bounds__(256) void explicit5_pgrad_kernel(const float* __restrict__ part,
                                                              const float* __restrict__ alpha,
                                                              const float* __restrict__ scale,
                                                              float* __restrict__ ga, float* __restrict__ gs, int B,
                                                              int C, float dt, float eps, float maxc, float relax) {
    __shared__ float sh[4];
    const int c = blockIdx.x;
    float s1 = 0.f, s2 = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        s1 += part[2 * ((size_t)b * C + c)];
        s2 += part[2 * ((size_t)b * C + c) + 1];
    }
    s1 = block_sum_256(s1, sh);
    s2 = block_sum_256(s2, sh);
    if (threadIdx.x == 0) {
        const float ab = alpha[c];
        const float a = fminf(fmaxf(ab, eps), maxc) * dt;
        gs[c] = relax * (s1 + a * s2);
        ga[c] = (ab >= eps && ab <= maxc) ? relax * dt * scale[c] * s2 : 0.f;
    }
}


// ---------------------------------------------------------------------------------------
// wave-per-plane kernels: the plane lives in registers for the whole call
// ---------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp_shift(float v) {     // 0 is shifted in at the ends of the wave
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
constexpr int kWaveShl1 = 0x130;    // lane i <- lane i+1
constexpr int kWaveShr1 = 0x138;    // lane i <- lane i-1
__device__ __forceinline__ float4 shfl_up4(float4 v, int d) {
    return make_float4(__shfl_up(v.x, d, 64), __shfl_up(v.y, d, 64), __shfl_up(v.z, d, 64), __shfl_up(v.w, d, 64));
}
__device__ __forceinline__ float4 shfl_down4(float4 v, int d) {
    return make_float4(__shfl_down(v.x, d, 64), __shfl_down(v.y, d, 64), __shfl_down(v.z, d, 64), __shfl_down(v.w, d, 64));
}

// Lap0 of the lane's R rows (zero ghost cells): same operation order as lap0_4
template <int R, int W4>
__device__ __forceinline__ void lap0_rows(const float4 (&c)[R], float4 (&lp)[R], int cg, int rg) {
    constexpr int RG = 64 / W4;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 top = shfl_up4(c[R - 1], W4), bot = shfl_down4(c[0], W4);
    if (rg == 0) top = z;
    if (rg == RG - 1) bot = z;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const float4 n = (i > 0) ? c[i - 1] : top;
        const float4 s = (i < R - 1) ? c[i + 1] : bot;
        float l = dpp_shift<kWaveShr1>(c[i].w), r = dpp_shift<kWaveShl1>(c[i].x);
        if (cg == 0) l = 0.f;
        if (cg == W4 - 1) r = 0.f;
        lp[i].x = n.x + s.x + l + c[i].y - 4.f * c[i].x;
        lp[i].y = n.y + s.y + c[i].x + c[i].z - 4.f * c[i].y;
        lp[i].z = n.z + s.z + c[i].y + c[i].w - 4.f * c[i].z;
        lp[i].w = n.w + s.w + c[i].z + r - 4.f * c[i].w;
    }
}

// EMIT: the state after every step of `em` also goes to traj[slot] in the tensors' type (pde_explicit5_forward_states)
template <typename IO, int R, int W4, bool EMIT = false>
__global__ __launch_bounds__(256) void explicit5_fwd_wave(const IO* __restrict__ u, const float* __restrict__ alpha,
                                                          const float* __restrict__ scale, IO* __restrict__ out,
                                                          float* __restrict__ states, int nplanes, int C, int num_steps,
                                                          float dt, float eps, float maxc, float relax,
                                                          IO* __restrict__ traj, EmitMask em) {
    constexpr int W = 4 * W4, H = R * (64 / W4);
    const int lane = threadIdx.x & 63;
    const int pc = blockIdx.x * 4 + (threadIdx.x >> 6);          // one wave per plane
    if (pc >= nplanes) return;
    const int c = pc % C;
    const float a = fminf(fmaxf(alpha[c], eps), maxc) * dt;
    const float s = scale[c];
    const int cg = lane % W4, rg = lane / W4;
    const size_t off = (size_t)pc * H * W + (size_t)(rg * R) * W + 4 * cg;
    float4 cur[R], lp[R];
#pragma unroll
    for (int i = 0; i < R; ++i) cur[i] = V4<IO>::ld_once(u + off + (size_t)i * W);
    for (int step = 0; step < num_steps; ++step) {
        lap0_rows<R, W4>(cur, lp, cg, rg);
#pragma unroll
        for (int i = 0; i < R; ++i) {
            // v = s u; new = v + a*(s*lap); out = u + relax*(new - u)      tiny_imagenet.py:43-49
            { const float v = s * cur[i].x; const float nw = v + a * (s * lp[i].x); cur[i].x = cur[i].x + relax * (nw - cur[i].x); }
            { const float v = s * cur[i].y; const float nw = v + a * (s * lp[i].y); cur[i].y = cur[i].y + relax * (nw - cur[i].y); }
            { const float v = s * cur[i].z; const float nw = v + a * (s * lp[i].z); cur[i].z = cur[i].z + relax * (nw - cur[i].z); }
            { const float v = s * cur[i].w; const float nw = v + a * (s * lp[i].w); cur[i].w = cur[i].w + relax * (nw - cur[i].w); }
        }
        // inputs of the later steps, for the backward: kept in fp32 whatever the tensors' type (with bf16 states the
        // alpha-gradient — a sum over the whole batch that cancels to a few units — was a quarter off on a drawn case)
        if (step + 1 < num_steps && states != nullptr) {
            float* sp = states + (size_t)step * nplanes * H * W;
#pragma unroll
            for (int i = 0; i < R; ++i) V4<float>::st(sp + off + (size_t)i * W, cur[i]);
        }
        if constexpr (EMIT) {
            const int slot = emit_slot(em, step + 1);
            if (slot >= 0) {
                IO* tp = traj + (size_t)slot * nplanes * H * W;
#pragma unroll
                for (int i = 0; i < R; ++i) V4<IO>::st(tp + off + (size_t)i * W, cur[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) V4<IO>::st(out + off + (size_t)i * W, cur[i]);
}

__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// backward of num_steps steps: g walks back through the steps in registers; u_{k-1} (the input of step k) is the
// layer input for k = 1 and states[k-2] otherwise
// EMIT: once g is the adjoint of an emitted state it gets += gtraj[slot] (pde_explicit5_backward_states)
template <typename IO, int R, int W4, bool EMIT = false>
__global__ __launch_bounds__(256) void explicit5_bwd_wave(const IO* __restrict__ u, const float* __restrict__ states,
                                                          const IO* __restrict__ g, const float* __restrict__ alpha,
                                                          const float* __restrict__ scale, IO* __restrict__ gu,
                                                          float* __restrict__ part, int nplanes, int C, int num_steps,
                                                          float dt, float eps, float maxc, float relax,
                                                          const IO* __restrict__ gtraj, EmitMask em) {
    constexpr int W = 4 * W4, H = R * (64 / W4);
    const int lane = threadIdx.x & 63;
    const int pc = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pc >= nplanes) return;
    const int c = pc % C;
    const float a = fminf(fmaxf(alpha[c], eps), maxc) * dt;
    const float s = scale[c];
    const int cg = lane % W4, rg = lane / W4;
    const size_t off = (size_t)pc * H * W + (size_t)(rg * R) * W + 4 * cg;
    float4 cg4[R], lg[R];
#pragma unroll
    for (int i = 0; i < R; ++i) cg4[i] = V4<IO>::ld_once(g + off + (size_t)i * W);
    float p1 = 0.f, p2 = 0.f;                                     // sum g*u, sum Lap0(g)*u over all steps
    for (int step = num_steps; step >= 1; --step) {
        const float* sp = states + (size_t)(step >= 2 ? step - 2 : 0) * nplanes * H * W;
        lap0_rows<R, W4>(cg4, lg, cg, rg);
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const float4 cu = (step == 1) ? V4<IO>::ld_once(u + off + (size_t)i * W) : V4<float>::ld_once(sp + off + (size_t)i * W);
            p1 += cg4[i].x * cu.x + cg4[i].y * cu.y + cg4[i].z * cu.z + cg4[i].w * cu.w;
            p2 += lg[i].x * cu.x + lg[i].y * cu.y + lg[i].z * cu.z + lg[i].w * cu.w;
            cg4[i].x = (1.f - relax) * cg4[i].x + relax * s * (cg4[i].x + a * lg[i].x);
            cg4[i].y = (1.f - relax) * cg4[i].y + relax * s * (cg4[i].y + a * lg[i].y);
            cg4[i].z = (1.f - relax) * cg4[i].z + relax * s * (cg4[i].z + a * lg[i].z);
            cg4[i].w = (1.f - relax) * cg4[i].w + relax * s * (cg4[i].w + a * lg[i].w);
        }
        if constexpr (EMIT) {                                     // g is now the adjoint of the state after step - 1
            const int slot = emit_slot(em, step - 1);
            if (slot >= 0) {
                const IO* tp = gtraj + (size_t)slot * nplanes * H * W;
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const float4 gi = V4<IO>::ld_once(tp + off + (size_t)i * W);
                    cg4[i].x += gi.x; cg4[i].y += gi.y; cg4[i].z += gi.z; cg4[i].w += gi.w;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) V4<IO>::st(gu + off + (size_t)i * W, cg4[i]);
    p1 = wave_sum(p1);
    p2 = wave_sum(p2);
    if (lane == 0) { part[2 * (size_t)pc] = p1; part[2 * (size_t)pc + 1] = p2; }
}

// The same reverse walk for the input alone (alpha_base and channel_scaling take no gradient): explicit5_bwd_wave without
// the u / states loads, the two dots, the wave sums and `part`; per step g goes through the operations it goes through
// there, in their order, so gu has the same bits.  Same grid and lane map.
template <typename IO, int R, int W4, bool EMIT = false>
__global__ __launch_bounds__(256) void explicit5_bwd_input_wave(const IO* __restrict__ g, const float* __restrict__ alpha,
                                                                const float* __restrict__ scale, IO* __restrict__ gu,
                                                                int nplanes, int C, int num_steps, float dt, float eps,
                                                                float maxc, float relax, const IO* __restrict__ gtraj,
                                                                EmitMask em) {
    constexpr int W = 4 * W4, H = R * (64 / W4);
    const int lane = threadIdx.x & 63;
    const int pc = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pc >= nplanes) return;
    const int c = pc % C;
    const float a = fminf(fmaxf(alpha[c], eps), maxc) * dt;
    const float s = scale[c];
    const int cg = lane % W4, rg = lane / W4;
    const size_t off = (size_t)pc * H * W + (size_t)(rg * R) * W + 4 * cg;
    float4 cg4[R], lg[R];
#pragma unroll
    for (int i = 0; i < R; ++i) cg4[i] = V4<IO>::ld_once(g + off + (size_t)i * W);
    for (int step = num_steps; step >= 1; --step) {
        lap0_rows<R, W4>(cg4, lg, cg, rg);
#pragma unroll
        for (int i = 0; i < R; ++i) {
            cg4[i].x = (1.f - relax) * cg4[i].x + relax * s * (cg4[i].x + a * lg[i].x);
            cg4[i].y = (1.f - relax) * cg4[i].y + relax * s * (cg4[i].y + a * lg[i].y);
            cg4[i].z = (1.f - relax) * cg4[i].z + relax * s * (cg4[i].z + a * lg[i].z);
            cg4[i].w = (1.f - relax) * cg4[i].w + relax * s * (cg4[i].w + a * lg[i].w);
        }
        if constexpr (EMIT) {                                     // g is now the adjoint of the state after step - 1
            const int slot = emit_slot(em, step - 1);
            if (slot >= 0) {
                const IO* tp = gtraj + (size_t)slot * nplanes * H * W;
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const float4 gi = V4<IO>::ld_once(tp + off + (size_t)i * W);
                    cg4[i].x += gi.x; cg4[i].y += gi.y; cg4[i].z += gi.z; cg4[i].w += gi.w;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) V4<IO>::st(gu + off + (size_t)i * W, cg4[i]);
}

// which plane sizes the wave-per-plane kernels cover
bool wave_plane_ok(int H, int W) { return (H == 64 && W == 64) || (H == 32 && W == 32) || (H == 16 && W == 16); }

template <typename IO, bool EMIT>
void launch_fwd_wave(int H, const IO* u, const float* alpha, const float* scale, IO* out, float* states, int nplanes, int C,
                     int num_steps, float dt, float eps, float maxc, float relax, IO* traj, EmitMask em, hipStream_t st) {
    const dim3 grid((nplanes + 3) / 4), block(256);
    if (H == 64) hipLaunchKernelGGL((explicit5_fwd_wave<IO, 16, 16, EMIT>), grid, block, 0, st, u, alpha, scale, out, states, nplanes, C, num_steps, dt, eps, maxc, relax, traj, em);
    else if (H == 32) hipLaunchKernelGGL((explicit5_fwd_wave<IO, 4, 8, EMIT>), grid, block, 0, st, u, alpha, scale, out, states, nplanes, C, num_steps, dt, eps, maxc, relax, traj, em);
    else hipLaunchKernelGGL((explicit5_fwd_wave<IO, 1, 4, EMIT>), grid, block, 0, st, u, alpha, scale, out, states, nplanes, C, num_steps, dt, eps, maxc, relax, traj, em);
}
template <typename IO, bool EMIT>
void launch_bwd_wave(int H, const IO* u, const float* states, const IO* g, const float* alpha, const float* scale, IO* gu,
                     float* part, int nplanes, int C, int num_steps, float dt, float eps, float maxc, float relax,
                     const IO* gtraj, EmitMask em, hipStream_t st) {
    const dim3 grid((nplanes + 3) / 4), block(256);
    if (H == 64) hipLaunchKernelGGL((explicit5_bwd_wave<IO, 16, 16, EMIT>), grid, block, 0, st, u, states, g, alpha, scale, gu, part, nplanes, C, num_steps, dt, eps, maxc, relax, gtraj, em);
    else if (H == 32) hipLaunchKernelGGL((explicit5_bwd_wave<IO, 4, 8, EMIT>), grid, block, 0, st, u, states, g, alpha, scale, gu, part, nplanes, C, num_steps, dt, eps, maxc, relax, gtraj, em);
    else hipLaunchKernelGGL((explicit5_bwd_wave<IO, 1, 4, EMIT>), grid, block, 0, st, u, states, g, alpha, scale, gu, part, nplanes, C, num_steps, dt, eps, maxc, relax, gtraj, em);
}
// the wave-per-plane call of one tensor type: the plain instantiations for an empty mask
template <typename IO>
void fwd_wave_io(int H, const void* u, const float* alpha, const float* scale, void* out, float* states, int nplanes, int C,
                 int num_steps, float dt, float eps, float maxc, float relax, void* traj, EmitMask em, hipStream_t st) {
    if (em.any()) launch_fwd_wave<IO, true>(H, (const IO*)u, alpha, scale, (IO*)out, states, nplanes, C, num_steps, dt, eps, maxc, relax, (IO*)traj, em, st);
    else launch_fwd_wave<IO, false>(H, (const IO*)u, alpha, scale, (IO*)out, states, nplanes, C, num_steps, dt, eps, maxc, relax, (IO*)nullptr, em, st);
}
template <typename IO>
void bwd_wave_io(int H, const void* u, const float* states, const void* g, const float* alpha, const float* scale, void* gu,
                 float* part, int nplanes, int C, int num_steps, float dt, float eps, float maxc, float relax,
                 const void* gtraj, EmitMask em, hipStream_t st) {
    if (em.any()) launch_bwd_wave<IO, true>(H, (const IO*)u, states, (const IO*)g, alpha, scale, (IO*)gu, part, nplanes, C, num_steps, dt, eps, maxc, relax, (const IO*)gtraj, em, st);
    else launch_bwd_wave<IO, false>(H, (const IO*)u, states, (const IO*)g, alpha, scale, (IO*)gu, part, nplanes, C, num_steps, dt, eps, maxc, relax, (const IO*)nullptr, em, st);
}

template <typename IO, bool EMIT>
void launch_bwd_input_wave(int H, const IO* g, const float* alpha, const float* scale, IO* gu, int nplanes, int C,
                           int num_steps, float dt, float eps, float maxc, float relax, const IO* gtraj, EmitMask em,
                           hipStream_t st) {
    const dim3 grid((nplanes + 3) / 4), block(256);
    if (H == 64) hipLaunchKernelGGL((explicit5_bwd_input_wave<IO, 16, 16, EMIT>), grid, block, 0, st, g, alpha, scale, gu, nplanes, C, num_steps, dt, eps, maxc, relax, gtraj, em);
    else if (H == 32) hipLaunchKernelGGL((explicit5_bwd_input_wave<IO, 4, 8, EMIT>), grid, block, 0, st, g, alpha, scale, gu, nplanes, C, num_steps, dt, eps, maxc, relax, gtraj, em);
    else hipLaunchKernelGGL((explicit5_bwd_input_wave<IO, 1, 4, EMIT>), grid, block, 0, st, g, alpha, scale, gu, nplanes, C, num_steps, dt, eps, maxc, relax, gtraj, em);
}
template <typename IO>
void bwd_input_wave_io(int H, const void* g, const float* alpha, const float* scale, void* gu, int nplanes, int C,
                       int num_steps, float dt, float eps, float maxc, float relax, const void* gtraj, EmitMask em,
                       hipStream_t st) {
    if (em.any()) launch_bwd_input_wave<IO, true>(H, (const IO*)g, alpha, scale, (IO*)gu, nplanes, C, num_steps, dt, eps, maxc, relax, (const IO*)gtraj, em, st);
    else launch_bwd_input_wave<IO, false>(H, (const IO*)g, alpha, scale, (IO*)gu, nplanes, C, num_steps, dt, eps, maxc, relax, (const IO*)nullptr, em, st);
}

// ---------------------------------------------------------------------------------------
// tangent-linear pass (pdecnn_explicit_tangent.h: pde_explicit5_tangent): the primal state u and the tangent state du
// advance together.  Per step, with a = clamp(alpha_c)*dt, s = scale_c, L = Lap0:
//     u'  = u + relax*((s u + a*(s*L u)) - u)                     the forward kernels' expressions, in their order
//     du' = the same expressions on du, then + relax*(ds*(u + a*L u) + da*(s*L u)),   u the step's input
//     da  = [eps <= alpha_c <= max_coeff] * dalpha_c * dt          (the mask of explicit5_pgrad_kernel: equality passes)
// With both parameter tangents NULL the source is not added at all (src == 0), so dy is bit for bit the forward at du.
// ---------------------------------------------------------------------------------------
struct ExTan {          // one channel's coefficients and their tangents
    float a, s, da, ds;
};
__device__ __forceinline__ ExTan ex_tan_coeffs(const float* alpha, const float* scale, const float* d_alpha,
                                               const float* d_scale, int c, float dt, float eps, float maxc) {
    ExTan t;
    const float ab = alpha[c];
    t.a = fminf(fmaxf(ab, eps), maxc) * dt;
    t.s = scale[c];
    t.da = (d_alpha && ab >= eps && ab <= maxc) ? d_alpha[c] * dt : 0.f;
    t.ds = d_scale ? d_scale[c] : 0.f;
    return t;
}
// One step of one state element, x -> x + relax*((s x + a*(s*L x)) - x), with the forward's roundings.  The forward writes
// `v + a * (s * lp)` and leaves the contraction to the compiler, which fuses one of the two products into the sum: s*x in
// every instantiation of the forward kernels but the 16x16 wave kernel (R = 1), where it fuses a*(s*L x).  Here s*L u is
// used twice and the choice would fall differently, so contraction is off and the forward's fused operations are spelled
// out (AFMA: the 16x16 form); the identity tests of tests/test_gpu_tangent_explicit.py hold the two to the same bits.
template <bool AFMA>
__device__ __forceinline__ float ex_step_elem(float a, float s, float relax, float x, float slx) {
#pragma clang fp contract(off)
    const float nw = AFMA ? __builtin_fmaf(a, slx, s * x) : __builtin_fmaf(s, x, a * slx);
    return __builtin_fmaf(relax, nw - x, x);
}
// one element: (u, L u, du, L du) -> (u', du')
template <bool AFMA>
__device__ __forceinline__ void ex_tan_elem(const ExTan& t, float relax, int src, float cu, float lp, float dcu, float dlp,
                                            float& o, float& od) {
#pragma clang fp contract(off)
    const float slp = t.s * lp;
    o = ex_step_elem<AFMA>(t.a, t.s, relax, cu, slp);
    od = ex_step_elem<AFMA>(t.a, t.s, relax, dcu, t.s * dlp);
    if (src) od = __builtin_fmaf(relax, __builtin_fmaf(t.ds, __builtin_fmaf(t.a, lp, cu), t.da * slp), od);
}
template <bool AFMA>
__device__ __forceinline__ void ex_tan_elem4(const ExTan& t, float relax, int src, const float4& cu, const float4& lp,
                                             const float4& dcu, const float4& dlp, float4& o, float4& od) {
    ex_tan_elem<AFMA>(t, relax, src, cu.x, lp.x, dcu.x, dlp.x, o.x, od.x);
    ex_tan_elem<AFMA>(t, relax, src, cu.y, lp.y, dcu.y, dlp.y, o.y, od.y);
    ex_tan_elem<AFMA>(t, relax, src, cu.z, lp.z, dcu.z, dlp.z, o.z, od.z);
    ex_tan_elem<AFMA>(t, relax, src, cu.w, lp.w, dcu.w, dlp.w, o.w, od.w);
}

// explicit5_fwd_kernel with a second state.  du NULL (first step only): a zero tangent; out NULL (last step only): y is
// not wanted.  TI / TO as there: the call's type at its first load and last store, fp32 between the steps.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void explicit5_tangent_kernel(const TI* __restrict__ u, const TI* __restrict__ du,
                                                                const float* __restrict__ alpha, const float* __restrict__ scale,
                                                                const float* __restrict__ d_alpha,
                                                                const float* __restrict__ d_scale, TO* __restrict__ out,
                                                                TO* __restrict__ dout, int C, int H, int W, float dt,
                                                                float eps, float maxc, float relax, int src) {
    const int pc = blockIdx.x;                         // plane index b*C + c
    const ExTan t = ex_tan_coeffs(alpha, scale, d_alpha, d_scale, pc % C, dt, eps, maxc);
    const size_t po = (size_t)pc * H * W;
    const TI* plane = u + po;
    const TI* dplane = du ? du + po : nullptr;
    const int W4 = W / 4;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int f = threadIdx.x; f < H * W4; f += 256) {
        const int h = f / W4, w0 = 4 * (f % W4);
        const size_t e = (size_t)h * W + w0;
        const float4 cu = V4<TI>::ld(plane + e);
        const float4 lp = lap0_4<TI>(plane, H, W, h, w0, cu);
        const float4 dcu = dplane ? V4<TI>::ld(dplane + e) : z;
        const float4 dlp = dplane ? lap0_4<TI>(dplane, H, W, h, w0, dcu) : z;
        float4 o, od;
        ex_tan_elem4<false>(t, relax, src, cu, lp, dcu, dlp, o, od);
        if (out) V4<TO>::st(out + po + e, o);
        V4<TO>::st(dout + po + e, od);
    }
}

// explicit5_fwd_col_kernel with a second state (widths that are not a multiple of 4)
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void explicit5_tangent_col_kernel(const TI* __restrict__ u, const TI* __restrict__ du,
                                                                    const float* __restrict__ alpha,
                                                                    const float* __restrict__ scale,
                                                                    const float* __restrict__ d_alpha,
                                                                    const float* __restrict__ d_scale, TO* __restrict__ out,
                                                                    TO* __restrict__ dout, int C, int H, int W, float dt,
                                                                    float eps, float maxc, float relax, int src) {
    const int pc = blockIdx.x;
    const ExTan t = ex_tan_coeffs(alpha, scale, d_alpha, d_scale, pc % C, dt, eps, maxc);
    const size_t po = (size_t)pc * H * W;
    const TI* plane = u + po;
    const TI* dplane = du ? du + po : nullptr;
    for (int f = threadIdx.x; f < H * W; f += 256) {
        const int h = f / W, w = f % W;
        const float cu = S1<TI>::ld(plane + f);
        const float lp = lap0_1<TI>(plane, H, W, h, w, cu);
        const float dcu = dplane ? S1<TI>::ld(dplane + f) : 0.f;
        const float dlp = dplane ? lap0_1<TI>(dplane, H, W, h, w, dcu) : 0.f;
        float o, od;
        ex_tan_elem<false>(t, relax, src, cu, lp, dcu, dlp, o, od);
        if (out) S1<TO>::st(out + po + f, o);
        S1<TO>::st(dout + po + f, od);
    }
}

// Lap0 of one of the lane's rows from the row above, itself and the row below: lap0_rows' operations, in its order
template <int W4>
__device__ __forceinline__ float4 lap0_row(const float4& n, const float4& c, const float4& s, int cg) {
    float l = dpp_shift<kWaveShr1>(c.w), r = dpp_shift<kWaveShl1>(c.x);
    if (cg == 0) l = 0.f;
    if (cg == W4 - 1) r = 0.f;
    float4 lp;
    lp.x = n.x + s.x + l + c.y - 4.f * c.x;
    lp.y = n.y + s.y + c.x + c.z - 4.f * c.y;
    lp.z = n.z + s.z + c.y + c.w - 4.f * c.z;
    lp.w = n.w + s.w + c.z + r - 4.f * c.w;
    return lp;
}

// explicit5_fwd_wave with a second state: both planes in registers over all steps, one launch.  The two Laplacians are
// formed row by row (the halo rows are fetched before the first row changes, the old row above is carried along), so a
// 64x64 plane holds cur and dcur (128 registers) and two rows of Laplacians, not four plane-sized arrays: no scratch.
template <typename IO, int R, int W4>
__global__ __launch_bounds__(256) void explicit5_tangent_wave(const IO* __restrict__ u, const IO* __restrict__ du,
                                                              const float* __restrict__ alpha, const float* __restrict__ scale,
                                                              const float* __restrict__ d_alpha,
                                                              const float* __restrict__ d_scale, IO* __restrict__ out,
                                                              IO* __restrict__ dout, int nplanes, int C, int num_steps,
                                                              float dt, float eps, float maxc, float relax, int src) {
    constexpr int W = 4 * W4, H = R * (64 / W4), RG = 64 / W4;
    const int lane = threadIdx.x & 63;
    const int pc = blockIdx.x * 4 + (threadIdx.x >> 6);          // one wave per plane
    if (pc >= nplanes) return;
    const ExTan t = ex_tan_coeffs(alpha, scale, d_alpha, d_scale, pc % C, dt, eps, maxc);
    const int cg = lane % W4, rg = lane / W4;
    const size_t off = (size_t)pc * H * W + (size_t)(rg * R) * W + 4 * cg;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 cur[R], dcur[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        cur[i] = V4<IO>::ld_once(u + off + (size_t)i * W);
        dcur[i] = du ? V4<IO>::ld_once(du + off + (size_t)i * W) : z;
    }
    for (int step = 0; step < num_steps; ++step) {
        float4 top = shfl_up4(cur[R - 1], W4), bot = shfl_down4(cur[0], W4);
        float4 dtop = shfl_up4(dcur[R - 1], W4), dbot = shfl_down4(dcur[0], W4);
        if (rg == 0) { top = z; dtop = z; }
        if (rg == RG - 1) { bot = z; dbot = z; }
        float4 pn = top, dpn = dtop;                              // the row above, as it was before this step
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const float4 c = cur[i], dc = dcur[i];
            const float4 lp = lap0_row<W4>(pn, c, (i < R - 1) ? cur[i + 1] : bot, cg);
            const float4 dlp = lap0_row<W4>(dpn, dc, (i < R - 1) ? dcur[i + 1] : dbot, cg);
            ex_tan_elem4<R == 1>(t, relax, src, c, lp, dc, dlp, cur[i], dcur[i]);
            pn = c;
            dpn = dc;
        }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
        if (out) V4<IO>::st(out + off + (size_t)i * W, cur[i]);
        V4<IO>::st(dout + off + (size_t)i * W, dcur[i]);
    }
}

template <typename IO>
void tangent_wave_io(int H, const void* u, const void* du, const float* alpha, const float* scale, const float* d_alpha,
                     const float* d_scale, void* out, void* dout, int nplanes, int C, int num_steps, float dt, float eps,
                     float maxc, float relax, int src, hipStream_t st) {
    const dim3 grid((nplanes + 3) / 4), block(256);
    if (H == 64) hipLaunchKernelGGL((explicit5_tangent_wave<IO, 16, 16>), grid, block, 0, st, (const IO*)u, (const IO*)du, alpha, scale, d_alpha, d_scale, (IO*)out, (IO*)dout, nplanes, C, num_steps, dt, eps, maxc, relax, src);
    else if (H == 32) hipLaunchKernelGGL((explicit5_tangent_wave<IO, 4, 8>), grid, block, 0, st, (const IO*)u, (const IO*)du, alpha, scale, d_alpha, d_scale, (IO*)out, (IO*)dout, nplanes, C, num_steps, dt, eps, maxc, relax, src);
    else hipLaunchKernelGGL((explicit5_tangent_wave<IO, 1, 4>), grid, block, 0, st, (const IO*)u, (const IO*)du, alpha, scale, d_alpha, d_scale, (IO*)out, (IO*)dout, nplanes, C, num_steps, dt, eps, maxc, relax, src);
}

// ---------------------------------------------------------------------------------------
// jacobi (emotion_recognition.PDELayer)
// ---------------------------------------------------------------------------------------
constexpr int kJMax = 64;                  // max H, W
constexpr int kJP = kJMax + 2;

__device__ __forceinline__ int reflect_src(int m, int n) {   // padded index m in [0,n+1] -> source index in [0,n)
    return m == 0 ? 1 : (m == n + 1 ? n - 2 : m - 1);
}

// one explicit update P -> Q of the interior; ring copied
__device__ __forceinline__ void jacobi_step(const float* P, float* Q, const float* a, const float* b, int H, int W) {
    const int Wp = W + 2;
    for (int e = threadIdx.x; e < (H + 2) * Wp; e += blockDim.x) {
        const int i = e / Wp, j = e % Wp;
        float v = P[e];
        if (i >= 1 && i <= H && j >= 1 && j <= W) {
            const float d1 = P[e + Wp] - 2.f * v + P[e - Wp];
            const float d2 = P[e + 1] - 2.f * v + P[e - 1];
            v = v + a[i - 1] * d1 + b[j - 1] * d2;
        }
        Q[e] = v;
    }
}

// EMIT: the interior of the state after every step of `em` also goes to traj[slot][B][H][W] (pde_jacobi_io_forward_states)
template <typename IO, bool EMIT = false>
__global__ __launch_bounds__(256) void jacobi_fwd_kernel(const IO* __restrict__ u, const float* __restrict__ a_row,
                                                         const float* __restrict__ b_col, IO* __restrict__ out,
                                                         int H, int W, int nt, IO* __restrict__ traj, EmitMask em) {
    extern __shared__ float sm[];
    const int Wp = W + 2, PN = (H + 2) * Wp;
    float* P = sm;
    float* Q = sm + PN;
    float* a = sm + 2 * PN;
    float* b = a + H;
    const IO* ub = u + (size_t)blockIdx.x * H * W;
    for (int e = threadIdx.x; e < H; e += blockDim.x) a[e] = a_row[e];
    for (int e = threadIdx.x; e < W; e += blockDim.x) b[e] = b_col[e];
    for (int e = threadIdx.x; e < PN; e += blockDim.x) {
        const int i = e / Wp, j = e % Wp;
        P[e] = S1<IO>::ld(ub + reflect_src(i, H) * W + reflect_src(j, W));          // F.pad(..., mode='reflect')
    }
    __syncthreads();
    for (int n = 0; n < nt; ++n) {
        jacobi_step(P, Q, a, b, H, W);
        __syncthreads();
        float* t = P; P = Q; Q = t;
        if constexpr (EMIT) {
            const int slot = emit_slot(em, n + 1);
            if (slot >= 0) {
                IO* tb = traj + ((size_t)slot * gridDim.x + blockIdx.x) * H * W;
                for (int e = threadIdx.x; e < H * W; e += blockDim.x) S1<IO>::st(tb + e, P[(e / W + 1) * Wp + (e % W) + 1]);
            }
        }
    }
    IO* ob = out + (size_t)blockIdx.x * H * W;
    for (int e = threadIdx.x; e < H * W; e += blockDim.x) S1<IO>::st(ob + e, P[(e / W + 1) * Wp + (e % W) + 1]);
}

// workspace per sample: nt states of PN floats, then H+W partial sums
// EMIT: once G is the adjoint of an emitted state its interior gets += gtraj[slot] (pde_jacobi_io_backward_states)
template <typename IO, bool EMIT = false>
__global__ __launch_bounds__(256) void jacobi_bwd_kernel(const IO* __restrict__ u, const IO* __restrict__ gout,
                                                         const float* __restrict__ a_row,
                                                         const float* __restrict__ b_col, IO* __restrict__ gu,
                                                         float* __restrict__ states, float* __restrict__ part,
                                                         int H, int W, int nt, const IO* __restrict__ gtraj, EmitMask em) {
    extern __shared__ float sm[];
    const int Wp = W + 2, PN = (H + 2) * Wp;
    float* P = sm;
    float* Q = sm + PN;
    float* a = sm + 2 * PN;
    float* b = a + H;
    float* ga = b + W;
    float* gb = ga + H;
    const int s = blockIdx.x;
    const IO* ub = u + (size_t)s * H * W;
    float* st = states + (size_t)s * nt * PN;
    for (int e = threadIdx.x; e < H; e += blockDim.x) { a[e] = a_row[e]; ga[e] = 0.f; }
    for (int e = threadIdx.x; e < W; e += blockDim.x) { b[e] = b_col[e]; gb[e] = 0.f; }
    for (int e = threadIdx.x; e < PN; e += blockDim.x) {
        const int i = e / Wp, j = e % Wp;
        P[e] = S1<IO>::ld(ub + reflect_src(i, H) * W + reflect_src(j, W));
    }
    __syncthreads();
    // forward recompute: park the state BEFORE each step
    for (int n = 0; n < nt; ++n) {
        for (int e = threadIdx.x; e < PN; e += blockDim.x) st[(size_t)n * PN + e] = P[e];
        jacobi_step(P, Q, a, b, H, W);
        __syncthreads();
        float* t = P; P = Q; Q = t;
    }
    // adjoint: G = dL/dP_nt (zero ring, gout inside)
    float* G = P;
    float* Gn = Q;
    const IO* gob = gout + (size_t)s * H * W;
    for (int e = threadIdx.x; e < PN; e += blockDim.x) {
        const int i = e / Wp, j = e % Wp;
        G[e] = (i >= 1 && i <= H && j >= 1 && j <= W) ? S1<IO>::ld(gob + (i - 1) * W + (j - 1)) : 0.f;
    }
    __threadfence_block();
    __syncthreads();
    for (int n = nt - 1; n >= 0; --n) {
        const float* Pn = st + (size_t)n * PN;                 // state before step n (this block wrote it)
        // coefficient gradients: dA_i += sum_j G[i,j] d1(Pn)[i,j];  dB_j += sum_i G[i,j] d2(Pn)[i,j]
        for (int r = threadIdx.x; r < H + W; r += blockDim.x) {
            float acc = 0.f;
            if (r < H) {
                const int i = r + 1;
                for (int j = 1; j <= W; ++j) {
                    const int e = i * Wp + j;
                    acc += G[e] * (Pn[e + Wp] - 2.f * Pn[e] + Pn[e - Wp]);
                }
                ga[r] += acc;
            } else {
                const int j = r - H + 1;
                for (int i = 1; i <= H; ++i) {
                    const int e = i * Wp + j;
                    acc += G[e] * (Pn[e + 1] - 2.f * Pn[e] + Pn[e - 1]);
                }
                gb[r - H] += acc;
            }
        }
        // dL/dP_n from dL/dP_{n+1}
        const IO* gt = nullptr;                                // dL/d(state after step n), where that state was emitted
        if constexpr (EMIT) {
            const int slot = emit_slot(em, n);
            if (slot >= 0) gt = gtraj + ((size_t)slot * gridDim.x + s) * H * W;
        }
        for (int e = threadIdx.x; e < PN; e += blockDim.x) {
            const int i = e / Wp, j = e % Wp;
            const bool in = (i >= 1 && i <= H && j >= 1 && j <= W);
            float v = in ? (1.f - 2.f * a[i - 1] - 2.f * b[j - 1]) * G[e] : G[e];
            if (j >= 1 && j <= W) {                                       // vertical neighbours are interior columns
                if (i - 1 >= 1 && i - 1 <= H) v += a[i - 2] * G[e - Wp];
                if (i + 1 >= 1 && i + 1 <= H) v += a[i] * G[e + Wp];
            }
            if (i >= 1 && i <= H) {
                if (j - 1 >= 1 && j - 1 <= W) v += b[j - 2] * G[e - 1];
                if (j + 1 >= 1 && j + 1 <= W) v += b[j] * G[e + 1];
            }
            if constexpr (EMIT) {
                if (gt && in) v += S1<IO>::ld(gt + (i - 1) * W + (j - 1));
            }
            Gn[e] = v;
        }
        __syncthreads();
        float* t = G; G = Gn; Gn = t;
    }
    // adjoint of the reflect padding: fold the ring back onto rows/cols 1 and H-2 / W-2
    IO* gub = gu + (size_t)s * H * W;
    for (int e = threadIdx.x; e < H * W; e += blockDim.x) {
        const int i = e / W, j = e % W;
        float v = 0.f;
        for (int di = 0; di < 2; ++di) {
            int m;
            if (di == 0) m = i + 1;
            else if (i == 1) m = 0;
            else if (i == H - 2) m = H + 1;
            else continue;
            for (int dj = 0; dj < 2; ++dj) {
                int nn;
                if (dj == 0) nn = j + 1;
                else if (j == 1) nn = 0;
                else if (j == W - 2) nn = W + 1;
                else continue;
                v += G[m * Wp + nn];
            }
            // rows 1 and H-2 coincide when H == 3; not supported (H,W >= 4 checked on the host)
        }
        S1<IO>::st(gub + e, v);
    }
    float* pp = part + (size_t)s * (H + W);
    for (int e = threadIdx.x; e < H; e += blockDim.x) pp[e] = ga[e];
    for (int e = threadIdx.x; e < W; e += blockDim.x) pp[H + e] = gb[e];
}

__global__ void jacobi_pgrad_kernel(const float* __restrict__ part, float* __restrict__ ga, float* __restrict__ gb,
                                    int B, int H, int W) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= H + W) return;
    float s = 0.f;
    for (int k = 0; k < B; ++k) s += part[(size_t)k * (H + W) + r];
    if (r < H) ga[r] = s; else gb[r - H] = s;
}

// The adjoint alone (pde_jacobi_io_backward_input[_states]: a_row and b_col take no gradient): jacobi_bwd_kernel without
// the forward recompute, the parked states and the row / column dots.  LDS: G, Gn, a, b.  The nt updates and the fold
// are written as they are there, so gu has the same bits; nt = 0 leaves gu = gout.
template <typename IO, bool EMIT = false>
__global__ __launch_bounds__(256) void jacobi_bwd_input_kernel(const IO* __restrict__ gout, const float* __restrict__ a_row,
                                                               const float* __restrict__ b_col, IO* __restrict__ gu,
                                                               int H, int W, int nt, const IO* __restrict__ gtraj,
                                                               EmitMask em) {
    extern __shared__ float sm[];
    const int Wp = W + 2, PN = (H + 2) * Wp;
    float* G = sm;
    float* Gn = sm + PN;
    float* a = sm + 2 * PN;
    float* b = a + H;
    const int s = blockIdx.x;
    for (int e = threadIdx.x; e < H; e += blockDim.x) a[e] = a_row[e];
    for (int e = threadIdx.x; e < W; e += blockDim.x) b[e] = b_col[e];
    // G = dL/dP_nt (zero ring, gout inside)
    const IO* gob = gout + (size_t)s * H * W;
    for (int e = threadIdx.x; e < PN; e += blockDim.x) {
        const int i = e / Wp, j = e % Wp;
        G[e] = (i >= 1 && i <= H && j >= 1 && j <= W) ? S1<IO>::ld(gob + (i - 1) * W + (j - 1)) : 0.f;
    }
    __syncthreads();
    for (int n = nt - 1; n >= 0; --n) {
        // dL/dP_n from dL/dP_{n+1}
        const IO* gt = nullptr;                                // dL/d(state after step n), where that state was emitted
        if constexpr (EMIT) {
            const int slot = emit_slot(em, n);
            if (slot >= 0) gt = gtraj + ((size_t)slot * gridDim.x + s) * H * W;
        }
        for (int e = threadIdx.x; e < PN; e += blockDim.x) {
            const int i = e / Wp, j = e % Wp;
            const bool in = (i >= 1 && i <= H && j >= 1 && j <= W);
            float v = in ? (1.f - 2.f * a[i - 1] - 2.f * b[j - 1]) * G[e] : G[e];
            if (j >= 1 && j <= W) {                                       // vertical neighbours are interior columns
                if (i - 1 >= 1 && i - 1 <= H) v += a[i - 2] * G[e - Wp];
                if (i + 1 >= 1 && i + 1 <= H) v += a[i] * G[e + Wp];
            }
            if (i >= 1 && i <= H) {
                if (j - 1 >= 1 && j - 1 <= W) v += b[j - 2] * G[e - 1];
                if (j + 1 >= 1 && j + 1 <= W) v += b[j] * G[e + 1];
            }
            if constexpr (EMIT) {
                if (gt && in) v += S1<IO>::ld(gt + (i - 1) * W + (j - 1));
            }
            Gn[e] = v;
        }
        __syncthreads();
        float* t = G; G = Gn; Gn = t;
    }
    // adjoint of the reflect padding: fold the ring back onto rows/cols 1 and H-2 / W-2
    IO* gub = gu + (size_t)s * H * W;
    for (int e = threadIdx.x; e < H * W; e += blockDim.x) {
        const int i = e / W, j = e % W;
        float v = 0.f;
        for (int di = 0; di < 2; ++di) {
            int m;
            if (di == 0) m = i + 1;
            else if (i == 1) m = 0;
            else if (i == H - 2) m = H + 1;
            else continue;
            for (int dj = 0; dj < 2; ++dj) {
                int nn;
                if (dj == 0) nn = j + 1;
                else if (j == 1) nn = 0;
                else if (j == W - 2) nn = W + 1;
                else continue;
                v += G[m * Wp + nn];
            }
        }
        S1<IO>::st(gub + e, v);
    }
}

// The tangent-linear pass (pdecnn_explicit_tangent.h: pde_jacobi_io_tangent), planes up to 64x64: jacobi_fwd_kernel with a
// second state.  dP is the reflect-padded du (zeros when du is NULL); both rings stay frozen.  Interior, per step:
//     P'  = P + a_i d1(P) + b_j d2(P)                              jacobi_step's expressions, in their order
//     dP' = the same on dP, then + da_i d1(P) + db_j d2(P),        P the step's input; not added at all when src == 0
// LDS (dynamic): P, Q, dP, dQ, a, b, da, db — 70720 bytes at 64x64.
__device__ __forceinline__ void jacobi_tangent_step(const float* P, float* Q, const float* dP, float* dQ, const float* a,
                                                    const float* b, const float* da, const float* db, int H, int W, int src) {
    const int Wp = W + 2;
    for (int e = threadIdx.x; e < (H + 2) * Wp; e += blockDim.x) {
        const int i = e / Wp, j = e % Wp;
        float v = P[e], dv = dP[e];
        if (i >= 1 && i <= H && j >= 1 && j <= W) {
            const float d1 = P[e + Wp] - 2.f * v + P[e - Wp];
            const float d2 = P[e + 1] - 2.f * v + P[e - 1];
            const float dd1 = dP[e + Wp] - 2.f * dv + dP[e - Wp];
            const float dd2 = dP[e + 1] - 2.f * dv + dP[e - 1];
            v = v + a[i - 1] * d1 + b[j - 1] * d2;
            dv = dv + a[i - 1] * dd1 + b[j - 1] * dd2;
            if (src) dv = dv + da[i - 1] * d1 + db[j - 1] * d2;
        }
        Q[e] = v;
        dQ[e] = dv;
    }
}

template <typename IO>
__global__ __launch_bounds__(256) void jacobi_tangent_kernel(const IO* __restrict__ u, const IO* __restrict__ du,
                                                             const float* __restrict__ a_row, const float* __restrict__ b_col,
                                                             const float* __restrict__ d_a_row,
                                                             const float* __restrict__ d_b_col, IO* __restrict__ out,
                                                             IO* __restrict__ dout, int H, int W, int nt, int src) {
    extern __shared__ float sm[];
    const int Wp = W + 2, PN = (H + 2) * Wp;
    float* P = sm;
    float* Q = sm + PN;
    float* dP = sm + 2 * PN;
    float* dQ = sm + 3 * PN;
    float* a = sm + 4 * PN;
    float* b = a + H;
    float* da = b + W;
    float* db = da + H;
    const IO* ub = u + (size_t)blockIdx.x * H * W;
    const IO* dub = du ? du + (size_t)blockIdx.x * H * W : nullptr;
    for (int e = threadIdx.x; e < H; e += blockDim.x) { a[e] = a_row[e]; da[e] = d_a_row ? d_a_row[e] : 0.f; }
    for (int e = threadIdx.x; e < W; e += blockDim.x) { b[e] = b_col[e]; db[e] = d_b_col ? d_b_col[e] : 0.f; }
    for (int e = threadIdx.x; e < PN; e += blockDim.x) {
        const int i = e / Wp, j = e % Wp;
        const int o = reflect_src(i, H) * W + reflect_src(j, W);                    // F.pad(..., mode='reflect')
        P[e] = S1<IO>::ld(ub + o);
        dP[e] = dub ? S1<IO>::ld(dub + o) : 0.f;
    }
    __syncthreads();
    for (int n = 0; n < nt; ++n) {
        jacobi_tangent_step(P, Q, dP, dQ, a, b, da, db, H, W, src);
        __syncthreads();
        float* t = P; P = Q; Q = t;
        t = dP; dP = dQ; dQ = t;
    }
    IO* ob = out ? out + (size_t)blockIdx.x * H * W : nullptr;
    IO* dob = dout + (size_t)blockIdx.x * H * W;
    for (int e = threadIdx.x; e < H * W; e += blockDim.x) {
        const int l = (e / W + 1) * Wp + (e % W) + 1;
        if (ob) S1<IO>::st(ob + e, P[l]);
        S1<IO>::st(dob + e, dP[l]);
    }
}

size_t align256(size_t x) { return (x + 255) / 256 * 256; }

#include "pde_jacobi_tiled.h"

// 0: not served, 1: the one-workgroup kernels above, 2: the tiled kernels
int jacobi_path(int H, int W) {
    if (H < 4 || W < 4 || H > PDE_JACOBI_MAX_HW || W > PDE_JACOBI_MAX_HW) return 0;
    return (H <= kJMax && W <= kJMax) ? 1 : 2;
}
// the tiled path's grid: one workgroup per (sample, tile), in an int
bool jacobi_tiled_grid_ok(int B, int H, int W) { return (size_t)B * jtiles(H) * jtiles(W) <= 0x7fffffffu; }

struct JTiledWs {       // the tiled backward's workspace: parked states 1..nt-1, two padded adjoint images, tile sums
    size_t states, gimg, part;
    size_t total() const { return states + 2 * gimg + part; }
};
JTiledWs jacobi_tiled_ws(int B, int H, int W, int nt) {
    JTiledWs w;
    w.states = align256((size_t)(nt > 1 ? nt - 1 : 0) * B * H * W * sizeof(float));
    w.gimg = align256((size_t)B * (H + 2) * (W + 2) * sizeof(float));
    w.part = align256((size_t)B * jtiles(H) * jtiles(W) * 2 * kJT * sizeof(float));
    return w;
}

template <typename IO, bool EMIT>
int jacobi_tiled_forward(int B, int H, int W, int nt, const void* u, const float* a_row, const float* b_col, void* out,
                         void* workspace, void* traj, EmitMask em, hipStream_t st) {
    const int nTy = jtiles(H), nTx = jtiles(W);
    const dim3 grid((unsigned)((size_t)B * nTy * nTx));
    float* img[2] = {static_cast<float*>(workspace),
                     workspace ? reinterpret_cast<float*>(static_cast<char*>(workspace) + align256((size_t)B * H * W * sizeof(float)))
                               : nullptr};
    int n0 = 0, l = 0;
    do {                                                    // nt = 0: one launch of no steps copies
        const int k = nt - n0 < kJK ? nt - n0 : kJK;
        const bool last = n0 + k == nt;
        hipLaunchKernelGGL((jacobi_tiled_fwd_kernel<IO, EMIT>), grid, dim3(256), 0, st, (const IO*)u,
                           l == 0 ? (const float*)nullptr : (const float*)img[(l - 1) & 1], a_row, b_col,
                           last ? out : (void*)img[l & 1], last ? 0 : 1, (float*)nullptr, (size_t)0, H, W, nTy, nTx, k,
                           (IO*)traj, (size_t)B * H * W, em, n0);
        n0 += k;
        ++l;
    } while (n0 < nt);
    return check_launch();
}

template <typename IO, bool EMIT>
int jacobi_tiled_backward(int B, int H, int W, int nt, const void* u, const void* gout, const float* a_row,
                          const float* b_col, void* gu, float* g_a_row, float* g_b_col, void* workspace, const void* gtraj,
                          EmitMask em, hipStream_t st) {
    static unsigned long long configured = 0;
    const size_t lds = kJBwdFloats * sizeof(float);
    if (ensure_dynamic_lds(reinterpret_cast<const void*>(jacobi_tiled_bwd_kernel<IO, EMIT>), (int)lds, configured) != PDE_OK)
        return PDE_E_LAUNCH;
    const int nTy = jtiles(H), nTx = jtiles(W);
    const dim3 grid((unsigned)((size_t)B * nTy * nTx));
    const JTiledWs w = jacobi_tiled_ws(B, H, W, nt);
    char* base = static_cast<char*>(workspace);
    float* states = reinterpret_cast<float*>(base);
    float* gimg[2] = {reinterpret_cast<float*>(base + w.states), reinterpret_cast<float*>(base + w.states + w.gimg)};
    float* part = reinterpret_cast<float*>(base + w.states + 2 * w.gimg);
    const size_t stride = (size_t)B * H * W;
    // forward again, parking P_1 .. P_{nt-1}; every launch continues from the last state the one before parked
    for (int n0 = 0; n0 < nt - 1; n0 += kJK) {
        const int k = nt - 1 - n0 < kJK ? nt - 1 - n0 : kJK;
        hipLaunchKernelGGL((jacobi_tiled_fwd_kernel<IO, false>), grid, dim3(256), 0, st, (const IO*)u,
                           n0 == 0 ? (const float*)nullptr : (const float*)(states + (size_t)(n0 - 1) * stride), a_row, b_col,
                           (void*)nullptr, 0, states + (size_t)n0 * stride, stride, H, W, nTy, nTx, k, (IO*)nullptr, (size_t)0,
                           EmitMask{0, 0}, 0);
    }
    int n_hi = nt, l = 0;
    do {                                                    // nt = 0: one launch of no steps pads gout
        const int k = n_hi < kJK ? n_hi : kJK;
        hipLaunchKernelGGL((jacobi_tiled_bwd_kernel<IO, EMIT>), grid, dim3(256), lds, st, (const IO*)u, (const float*)states,
                           stride, l == 0 ? (const IO*)gout : (const IO*)nullptr, (const float*)gimg[(l + 1) & 1], gimg[l & 1],
                           a_row, b_col, part, l == 0 ? 0 : 1, H, W, nTy, nTx, n_hi, k, (const IO*)gtraj, em);
        n_hi -= k;
        ++l;
    } while (n_hi > 0);
    const int nRb = (H + 31) / 32, nCb = (W + 31) / 32;
    hipLaunchKernelGGL(jacobi_tiled_fold_kernel<IO>, dim3((unsigned)((size_t)B * nRb * nCb)), dim3(256), 0, st,
                       (const float*)gimg[(l - 1) & 1], (IO*)gu, H, W, nRb, nCb);
    hipLaunchKernelGGL(jacobi_tiled_pgrad_kernel, dim3((H + W + 63) / 64), dim3(64), 0, st, (const float*)part, g_a_row,
                       g_b_col, B, H, W, nTy, nTx);
    return check_launch();
}

// the tiled adjoint alone: the adjoint launches without P_n, chained through the two padded fp32 images, then the fold
size_t jacobi_tiled_gimg_bytes(int B, int H, int W) { return align256((size_t)B * (H + 2) * (W + 2) * sizeof(float)); }
template <typename IO, bool EMIT>
int jacobi_tiled_backward_input(int B, int H, int W, int nt, const void* gout, const float* a_row, const float* b_col,
                                void* gu, void* workspace, const void* gtraj, EmitMask em, hipStream_t st) {
    const int nTy = jtiles(H), nTx = jtiles(W);
    const dim3 grid((unsigned)((size_t)B * nTy * nTx));
    char* base = static_cast<char*>(workspace);
    float* gimg[2] = {reinterpret_cast<float*>(base), reinterpret_cast<float*>(base + jacobi_tiled_gimg_bytes(B, H, W))};
    int n_hi = nt, l = 0;
    do {                                                    // nt = 0: one launch of no steps pads gout
        const int k = n_hi < kJK ? n_hi : kJK;
        hipLaunchKernelGGL((jacobi_tiled_bwd_input_kernel<IO, EMIT>), grid, dim3(256), 0, st,
                           l == 0 ? (const IO*)gout : (const IO*)nullptr, (const float*)gimg[(l + 1) & 1], gimg[l & 1], a_row,
                           b_col, (size_t)B * H * W, H, W, nTy, nTx, n_hi, k, (const IO*)gtraj, em);
        n_hi -= k;
        ++l;
    } while (n_hi > 0);
    const int nRb = (H + 31) / 32, nCb = (W + 31) / 32;
    hipLaunchKernelGGL(jacobi_tiled_fold_kernel<IO>, dim3((unsigned)((size_t)B * nRb * nCb)), dim3(256), 0, st,
                       (const float*)gimg[(l - 1) & 1], (IO*)gu, H, W, nRb, nCb);
    return check_launch();
}

// One step of the generic-size path: the tensors of the call are of type T (float, bf16e, f16e) — the layer's input is
// read in the first step, its output written in the last; what passes between the steps is fp32.
struct ExArgs {
    const float *alpha, *scale;
    int nplanes, C, H, W;
    float dt, eps, maxc, relax;
};
template <typename TI, typename TO, typename TE = void>
void ex_fwd(const ExArgs& a, const void* src, void* dst, typename EmitPtr<TE>::type emit, hipStream_t st) {
    if (a.W % 4)                                           // rows not 16-byte aligned: the scalar-column variant
        hipLaunchKernelGGL((explicit5_fwd_col_kernel<TI, TO, TE>), dim3(a.nplanes), dim3(256), 0, st, (const TI*)src, a.alpha,
                           a.scale, (TO*)dst, a.C, a.H, a.W, a.dt, a.eps, a.maxc, a.relax, emit);
    else
        hipLaunchKernelGGL((explicit5_fwd_kernel<TI, TO, TE>), dim3(a.nplanes), dim3(256), 0, st, (const TI*)src, a.alpha,
                           a.scale, (TO*)dst, a.C, a.H, a.W, a.dt, a.eps, a.maxc, a.relax, emit);
}
// emit: NULL, or the slot of the trajectory tensor (type T) this step's output goes to as well; never at the last step
template <typename T>
void ex_fwd_step(const ExArgs& a, bool first, bool last, const void* src, void* dst, void* emit, hipStream_t st) {
    if (emit && first) ex_fwd<T, float, T>(a, src, dst, (T*)emit, st);
    else if (emit) ex_fwd<float, float, T>(a, src, dst, (T*)emit, st);
    else if (first && last) ex_fwd<T, T>(a, src, dst, NoEmit{}, st);
    else if (first) ex_fwd<T, float>(a, src, dst, NoEmit{}, st);
    else if (last) ex_fwd<float, T>(a, src, dst, NoEmit{}, st);
    else ex_fwd<float, float>(a, src, dst, NoEmit{}, st);
}
// backward step k: u is the caller's (type T) for the first step, a parked fp32 state otherwise; the incoming gradient
// is the caller's for the last step; gu is written to the caller's tensor at the first step
template <typename TU, typename TG, typename TO, typename TE = void>
void ex_bwd(const ExArgs& a, const void* up, const void* gin, void* gdst, float* part, int acc,
            typename EmitPtr<const TE>::type ginj, hipStream_t st) {
    if (a.W % 4)
        hipLaunchKernelGGL((explicit5_bwd_col_kernel<TU, TG, TO, TE>), dim3(a.nplanes), dim3(256), 0, st, (const TU*)up,
                           (const TG*)gin, a.alpha, a.scale, (TO*)gdst, part, a.C, a.H, a.W, a.dt, a.eps, a.maxc, a.relax, acc,
                           ginj);
    else
        hipLaunchKernelGGL((explicit5_bwd_kernel<TU, TG, TO, TE>), dim3(a.nplanes), dim3(256), 0, st, (const TU*)up,
                           (const TG*)gin, a.alpha, a.scale, (TO*)gdst, part, a.C, a.H, a.W, a.dt, a.eps, a.maxc, a.relax, acc,
                           ginj);
}
// ginj: NULL, or the slot of the trajectory's gradient (type T) that is added to this step's output; never at step 1
template <typename T>
void ex_bwd_step(const ExArgs& a, bool ufirst, bool gfirst, const void* up, const void* gin, void* gdst, float* part, int acc,
                 const void* ginj, hipStream_t st) {
    if (ginj && gfirst) ex_bwd<float, T, float, T>(a, up, gin, gdst, part, acc, (const T*)ginj, st);
    else if (ginj) ex_bwd<float, float, float, T>(a, up, gin, gdst, part, acc, (const T*)ginj, st);
    else if (ufirst && gfirst) ex_bwd<T, T, T>(a, up, gin, gdst, part, acc, NoEmit{}, st);
    else if (ufirst) ex_bwd<T, float, T>(a, up, gin, gdst, part, acc, NoEmit{}, st);
    else if (gfirst) ex_bwd<float, T, float>(a, up, gin, gdst, part, acc, NoEmit{}, st);
    else ex_bwd<float, float, float>(a, up, gin, gdst, part, acc, NoEmit{}, st);
}

// the same step for the input alone: no u, no partial sums
template <typename TG, typename TO, typename TE = void>
void ex_bwd_input(const ExArgs& a, const void* gin, void* gdst, typename EmitPtr<const TE>::type ginj, hipStream_t st) {
    if (a.W % 4)
        hipLaunchKernelGGL((explicit5_bwd_input_col_kernel<TG, TO, TE>), dim3(a.nplanes), dim3(256), 0, st, (const TG*)gin,
                           a.alpha, a.scale, (TO*)gdst, a.C, a.H, a.W, a.dt, a.eps, a.maxc, a.relax, ginj);
    else
        hipLaunchKernelGGL((explicit5_bwd_input_kernel<TG, TO, TE>), dim3(a.nplanes), dim3(256), 0, st, (const TG*)gin,
                           a.alpha, a.scale, (TO*)gdst, a.C, a.H, a.W, a.dt, a.eps, a.maxc, a.relax, ginj);
}
// glast: the step that writes the caller's gu (step 1); gfirst: the step that reads the caller's gout (step num_steps)
template <typename T>
void ex_bwd_input_step(const ExArgs& a, bool glast, bool gfirst, const void* gin, void* gdst, const void* ginj,
                       hipStream_t st) {
    if (ginj && gfirst) ex_bwd_input<T, float, T>(a, gin, gdst, (const T*)ginj, st);
    else if (ginj) ex_bwd_input<float, float, T>(a, gin, gdst, (const T*)ginj, st);
    else if (glast && gfirst) ex_bwd_input<T, T>(a, gin, gdst, NoEmit{}, st);
    else if (glast) ex_bwd_input<float, T>(a, gin, gdst, NoEmit{}, st);
    else if (gfirst) ex_bwd_input<T, float>(a, gin, gdst, NoEmit{}, st);
    else ex_bwd_input<float, float>(a, gin, gdst, NoEmit{}, st);
}

// Where the call's own tensors may begin (pdecnn.h, "Alignment"): planes whose rows are whole groups of four columns move
// four elements wide (float4, or four 16-bit values in 8 bytes), every other plane one element at a time.  alpha_base and
// channel_scaling (C values each) are read one at a time whatever the plane.
unsigned ex_tensor_align(int W, int io_dtype) { return (W % 4 ? 1u : 4u) * io_elem_bytes(io_dtype); }

}  // namespace
}  // namespace pde

using namespace pde;

extern "C" {

int pde_explicit5_forward(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype, const void* u,
                          const float* alpha_base, const float* channel_scaling, float dt, float eps, float max_coeff,
                          float relax, int32_t num_steps, void* states, void* out, void* stream) {
    return pde_explicit5_forward_states(B, C, H, W, io_dtype, u, alpha_base, channel_scaling, dt, eps, max_coeff, relax,
                                        num_steps, states, out, nullptr, nullptr, stream);
}

int pde_explicit5_forward_states(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype, const void* u,
                                 const float* alpha_base, const float* channel_scaling, float dt, float eps, float max_coeff,
                                 float relax, int32_t num_steps, void* states, void* out, void* traj,
                                 const uint64_t emit_mask[2], void* stream) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_steps < 1 || !u || !alpha_base || !channel_scaling || !out)
        return PDE_E_BADARG;
    if (io_dtype != PDE_IO_F32 && io_dtype != PDE_IO_BF16 && io_dtype != PDE_IO_F16) return PDE_E_BADARG;
    if (misaligned(ex_tensor_align(W, io_dtype), u, out, traj) || misaligned(ex_tensor_align(W, PDE_IO_F32), states) ||
        misaligned(4, alpha_base, channel_scaling))
        return PDE_E_BADARG;
    EmitMask em;
    const int erc = emit_check(emit_mask, num_steps, traj, em);
    if (erc != PDE_OK) return erc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nplanes = B * C;
    if (wave_plane_ok(H, W)) {                             // the plane stays in registers over all steps
        if (io_dtype == PDE_IO_F32)
            fwd_wave_io<float>(H, u, alpha_base, channel_scaling, out, (float*)states, nplanes, C, num_steps, dt, eps,
                               max_coeff, relax, traj, em, st);
        else if (io_dtype == PDE_IO_F16)
            fwd_wave_io<f16e>(H, u, alpha_base, channel_scaling, out, (float*)states, nplanes, C, num_steps, dt, eps,
                              max_coeff, relax, traj, em, st);
        else
            fwd_wave_io<bf16e>(H, u, alpha_base, channel_scaling, out, (float*)states, nplanes, C, num_steps, dt, eps,
                               max_coeff, relax, traj, em, st);
        return check_launch();
    }
    if (num_steps > 1 && !states) return PDE_E_BADARG;     // generic sizes: one launch per step through `states` (fp32)
    const size_t tf = (size_t)nplanes * H * W;
    const size_t esz = io_dtype == PDE_IO_F32 ? 4 : 2;
    float* sf = static_cast<float*>(states);
    const ExArgs ea{alpha_base, channel_scaling, nplanes, C, H, W, dt, eps, max_coeff, relax};
    for (int k = 0; k < num_steps; ++k) {
        const bool first = k == 0, last = k == num_steps - 1;
        const void* src = first ? u : static_cast<const void*>(sf + (size_t)(k - 1) * tf);
        void* dst = last ? out : static_cast<void*>(sf + (size_t)k * tf);
        const int slot = emit_slot(em, k + 1);             // the step's own launch writes the emitted state too
        void* emit = slot >= 0 ? static_cast<void*>(static_cast<char*>(traj) + (size_t)slot * tf * esz) : nullptr;
        if (io_dtype == PDE_IO_F32) ex_fwd_step<float>(ea, first, last, src, dst, emit, st);
        else if (io_dtype == PDE_IO_F16) ex_fwd_step<f16e>(ea, first, last, src, dst, emit, st);
        else ex_fwd_step<bf16e>(ea, first, last, src, dst, emit, st);
    }
    return check_launch();
}

size_t pde_explicit5_backward_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype,
                                              int32_t num_steps) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_steps < 1) return 0;
    size_t b = align256((size_t)B * C * 2 * sizeof(float));
    if (num_steps > 1 && !wave_plane_ok(H, W))             // generic sizes: two gradient buffers to ping-pong through
        b += 2 * align256((size_t)B * C * H * W * sizeof(float));
    return b;
}

int pde_explicit5_backward(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype, const void* u,
                           const void* states, const void* gout, const float* alpha_base, const float* channel_scaling,
                           float dt, float eps, float max_coeff, float relax, int32_t num_steps, void* gu,
                           float* g_alpha_base, float* g_channel_scaling, void* workspace, size_t workspace_bytes,
                           void* stream) {
    return pde_explicit5_backward_states(B, C, H, W, io_dtype, u, states, gout, nullptr, nullptr, alpha_base, channel_scaling,
                                         dt, eps, max_coeff, relax, num_steps, gu, g_alpha_base, g_channel_scaling, workspace,
                                         workspace_bytes, stream);
}

int pde_explicit5_backward_states(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype, const void* u,
                                  const void* states, const void* gout, const void* gtraj, const uint64_t emit_mask[2],
                                  const float* alpha_base, const float* channel_scaling, float dt, float eps,
                                  float max_coeff, float relax, int32_t num_steps, void* gu, float* g_alpha_base,
                                  float* g_channel_scaling, void* workspace, size_t workspace_bytes, void* stream) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_steps < 1 || !u || !gout || !alpha_base ||
        !channel_scaling || !gu || !g_alpha_base || !g_channel_scaling || !workspace || (num_steps > 1 && !states))
        return PDE_E_BADARG;
    if (io_dtype != PDE_IO_F32 && io_dtype != PDE_IO_BF16 && io_dtype != PDE_IO_F16) return PDE_E_BADARG;
    if (misaligned(ex_tensor_align(W, io_dtype), u, gout, gtraj, gu) || misaligned(ex_tensor_align(W, PDE_IO_F32), states) ||
        misaligned(4, alpha_base, channel_scaling, g_alpha_base, g_channel_scaling))
        return PDE_E_BADARG;
    EmitMask em;
    const int erc = emit_check(emit_mask, num_steps, gtraj, em);
    if (erc != PDE_OK) return erc;
    // the two gradient buffers behind the partial sums are read and written as float4 on the generic float4 path
    if (workspace_bytes < pde_explicit5_backward_workspace_bytes(B, C, H, W, io_dtype, num_steps) ||
        misaligned(kVecAlign, workspace))
        return PDE_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(workspace);
    const int nplanes = B * C;
    if (wave_plane_ok(H, W)) {
        if (io_dtype == PDE_IO_F32)
            bwd_wave_io<float>(H, u, (const float*)states, gout, alpha_base, channel_scaling, gu, part, nplanes, C, num_steps,
                               dt, eps, max_coeff, relax, gtraj, em, st);
        else if (io_dtype == PDE_IO_F16)
            bwd_wave_io<f16e>(H, u, (const float*)states, gout, alpha_base, channel_scaling, gu, part, nplanes, C, num_steps,
                              dt, eps, max_coeff, relax, gtraj, em, st);
        else
            bwd_wave_io<bf16e>(H, u, (const float*)states, gout, alpha_base, channel_scaling, gu, part, nplanes, C, num_steps,
                               dt, eps, max_coeff, relax, gtraj, em, st);
    } else {
        // what passes between the steps is fp32 (the states the forward left, the gradient buffers here), whatever io_dtype
        const size_t tf = (size_t)nplanes * H * W;
        float* buf0 = reinterpret_cast<float*>(static_cast<char*>(workspace) + align256((size_t)nplanes * 2 * sizeof(float)));
        float* buf1 = reinterpret_cast<float*>(reinterpret_cast<char*>(buf0) + align256(tf * sizeof(float)));
        const float* sf = static_cast<const float*>(states);
        const size_t esz = io_dtype == PDE_IO_F32 ? 4 : 2;
        const ExArgs ea{alpha_base, channel_scaling, nplanes, C, H, W, dt, eps, max_coeff, relax};
        const void* gin = gout;
        for (int k = num_steps; k >= 1; --k) {
            const bool ufirst = k == 1, gfirst = k == num_steps;       // u / gu are the caller's tensors, gout too
            const void* up = ufirst ? u : static_cast<const void*>(sf + (size_t)(k - 2) * tf);
            void* gdst = ufirst ? gu : static_cast<void*>(gin == buf0 ? buf1 : buf0);
            const int acc = gfirst ? 0 : 1;
            const int slot = emit_slot(em, k - 1);         // gdst is the adjoint of the state after step k-1
            const void* ginj = slot >= 0 ? static_cast<const void*>(static_cast<const char*>(gtraj) + (size_t)slot * tf * esz)
                                         : nullptr;
            if (io_dtype == PDE_IO_F32) ex_bwd_step<float>(ea, ufirst, gfirst, up, gin, gdst, part, acc, ginj, st);
            else if (io_dtype == PDE_IO_F16) ex_bwd_step<f16e>(ea, ufirst, gfirst, up, gin, gdst, part, acc, ginj, st);
            else ex_bwd_step<bf16e>(ea, ufirst, gfirst, up, gin, gdst, part, acc, ginj, st);
            gin = gdst;
        }
    }
    hipLaunchKernelGGL(explicit5_pgrad_kernel, dim3(C), dim3(256), 0, st, part, alpha_base, channel_scaling,
                       g_alpha_base, g_channel_scaling, B, C, dt, eps, max_coeff, relax);
    return check_launch();
}

static size_t jacobi_lds(int H, int W, bool bwd) {
    const size_t PN = (size_t)(H + 2) * (W + 2);
    return (2 * PN + (bwd ? 2 : 1) * (H + W)) * sizeof(float);
}

int pde_jacobi_plane_path(int32_t H, int32_t W) { return jacobi_path(H, W); }

int pde_jacobi_forward(int32_t B, int32_t H, int32_t W, int32_t nt, const float* u, const float* a_row,
                       const float* b_col, float* out, void* stream) {
    return pde_jacobi_io_forward_ws(B, H, W, nt, PDE_IO_F32, u, a_row, b_col, out, nullptr, 0, stream);
}

int pde_jacobi_io_forward(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype, const void* u, const float* a_row,
                          const float* b_col, void* out, void* stream) {
    return pde_jacobi_io_forward_ws(B, H, W, nt, io_dtype, u, a_row, b_col, out, nullptr, 0, stream);
}

size_t pde_jacobi_forward_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t nt) {
    if (B <= 0 || nt <= kJK || jacobi_path(H, W) != 2) return 0;
    return 2 * align256((size_t)B * H * W * sizeof(float));     // two fp32 images for the launches to alternate between
}

}  // extern "C"

// one tensor type of the Jacobi calls: the plain instantiations for an empty mask, the emitting ones otherwise
template <typename IO>
static int jacobi_forward_io(int path, int B, int H, int W, int nt, const void* u, const float* a_row, const float* b_col,
                             void* out, void* workspace, void* traj, EmitMask em, hipStream_t st) {
    if (path == 2)
        return em.any() ? jacobi_tiled_forward<IO, true>(B, H, W, nt, u, a_row, b_col, out, workspace, traj, em, st)
                        : jacobi_tiled_forward<IO, false>(B, H, W, nt, u, a_row, b_col, out, workspace, nullptr, em, st);
    const size_t lds = jacobi_lds(H, W, false);
    if (em.any())
        hipLaunchKernelGGL((jacobi_fwd_kernel<IO, true>), dim3(B), dim3(256), lds, st, (const IO*)u, a_row, b_col, (IO*)out, H, W,
                           nt, (IO*)traj, em);
    else
        hipLaunchKernelGGL((jacobi_fwd_kernel<IO, false>), dim3(B), dim3(256), lds, st, (const IO*)u, a_row, b_col, (IO*)out, H,
                           W, nt, (IO*)nullptr, em);
    return check_launch();
}

extern "C" {

int pde_jacobi_io_forward_ws(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype, const void* u,
                             const float* a_row, const float* b_col, void* out, void* workspace, size_t workspace_bytes,
                             void* stream) {
    return pde_jacobi_io_forward_states(B, H, W, nt, io_dtype, u, a_row, b_col, out, nullptr, nullptr, workspace,
                                        workspace_bytes, stream);
}

int pde_jacobi_io_forward_states(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype, const void* u,
                                 const float* a_row, const float* b_col, void* out, void* states,
                                 const uint64_t emit_mask[2], void* workspace, size_t workspace_bytes, void* stream) {
    const int path = jacobi_path(H, W);
    if (B <= 0 || path == 0 || nt < 0 || !u || !a_row || !b_col || !out) return PDE_E_BADARG;
    if (io_dtype != PDE_IO_F32 && io_dtype != PDE_IO_BF16 && io_dtype != PDE_IO_F16) return PDE_E_BADARG;
    // the Jacobi kernels move one element at a time, tensors and workspace alike; the header asks 16 bytes of every workspace
    if (misaligned(io_elem_bytes(io_dtype), u, out, states) || misaligned(4, a_row, b_col)) return PDE_E_BADARG;
    if (misaligned(kVecAlign, workspace)) return PDE_E_WORKSPACE;
    EmitMask em;
    const int erc = emit_check(emit_mask, nt, states, em);
    if (erc != PDE_OK) return erc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (path == 2) {
        if (!jacobi_tiled_grid_ok(B, H, W)) return PDE_E_BADARG;
        const size_t need = pde_jacobi_forward_workspace_bytes(B, H, W, nt);
        if (need && (!workspace || workspace_bytes < need)) return PDE_E_WORKSPACE;
    }
    if (io_dtype == PDE_IO_F32) return jacobi_forward_io<float>(path, B, H, W, nt, u, a_row, b_col, out, workspace, states, em, st);
    if (io_dtype == PDE_IO_BF16) return jacobi_forward_io<bf16e>(path, B, H, W, nt, u, a_row, b_col, out, workspace, states, em, st);
    return jacobi_forward_io<f16e>(path, B, H, W, nt, u, a_row, b_col, out, workspace, states, em, st);
}

size_t pde_jacobi_backward_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t nt) {
    if (B <= 0 || H <= 0 || W <= 0 || nt < 0) return 0;
    if (H > kJMax || W > kJMax) return jacobi_path(H, W) == 2 ? jacobi_tiled_ws(B, H, W, nt).total() : 0;
    const size_t PN = (size_t)(H + 2) * (W + 2);
    return align256((size_t)B * nt * PN * sizeof(float)) + align256((size_t)B * (H + W) * sizeof(float));
}

size_t pde_jacobi_io_backward_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype) {
    if (io_dtype != PDE_IO_F32 && io_dtype != PDE_IO_BF16 && io_dtype != PDE_IO_F16) return 0;
    return pde_jacobi_backward_workspace_bytes(B, H, W, nt);          // the parked states are fp32 whatever the tensors' type
}

int pde_jacobi_backward(int32_t B, int32_t H, int32_t W, int32_t nt, const float* u, const float* gout,
                        const float* a_row, const float* b_col, float* gu, float* g_a_row, float* g_b_col,
                        void* workspace, size_t workspace_bytes, void* stream) {
    return pde_jacobi_io_backward(B, H, W, nt, PDE_IO_F32, u, gout, a_row, b_col, gu, g_a_row, g_b_col, workspace,
                                  workspace_bytes, stream);
}

}  // extern "C"

template <typename IO>
static int jacobi_backward_io(int path, int B, int H, int W, int nt, const void* u, const void* gout, const float* a_row,
                              const float* b_col, void* gu, float* g_a_row, float* g_b_col, void* workspace,
                              const void* gtraj, EmitMask em, hipStream_t st) {
    if (path == 2)
        return em.any() ? jacobi_tiled_backward<IO, true>(B, H, W, nt, u, gout, a_row, b_col, gu, g_a_row, g_b_col, workspace,
                                                          gtraj, em, st)
                        : jacobi_tiled_backward<IO, false>(B, H, W, nt, u, gout, a_row, b_col, gu, g_a_row, g_b_col, workspace,
                                                           nullptr, em, st);
    const size_t PN = (size_t)(H + 2) * (W + 2);
    float* states = static_cast<float*>(workspace);
    float* part = reinterpret_cast<float*>(static_cast<char*>(workspace) + align256((size_t)B * nt * PN * sizeof(float)));
    const size_t lds = jacobi_lds(H, W, true);
    if (em.any())
        hipLaunchKernelGGL((jacobi_bwd_kernel<IO, true>), dim3(B), dim3(256), lds, st, (const IO*)u, (const IO*)gout, a_row,
                           b_col, (IO*)gu, states, part, H, W, nt, (const IO*)gtraj, em);
    else
        hipLaunchKernelGGL((jacobi_bwd_kernel<IO, false>), dim3(B), dim3(256), lds, st, (const IO*)u, (const IO*)gout, a_row,
                           b_col, (IO*)gu, states, part, H, W, nt, (const IO*)nullptr, em);
    hipLaunchKernelGGL(jacobi_pgrad_kernel, dim3((H + W + 63) / 64), dim3(64), 0, st, part, g_a_row, g_b_col, B, H, W);
    return check_launch();
}

extern "C" {

int pde_jacobi_io_backward(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype, const void* u, const void* gout,
                           const float* a_row, const float* b_col, void* gu, float* g_a_row, float* g_b_col,
                           void* workspace, size_t workspace_bytes, void* stream) {
    return pde_jacobi_io_backward_states(B, H, W, nt, io_dtype, u, gout, nullptr, nullptr, a_row, b_col, gu, g_a_row, g_b_col,
                                         workspace, workspace_bytes, stream);
}

int pde_jacobi_io_backward_states(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype, const void* u,
                                  const void* gout, const void* gstates, const uint64_t emit_mask[2], const float* a_row,
                                  const float* b_col, void* gu, float* g_a_row, float* g_b_col, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    const int path = jacobi_path(H, W);
    if (B <= 0 || path == 0 || nt < 0 || !u || !gout || !a_row || !b_col || !gu || !g_a_row || !g_b_col || !workspace)
        return PDE_E_BADARG;
    if (io_dtype != PDE_IO_F32 && io_dtype != PDE_IO_BF16 && io_dtype != PDE_IO_F16) return PDE_E_BADARG;
    if (misaligned(io_elem_bytes(io_dtype), u, gout, gstates, gu) || misaligned(4, a_row, b_col, g_a_row, g_b_col)) return PDE_E_BADARG;
    EmitMask em;
    const int erc = emit_check(emit_mask, nt, gstates, em);
    if (erc != PDE_OK) return erc;
    if (workspace_bytes < pde_jacobi_backward_workspace_bytes(B, H, W, nt) || misaligned(kVecAlign, workspace)) return PDE_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (path == 2 && !jacobi_tiled_grid_ok(B, H, W)) return PDE_E_BADARG;
    if (io_dtype == PDE_IO_F32)
        return jacobi_backward_io<float>(path, B, H, W, nt, u, gout, a_row, b_col, gu, g_a_row, g_b_col, workspace, gstates, em, st);
    if (io_dtype == PDE_IO_BF16)
        return jacobi_backward_io<bf16e>(path, B, H, W, nt, u, gout, a_row, b_col, gu, g_a_row, g_b_col, workspace, gstates, em, st);
    return jacobi_backward_io<f16e>(path, B, H, W, nt, u, gout, a_row, b_col, gu, g_a_row, g_b_col, workspace, gstates, em, st);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------
// the backward for the input alone (pdecnn_explicit_input.h): the parameters take no gradient
// ---------------------------------------------------------------------------------------
extern "C" {

size_t pde_explicit5_backward_input_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype,
                                                    int32_t num_steps) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_steps < 2 || wave_plane_ok(H, W)) return 0;
    return 2 * align256((size_t)B * C * H * W * sizeof(float));     // generic sizes: two gradient buffers to ping-pong through
}

int pde_explicit5_backward_input(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype, const void* gout,
                                 const float* alpha_base, const float* channel_scaling, float dt, float eps, float max_coeff,
                                 float relax, int32_t num_steps, void* gu, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    return pde_explicit5_backward_input_states(B, C, H, W, io_dtype, gout, nullptr, nullptr, alpha_base, channel_scaling, dt,
                                               eps, max_coeff, relax, num_steps, gu, workspace, workspace_bytes, stream);
}

int pde_explicit5_backward_input_states(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype, const void* gout,
                                        const void* gtraj, const uint64_t emit_mask[2], const float* alpha_base,
                                        const float* channel_scaling, float dt, float eps, float max_coeff, float relax,
                                        int32_t num_steps, void* gu, void* workspace, size_t workspace_bytes, void* stream) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_steps < 1 || !gout || !alpha_base || !channel_scaling || !gu)
        return PDE_E_BADARG;
    if (io_dtype != PDE_IO_F32 && io_dtype != PDE_IO_BF16 && io_dtype != PDE_IO_F16) return PDE_E_BADARG;
    if (misaligned(ex_tensor_align(W, io_dtype), gout, gtraj, gu) || misaligned(4, alpha_base, channel_scaling))
        return PDE_E_BADARG;
    EmitMask em;
    const int erc = emit_check(emit_mask, num_steps, gtraj, em);
    if (erc != PDE_OK) return erc;
    // the two gradient buffers are read and written as float4 on the generic float4 path
    const size_t need = pde_explicit5_backward_input_workspace_bytes(B, C, H, W, io_dtype, num_steps);
    if ((need && (!workspace || workspace_bytes < need)) || misaligned(kVecAlign, workspace)) return PDE_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nplanes = B * C;
    if (wave_plane_ok(H, W)) {
        if (io_dtype == PDE_IO_F32)
            bwd_input_wave_io<float>(H, gout, alpha_base, channel_scaling, gu, nplanes, C, num_steps, dt, eps, max_coeff, relax,
                                     gtraj, em, st);
        else if (io_dtype == PDE_IO_F16)
            bwd_input_wave_io<f16e>(H, gout, alpha_base, channel_scaling, gu, nplanes, C, num_steps, dt, eps, max_coeff, relax,
                                    gtraj, em, st);
        else
            bwd_input_wave_io<bf16e>(H, gout, alpha_base, channel_scaling, gu, nplanes, C, num_steps, dt, eps, max_coeff, relax,
                                     gtraj, em, st);
        return check_launch();
    }
    // what passes between the steps is fp32, whatever io_dtype
    const size_t tf = (size_t)nplanes * H * W;
    float* buf0 = static_cast<float*>(workspace);
    float* buf1 = need ? reinterpret_cast<float*>(static_cast<char*>(workspace) + align256(tf * sizeof(float))) : nullptr;
    const size_t esz = io_dtype == PDE_IO_F32 ? 4 : 2;
    const ExArgs ea{alpha_base, channel_scaling, nplanes, C, H, W, dt, eps, max_coeff, relax};
    const void* gin = gout;
    for (int k = num_steps; k >= 1; --k) {
        const bool glast = k == 1, gfirst = k == num_steps;            // gu / gout are the caller's tensors
        void* gdst = glast ? gu : static_cast<void*>(gin == buf0 ? buf1 : buf0);
        const int slot = emit_slot(em, k - 1);             // gdst is the adjoint of the state after step k-1
        const void* ginj = slot >= 0 ? static_cast<const void*>(static_cast<const char*>(gtraj) + (size_t)slot * tf * esz)
                                     : nullptr;
        if (io_dtype == PDE_IO_F32) ex_bwd_input_step<float>(ea, glast, gfirst, gin, gdst, ginj, st);
        else if (io_dtype == PDE_IO_F16) ex_bwd_input_step<f16e>(ea, glast, gfirst, gin, gdst, ginj, st);
        else ex_bwd_input_step<bf16e>(ea, glast, gfirst, gin, gdst, ginj, st);
        gin = gdst;
    }
    return check_launch();
}

size_t pde_jacobi_io_backward_input_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype) {
    if (io_dtype != PDE_IO_F32 && io_dtype != PDE_IO_BF16 && io_dtype != PDE_IO_F16) return 0;
    if (B <= 0 || nt < 0 || jacobi_path(H, W) != 2) return 0;
    return 2 * jacobi_tiled_gimg_bytes(B, H, W);           // the two padded fp32 images the adjoint launches chain through
}

}  // extern "C"

template <typename IO>
static int jacobi_backward_input_io(int path, int B, int H, int W, int nt, const void* gout, const float* a_row,
                                    const float* b_col, void* gu, void* workspace, const void* gtraj, EmitMask em,
                                    hipStream_t st) {
    if (path == 2)
        return em.any() ? jacobi_tiled_backward_input<IO, true>(B, H, W, nt, gout, a_row, b_col, gu, workspace, gtraj, em, st)
                        : jacobi_tiled_backward_input<IO, false>(B, H, W, nt, gout, a_row, b_col, gu, workspace, nullptr, em, st);
    const size_t lds = jacobi_lds(H, W, false);            // G, Gn, a, b
    if (em.any())
        hipLaunchKernelGGL((jacobi_bwd_input_kernel<IO, true>), dim3(B), dim3(256), lds, st, (const IO*)gout, a_row, b_col,
                           (IO*)gu, H, W, nt, (const IO*)gtraj, em);
    else
        hipLaunchKernelGGL((jacobi_bwd_input_kernel<IO, false>), dim3(B), dim3(256), lds, st, (const IO*)gout, a_row, b_col,
                           (IO*)gu, H, W, nt, (const IO*)nullptr, em);
    return check_launch();
}

extern "C" {

int pde_jacobi_io_backward_input(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype, const void* gout,
                                 const float* a_row, const float* b_col, void* gu, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    return pde_jacobi_io_backward_input_states(B, H, W, nt, io_dtype, gout, nullptr, nullptr, a_row, b_col, gu, workspace,
                                               workspace_bytes, stream);
}

int pde_jacobi_io_backward_input_states(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype, const void* gout,
                                        const void* gstates, const uint64_t emit_mask[2], const float* a_row,
                                        const float* b_col, void* gu, void* workspace, size_t workspace_bytes, void* stream) {
    const int path = jacobi_path(H, W);
    if (B <= 0 || path == 0 || nt < 0 || !gout || !a_row || !b_col || !gu) return PDE_E_BADARG;
    if (io_dtype != PDE_IO_F32 && io_dtype != PDE_IO_BF16 && io_dtype != PDE_IO_F16) return PDE_E_BADARG;
    if (misaligned(io_elem_bytes(io_dtype), gout, gstates, gu) || misaligned(4, a_row, b_col)) return PDE_E_BADARG;
    EmitMask em;
    const int erc = emit_check(emit_mask, nt, gstates, em);
    if (erc != PDE_OK) return erc;
    const size_t need = pde_jacobi_io_backward_input_workspace_bytes(B, H, W, nt, io_dtype);
    if ((need && (!workspace || workspace_bytes < need)) || misaligned(kVecAlign, workspace)) return PDE_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (path == 2 && !jacobi_tiled_grid_ok(B, H, W)) return PDE_E_BADARG;
    if (io_dtype == PDE_IO_F32)
        return jacobi_backward_input_io<float>(path, B, H, W, nt, gout, a_row, b_col, gu, workspace, gstates, em, st);
    if (io_dtype == PDE_IO_BF16)
        return jacobi_backward_input_io<bf16e>(path, B, H, W, nt, gout, a_row, b_col, gu, workspace, gstates, em, st);
    return jacobi_backward_input_io<f16e>(path, B, H, W, nt, gout, a_row, b_col, gu, workspace, gstates, em, st);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------
// the tangent-linear pass (pdecnn_explicit_tangent.h): (y, dy) from (u, du) and the parameter tangents
// ---------------------------------------------------------------------------------------
namespace {

// one step of the generic-size path: T at the call's first load and last store, fp32 images between the steps
template <typename TI, typename TO>
void ex_tangent(const ExArgs& a, const float* d_alpha, const float* d_scale, const void* src, const void* dsrc, void* dst,
                void* ddst, int has_src, hipStream_t st) {
    if (a.W % 4)
        hipLaunchKernelGGL((explicit5_tangent_col_kernel<TI, TO>), dim3(a.nplanes), dim3(256), 0, st, (const TI*)src,
                           (const TI*)dsrc, a.alpha, a.scale, d_alpha, d_scale, (TO*)dst, (TO*)ddst, a.C, a.H, a.W, a.dt, a.eps,
                           a.maxc, a.relax, has_src);
    else
        hipLaunchKernelGGL((explicit5_tangent_kernel<TI, TO>), dim3(a.nplanes), dim3(256), 0, st, (const TI*)src,
                           (const TI*)dsrc, a.alpha, a.scale, d_alpha, d_scale, (TO*)dst, (TO*)ddst, a.C, a.H, a.W, a.dt, a.eps,
                           a.maxc, a.relax, has_src);
}
template <typename T>
void ex_tangent_step(const ExArgs& a, const float* d_alpha, const float* d_scale, bool first, bool last, const void* src,
                     const void* dsrc, void* dst, void* ddst, int has_src, hipStream_t st) {
    if (first && last) ex_tangent<T, T>(a, d_alpha, d_scale, src, dsrc, dst, ddst, has_src, st);
    else if (first) ex_tangent<T, float>(a, d_alpha, d_scale, src, dsrc, dst, ddst, has_src, st);
    else if (last) ex_tangent<float, T>(a, d_alpha, d_scale, src, dsrc, dst, ddst, has_src, st);
    else ex_tangent<float, float>(a, d_alpha, d_scale, src, dsrc, dst, ddst, has_src, st);
}

size_t jacobi_tangent_lds(int H, int W) { return (4 * (size_t)(H + 2) * (W + 2) + 2 * (size_t)(H + W)) * sizeof(float); }

template <typename IO>
int jacobi_tangent_io(int path, int B, int H, int W, int nt, const void* u, const void* du, const float* a_row,
                      const float* b_col, const float* d_a_row, const float* d_b_col, void* y, void* dy, void* workspace,
                      hipStream_t st) {
    const int has_src = (d_a_row || d_b_col) ? 1 : 0;
    static unsigned long long configured = 0, configured_tiled = 0;
    if (path == 1) {
        if (ensure_dynamic_lds(reinterpret_cast<const void*>(jacobi_tangent_kernel<IO>), (int)jacobi_tangent_lds(kJMax, kJMax),
                               configured) != PDE_OK)
            return PDE_E_LAUNCH;
        hipLaunchKernelGGL((jacobi_tangent_kernel<IO>), dim3(B), dim3(256), jacobi_tangent_lds(H, W), st, (const IO*)u,
                           (const IO*)du, a_row, b_col, d_a_row, d_b_col, (IO*)y, (IO*)dy, H, W, nt, has_src);
        return check_launch();
    }
    const size_t lds = kJTanFloats * sizeof(float);
    if (ensure_dynamic_lds(reinterpret_cast<const void*>(jacobi_tiled_tangent_kernel<IO>), (int)lds, configured_tiled) != PDE_OK)
        return PDE_E_LAUNCH;
    const int nTy = jtiles(H), nTx = jtiles(W);
    const dim3 grid((unsigned)((size_t)B * nTy * nTx));
    // the launches hand P and dP on through two fp32 images each: P0, P1, dP0, dP1
    const size_t ib = align256((size_t)B * H * W * sizeof(float));
    char* base = static_cast<char*>(workspace);
    float* img[2] = {reinterpret_cast<float*>(base), base ? reinterpret_cast<float*>(base + ib) : nullptr};
    float* dimg[2] = {base ? reinterpret_cast<float*>(base + 2 * ib) : nullptr,
                      base ? reinterpret_cast<float*>(base + 3 * ib) : nullptr};
    int n0 = 0, l = 0;
    do {                                                    // nt = 0: one launch of no steps copies
        const int k = nt - n0 < kJTanK ? nt - n0 : kJTanK;
        const bool last = n0 + k == nt;
        hipLaunchKernelGGL((jacobi_tiled_tangent_kernel<IO>), grid, dim3(256), lds, st, (const IO*)u, (const IO*)du,
                           l == 0 ? (const float*)nullptr : (const float*)img[(l - 1) & 1],
                           l == 0 ? (const float*)nullptr : (const float*)dimg[(l - 1) & 1], a_row, b_col, d_a_row, d_b_col,
                           last ? y : (void*)img[l & 1], last ? dy : (void*)dimg[l & 1], last ? 0 : 1, H, W, nTy, nTx, k,
                           has_src);
        n0 += k;
        ++l;
    } while (n0 < nt);
    return check_launch();
}

}  // namespace

extern "C" {

size_t pde_explicit5_tangent_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype,
                                             int32_t num_steps) {
    if (io_dtype != PDE_IO_F32 && io_dtype != PDE_IO_BF16 && io_dtype != PDE_IO_F16) return 0;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_steps < 2 || wave_plane_ok(H, W)) return 0;
    return 4 * align256((size_t)B * C * H * W * sizeof(float));     // generic sizes: u and du ping-pong through two images each
}

int pde_explicit5_tangent(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype, const void* u, const void* du,
                          const float* alpha_base, const float* channel_scaling, const float* d_alpha_base,
                          const float* d_channel_scaling, float dt, float eps, float max_coeff, float relax,
                          int32_t num_steps, void* y, void* dy, void* workspace, size_t workspace_bytes, void* stream) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_steps < 1 || !u || !alpha_base || !channel_scaling || !dy)
        return PDE_E_BADARG;
    if (!du && !d_alpha_base && !d_channel_scaling) return PDE_E_BADARG;       // nothing to differentiate: call the forward
    if (io_dtype != PDE_IO_F32 && io_dtype != PDE_IO_BF16 && io_dtype != PDE_IO_F16) return PDE_E_BADARG;
    if (misaligned(ex_tensor_align(W, io_dtype), u, du, y, dy) ||
        misaligned(4, alpha_base, channel_scaling, d_alpha_base, d_channel_scaling))
        return PDE_E_BADARG;
    // the four images are read and written as float4 on the generic float4 path
    const size_t need = pde_explicit5_tangent_workspace_bytes(B, C, H, W, io_dtype, num_steps);
    if ((need && (!workspace || workspace_bytes < need)) || misaligned(kVecAlign, workspace)) return PDE_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nplanes = B * C;
    const int has_src = (d_alpha_base || d_channel_scaling) ? 1 : 0;
    if (wave_plane_ok(H, W)) {                             // both planes stay in registers over all steps
        if (io_dtype == PDE_IO_F32)
            tangent_wave_io<float>(H, u, du, alpha_base, channel_scaling, d_alpha_base, d_channel_scaling, y, dy, nplanes, C,
                                   num_steps, dt, eps, max_coeff, relax, has_src, st);
        else if (io_dtype == PDE_IO_F16)
            tangent_wave_io<f16e>(H, u, du, alpha_base, channel_scaling, d_alpha_base, d_channel_scaling, y, dy, nplanes, C,
                                  num_steps, dt, eps, max_coeff, relax, has_src, st);
        else
            tangent_wave_io<bf16e>(H, u, du, alpha_base, channel_scaling, d_alpha_base, d_channel_scaling, y, dy, nplanes, C,
                                   num_steps, dt, eps, max_coeff, relax, has_src, st);
        return check_launch();
    }
    const size_t ib = align256((size_t)nplanes * H * W * sizeof(float));
    char* base = static_cast<char*>(workspace);
    float* img[2] = {need ? reinterpret_cast<float*>(base) : nullptr, need ? reinterpret_cast<float*>(base + ib) : nullptr};
    float* dimg[2] = {need ? reinterpret_cast<float*>(base + 2 * ib) : nullptr,
                      need ? reinterpret_cast<float*>(base + 3 * ib) : nullptr};
    const ExArgs ea{alpha_base, channel_scaling, nplanes, C, H, W, dt, eps, max_coeff, relax};
    for (int k = 0; k < num_steps; ++k) {
        const bool first = k == 0, last = k == num_steps - 1;
        const void* src = first ? u : static_cast<const void*>(img[(k - 1) & 1]);
        const void* dsrc = first ? du : static_cast<const void*>(dimg[(k - 1) & 1]);
        void* dst = last ? y : static_cast<void*>(img[k & 1]);
        void* ddst = last ? dy : static_cast<void*>(dimg[k & 1]);
        if (io_dtype == PDE_IO_F32)
            ex_tangent_step<float>(ea, d_alpha_base, d_channel_scaling, first, last, src, dsrc, dst, ddst, has_src, st);
        else if (io_dtype == PDE_IO_F16)
            ex_tangent_step<f16e>(ea, d_alpha_base, d_channel_scaling, first, last, src, dsrc, dst, ddst, has_src, st);
        else
            ex_tangent_step<bf16e>(ea, d_alpha_base, d_channel_scaling, first, last, src, dsrc, dst, ddst, has_src, st);
    }
    return check_launch();
}

size_t pde_jacobi_io_tangent_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype) {
    if (io_dtype != PDE_IO_F32 && io_dtype != PDE_IO_BF16 && io_dtype != PDE_IO_F16) return 0;
    if (B <= 0 || nt <= kJTanK || jacobi_path(H, W) != 2 || !jacobi_tiled_grid_ok(B, H, W)) return 0;
    return 4 * align256((size_t)B * H * W * sizeof(float));         // P and dP, two fp32 images each, for the launches to alternate between
}

int pde_jacobi_io_tangent(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype, const void* u, const void* du,
                          const float* a_row, const float* b_col, const float* d_a_row, const float* d_b_col, void* y,
                          void* dy, void* workspace, size_t workspace_bytes, void* stream) {
    const int path = jacobi_path(H, W);
    if (B <= 0 || path == 0 || nt < 0 || !u || !a_row || !b_col || !dy) return PDE_E_BADARG;
    if (!du && !d_a_row && !d_b_col) return PDE_E_BADARG;                     // nothing to differentiate: call the forward
    if (io_dtype != PDE_IO_F32 && io_dtype != PDE_IO_BF16 && io_dtype != PDE_IO_F16) return PDE_E_BADARG;
    if (misaligned(io_elem_bytes(io_dtype), u, du, y, dy) || misaligned(4, a_row, b_col, d_a_row, d_b_col)) return PDE_E_BADARG;
    if (misaligned(kVecAlign, workspace)) return PDE_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (path == 2) {
        if (!jacobi_tiled_grid_ok(B, H, W)) return PDE_E_BADARG;
        const size_t need = pde_jacobi_io_tangent_workspace_bytes(B, H, W, nt, io_dtype);
        if (need && (!workspace || workspace_bytes < need)) return PDE_E_WORKSPACE;
    }
    if (io_dtype == PDE_IO_F32)
        return jacobi_tangent_io<float>(path, B, H, W, nt, u, du, a_row, b_col, d_a_row, d_b_col, y, dy, workspace, st);
    if (io_dtype == PDE_IO_BF16)
        return jacobi_tangent_io<bf16e>(path, B, H, W, nt, u, du, a_row, b_col, d_a_row, d_b_col, y, dy, workspace, st);
    return jacobi_tangent_io<f16e>(path, B, H, W, nt, u, du, a_row, b_col, d_a_row, d_b_col, y, dy, workspace, st);
}

}  // extern "C"
