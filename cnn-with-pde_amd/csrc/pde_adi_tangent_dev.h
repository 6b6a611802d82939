// Device code of the tangent-linear pass on the fused two-sided solver (include/pdecnn_tangent_fused.h): included by
// pde_adi_tangent_inst.hip once per line length N, and by pde_adi.hip for the argument structures.
//
// adi_factor_tangent_kernel<N>  d(coeff) of every (sweep, channel) from the four parameter tangents, one image per record
//                               in the line layout of that sweep (what E and INV of the primal record have)
// adi_tangent_kernel<N, J, IO>  the fused forward's layout with two planes per plane: lane (hf, l) keeps its half of line l
//                               of the primal x AND of the tangent dx in VGPRs for the whole schedule
//
// Per sweep and line the forward solves (A(co) + eps I) x = d; the tangent of that is the same operator on
//     d(dx) + dco_k (x_{k-1} - m_k x_k + x_{k+1})        x: the sweep's SOLVED line, m = 1 at a line's two ends, 2 inside
// so a sweep is: solve x (the forward's own solve_fwd_rows: y has the fused forward's bits), add the source term to dx,
// solve dx with the same rows.  A y sweep re-lays out both planes, before and after.
//
// Schedule: the forward's barrier-per-sweep one with the axis read from the sweep table (kSplitAny's way), WITHOUT the
// phase skew: every wave runs sweep t out of ring slot t % kRing while its pieces of record t + 1 arrive by LDS-DMA, one
// barrier per sweep.  A launch of at most kRing sweeps keeps all its records resident and has no barrier per sweep.
//
// LDS and registers (profiles/tangent_fused_kernel_resources.txt):
//   ring      kRing = 3 slots of the forward window [INV|JN|E] (10 KB, whole 1-KB DMA pieces) ............ 30 KB
//   dco ring  kRing slots of ONE image, 4608 B each — not padded to 5 KB: the image is 18 pieces of 256 B, brought in
//             with the 4-byte-per-lane form of the DMA, so no piece is partial and no lane is masked ......... 13.5 KB
//   images    one 4.5 KB re-layout image per wave .................................................................... 36 KB
//   79.5 KB: two workgroups share a CU's 160 KB, as in the forward.  Launches without a parameter tangent (PAR = false)
//   leave the dco ring out (66 KB).
//   J = kJTan = 2 planes per lane: x and dx are 4 x 16 = 64 VGPRs at N = 32, the rows of the sweep 33 more.
#pragma once
#include "pde_adi_dev.h"
#include "pde_adi_factor.h"

namespace pde {
namespace {

#ifndef PDE_JT
#define PDE_JT 2
#endif
constexpr int kJTan = PDE_JT;                    // planes per lane (of x, and as many of dx)
constexpr int kDcoStride = kImage;               // floats per (sweep, channel) dco record: one line image
constexpr int kDcoPieces = kDcoStride / 64;      // 256-byte DMA pieces per record
static_assert(kDcoStride % 64 == 0, "the dco image is a whole number of 256-byte pieces");

struct FactorTangentArgs {
    FactorArgs f;                                // the primal call's own: parameters, schedule, clamp, smoothing
    const float *dab, *dbb, *das, *dbs;          // each nullptr (zero) | [C][N][N]
    float* dco;                                  // [S][C][kDcoStride]
};

// Grid and thread mapping of adi_factor_kernel: one thread per (sweep, channel, half line), one wave per channel.
//   dco = ((smooth3(pass . (dbase + dslope t))) delta) / h2
// pass: clamp_theta's own comparison on base + slope t (the record's MASKX image is in row layout and does not serve a
// y sweep's lines); the 3-tap association and the order of delta and h2 are the primal's.
template <int N>
__global__ __launch_bounds__(128) void adi_factor_tangent_kernel(FactorTangentArgs a) {
    constexpr int m = N / 2;
    __shared__ float psm[2 * kFacLd * PDE_MAX_N];                           // per wave: the plane of pass . (dbase + dslope t)
    __shared__ __attribute__((aligned(16))) float rsm[2 * kDcoStride];      // per wave: the image, assembled before it is stored
    const FactorArgs& f = a.f;
    const int pairs = (f.C + 1) / 2;
    const int s = blockIdx.x / pairs;
    const int wv = threadIdx.x >> 6;
    const int c = 2 * (blockIdx.x % pairs) + wv;
    if (c >= f.C) return;                                                   // wave-uniform; the waves never meet
    const int hf = (threadIdx.x >> 5) & 1, line = threadIdx.x & 31, wl = threadIdx.x & 63;
    const PdeSweep sw = f.sweep[s];
    const bool xax = sw.axis == PDE_AXIS_X;
    const float* base = xax ? f.ab : f.bb;
    const float* slope = xax ? f.as : f.bs;
    const float* dbase = xax ? a.dab : a.dbb;
    const float* dslope = xax ? a.das : a.dbs;
    const size_t cbase = (size_t)c * N * N;
    float* P = psm + wv * (kFacLd * PDE_MAX_N);
    {
        const float4* b4 = reinterpret_cast<const float4*>(base + cbase);
        const float4* s4 = reinterpret_cast<const float4*>(slope + cbase);
        const float4* db4 = dbase ? reinterpret_cast<const float4*>(dbase + cbase) : nullptr;
        const float4* ds4 = dslope ? reinterpret_cast<const float4*>(dslope + cbase) : nullptr;
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int q4 = wl; q4 < N * N / 4; q4 += 64) {
            const float4 bv = b4[q4], sv = s4[q4];
            const float4 dbv = db4 ? db4[q4] : zero4, dsv = ds4 ? ds4[q4] : zero4;
            const int hh = (4 * q4) / N, ww = (4 * q4) % N;
            const float bb[4] = {bv.x, bv.y, bv.z, bv.w}, ss[4] = {sv.x, sv.y, sv.z, sv.w};
            const float dbb[4] = {dbv.x, dbv.y, dbv.z, dbv.w}, dss[4] = {dsv.x, dsv.y, dsv.z, dsv.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                bool ps;
                (void)clamp_theta(bb[q] + ss[q] * sw.t, f, ps);
                P[hh * kFacLd + ww + q] = ps ? dbb[q] + dss[q] * sw.t : 0.f;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    const bool idle = line >= N;
    const int ln = idle ? N - 1 : line;
    // my unknowns: k = 0..m-1 at global index i(k) = hf ? N-1-k : k, and one step beyond my inner end for the smoothing
    float p[m + 1];
#pragma unroll
    for (int k = 0; k <= m; ++k) {
        const int i = hf ? N - 1 - k : k;
        p[k] = P[xax ? ln * kFacLd + i : i * kFacLd + ln];
    }
    const float third = 1.0f / 3.0f;
    float dco[m];
#pragma unroll
    for (int k = 0; k < m; ++k) {
        float v = p[k];
        if (f.smooth3) {
            const float outer = p[k > 0 ? k - 1 : 0];                       // towards my end (replicated at k = 0)
            const float inner = p[k + 1];
            const float prev = hf ? inner : outer, nxt = hf ? outer : inner;   // in increasing global index
            v = (prev * third + p[k] * third) + nxt * third;
        }
        dco[k] = idle ? 0.f : (v * sw.delta) / sw.h2;
    }
    float* rec = rsm + wv * kDcoStride;
    store_half_row<N>(rec + line * kLineStride, hf, dco);
    __builtin_amdgcn_wave_barrier();
    const float4* src = reinterpret_cast<const float4*>(rec);
    float4* dst = reinterpret_cast<float4*>(a.dco + ((size_t)s * f.C + c) * kDcoStride);
    for (int q4 = wl; q4 < kDcoStride / 4; q4 += 64) dst[q4] = src[q4];
}

struct TangentArgs {
    const void* u;          // primal input
    const void* du;         // its tangent; nullptr: zero
    void* y;                // primal output; nullptr: not stored
    void* dy;               // tangent output
    const float* coef;      // [S][C][kRecStride], the fused forward's records
    const float* dco;       // [S][C][kDcoStride]; read by the PAR kernels only
    const SweepTab* tab;
    int B, C, S, G;
    int xcd_map;
};

// 4 bytes per lane, global -> LDS (LDS address = wave-uniform base + 4*lane): lds_dma16_a's narrow twin, for images
// that are a whole number of 256-byte pieces but not of 1-KB ones
__device__ __forceinline__ void lds_dma4_a(const float* sbase, unsigned voff, unsigned lds_bytes) {
    const unsigned lds = __builtin_amdgcn_readfirstlane(lds_bytes);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2" ::"s"(lds), "v"(voff), "s"(sbase) : "memory");
}

// dx_k += dco_k (x_{k-1} - m_k x_k + x_{k+1}) on the J planes of a lane; x is the solved line.  k = 0 is my end of the
// line (m = 1, no outer neighbour); the inner neighbour of k = M-1 is the partner half's k = M-1.
template <int M, int J>
__device__ __forceinline__ void tangent_source(const typename Pack<J>::P (&x)[M], typename Pack<J>::P (&dx)[M],
                                               const float* drow, int hf) {
    using P = typename Pack<J>::P;
    const P xin = pk_map(x[M - 1], [&](float z) { return xchg_half(z, hf); });
    // the dco half row four values at a time, each quarter consumed before the next is requested: with the whole half row
    // in flight beside x, dx and the sweep's rows the N = 32 kernels spill
    sfor<0, (M + 3) / 4>([&](auto IC) __attribute__((always_inline)) {
        constexpr int i = decltype(IC)::value;
        const float4 d4 = *reinterpret_cast<const float4*>(drow + 4 * i);
        const float dc[4] = {d4.x, d4.y, d4.z, d4.w};
        sfor<0, 4>([&](auto QC) __attribute__((always_inline)) {
            constexpr int k = 4 * i + decltype(QC)::value;
            if constexpr (k < M) {
                P lap;
                if constexpr (k == 0) lap = x[1] - x[0];
                else if constexpr (k == M - 1) lap = pk_fma(pk_bc<P>(-2.0f), x[k], x[k - 1] + xin);
                else lap = pk_fma(pk_bc<P>(-2.0f), x[k], x[k - 1] + x[k + 1]);
                dx[k] = pk_fma(pk_bc<P>(dc[decltype(QC)::value]), lap, dx[k]);
            }
        });
        asm volatile("" ::: "memory");
    });
}

// PAR: a parameter carries a tangent (source term, dco staging); without it dy is the fused forward at du, bit for bit
template <int N, int J, typename IO, bool PAR>
__global__ __launch_bounds__(kThreads, (kWaves == 8 ? 4 : 1)) void adi_tangent_kernel(TangentArgs a) {
    constexpr int M = Geo<N>::M;
    using P = typename Pack<J>::P;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* cbuf = smem;                                   // [kRing][kRecFwdPad]
    float* tbuf = smem + kRing * kRecFwdPad;              // [kWaves][kImage]
    float* dbuf = tbuf + kWaves * kImage;                 // PAR: [kRing][kDcoStride]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hf = lane >> 5, l = lane & 31;
    int c, g;
    block_to_work(blockIdx.x, a.C, a.G, a.xcd_map, c, g);
    float* T = tbuf + wave * kImage;
    const IO* u = static_cast<const IO*>(a.u);
    const IO* du = static_cast<const IO*>(a.du);
    IO* y = static_cast<IO*>(a.y);
    IO* dy = static_cast<IO*>(a.dy);
    const ConstTab tab = as_const(a.tab);
    constexpr int PPI = kWaves * J;                       // planes (of x, and of dx) per workgroup iteration
    const int nchunk = (a.B + PPI - 1) / PPI;
    const bool resident = a.S <= kRing;
    young_half_priority(wave);

    // rows >= N of the wave images are never written: zero them once so idle lanes read zeros
    for (int e = tid; e < kWaves * kImage; e += kThreads) tbuf[e] = 0.f;

    // Wave w brings pieces w, w + kWaves, ... of a record (see adi_fwd_kernel), and of its dco image
    constexpr int PPRF = kRecFwdPad / 256;                // 1-KB pieces per forward window
    static_assert(kG_Inv + kRecFwdPad <= kRecStride, "the padded forward window must stay inside the record");
    const float* dma_src0 = uniform_ptr(a.coef + (size_t)c * kRecStride + kG_Inv + wave * 256);
    const unsigned dma_step = (unsigned)a.C * kRecStride;
    const unsigned dma_lds0 = lds_byte_address(cbuf) + wave * 1024u;
    const unsigned dma_voff = 16u * lane;
    const float* dco_src0 = PAR ? uniform_ptr(a.dco + (size_t)c * kDcoStride + wave * 64) : nullptr;
    const unsigned dco_step = (unsigned)a.C * kDcoStride;
    const unsigned dco_lds0 = lds_byte_address(dbuf) + wave * 256u;
    const unsigned dco_voff = 4u * lane;
    auto dma_rec = [&](int slot, int s) __attribute__((always_inline)) {
        const float* src = dma_src0 + (size_t)((unsigned)s * dma_step);
        const unsigned dst = dma_lds0 + (unsigned)slot * (kRecFwdPad * 4u);
#pragma unroll
        for (int i = 0; i < (PPRF + kWaves - 1) / kWaves; ++i) {
            if ((i + 1) * kWaves <= PPRF || wave + i * kWaves < PPRF)
                lds_dma16_a(src + i * kWaves * 256, dma_voff, dst + i * kWaves * 1024u);
        }
        if constexpr (PAR) {
            const float* dsrc = dco_src0 + (size_t)((unsigned)s * dco_step);
            const unsigned ddst = dco_lds0 + (unsigned)slot * (kDcoStride * 4u);
#pragma unroll
            for (int i = 0; i < (kDcoPieces + kWaves - 1) / kWaves; ++i) {
                if ((i + 1) * kWaves <= kDcoPieces || wave + i * kWaves < kDcoPieces)
                    lds_dma4_a(dsrc + i * kWaves * 64, dco_voff, ddst + i * kWaves * 256u);
            }
        }
    };
    if (resident) {
        for (int s = 0; s < a.S; ++s) dma_rec(s, s);
    } else {
        dma_rec(0, 0);
    }
    dma_wait_all();
    __syncthreads();

    int cur = 0;                                          // ring slot of the current sweep
    for (int q = g; q < nchunk; q += a.G) {
        P x[M], dx[M];
        load_planes_seq<N, J, IO>(u, q, wave, lane, l, hf, a.B, a.C, c, T, x);
        if (du != nullptr) {
            load_planes_seq<N, J, IO>(du, q, wave, lane, l, hf, a.B, a.C, c, T, dx);
        } else {
#pragma unroll
            for (int k = 0; k < M; ++k) dx[k] = pk_bc<P>(0.f);
        }
        for (int s = 0; s < a.S; ++s) {
            if (!resident) {                              // the next sweep's record (of the next chunk after the last)
                const int sp = (s + 1 < a.S) ? s + 1 : 0;
                dma_rec(cur == kRing - 1 ? 0 : cur + 1, sp);
            }
            const int slot = resident ? s : cur;
            const float* rec = cbuf + slot * kRecFwdPad;
            const int axs = tab->axis[s];
            if (axs == PDE_AXIS_Y) {
                relayout_all<N, J>(x, T, l, hf);
                relayout_all<N, J>(dx, T, l, hf);
            }
            float ce[M], cinv[M], cjn;
            load_fwd_rows<M>(rec, l, hf, ce, cinv, cjn);
            solve_fwd_rows<M, J>(x, ce, cinv, cjn, hf);
            if constexpr (PAR) {
                tangent_source<M, J>(x, dx, dbuf + slot * kDcoStride + l * kLineStride + hf * kHalfPad, hf);
                // N = 32: x, dx, both row sets and the source term's temporaries do not fit 128 VGPRs (7 spilled).  The
                // elimination alone reads INV, so its half row is read again behind the source term (tangent_source ends
                // on a compiler fence) instead of being kept alive across it: 16 more LDS dwords per sweep, no scratch
                if constexpr (N == 32) load_half<M>(rec + kF_Inv + l * kLineStride + hf * kHalfPad, cinv);
            }
            solve_fwd_rows<M, J>(dx, ce, cinv, cjn, hf);
            if (axs == PDE_AXIS_Y) {
                relayout_all<N, J>(x, T, l, hf);
                relayout_all<N, J>(dx, T, l, hf);
            }
            if (!resident) {
                dma_wait_all();                           // my pieces of the next record have landed
                __syncthreads();
                cur = (cur == kRing - 1) ? 0 : cur + 1;
            }
        }
        if (y != nullptr) store_planes<N, J, IO>(y, q, wave, lane, l, hf, a.B, a.C, c, T, x);
        store_planes<N, J, IO>(dy, q, wave, lane, l, hf, a.B, a.C, c, T, dx);
    }
}

}  // namespace
}  // namespace pde
