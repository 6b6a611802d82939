// Tiled Jacobi kernels (emotion_recognition.PDELayer on planes larger than 64x64).  Included by pde_explicit.hip inside
// its anonymous namespace, after S1<IO>, reflect_src and the one-workgroup Jacobi kernels, which stay as they are.
//
// Coordinates are those of the reflect-padded plane, (H+2) x (W+2): cells 1..H x 1..W are the interior, the ring
// (row 0, row H+1, column 0, column W+1) keeps the values it got from u for the whole time loop.
//
// A workgroup owns one tile of one sample: kJT x kJT interior cells; the first and last tile of a dimension also own
// that side's ring cell.  For a launch of k <= kJK steps it loads the tile plus k cells on every side ("region"),
// clipped at the plane's edge, where the frozen ring ends the dependence.  Step s is computed on the region shrunk by
// s on every side that was not clipped, so after k steps exactly tile + 0 is left valid.  Two LDS images ping-pong.
//
// Thread (tx, ty) = (lane & 31, thread >> 5): a wave covers two rows of 32 consecutive columns.  With a row stride of
// kJS = 96 floats (= 32 mod 64 banks) the two rows fall on the two halves of the 64 banks: the centre, east/west and
// north/south reads are all conflict-free, and no per-cell division is needed.
//
// forward   u -> [k steps] -> fp32 image -> [k steps] -> ... -> out; with `park`, the state after every step goes to
//           the workspace instead (interior only, fp32): that is the input of the next step, which the adjoint needs.
// adjoint   G_nt = gout (zero ring).  One launch takes G_{n_hi} on tile + k and leaves G_{n_hi-k} on the tile, ring
//           cells included (they accumulate adjoint from their interior neighbours at every step).  At step n it stages
//           P_n on tile + 1 from the parked states (n = 0: from u) and adds G_{n+1} d1(P_n), G_{n+1} d2(P_n) over the
//           tile's own cells into per-thread registers; at the end of the launch the registers are summed per row and
//           per column in a fixed order into the tile's slot of `part`.  Launches chain through padded fp32 images.
// adjoint for the input alone (jacobi_tiled_bwd_input_kernel): the adjoint above without P_n and without the sums —
//           no parked state is read, so no forward launch precedes it; the same chain of padded images, the same fold.
// fold      gu = interior of G_0 + the ring folded back onto rows / columns 1 and H-2 / W-2 (a pass of its own: the
//           ring cell and the row it folds onto can lie in different tiles, e.g. H = 65).
// pgrad     g_a_row / g_b_col = sum of the tiles' slots over samples and tiles, in a fixed order.  No float atomics.
// trajectory (EMIT variants, pde_jacobi_io_*_states): the forward writes the tile's own cells of an emitted state to
//           traj[slot] in the tensors' type right after the step, where `park` writes; the adjoint adds gtraj[slot(n)] to
//           G_n as it computes it, on every interior cell of the region still valid at that step (ring cells get nothing),
//           so tiles agree on their shared halo cells exactly as they do without it and no launch is cut.

constexpr int kJT = 64;                     // tile edge, interior cells
constexpr int kJK = PDE_JACOBI_TILED_K;     // time steps per launch
constexpr int kJR = kJT + 2 * kJK;          // region edge, at most
constexpr int kJS = 96;                     // LDS row stride in floats
static_assert(kJR <= kJS && (kJS % 64) == 32, "a wave's two rows must fall on disjoint banks");
constexpr int kJFwdFloats = 2 * kJR * kJS + 2 * kJR;                         // P, Q, a, b: 65184 B
constexpr int kJBwdFloats = 2 * kJR * kJS + (kJT + 2) * kJS + 2 * kJR;       // G, Gn, P_n on tile + 1, a, b: 90528 B
static_assert(kJFwdFloats * 4 <= 65536, "the forward's LDS is static");

struct JSpan {          // one dimension of a tile: region [lo, hi), own cells [olo, ohi) (ring included at the edges)
    int lo, hi, olo, ohi;
};
__host__ __device__ inline int jtiles(int n) { return (n + kJT - 1) / kJT; }
__device__ __forceinline__ JSpan jspan(int t, int nT, int n, int halo) {
    JSpan s;
    const int i0 = 1 + t * kJT;
    s.olo = t == 0 ? 0 : i0;
    s.ohi = t == nT - 1 ? n + 2 : i0 + kJT;
    s.lo = max(0, s.olo - halo);
    s.hi = min(n + 2, s.ohi + halo);
    return s;
}

// (EMIT: n0 = the time steps taken before this launch; traj_stride = B*H*W)
template <typename IO, bool EMIT = false>
__global__ __launch_bounds__(256) void jacobi_tiled_fwd_kernel(const IO* __restrict__ u, const float* __restrict__ fsrc,
                                                               const float* __restrict__ a_row,
                                                               const float* __restrict__ b_col, void* __restrict__ dst,
                                                               int dst_f32, float* __restrict__ park, size_t park_stride,
                                                               int H, int W, int nTy, int nTx, int k,
                                                               IO* __restrict__ traj, size_t traj_stride, EmitMask em, int n0) {
    __shared__ float sm[kJFwdFloats];
    float* P = sm;
    float* Q = sm + kJR * kJS;
    float* sa = sm + 2 * kJR * kJS;
    float* sb = sa + kJR;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    int bid = blockIdx.x;                                  // one division per workgroup, none per cell
    const int tX = bid % nTx;
    bid /= nTx;
    const int tY = bid % nTy;
    const size_t s = bid / nTy;
    const JSpan rs = jspan(tY, nTy, H, k), cs = jspan(tX, nTx, W, k);
    const size_t plane = (size_t)H * W;
    const IO* ub = u + s * plane;
    for (int e = threadIdx.x; e < rs.hi - rs.lo; e += 256) {
        const int i = rs.lo + e;
        sa[e] = (i >= 1 && i <= H) ? a_row[i - 1] : 0.f;
    }
    for (int e = threadIdx.x; e < cs.hi - cs.lo; e += 256) {
        const int j = cs.lo + e;
        sb[e] = (j >= 1 && j <= W) ? b_col[j - 1] : 0.f;
    }
    // the region: interior cells from the image this launch continues from, ring cells always from u (reflect)
    for (int i = rs.lo + ty; i < rs.hi; i += 8) {
        const bool ri = i >= 1 && i <= H;
        const size_t ro = (size_t)reflect_src(i, H) * W;
        for (int j = cs.lo + tx; j < cs.hi; j += 32) {
            const size_t off = ro + reflect_src(j, W);
            const float v = (fsrc && ri && j >= 1 && j <= W) ? fsrc[s * plane + off] : S1<IO>::ld(ub + off);
            const int l = (i - rs.lo) * kJS + (j - cs.lo);
            P[l] = v;
            Q[l] = v;                                      // the ring is never written again: both images hold it
        }
    }
    __syncthreads();
    const int oi0 = max(rs.olo, 1), oi1 = min(rs.ohi, H + 1), oj0 = max(cs.olo, 1), oj1 = min(cs.ohi, W + 1);
    for (int st = 1; st <= k; ++st) {
        const int r0 = max(rs.lo == 0 ? 0 : rs.lo + st, 1), r1 = min(rs.hi == H + 2 ? H + 2 : rs.hi - st, H + 1);
        const int c0 = max(cs.lo == 0 ? 0 : cs.lo + st, 1), c1 = min(cs.hi == W + 2 ? W + 2 : cs.hi - st, W + 1);
        for (int i = r0 + ty; i < r1; i += 8) {
            const float ai = sa[i - rs.lo];
            const float* p = P + (i - rs.lo) * kJS - cs.lo;
            float* q = Q + (i - rs.lo) * kJS - cs.lo;
            for (int j = c0 + tx; j < c1; j += 32) {
                const float v = p[j];
                const float d1 = p[j + kJS] - 2.f * v + p[j - kJS];
                const float d2 = p[j + 1] - 2.f * v + p[j - 1];
                q[j] = v + ai * d1 + sb[j - cs.lo] * d2;
            }
        }
        __syncthreads();
        float* t = P; P = Q; Q = t;
        if (park) {                                        // the state after step st = the input of the next step
            float* pk = park + (size_t)(st - 1) * park_stride + s * plane;
            for (int i = oi0 + ty; i < oi1; i += 8)
                for (int j = oj0 + tx; j < oj1; j += 32)
                    pk[(size_t)(i - 1) * W + (j - 1)] = P[(i - rs.lo) * kJS + (j - cs.lo)];
        }
        if constexpr (EMIT) {
            const int slot = emit_slot(em, n0 + st);
            if (slot >= 0) {
                IO* tp = traj + (size_t)slot * traj_stride + s * plane;
                for (int i = oi0 + ty; i < oi1; i += 8)
                    for (int j = oj0 + tx; j < oj1; j += 32)
                        S1<IO>::st(tp + (size_t)(i - 1) * W + (j - 1), P[(i - rs.lo) * kJS + (j - cs.lo)]);
            }
        }
    }
    if (!dst) return;
    for (int i = oi0 + ty; i < oi1; i += 8)
        for (int j = oj0 + tx; j < oj1; j += 32) {
            const float v = P[(i - rs.lo) * kJS + (j - cs.lo)];
            const size_t o = s * plane + (size_t)(i - 1) * W + (j - 1);
            if (dst_f32) static_cast<float*>(dst)[o] = v;
            else S1<IO>::st(static_cast<IO*>(dst) + o, v);
        }
}

// states: slot n-1 holds P_n (n >= 1), interior only; P_0 is u.  gout != nullptr: the launch that starts from G_nt.
template <typename IO, bool EMIT = false>
__global__ __launch_bounds__(256) void jacobi_tiled_bwd_kernel(const IO* __restrict__ u, const float* __restrict__ states,
                                                               size_t state_stride, const IO* __restrict__ gout,
                                                               const float* __restrict__ gsrc, float* __restrict__ gdst,
                                                               const float* __restrict__ a_row,
                                                               const float* __restrict__ b_col, float* __restrict__ part,
                                                               int acc, int H, int W, int nTy, int nTx, int n_hi, int k,
                                                               const IO* __restrict__ gtraj, EmitMask em) {
    extern __shared__ float smd[];
    float* G = smd;
    float* Gn = G + kJR * kJS;
    float* Pm = Gn + kJR * kJS;
    float* sa = Pm + (kJT + 2) * kJS;
    float* sb = sa + kJR;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int tile = blockIdx.x;
    int bid = tile;
    const int tX = bid % nTx;
    bid /= nTx;
    const int tY = bid % nTy;
    const size_t s = bid / nTy;
    const JSpan rs = jspan(tY, nTy, H, k), cs = jspan(tX, nTx, W, k);
    const int Wp = W + 2;
    const size_t plane = (size_t)H * W, pplane = (size_t)(H + 2) * Wp;
    const IO* ub = u + s * plane;
    for (int e = threadIdx.x; e < rs.hi - rs.lo; e += 256) {
        const int i = rs.lo + e;
        sa[e] = (i >= 1 && i <= H) ? a_row[i - 1] : 0.f;
    }
    for (int e = threadIdx.x; e < cs.hi - cs.lo; e += 256) {
        const int j = cs.lo + e;
        sb[e] = (j >= 1 && j <= W) ? b_col[j - 1] : 0.f;
    }
    for (int i = rs.lo + ty; i < rs.hi; i += 8) {
        const bool ri = i >= 1 && i <= H;
        for (int j = cs.lo + tx; j < cs.hi; j += 32) {
            float v;
            if (gout) v = (ri && j >= 1 && j <= W) ? S1<IO>::ld(gout + s * plane + (size_t)(i - 1) * W + (j - 1)) : 0.f;
            else v = gsrc[s * pplane + (size_t)i * Wp + j];
            G[(i - rs.lo) * kJS + (j - cs.lo)] = v;
        }
    }
    const int oi0 = max(rs.olo, 1), oi1 = min(rs.ohi, H + 1), oj0 = max(cs.olo, 1), oj1 = min(cs.ohi, W + 1);
    float accA[kJT / 8][kJT / 32], accB[kJT / 8][kJT / 32];
#pragma unroll
    for (int r = 0; r < kJT / 8; ++r)
#pragma unroll
        for (int c = 0; c < kJT / 32; ++c) accA[r][c] = accB[r][c] = 0.f;
    for (int st = 1; st <= k; ++st) {
        const int n = n_hi - st;                           // this step takes G_{n+1} to G_n and needs P_n
        const float* Pn = n > 0 ? states + (size_t)(n - 1) * state_stride + s * plane : nullptr;
        for (int i = oi0 - 1 + ty; i < oi1 + 1; i += 8) {
            const bool ri = i >= 1 && i <= H;
            const size_t ro = (size_t)reflect_src(i, H) * W;
            for (int j = oj0 - 1 + tx; j < oj1 + 1; j += 32) {
                const size_t off = ro + reflect_src(j, W);
                Pm[(i - oi0 + 1) * kJS + (j - oj0 + 1)] = (Pn && ri && j >= 1 && j <= W) ? Pn[off] : S1<IO>::ld(ub + off);
            }
        }
        __syncthreads();                                   // Pm staged; G complete (the load above, or the last step)
        // coefficient gradients over the tile's own cells: every cell of the plane is counted by exactly one tile
#pragma unroll
        for (int r = 0; r < kJT / 8; ++r) {
            const int i = oi0 + ty + 8 * r;
#pragma unroll
            for (int c = 0; c < kJT / 32; ++c) {
                const int j = oj0 + tx + 32 * c;
                if (i < oi1 && j < oj1) {
                    const float g = G[(i - rs.lo) * kJS + (j - cs.lo)];
                    const float* p = Pm + (i - oi0 + 1) * kJS + (j - oj0 + 1);
                    const float v = p[0];
                    accA[r][c] += g * (p[kJS] - 2.f * v + p[-kJS]);
                    accB[r][c] += g * (p[1] - 2.f * v + p[-1]);
                }
            }
        }
        // dL/dP_n from dL/dP_{n+1}; ring cells (clipped sides) are cells like any other here
        const int r0 = rs.lo == 0 ? 0 : rs.lo + st, r1 = rs.hi == H + 2 ? H + 2 : rs.hi - st;
        const int c0 = cs.lo == 0 ? 0 : cs.lo + st, c1 = cs.hi == W + 2 ? W + 2 : cs.hi - st;
        const IO* gt = nullptr;                            // dL/d(state after step n), where that state was emitted
        if constexpr (EMIT) {
            const int slot = emit_slot(em, n);
            if (slot >= 0) gt = gtraj + (size_t)slot * state_stride + s * plane;
        }
        for (int i = r0 + ty; i < r1; i += 8) {
            const bool ri = i >= 1 && i <= H;
            const bool up = i - 1 >= 1 && i - 1 <= H, dn = i + 1 >= 1 && i + 1 <= H;   // vertical neighbour is interior
            const float a0 = sa[i - rs.lo];
            const float aup = up ? sa[i - 1 - rs.lo] : 0.f, adn = dn ? sa[i + 1 - rs.lo] : 0.f;
            const float* grow = G + (i - rs.lo) * kJS - cs.lo;
            float* qrow = Gn + (i - rs.lo) * kJS - cs.lo;
            for (int j = c0 + tx; j < c1; j += 32) {
                const bool cj = j >= 1 && j <= W;
                const float* g = grow + j;
                float v = (ri && cj) ? (1.f - 2.f * a0 - 2.f * sb[j - cs.lo]) * g[0] : g[0];
                if (cj) {
                    if (up) v += aup * g[-kJS];
                    if (dn) v += adn * g[kJS];
                }
                if (ri) {
                    if (j - 1 >= 1 && j - 1 <= W) v += sb[j - 1 - cs.lo] * g[-1];
                    if (j + 1 >= 1 && j + 1 <= W) v += sb[j + 1 - cs.lo] * g[1];
                }
                if constexpr (EMIT) {
                    if (gt && ri && cj) v += S1<IO>::ld(gt + (size_t)(i - 1) * W + (j - 1));
                }
                qrow[j] = v;
            }
        }
        __syncthreads();
        float* t = G; G = Gn; Gn = t;
    }
    if (k == 0) __syncthreads();
    float* gd = gdst + s * pplane;
    for (int i = rs.olo + ty; i < rs.ohi; i += 8)
        for (int j = cs.olo + tx; j < cs.ohi; j += 32) gd[(size_t)i * Wp + j] = G[(i - rs.lo) * kJS + (j - cs.lo)];
    __syncthreads();
    // the per-thread sums -> one sum per own row and per own column, in a fixed order
    float* SA = G;                                         // [kJT][kJT + 1]
    float* SB = Gn;
#pragma unroll
    for (int r = 0; r < kJT / 8; ++r)
#pragma unroll
        for (int c = 0; c < kJT / 32; ++c) {
            SA[(ty + 8 * r) * (kJT + 1) + tx + 32 * c] = accA[r][c];
            SB[(ty + 8 * r) * (kJT + 1) + tx + 32 * c] = accB[r][c];
        }
    __syncthreads();
    if (threadIdx.x < 2 * kJT) {
        const int t = threadIdx.x & (kJT - 1);
        float sum = 0.f;
        if (threadIdx.x < kJT) for (int c = 0; c < kJT; ++c) sum += SA[t * (kJT + 1) + c];
        else for (int r = 0; r < kJT; ++r) sum += SB[r * (kJT + 1) + t];
        float* pp = part + (size_t)tile * (2 * kJT) + threadIdx.x;
        *pp = acc ? *pp + sum : sum;                       // launches of one call follow each other on the stream
    }
}

// The adjoint part of jacobi_tiled_bwd_kernel alone (pde_jacobi_io_backward_input[_states]: a_row and b_col take no
// gradient): no P_n staging, no per-thread row / column sums, no `part`.  G_{n_hi} on tile + k -> G_{n_hi-k} on the tile,
// every update written as it is there, so the padded G_0 — and the gu folded from it — has the same bits.  LDS: G, Gn,
// a, b, the forward's static size.
template <typename IO, bool EMIT = false>
__global__ __launch_bounds__(256) void jacobi_tiled_bwd_input_kernel(const IO* __restrict__ gout, const float* __restrict__ gsrc,
                                                                     float* __restrict__ gdst, const float* __restrict__ a_row,
                                                                     const float* __restrict__ b_col, size_t traj_stride,
                                                                     int H, int W, int nTy, int nTx, int n_hi, int k,
                                                                     const IO* __restrict__ gtraj, EmitMask em) {
    __shared__ float sm[kJFwdFloats];
    float* G = sm;
    float* Gn = sm + kJR * kJS;
    float* sa = sm + 2 * kJR * kJS;
    float* sb = sa + kJR;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    int bid = blockIdx.x;
    const int tX = bid % nTx;
    bid /= nTx;
    const int tY = bid % nTy;
    const size_t s = bid / nTy;
    const JSpan rs = jspan(tY, nTy, H, k), cs = jspan(tX, nTx, W, k);
    const int Wp = W + 2;
    const size_t plane = (size_t)H * W, pplane = (size_t)(H + 2) * Wp;
    for (int e = threadIdx.x; e < rs.hi - rs.lo; e += 256) {
        const int i = rs.lo + e;
        sa[e] = (i >= 1 && i <= H) ? a_row[i - 1] : 0.f;
    }
    for (int e = threadIdx.x; e < cs.hi - cs.lo; e += 256) {
        const int j = cs.lo + e;
        sb[e] = (j >= 1 && j <= W) ? b_col[j - 1] : 0.f;
    }
    for (int i = rs.lo + ty; i < rs.hi; i += 8) {
        const bool ri = i >= 1 && i <= H;
        for (int j = cs.lo + tx; j < cs.hi; j += 32) {
            float v;
            if (gout) v = (ri && j >= 1 && j <= W) ? S1<IO>::ld(gout + s * plane + (size_t)(i - 1) * W + (j - 1)) : 0.f;
            else v = gsrc[s * pplane + (size_t)i * Wp + j];
            G[(i - rs.lo) * kJS + (j - cs.lo)] = v;
        }
    }
    __syncthreads();
    for (int st = 1; st <= k; ++st) {
        const int n = n_hi - st;                           // this step takes G_{n+1} to G_n
        // dL/dP_n from dL/dP_{n+1}; ring cells (clipped sides) are cells like any other here
        const int r0 = rs.lo == 0 ? 0 : rs.lo + st, r1 = rs.hi == H + 2 ? H + 2 : rs.hi - st;
        const int c0 = cs.lo == 0 ? 0 : cs.lo + st, c1 = cs.hi == W + 2 ? W + 2 : cs.hi - st;
        const IO* gt = nullptr;                            // dL/d(state after step n), where that state was emitted
        if constexpr (EMIT) {
            const int slot = emit_slot(em, n);
            if (slot >= 0) gt = gtraj + (size_t)slot * traj_stride + s * plane;
        }
        for (int i = r0 + ty; i < r1; i += 8) {
            const bool ri = i >= 1 && i <= H;
            const bool up = i - 1 >= 1 && i - 1 <= H, dn = i + 1 >= 1 && i + 1 <= H;   // vertical neighbour is interior
            const float a0 = sa[i - rs.lo];
            const float aup = up ? sa[i - 1 - rs.lo] : 0.f, adn = dn ? sa[i + 1 - rs.lo] : 0.f;
            const float* grow = G + (i - rs.lo) * kJS - cs.lo;
            float* qrow = Gn + (i - rs.lo) * kJS - cs.lo;
            for (int j = c0 + tx; j < c1; j += 32) {
                const bool cj = j >= 1 && j <= W;
                const float* g = grow + j;
                float v = (ri && cj) ? (1.f - 2.f * a0 - 2.f * sb[j - cs.lo]) * g[0] : g[0];
                if (cj) {
                    if (up) v += aup * g[-kJS];
                    if (dn) v += adn * g[kJS];
                }
                if (ri) {
                    if (j - 1 >= 1 && j - 1 <= W) v += sb[j - 1 - cs.lo] * g[-1];
                    if (j + 1 >= 1 && j + 1 <= W) v += sb[j + 1 - cs.lo] * g[1];
                }
                if constexpr (EMIT) {
                    if (gt && ri && cj) v += S1<IO>::ld(gt + (size_t)(i - 1) * W + (j - 1));
                }
                qrow[j] = v;
            }
        }
        __syncthreads();
        float* t = G; G = Gn; Gn = t;
    }
    float* gd = gdst + s * pplane;
    for (int i = rs.olo + ty; i < rs.ohi; i += 8)
        for (int j = cs.olo + tx; j < cs.ohi; j += 32) gd[(size_t)i * Wp + j] = G[(i - rs.lo) * kJS + (j - cs.lo)];
}

// gu from the padded G_0: the adjoint of the reflect padding
template <typename IO>
__global__ __launch_bounds__(256) void jacobi_tiled_fold_kernel(const float* __restrict__ g0, IO* __restrict__ gu, int H,
                                                                int W, int nRb, int nCb) {
    int bid = blockIdx.x;
    const int cb = bid % nCb;
    bid /= nCb;
    const int rb = bid % nRb;
    const size_t s = bid / nRb;
    const int j = cb * 32 + (threadIdx.x & 31);
    const int Wp = W + 2;
    const float* g = g0 + s * (size_t)(H + 2) * Wp;
    if (j >= W) return;
    for (int i = rb * 32 + (threadIdx.x >> 5); i < min(rb * 32 + 32, H); i += 8) {
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
                v += g[(size_t)m * Wp + nn];
            }
        }
        S1<IO>::st(gu + s * (size_t)H * W + (size_t)i * W + j, v);
    }
}

__global__ void jacobi_tiled_pgrad_kernel(const float* __restrict__ part, float* __restrict__ ga, float* __restrict__ gb,
                                          int B, int H, int W, int nTy, int nTx) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= H + W) return;
    float sum = 0.f;
    if (r < H) {
        const int tY = r / kJT, l = r % kJT;
        for (int s = 0; s < B; ++s)
            for (int tX = 0; tX < nTx; ++tX) sum += part[(((size_t)s * nTy + tY) * nTx + tX) * (2 * kJT) + l];
        ga[r] = sum;
    } else {
        const int j = r - H, tX = j / kJT, l = j % kJT;
        for (int s = 0; s < B; ++s)
            for (int tY = 0; tY < nTy; ++tY) sum += part[(((size_t)s * nTy + tY) * nTx + tX) * (2 * kJT) + kJT + l];
        gb[j] = sum;
    }
}

// ---- tangent-linear pass (pdecnn_explicit_tangent.h: pde_jacobi_io_tangent on planes above 64x64) -----------------------
// jacobi_tiled_fwd_kernel with a second state: the same tiles, the same halo, the same shrinking region per step.  Four
// region images (P, Q, dP, dQ) and four coefficient vectors (a, b, da, db) fit one workgroup's LDS at the forward's own
// kJK steps per launch, so a launch of the tangent pass advances as many steps as one of the forward:
constexpr int kJTanK = kJK;                                              // time steps per launch of the tangent pass
constexpr int kJTanFloats = 4 * kJR * kJS + 4 * kJR;                     // P, Q, dP, dQ, a, b, da, db: 130368 B, dynamic
static_assert(kJTanK == kJK && kJTanFloats * 4 <= 160 * 1024, "one workgroup's LDS");
// Ring cells of P come from u and those of dP from du (zero when du is NULL) in every launch; interior cells from the
// fp32 images the launch continues from (fsrc / dfsrc; NULL: the first launch, from u / du).  dst NULL: y is not wanted
// (last launch only).  src == 0 (both coefficient tangents NULL): the source term is not added at all.
template <typename IO>
__global__ __launch_bounds__(256) void jacobi_tiled_tangent_kernel(const IO* __restrict__ u, const IO* __restrict__ du,
                                                                   const float* __restrict__ fsrc,
                                                                   const float* __restrict__ dfsrc,
                                                                   const float* __restrict__ a_row,
                                                                   const float* __restrict__ b_col,
                                                                   const float* __restrict__ d_a_row,
                                                                   const float* __restrict__ d_b_col, void* __restrict__ dst,
                                                                   void* __restrict__ ddst, int dst_f32, int H, int W,
                                                                   int nTy, int nTx, int k, int src) {
    extern __shared__ float smt[];
    float* P = smt;
    float* Q = P + kJR * kJS;
    float* dP = Q + kJR * kJS;
    float* dQ = dP + kJR * kJS;
    float* sa = dQ + kJR * kJS;
    float* sb = sa + kJR;
    float* sda = sb + kJR;
    float* sdb = sda + kJR;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    int bid = blockIdx.x;                                  // one division per workgroup, none per cell
    const int tX = bid % nTx;
    bid /= nTx;
    const int tY = bid % nTy;
    const size_t s = bid / nTy;
    const JSpan rs = jspan(tY, nTy, H, k), cs = jspan(tX, nTx, W, k);
    const size_t plane = (size_t)H * W;
    const IO* ub = u + s * plane;
    const IO* dub = du ? du + s * plane : nullptr;
    for (int e = threadIdx.x; e < rs.hi - rs.lo; e += 256) {
        const int i = rs.lo + e;
        const bool in = i >= 1 && i <= H;
        sa[e] = in ? a_row[i - 1] : 0.f;
        sda[e] = (in && d_a_row) ? d_a_row[i - 1] : 0.f;
    }
    for (int e = threadIdx.x; e < cs.hi - cs.lo; e += 256) {
        const int j = cs.lo + e;
        const bool in = j >= 1 && j <= W;
        sb[e] = in ? b_col[j - 1] : 0.f;
        sdb[e] = (in && d_b_col) ? d_b_col[j - 1] : 0.f;
    }
    for (int i = rs.lo + ty; i < rs.hi; i += 8) {
        const bool ri = i >= 1 && i <= H;
        const size_t ro = (size_t)reflect_src(i, H) * W;
        for (int j = cs.lo + tx; j < cs.hi; j += 32) {
            const size_t off = ro + reflect_src(j, W);
            const bool in = ri && j >= 1 && j <= W;
            const float v = (fsrc && in) ? fsrc[s * plane + off] : S1<IO>::ld(ub + off);
            const float dv = (dfsrc && in) ? dfsrc[s * plane + off] : (dub ? S1<IO>::ld(dub + off) : 0.f);
            const int l = (i - rs.lo) * kJS + (j - cs.lo);
            P[l] = v;
            Q[l] = v;                                      // the rings are never written again: both images hold them
            dP[l] = dv;
            dQ[l] = dv;
        }
    }
    __syncthreads();
    for (int st = 1; st <= k; ++st) {
        const int r0 = max(rs.lo == 0 ? 0 : rs.lo + st, 1), r1 = min(rs.hi == H + 2 ? H + 2 : rs.hi - st, H + 1);
        const int c0 = max(cs.lo == 0 ? 0 : cs.lo + st, 1), c1 = min(cs.hi == W + 2 ? W + 2 : cs.hi - st, W + 1);
        for (int i = r0 + ty; i < r1; i += 8) {
            const float ai = sa[i - rs.lo], dai = sda[i - rs.lo];
            const float* p = P + (i - rs.lo) * kJS - cs.lo;
            float* q = Q + (i - rs.lo) * kJS - cs.lo;
            const float* dp = dP + (i - rs.lo) * kJS - cs.lo;
            float* dq = dQ + (i - rs.lo) * kJS - cs.lo;
            for (int j = c0 + tx; j < c1; j += 32) {
                const float v = p[j];
                const float d1 = p[j + kJS] - 2.f * v + p[j - kJS];
                const float d2 = p[j + 1] - 2.f * v + p[j - 1];
                q[j] = v + ai * d1 + sb[j - cs.lo] * d2;
                const float dv = dp[j];
                const float dd1 = dp[j + kJS] - 2.f * dv + dp[j - kJS];
                const float dd2 = dp[j + 1] - 2.f * dv + dp[j - 1];
                float dn = dv + ai * dd1 + sb[j - cs.lo] * dd2;
                if (src) dn = dn + dai * d1 + sdb[j - cs.lo] * d2;
                dq[j] = dn;
            }
        }
        __syncthreads();
        float* t = P; P = Q; Q = t;
        t = dP; dP = dQ; dQ = t;
    }
    const int oi0 = max(rs.olo, 1), oi1 = min(rs.ohi, H + 1), oj0 = max(cs.olo, 1), oj1 = min(cs.ohi, W + 1);
    for (int i = oi0 + ty; i < oi1; i += 8)
        for (int j = oj0 + tx; j < oj1; j += 32) {
            const int l = (i - rs.lo) * kJS + (j - cs.lo);
            const size_t o = s * plane + (size_t)(i - 1) * W + (j - 1);
            if (dst_f32) {
                static_cast<float*>(dst)[o] = P[l];
                static_cast<float*>(ddst)[o] = dP[l];
            } else {
                if (dst) S1<IO>::st(static_cast<IO*>(dst) + o, P[l]);
                S1<IO>::st(static_cast<IO*>(ddst) + o, dP[l]);
            }
        }
}
