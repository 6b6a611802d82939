/* pdecnn_tangent_fused.h — the tangent-linear (forward-mode) pass of the square fp32-parameter ADI family (pde_adi_*) on the
 * fused two-sided solver, for the line lengths that have register-resident sweep kernels: N = 8, 12, ..., 32.
 * Part of the C ABI of pdecnn.h, which includes this file (inside its extern "C" block, behind the types it uses):
 * include pdecnn.h, not this file.  Error codes, io_dtype values and the descriptor are those of pdecnn.h. */
#ifndef PDECNN_TANGENT_FUSED_H
#define PDECNN_TANGENT_FUSED_H
#ifndef PDECNN_H
#error "include pdecnn.h: it includes this header"
#endif

/* What pde_adi_tangent (pdecnn_tangent.h) computes, y = F(theta) u and dy = F(theta) du + (dF/dtheta . dtheta) u with the
 * same dco and the same source term per sweep and line, in the layout of pde_adi_forward's fused kernels: one wave owns
 * two planes, lane (half, line) keeps its half of that line of the primal x and of the tangent dx in registers for the
 * whole schedule, records arrive by LDS-DMA into a ring, a y sweep re-lays out both planes through the wave's LDS image.
 * Launches: the forward's factorisation (adi_factor_kernel, without the channel flags), then adi_factor_tangent_kernel (dco of
 * every (sweep, channel), one line image each; skipped when all four parameter tangents are NULL), then
 * adi_tangent_kernel: per sweep the forward's own two-sided solve on x, dx_k += dco_k (x_{k-1} - m_k x_k + x_{k+1}) on the
 * solved line, and the same solve with the same rows on dx.  Without a parameter tangent the source term and the dco ring
 * are compiled out.  bf16 / fp16 tensors: fp32 arithmetic, y and dy rounded once on the store.  No reduction, no atomic;
 * nothing is allocated, synchronised or waited for.
 *
 * Identities (tests/test_gpu_tangent_fused.py holds them bit for bit):
 *   y is pde_adi_forward's y at the same arguments;
 *   dy with no parameter tangent is pde_adi_forward's y at du;
 *   dy is exactly linear under a scaling of all tangents by a power of two;
 *   dy does not depend on whether y is stored;
 *   on bf16 / fp16 tensors y and dy are the fp32 call's on the same values, rounded once.
 * dy with a parameter tangent agrees with pde_adi_tangent's to rounding, not bit for bit: the recurrences differ.
 *
 * Arguments: those of pde_adi_tangent.  u, du, y, dy: [B][C][N][N] in io_dtype; the parameters and their tangents:
 * [C][N][N] in float.  du NULL: a zero input tangent.  Each parameter tangent may be NULL: zero.  All five NULL:
 * PDE_E_BADARG.  y may be NULL (not written); dy is required.  No output may overlap an input or the other output.
 * What differs from pde_adi_tangent:
 *   N must be 8, 12, ..., 32: any other N is PDE_E_UNSUPPORTED_N, and the query answers 0;
 *   tensors, parameters and parameter tangents are read 16 bytes wide: each must be 16-byte aligned, like the workspace;
 *   anything less is PDE_E_BADARG before the first launch;
 *   workspace bytes = pde_adi_forward_workspace_bytes(d) + round_up(num_sweeps * C * 4608, 256): the fused forward's
 *   factorisation followed by the dco records, one 32 x 36 line image of floats per (sweep, channel).
 *
 * Checks, their order and their codes are those of pde_adi_forward at a fused N, all on the host before the first launch:
 * the descriptor (PDE_E_BADARG, PDE_E_UNSUPPORTED_N, PDE_E_TOO_MANY_SWEEPS; io_dtype), required pointers and "all five
 * NULL" (PDE_E_BADARG), alignment (PDE_E_BADARG), then the workspace (short or not 16-byte aligned: PDE_E_WORKSPACE).
 * .._workspace_bytes: 0 for a descriptor the call refuses.  The workspace is scratch: nothing in it outlives the call. */
size_t pde_adi_tangent_fused_workspace_bytes(const PdeAdiDesc* d);
int pde_adi_tangent_fused(const PdeAdiDesc* d, const void* u, const void* du,
                          const float* alpha_base, const float* beta_base, const float* alpha_slope, const float* beta_slope,
                          const float* d_alpha_base, const float* d_beta_base, const float* d_alpha_slope,
                          const float* d_beta_slope, void* y, void* dy, void* workspace, size_t workspace_bytes,
                          void* stream);

#endif /* PDECNN_TANGENT_FUSED_H */
