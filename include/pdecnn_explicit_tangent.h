/* pdecnn_explicit_tangent.h — the tangent-linear (forward-mode) pass of the explicit 5-point layer (tiny_imagenet.py:34-72:
 * pde_explicit5_*) and of the Jacobi layer (emotion_recognition.py:82-97: pde_jacobi_*) of libpdecnn_hip.
 * Part of the C ABI of pdecnn.h, which includes this file (inside its extern "C" block, behind the types it uses):
 * include pdecnn.h, not this file.  Error codes, io_dtype values and the Alignment rules are those of pdecnn.h. */
#ifndef PDECNN_EXPLICIT_TANGENT_H
#define PDECNN_EXPLICIT_TANGENT_H
#ifndef PDECNN_H
#error "include pdecnn.h: it includes this header"
#endif

/* One call returns y = F(theta) u, the family's forward, and its directional derivative
 *     dy = F(theta) du + (dF/dtheta . dtheta) u.
 * Both time loops are linear in u, so the primal state and the tangent state advance together, step by step, and the
 * tangent step is the primal step on du plus a source term that reads the step's INPUT state.
 *
 * Explicit 5-point, theta = (alpha_base, channel_scaling), per step with a = clamp(alpha_c, eps, max_coeff) dt, s = scale_c,
 * L = the 5-point Laplacian with zero ghost cells:
 *     u'  = u + relax ((s u + a (s L u)) - u)                          the forward kernels' expressions, in their order
 *     du' = the same expressions on du,  + relax (ds (u + a L u) + da (s L u)),     da = pass . dalpha_c . dt
 * pass = 1 where eps <= alpha_c <= max_coeff (equality passes: the mask of the backward's alpha gradient and of torch's
 * clamp).  Planes of 64x64, 32x32 and 16x16: one launch, one wave per plane, both planes in registers over all steps.
 * Every other plane: one launch per step — float4 columns when W is a multiple of 4, single columns otherwise — with both
 * states handed on through fp32 images in `workspace`.  float64 (pde_explicit5_f64_tangent): one launch per step.
 *
 * Jacobi, theta = (a_row, b_col): P = reflect-pad(u), dP = reflect-pad(du); both rings keep those values.  Interior, per step:
 *     P'  = P + a_i d1(P) + b_j d2(P)                                  the forward's expressions, in their order
 *     dP' = the same expressions on dP,  + da_i d1(P) + db_j d2(P)
 * Planes up to 64x64: one workgroup per sample, P, Q, dP, dQ and the four coefficient vectors in its LDS (70720 bytes at
 * 64x64).  Larger planes, up to PDE_JACOBI_MAX_HW: the tiled kernel — the forward's 64x64 tiles and halo,
 * PDE_JACOBI_TANGENT_TILED_K time steps per launch (the forward's PDE_JACOBI_TILED_K: four region images fit one
 * workgroup's LDS), P and dP handed from launch to launch through fp32 images in `workspace`.  float64
 * (pde_jacobi_f64_tangent): H, W <= 64 only, as the float64 forward; no workspace.
 *
 * So y is bit for bit the y of the family's forward, dy with no parameter tangent is bit for bit that forward at du (the
 * source term is then not added at all), and dy is exactly linear under a scaling of all tangents by a power of two.
 * bf16 / fp16 tensors: fp32 arithmetic, y and dy rounded once on the store, fp32 between the launches.  No reduction, no
 * atomic; nothing is allocated, synchronised or waited for.
 *
 * Arguments.  u, du, y, dy: [B][C][H][W] (explicit) or [B][H][W] (Jacobi) in io_dtype (double in the f64 calls); the
 * parameters and their tangents: [C] (alpha_base, channel_scaling), [H] (a_row), [W] (b_col) in float (double in the f64
 * calls).  du NULL: a zero input tangent.  Each parameter tangent may be NULL: zero.  All three NULL: PDE_E_BADARG (nothing
 * to differentiate: call the forward).  y may be NULL (not written); dy is required.  No output may overlap the other
 * output or an input.
 * Alignment, as in the family's forward.  pde_explicit5_tangent: u, du, y, dy begin on FOUR ELEMENTS (16 bytes of fp32, 8
 * bytes of bf16 / fp16) when W is a multiple of 4, on the element otherwise; alpha_base, channel_scaling and their tangents
 * on the element.  pde_jacobi_io_tangent and both f64 calls: the element, tensors and parameters alike.  Every workspace:
 * 16 bytes.
 *
 * Checks, their order and their codes are those of the family's forward, all on the host before the first launch: sizes
 * (B, C, H, W > 0, num_steps >= 1; Jacobi: 4 <= H, W <= PDE_JACOBI_MAX_HW — 2 <= H, W <= 64 in float64 —, nt >= 0), required
 * pointers and the three tangents (PDE_E_BADARG), io_dtype (PDE_E_BADARG), alignment (PDE_E_BADARG), then the workspace
 * (short, missing where one is needed, or not 16-byte aligned: PDE_E_WORKSPACE).
 * .._workspace_bytes, with align256(n) = n rounded up to 256:
 *     pde_explicit5_tangent, pde_explicit5_f64_tangent: 4 align256(B C H W sizeof(float | double)) when num_steps > 1 and
 *         the plane is not one of the three register sizes (float64: whenever num_steps > 1), else 0;
 *     pde_jacobi_io_tangent: 4 align256(B H W sizeof(float)) for a tiled plane (H or W above 64) with
 *         nt > PDE_JACOBI_TANGENT_TILED_K, else 0;
 * and 0 for a call that would be refused.  A call whose query is 0 takes workspace NULL.  The workspace is scratch: nothing
 * in it outlives the call. */
#define PDE_JACOBI_TANGENT_TILED_K PDE_JACOBI_TILED_K
size_t pde_explicit5_tangent_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype,
                                             int32_t num_steps);
int pde_explicit5_tangent(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype, const void* u, const void* du,
                          const float* alpha_base, const float* channel_scaling, const float* d_alpha_base,
                          const float* d_channel_scaling, float dt, float eps, float max_coeff, float relax,
                          int32_t num_steps, void* y, void* dy, void* workspace, size_t workspace_bytes, void* stream);
size_t pde_explicit5_f64_tangent_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_steps);
int pde_explicit5_f64_tangent(int32_t B, int32_t C, int32_t H, int32_t W, const double* u, const double* du,
                              const double* alpha_base, const double* channel_scaling, const double* d_alpha_base,
                              const double* d_channel_scaling, double dt, double eps, double max_coeff, double relax,
                              int32_t num_steps, double* y, double* dy, void* workspace, size_t workspace_bytes,
                              void* stream);
size_t pde_jacobi_io_tangent_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype);
int pde_jacobi_io_tangent(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype, const void* u, const void* du,
                          const float* a_row, const float* b_col, const float* d_a_row, const float* d_b_col, void* y,
                          void* dy, void* workspace, size_t workspace_bytes, void* stream);
int pde_jacobi_f64_tangent(int32_t B, int32_t H, int32_t W, int32_t nt, const double* u, const double* du,
                           const double* a_row, const double* b_col, const double* d_a_row, const double* d_b_col,
                           double* y, double* dy, void* stream);

#endif /* PDECNN_EXPLICIT_TANGENT_H */
