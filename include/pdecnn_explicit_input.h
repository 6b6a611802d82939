/* pdecnn_explicit_input.h — the input-only backward of the explicit 5-point layer (tiny_imagenet.py:34-72,
 * ImprovedDiffusionLayer: pde_explicit5_*) and of the Jacobi layer (emotion_recognition.py:82-97, PDELayer: pde_jacobi_*)
 * of libpdecnn_hip.
 * Part of the C ABI of pdecnn.h, which includes this file (inside its extern "C" block, behind the types it uses):
 * include pdecnn.h, not this file.  Error codes, io_dtype values, the emission mask and the Alignment rules are those of
 * pdecnn.h. */
#ifndef PDECNN_EXPLICIT_INPUT_H
#define PDECNN_EXPLICIT_INPUT_H
#ifndef PDECNN_H
#error "include pdecnn.h: it includes this header"
#endif

/* The backward for the input alone (pdecnn.h, "the backward of a layer whose coefficients take no gradient") when
 * alpha_base / channel_scaling, or a_row / b_col, take no gradient.  Both layers are linear in u — the zero ghost cells of
 * the explicit step, the reflect padding and the frozen ring of the Jacobi layer too — so gu is the adjoint alone.  No call
 * below takes u, `states` or a parameter-gradient output; none re-runs the forward, parks a state, forms a dot product or
 * runs a reduction; and every gu is bit for bit the gu of the full call named with it, given the same gout, cotangents,
 * mask and parameters.  No forward entry point is needed: a forward of 64x64, 32x32 or 16x16 planes takes states = NULL,
 * and the other plane sizes need `states` to chain their steps during the forward only.
 *
 * The plain form is the _states form with a NULL mask.  Checks, their order and their codes are those of the full
 * _backward_states calls, all on the host before the first launch: dimensions, required pointers and io_dtype
 * (PDE_E_BADARG), alignment (PDE_E_BADARG), the emission mask (bits 0 .. steps-2 only and the cotangent tensor present:
 * PDE_E_BADARG; a non-empty mask above 128 steps: PDE_E_TOO_MANY_SWEEPS), then the workspace (short, missing or not
 * 16-byte aligned: PDE_E_WORKSPACE; where the query is 0 the workspace may be NULL).  Nothing is allocated, synchronised
 * or waited for.
 *
 * pde_explicit5_backward_input[_states]      tiny_imagenet.py:34-72.  The gu of pde_explicit5_backward[_states]:
 *     num_steps times  g <- (1-relax) g + relax s_c (g + a_c dt Lap0 g),  += gtraj[slot] once g is the adjoint of an
 *     emitted state.  64x64, 32x32 and 16x16 planes: one launch, the plane in registers (explicit5_bwd_input_wave), no
 *     workspace.  Other planes: one launch per step (explicit5_bwd_input_kernel in float4 columns, .._col_kernel when W is
 *     no multiple of 4) through two fp32 buffers in `workspace`; the first launch reads gout, the last writes gu in the
 *     tensors' type.  gout, gtraj, gu: io_dtype, aligned as the tensors of pde_explicit5_backward_states.
 *     .._workspace_bytes: 0 for the three register plane sizes and for num_steps == 1, two fp32 tensors otherwise.
 * pde_explicit5_f64_backward_input[_states]  the same in double, the gu of pde_explicit5_f64_backward[_states]; one launch
 *     per step.  .._workspace_bytes: 0 for num_steps == 1, two double tensors otherwise.
 * pde_jacobi_io_backward_input[_states]      emotion_recognition.py:82-97.  The gu of pde_jacobi_io_backward[_states]:
 *     G_nt = gout with a zero ring, nt adjoint updates (+= gstates[slot] on the interior of an emitted state), the ring
 *     folded back onto rows / columns 1 and H-2 / W-2; nt = 0 gives gu = gout.  Plane path 1 (pde_jacobi_plane_path): one
 *     workgroup per sample, no workspace.  Path 2: PDE_JACOBI_TILED_K steps per launch on tile + k
 *     (jacobi_tiled_bwd_input_kernel) chained through two padded fp32 images in `workspace`, then the fold kernel of the
 *     full call; no forward launch.  .._workspace_bytes: 0 on path 1, the two padded images on path 2.
 * pde_jacobi_f64_backward_input[_states]     the same in double (planes up to 64x64, as pde_jacobi_f64_backward): the gu of
 *     pde_jacobi_f64_backward[_states]; no workspace. */
size_t pde_explicit5_backward_input_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype,
                                                    int32_t num_steps);
int pde_explicit5_backward_input(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype, const void* gout,
                                 const float* alpha_base, const float* channel_scaling, float dt, float eps, float max_coeff,
                                 float relax, int32_t num_steps, void* gu, void* workspace, size_t workspace_bytes,
                                 void* stream);
int pde_explicit5_backward_input_states(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype, const void* gout,
                                        const void* gtraj, const uint64_t emit_mask[2], const float* alpha_base,
                                        const float* channel_scaling, float dt, float eps, float max_coeff, float relax,
                                        int32_t num_steps, void* gu, void* workspace, size_t workspace_bytes, void* stream);
size_t pde_explicit5_f64_backward_input_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_steps);
int pde_explicit5_f64_backward_input(int32_t B, int32_t C, int32_t H, int32_t W, const double* gout, const double* alpha_base,
                                     const double* channel_scaling, double dt, double eps, double max_coeff, double relax,
                                     int32_t num_steps, double* gu, void* workspace, size_t workspace_bytes, void* stream);
int pde_explicit5_f64_backward_input_states(int32_t B, int32_t C, int32_t H, int32_t W, const double* gout,
                                            const double* gtraj, const uint64_t emit_mask[2], const double* alpha_base,
                                            const double* channel_scaling, double dt, double eps, double max_coeff,
                                            double relax, int32_t num_steps, double* gu, void* workspace,
                                            size_t workspace_bytes, void* stream);
size_t pde_jacobi_io_backward_input_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype);
int pde_jacobi_io_backward_input(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype, const void* gout,
                                 const float* a_row, const float* b_col, void* gu, void* workspace, size_t workspace_bytes,
                                 void* stream);
int pde_jacobi_io_backward_input_states(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype, const void* gout,
                                        const void* gstates, const uint64_t emit_mask[2], const float* a_row,
                                        const float* b_col, void* gu, void* workspace, size_t workspace_bytes, void* stream);
int pde_jacobi_f64_backward_input(int32_t B, int32_t H, int32_t W, int32_t nt, const double* gout, const double* a_row,
                                  const double* b_col, double* gu, void* stream);
int pde_jacobi_f64_backward_input_states(int32_t B, int32_t H, int32_t W, int32_t nt, const double* gout,
                                         const double* gstates, const uint64_t emit_mask[2], const double* a_row,
                                         const double* b_col, double* gu, void* stream);

#endif /* PDECNN_EXPLICIT_INPUT_H */
