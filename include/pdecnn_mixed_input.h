/* pdecnn_mixed_input.h — the input-only backward of the layers with a channel operator above C = 4 (the per-step and
 * wide paths: pde_adi_mixed_*, pde_channel_mix_*, pde_skip_blend_*) of libpdecnn_hip.
 * Part of the C ABI of pdecnn.h, which includes this file (inside its extern "C" block, behind the types it uses):
 * include pdecnn.h, not this file.  Error codes, descriptors and the Alignment rules are those of pdecnn.h. */
#ifndef PDECNN_MIXED_INPUT_H
#define PDECNN_MIXED_INPUT_H
#ifndef PDECNN_H
#error "include pdecnn.h: it includes this header"
#endif

/* The backward for the input alone (pdecnn.h, "the backward of a layer whose coefficients take no gradient") when neither
 * the coefficients, M nor skip_weight take a gradient.  Sweeps, channel operator and skip blend are all linear in the
 * input, so gu is the adjoint alone; no call below reads u, `states`, y or a checkpoint mask, forms a partial sum or
 * runs a reduction, and every gu is bit for bit the gu of the full call named with it.  All checks run on the host before
 * the first launch; nothing is allocated, synchronised or waited for.  Tensors, M and workspaces are 16-byte aligned
 * (float64: 8 bytes for tensors and matrices), skip_weight 4 bytes; a misaligned or missing workspace is PDE_E_WORKSPACE,
 * any other bad pointer PDE_E_BADARG.
 *
 * pde_channel_mix_backward_input        gu = M^T gout, the gu of pde_channel_mix_backward[_steps].  It dispatches on the
 *                                       same plan (pde_channel_mix_path(..., backward = 1)), so every path keeps its
 *                                       arithmetic: the transposed apply kernels alone on PDE_MIX_PATH_SCALAR / _MFMA_F32,
 *                                       the gu half of mix_bwd_split_kernel / mix_bwd_fused_kernel / mix_bwd_bf16_kernel
 *                                       (their GM = false instantiations:  no u loads, no gM MFMAs, no partial
 *                                       matrices) on the other three.  workspace: .._workspace_bytes(B, C, HW), the M^T
 *                                       fragment table of the C = 128 fused path and 0 (NULL allowed) everywhere else.
 * pde_channel_mix_f64_backward_input    the same for the double operator; no workspace.
 * pde_skip_blend_backward_input         g_u0 = sigmoid(w) g and g_u = sigmoid(-w) g, the two tensor outputs of
 * pde_skip_blend_f64_backward_input     pde_skip_blend[_f64]_backward; no workspace, no reduction.
 *
 * pde_adi_backward_input_step           the adjoint of one step's sweeps from the steps workspace of pde_adi_factor_steps
 *                                       (adi_bwd_input_kernel on the step's own pattern): the gu of pde_adi_backward_step
 *                                       on the same step, its (1+eps)^-sweeps_per_step scaling included.  Line lengths
 *                                       with fused kernels only, as every per-step call (PDE_E_UNSUPPORTED_N otherwise).
 * pde_adi_mixed_forward_input           pde_adi_mixed_forward that keeps nothing: the same kernels in the same order, y
 *                                       (required) bit for bit.  The one-launch C = 32 / 64 forward runs with keep = 0
 *                                       and needs no scratch (the query is 0; workspace may be NULL); the per-step route
 *                                       walks through two scratch tensors in `workspace`
 *                                       (.._workspace_bytes(d, sweeps_per_step)).  steps_workspace /
 *                                       steps_workspace_bytes and the three kappa arguments: as in pde_adi_mixed_forward.
 * pde_adi_mixed_backward_input          for k = K-1 .. 0 the step's two adjoint pieces in the order of
 *                                       pde_adi_mixed_backward (mode 1: sweeps^T then M^T; mode 2: M^T then sweeps^T), each
 *                                       intermediate gradient in a tensor of the I/O type (16-bit tensors round where the
 *                                       full backward rounds).  steps_workspace: the factorisation the forward left
 *                                       (required).  workspace: .._workspace_bytes(d, sweeps_per_step).
 * pde_adi_mixed_backward_input_one_launch   1 where the call above takes a one-launch reverse walk, 0 where it composes the
 *                                       per-step calls.  No one-launch kernel is built: 0 for every descriptor. */
size_t pde_channel_mix_backward_input_workspace_bytes(int32_t B, int32_t C, int32_t HW);
int pde_channel_mix_backward_input(int32_t B, int32_t C, int32_t HW, int32_t io_dtype, const void* gout, const float* M,
                                   void* gu, void* workspace, size_t workspace_bytes, void* stream);
int pde_channel_mix_f64_backward_input(int32_t B, int32_t C, int32_t HW, const double* gout, const double* M, double* gu,
                                       void* stream);
int pde_skip_blend_backward_input(int64_t n, int32_t io_dtype, const void* g, const float* skip_weight, void* g_u0, void* g_u,
                                  void* stream);
int pde_skip_blend_f64_backward_input(int64_t n, const double* g, const double* skip_weight, double* g_u0, double* g_u,
                                      void* stream);
int pde_adi_backward_input_step(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t step, const void* gy, void* gu,
                                const void* steps_workspace, void* stream);
size_t pde_adi_mixed_forward_input_workspace_bytes(const PdeAdiDesc* d, int32_t sweeps_per_step);
int pde_adi_mixed_forward_input(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t mode, const void* u, void* y,
                                const float* M, const float* alpha_base, const float* beta_base,
                                const float* alpha_slope, const float* beta_slope,
                                float* kappa_max, float* kappa_max_host, void* kappa_event,
                                void* steps_workspace, size_t steps_workspace_bytes,
                                void* workspace, size_t workspace_bytes, void* stream);
size_t pde_adi_mixed_backward_input_workspace_bytes(const PdeAdiDesc* d, int32_t sweeps_per_step);
int pde_adi_mixed_backward_input(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t mode, const void* gy, const float* M,
                                 void* gu, const void* steps_workspace, void* workspace, size_t workspace_bytes, void* stream);
int pde_adi_mixed_backward_input_one_launch(const PdeAdiDesc* d, int32_t sweeps_per_step);

#endif /* PDECNN_MIXED_INPUT_H */
