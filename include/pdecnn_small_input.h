/* pdecnn_small_input.h — the input-only backward of the one-launch C <= 4 layers of libpdecnn_hip.
 * Part of the C ABI of pdecnn.h, which includes this file (inside its extern "C" block, behind the types it uses):
 * include pdecnn.h, not this file.  Error codes, descriptors, PdeSmallLayer and the Alignment rules are those of pdecnn.h. */
#ifndef PDECNN_SMALL_INPUT_H
#define PDECNN_SMALL_INPUT_H
#ifndef PDECNN_H
#error "include pdecnn.h: it includes this header"
#endif

/* The backward for the input alone (pdecnn.h, "the backward of a layer whose coefficients take no gradient") for the
 * one-launch C <= 4 layers (pde_adi_small_*, pde_adi_multi_*) when neither the coefficients, M, skip_weight nor the
 * weights take a gradient.  The channel operator and the skip blend are linear in the input too, so
 * gu is again the adjoint alone: per sweep the transposed solve, at a step boundary the column of M, the skip split
 * (sigmoid(w) gy goes straight to gu), the weights, gys and g_plane_sums.  One launch (plus the small combine launch
 * when a group runs side by side); neither u nor `states` is read, no step-local checkpoint is parked (there is no
 * pre-pass), no coefficient sum, gM, g_skip_weight or g_weight is formed and no parameter-gradient epilogue runs: 2 tensor
 * passes per element where the full backward moves K + 3.  gu is bit for bit the gu of pde_adi_small_backward[_states] /
 * pde_adi_multi_backward on the same arguments, in both launch arrangements and for any ckpt_mask there.
 *   steps_workspace   the factorisation the forward of the same call left behind; required (these calls do not
 *                     factorise).  NULL or misaligned: PDE_E_WORKSPACE.
 *   workspace         pde_adi_small_backward_input_workspace_bytes(d, sweeps_per_step): the layer's slab of a
 *                     side-by-side group (num_layers > 1, B < 1024), the only scratch there is.  A one-layer call and
 *                     a group one after the other touch none and may pass NULL; a group side by side needs one per
 *                     layer (missing or short: PDE_E_WORKSPACE).  Where given it is 16-byte aligned.  The query is 0
 *                     for a descriptor pde_adi_small_supported refuses.
 *   _states           gtraj / emit_mask as in pde_adi_small_backward_states (same checks, same codes); no skip blend.
 *   multi             reads from each PdeSmallLayer desc, sweeps_per_step, mode, M, skip_weight, weight / weight_ptr,
 *                     steps_workspace, gys, g_plane_sums, workspace / workspace_bytes.  The coefficient pointers,
 *                     states, every g_* output and ckpt_mask may be NULL and are not touched; every non-NULL device
 *                     pointer of the struct still has to meet its alignment (PDE_E_BADARG), as in pde_adi_multi_backward.
 * A NULL gy (one-layer calls), gu or M, an unsupported descriptor, skip_weight in mode 1, several layers in mode 2,
 * layers that disagree, a bad emission mask: PDE_E_BADARG.  All checks run on the host before the launch; nothing is
 * allocated, synchronised or waited for.
 * pde_adi_small_forward_input is the forward of such a call: pde_adi_small_forward that parks nothing (there is no
 * `states`) and returns the y pde_adi_small_forward returns WITH states kept, bit for bit.  With 16-bit tensors the
 * kept-states forward goes on from the rounded sweep output of every step and the inference launch (states NULL) does
 * not; this call rounds without storing.  With fp32 tensors it is the inference launch.  A shared-input group has no
 * such call: its y_i outputs are the last kept states, so its forward is pde_adi_multi_forward unchanged. */
size_t pde_adi_small_backward_input_workspace_bytes(const PdeAdiDesc* d, int32_t sweeps_per_step);
int pde_adi_small_forward_input(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t mode,
                                const void* u, void* y, const float* M, const float* skip_weight,
                                const float* alpha_base, const float* beta_base,
                                const float* alpha_slope, const float* beta_slope,
                                float* kappa_max, float* kappa_max_host, void* kappa_event,
                                void* steps_workspace, size_t workspace_bytes, void* stream);
int pde_adi_small_backward_input(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t mode,
                                 const void* gy, const float* M, const float* skip_weight, void* gu,
                                 const void* steps_workspace, void* workspace, size_t workspace_bytes, void* stream);
int pde_adi_small_backward_input_states(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t mode,
                                        const void* gy, const void* gtraj, const uint64_t emit_mask[2],
                                        const float* M, void* gu,
                                        const void* steps_workspace, void* workspace, size_t workspace_bytes, void* stream);
int pde_adi_multi_backward_input(int32_t num_layers, const PdeSmallLayer* layers, const void* gy, void* gu, void* stream);

#endif /* PDECNN_SMALL_INPUT_H */
