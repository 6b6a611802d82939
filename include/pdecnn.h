/*
 * pdecnn.h — C ABI of libpdecnn_hip.so: the MI355X (gfx950) implementation of the
 * PDE diffusion-layer hot path of MariMamgo/CNN-with-PDE.
 *
 * Boundary.  The reference has no FFI; its boundary is the nn.Module surface of the
 * layer classes.  This library is what a Python autograd.Function
 * binds with ctypes; every entry point cites the reference code
 * it replaces.  Conventions:
 *   - plain pointers and sizes only; all tensor pointers are DEVICE pointers
 *     (the caller owns every buffer), NCHW contiguous;
 *   - every call enqueues work on `stream` (a hipStream_t passed as void*) and
 *     returns immediately; no allocation, no synchronisation.  Process-wide state is limited to
 *     bookkeeping that never changes a result: one "dynamic-LDS attribute set" bit per (kernel,
 *     device) behind a mutex, and the optional timing recorder of pde_timing_*;
 *   - return value: 0 on success, a negative PDE_E_* code otherwise (never throws).
 *
 * Contents on entry, and what a call may touch (tests/test_gpu_bounds.py holds every entry point to this).  A call writes
 * inside the buffers it is given and nowhere else: an output of n elements gets exactly n elements, a workspace exactly the
 * bytes its *_workspace_bytes() query returned.  Unless a function's own comment says otherwise:
 *   - OUTPUT (every pointer to non-const tensor memory: y, out, gu, states, traj, the parameter gradients, gM, g_weight,
 *     g_skip_weight, plane_sums, kappa_max, P, H, dP, mean, invstd, argmax, K16, ...): overwritten in full — every element
 *     is stored, none is read or added to — so its contents on entry do not matter;
 *   - WORKSPACE (`workspace`, and `steps_workspace` in the call that fills it): scratch whose contents on entry do not
 *     matter: nothing in it is read before the call itself has written it;
 *   - CARRIED between the calls of a sequence — contents do not matter before the FIRST call, must stay intact until the last:
 *       `steps_workspace`  filled by pde_adi_factor_steps or by the forward of pde_adi_mixed_* / pde_adi_small_* /
 *                          pde_adi_multi_*, read by every later call of that layer call;
 *       `workspace` of pde_adi_backward_step        accumulate = 0 starts the partial sums in it (the first call of a
 *                          sequence), accumulate = 1 adds to them, pde_adi_param_grads reads them;
 *       `workspace` of pde_channel_mix[_f64]_backward_steps   likewise: accumulate = 0 starts, 1 adds, finalize = 1 reduces;
 *       `fwd_workspace`    the forward's workspace, read only;
 *       `states` of pde_adi_mixed_forward in the one-launch case: written in part (see there); the rest is left as it was,
 *                          and the backward recomputes what it needs of it instead of reading it;
 *   - UPDATED in place (read, then written): running_mean / running_var, in training mode only.
 * Inputs (pointers to const) are never written.
 *
 * Alignment.  Where a buffer may begin: the width of the widest access any kernel behind the parameter makes through it,
 * in every dispatch variant and under every environment switch (DESIGN.md section 5 has the evidence per family).  A
 * non-NULL device pointer below its requirement is refused on the host, with the NULL and shape checks and before anything
 * touches the runtime: PDE_E_BADARG, for a workspace PDE_E_WORKSPACE.  A pointer that is given is checked, also where the
 * call would not read it (states with an empty mask).  Only the base address is constrained, never a buffer's length.
 *   - DEFAULT, 16 bytes: every tensor, coefficient plane and matrix (u, y, gy, gu, states, traj, out, gout, x, X, K, K16, P, H,
 *     M, alpha_base ..., their gradients, the tensors ys[i] / gys[i] point to, ...) and EVERY workspace (`workspace`,
 *     `steps_workspace`, `fwd_workspace`).  The kernels move these as float4 / uint4 (uint2 for four 16-bit values).
 *   - ELEMENT, the alignment of one element (4 bytes for float and int32_t, 8 for double, 2 for 16-bit values): what
 *     the kernels read and write one element at a time, by parameter name, struct fields of PdeSmallLayer included:
 *     ELEMENT-ALIGNED: kappa_max, kappa_max_host, skip_weight, g_skip_weight, weight_ptr, g_weight, plane_sums, weights,
 *                      gates, dots, gamma, beta, mean, invstd, running_mean, running_var, ggamma, gbeta, argmax,
 *                      bn_weight, bn_bias, g_bn_weight, g_bn_bias, a_row, b_col, g_a_row, g_b_col, channel_scaling,
 *                      g_channel_scaling
 *     (gates and dots: the arrays their entries point to; so weight_ptr = weights + i of a shared-input group is legal).
 *     Two families read a parameter one element at a time whose NAME is a 16-byte tensor everywhere else:
 *     ELEMENT-ALIGNED IN pde_explicit5_: alpha_base, g_alpha_base    (C values, not the implicit layers' (C,N,N) planes)
 *     ELEMENT-ALIGNED IN pde_bn_pool_: out, gout                      (the pooled cells, stored and read one at a time)
 *   - ELEMENT-WISE CALLS: a call whose kernels all move one element at a time asks the element's alignment of every tensor
 *     and coefficient pointer (its workspaces stay at 16): every pde_*_f64_* function; every pde_adi_rect_* function;
 *     pde_adi_forward / _backward / _backward_input[_states] / _forward_states / _backward_states / _kappa_max when N is not
 *     one of the fused line lengths (pde_adi_line_length_path(N) == 2); every pde_jacobi_* function; pde_explicit5_* when W
 *     is no multiple of 4.  This is what lets `y` (`out`) be the last slice of a stacked trajectory tensor at any plane size.
 *   - FOUR ELEMENTS: pde_explicit5_* with W a multiple of 4 and 16-bit tensors asks 8 bytes of u, out, gout, gu, traj,
 *     gtraj (four 16-bit values per access; a slice of a (slots, B, C, H, W) tensor begins on such a boundary); its fp32
 *     `states` and everything else follow the default.
 */
#ifndef PDECNN_H
#define PDECNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDE_MAX_SWEEPS 96          /* e.g. 32 Strang steps */
#define PDE_MAX_N 32               /* longest line of the fused implicit kernels (N = 8, 12, ..., 32; the reference uses 28, 32) */
#define PDE_MAX_N_GENERIC 128      /* longest line of the any-size path (one thread per line, plane in LDS)              */

#define PDE_OK 0
#define PDE_E_BADARG (-1)          /* null or misaligned pointer (see Alignment above), non-positive dim, bad enum */
#define PDE_E_UNSUPPORTED_N (-2)   /* whole-schedule calls: N < 2 or > PDE_MAX_N_GENERIC; per-step / one-launch
                                      families: N not one of the fused line lengths */
#define PDE_E_TOO_MANY_SWEEPS (-3)
#define PDE_E_LAUNCH (-4)          /* hipLaunch failed; hipPeekAtLastError/hipGetLastError has details */
#define PDE_E_WORKSPACE (-5)       /* workspace too small / misaligned */

#define PDE_IO_F32 0
#define PDE_IO_BF16 1
#define PDE_IO_F64 2               /* PdeAdiDescF64 only: the pde_*_f64_* entry points */
#define PDE_IO_F16 3               /* float16 tensors (a half()-converted model): I/O rounded to fp16 where the bf16 route
                                      rounds to bf16, math in fp32 */

#define PDE_AXIS_X 0               /* solve along W with alpha (mnist_test.py:67-98)  */
#define PDE_AXIS_Y 1               /* solve along H with beta  (mnist_test.py:100-133) */

/* One implicit (backward-Euler) sweep of the split scheme, in execution order.
 * Mirrors one diffuse_x/diffuse_y call of the reference time loop
 * (mnist_test.py:50-63, cifar10.py:86-110, cifar_2version.py:81-101). */
typedef struct PdeSweep {
    int32_t axis;       /* PDE_AXIS_X / PDE_AXIS_Y */
    float   delta;      /* (float) time increment of this sweep: dt/2 or dt           */
    float   h2;         /* (float) dx**2 or dy**2: coeff = theta*delta/h2              */
    float   t;          /* (float) current_time at which alpha/beta are evaluated      */
} PdeSweep;

/* Static description of one fused run of sweeps over a (B,C,N,N) tensor. */
typedef struct PdeAdiDesc {
    int32_t B, C, N;            /* H = W = N                                             */
    int32_t io_dtype;           /* PDE_IO_F32 | PDE_IO_BF16 | PDE_IO_F16 (tensor I/O; math is fp32) */
    int32_t num_sweeps;
    int32_t smooth3;            /* 1: 3-tap replicate average of the coefficient along the
                                   solve axis (mnist_test.py:135-149)                     */
    int32_t has_clamp_max;      /* 1: clamp(theta, eps, clamp_max) (cifar10.py:60-61)     */
    float   clamp_max;
    float   eps;                /* stability_eps: clamp floor AND the Thomas +eps          */
    PdeSweep sweep[PDE_MAX_SWEEPS];
} PdeAdiDesc;

/* ---- K1: implicit ADI time-stepper -------------------- */

/* Which kernels serve line length N: 1 = fused register-resident sweeps (N = 8, 12, ..., 32: every entry point of
 * this header), 2 = the any-size path (2 <= N <= PDE_MAX_N_GENERIC, any other N: the reference's classes take any `size`,
 * mnist_test.py:12, cifar10.py:25, SVHN.py:13) — pde_adi_forward / pde_adi_backward / pde_adi_kappa_max and their
 * workspace queries only, one thread per line with the reference's own Thomas recurrences (mnist_test.py:151-198); a
 * layer with a channel operator is then composed per step by the caller (pde_channel_mix_* + one-step schedules),
 * 0 = unsupported. */
int pde_adi_line_length_path(int32_t N);

/* Which kernel pde_adi_forward runs for this schedule: 0 = the HIP kernel with a barrier per sweep (adi_fwd_kernel), 1 = the
 * hand-scheduled assembly kernel (opt-in, PDE_ASM_FWD=1), 2 = the any-size kernels, 3 = the HIP kernel's hand-over schedule
 * (N = 32, fp32 tensors, Strang steps, more sweeps than stay resident: counters in LDS instead of the barrier per sweep).
 * Same arithmetic in the same order for 0, 1 and 3; PDE_FWD_SCHED=0 in the environment turns 3 into 0;
 * PDE_FWD_STAGGER=0 runs 3 without the stagger of the two workgroups of a CU (scheduling only). */
int pde_adi_forward_kernel(const PdeAdiDesc* d);

/* Which kernel pde_adi_backward runs for this schedule's unmasked channels: 0 = the HIP kernel (adi_bwd_kernel), 1 = the
 * hand-scheduled gfx950 assembly kernel (csrc/gen_adi_bwd_asm.py: N = 32, fp32 tensors, Strang steps — mnist_test.py:55-63,
 * cifar10.py:84-110 — two or more of them, no checkpoints), 2 = the any-size kernels.  Same arithmetic either way: the
 * adjoint of the time loop and the batch sums of the coefficient gradients; PDE_ASM_BWD=0 in the
 * environment keeps the library on 0. */
int pde_adi_backward_kernel(const PdeAdiDesc* d, int32_t num_checkpoints);

/* Bytes of scratch the forward/backward calls need (the base 16-byte aligned, as every workspace: Alignment above). */
size_t pde_adi_forward_workspace_bytes(const PdeAdiDesc* d);
size_t pde_adi_backward_workspace_bytes(const PdeAdiDesc* d, int32_t num_checkpoints);

/* y = (prod_s (A_s + eps I)^-1) u.  Replaces DiffusionLayer.forward's time loop with its
 * diffuse_x/diffuse_y/thomas_solver_batch calls (mnist_test.py:44-198; cifar10.py:74-211
 * without apply_channel_mixing, which is pde_channel_mix_*).
 * alpha_xxx / beta_xxx: (C,N,N) fp32.  u, y: (B,C,N,N) of io_dtype; y must not alias u.
 * kappa_max: NULL, or a device buffer of num_sweeps floats that receives the maximum
 * coefficient of every sweep (same values as pde_adi_kappa_max, at no extra launch).
 * kappa_max_host: NULL, or PINNED host memory of num_sweeps floats: the maxima are written there by the
 * factorisation's own second kernel when the buffer is mapped into the device's address space and the
 * process sees one device, else copied asynchronously — either way BEFORE the sweep kernel is launched
 * (needs kappa_max).  kappa_event: NULL, or a hipEvent_t the call records on `stream` behind that copy:
 * the host can plan the backward's checkpoints from this call's own coefficients after a wait of
 * microseconds, long before the forward has finished.
 * After the call the workspace holds the factorisation of every sweep; while it stays intact it
 * may be handed to pde_adi_backward as fwd_workspace to skip refactorising. */
int pde_adi_forward(const PdeAdiDesc* d, const void* u, void* y,
                    const float* alpha_base, const float* beta_base,
                    const float* alpha_slope, const float* beta_slope,
                    float* kappa_max, float* kappa_max_host, void* kappa_event,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Exact reverse-mode derivative of pde_adi_forward (the reference gets it from autograd,
 * SURVEY.md §3d).  Inputs: gy = dL/dy, y = forward output.  Outputs: gu = dL/du and the
 * four parameter gradients (C,N,N) fp32 (overwritten, not accumulated).
 * States needed for the coefficient gradients are rebuilt backwards from y
 * (x_{s-1} = (A_s+eps I) x_s).  `ckpt_mask` bit s set means: do NOT rebuild the state
 * after sweep s, read it from a checkpoint instead; the kernel then first recomputes the
 * forward from `u` to write those checkpoints into the workspace.  ckpt_mask == 0 needs
 * neither u nor checkpoint space (u may be NULL).  Bits are given low word first:
 * sweep s is bit (s%64) of ckpt_mask[s/64].
 * Restriction: all sweeps of one axis must share delta/h2 (true for every reference variant:
 * Strang x(dt/2) y(dt) x(dt/2), Lie x(dt/2) y(dt/2)); otherwise PDE_E_BADARG. */
int pde_adi_backward(const PdeAdiDesc* d, const void* gy, const void* y, const void* u,
                     const uint64_t ckpt_mask[2], void* gu,
                     const float* alpha_base, const float* beta_base,
                     const float* alpha_slope, const float* beta_slope,
                     float* g_alpha_base, float* g_beta_base,
                     float* g_alpha_slope, float* g_beta_slope,
                     const void* fwd_workspace /* NULL, or the intact workspace of the matching
                                                  pde_adi_forward call (same desc, same parameters) */,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- the trajectory: intermediate states of the time loop out of the SAME launch ------------------------
 * pde_adi_forward that also returns the state after chosen sweeps, and the backward that takes an upstream gradient for
 * every one of them.  emit_mask is shaped like ckpt_mask (sweep s is bit s%64 of emit_mask[s/64]); only bits
 * 0 .. num_sweeps-2 may be set (the state after the last sweep is y itself).
 * forward_states: bit s set = the true state after sweep s is written to states[slot(s)][B][C][N][N] in io_dtype (slots
 * in the order of the set bits; with 16-bit tensors the fp32 state rounded once — the time loop goes on unrounded).  y is
 * the final state as in the plain call; a caller that wants one stacked tensor points y at the slice behind the last slot.
 * backward_states: gstates has the layout of states and holds dL/d(state); when the reverse walk has undone sweep s+1
 * and is about to enter sweep s the adjoint gets += gstates[slot(s)].  State rebuild, checkpoints, masked channels and
 * the parameter-gradient sums are those of pde_adi_backward.
 * Workspaces are those of the plain calls (pde_adi_forward_workspace_bytes / pde_adi_backward_workspace_bytes).
 * Checked on the host before any launch: states / gstates NULL with a non-empty mask, or a bit at or above
 * num_sweeps-1: PDE_E_BADARG.  An empty (or NULL) mask is the plain call exactly, states / gstates are then not read.
 * A non-empty mask runs the emitting variants of the HIP kernels: the forward on the barrier-per-sweep schedule, the HIP
 * backward — never the assembly kernels (pde_adi_forward_kernel / pde_adi_backward_kernel answer for the plain call).
 * One sweep launch per pass, as the plain call. */
int pde_adi_forward_states(const PdeAdiDesc* d, const void* u, void* y, void* states, const uint64_t emit_mask[2],
                           const float* alpha_base, const float* beta_base,
                           const float* alpha_slope, const float* beta_slope,
                           float* kappa_max, float* kappa_max_host, void* kappa_event,
                           void* workspace, size_t workspace_bytes, void* stream);
int pde_adi_backward_states(const PdeAdiDesc* d, const void* gy, const void* gstates, const uint64_t emit_mask[2],
                            const void* y, const void* u, const uint64_t ckpt_mask[2], void* gu,
                            const float* alpha_base, const float* beta_base,
                            const float* alpha_slope, const float* beta_slope,
                            float* g_alpha_base, float* g_beta_base,
                            float* g_alpha_slope, float* g_beta_slope,
                            const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream);

/* max over the tensor of coeff_s = theta_s*delta_s/h2_s for every sweep, written to
 * kappa_max[num_sweeps] (device, fp32).  Host code uses it to choose ckpt_mask.  */
int pde_adi_kappa_max(const PdeAdiDesc* d,
                      const float* alpha_base, const float* beta_base,
                      const float* alpha_slope, const float* beta_slope,
                      float* kappa_max, void* stream);

/* ---- K1 as a sequence of per-step launches --------------------------------------------------
 * The variants with a channel operator between the time steps (cifar10.py:91 mixing before every
 * step, SVHN.py:71 coupling after every step) cannot run their whole time loop in one launch.
 * These entry points serve ONE layer call as: one factorisation of the whole schedule, then one
 * sweep launch per step (`sweeps_per_step` consecutive sweeps of `d`, 3 for Strang, 2 for Lie), the
 * backward accumulating the parameter-gradient partial sums across its per-step launches so that
 * pde_adi_param_grads runs once.  `d` is always the descriptor of the WHOLE schedule. */
size_t pde_adi_steps_workspace_bytes(const PdeAdiDesc* d, int32_t sweeps_per_step);
/* zero + factorise every sweep, one sweep table per step; kappa_max as in pde_adi_forward.  steps_workspace: contents on
 * entry do not matter; every later call of the sequence reads it */
int pde_adi_factor_steps(const PdeAdiDesc* d, int32_t sweeps_per_step,
                         const float* alpha_base, const float* beta_base,
                         const float* alpha_slope, const float* beta_slope,
                         float* kappa_max, void* steps_workspace, size_t workspace_bytes, void* stream);
/* y = sweeps of step `step` applied to u */
int pde_adi_forward_step(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t step,
                         const void* u, void* y, const void* steps_workspace, void* stream);
size_t pde_adi_backward_step_workspace_bytes(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t num_checkpoints);
/* gu = adjoint of step `step`; ckpt_mask bits are relative to the step (bit 0 = state after its first
 * sweep).  accumulate = 0 starts the partial sums held in `workspace` (whose contents then do not matter), 1 adds to
 * them: use the same workspace for every step of a call and keep it intact up to pde_adi_param_grads. */
int pde_adi_backward_step(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t step,
                          const void* gy, const void* y, const void* u, const uint64_t ckpt_mask[2], void* gu,
                          const void* steps_workspace, void* workspace, size_t workspace_bytes,
                          int32_t accumulate, void* stream);
/* the four parameter gradients from the partial sums accumulated in `workspace` */
int pde_adi_param_grads(const PdeAdiDesc* d, int32_t sweeps_per_step,
                        const float* alpha_base, const float* beta_base,
                        const float* alpha_slope, const float* beta_slope,
                        float* g_alpha_base, float* g_beta_base, float* g_alpha_slope, float* g_beta_slope,
                        const void* steps_workspace, const void* workspace, void* stream);

/* The same sequence looped on the host inside the library: ONE call per layer forward / backward.
 * mode 1: u <- M u before every step (cifar10.py:91, cifar_2version.py:86); 2: after every step
 * (SVHN.py:71).  `states`: K*2 tensors of u's shape and type, K = num_sweeps / sweeps_per_step —
 * states[2k] the output of step k's first operator, states[2k+1] of its second; the layer output is
 * states[2K-1].  The backward needs them intact, and `u`.  ckpt_mask is relative to a step.
 * pde_adi_mixed_one_launch: 1 when the forward of (d, sweeps_per_step) runs as the factorisation plus ONE launch
 * (fp32 tensors, C = 32 or 64, N = 28 or 32, every step x,y,x or x,y: a workgroup owns all channels of a sample for
 * the whole time loop and mixes them with the fp32 MFMA through LDS; the environment variable PDE_WIDE=0 turns it
 * off), else 0: one mixing launch and one sweep launch per step.  In the one-launch case the forward writes only
 * the sweep output of every step (states[2k+1] for mode 1, states[2k] for mode 2) and states[2K-1]; the backward
 * recomputes the other slots itself when its checkpoints need them, so the contract above is unchanged. */
int pde_adi_mixed_one_launch(const PdeAdiDesc* d, int32_t sweeps_per_step);
int pde_adi_mixed_forward(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t mode,
                          const void* u, void* states,
                          void* y /* NULL, or where the layer output goes INSTEAD of states[2K-1] (`states` then needs 2K-1
                                     tensors only; hand the same `y` to pde_adi_mixed_backward) */,
                          const float* M,
                          const float* alpha_base, const float* beta_base,
                          const float* alpha_slope, const float* beta_slope,
                          float* kappa_max, float* kappa_max_host, void* kappa_event /* as in pde_adi_forward */,
                          void* steps_workspace, size_t workspace_bytes, void* stream);
size_t pde_adi_mixed_backward_workspace_bytes(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t num_checkpoints);
int pde_adi_mixed_backward(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t mode,
                           const void* gy, const void* u, const void* states, const void* y /* as in the forward */,
                           const float* M,
                           const uint64_t ckpt_mask[2], void* gu,
                           const float* alpha_base, const float* beta_base,
                           const float* alpha_slope, const float* beta_slope,
                           float* g_alpha_base, float* g_beta_base, float* g_alpha_slope, float* g_beta_slope,
                           float* gM, const void* steps_workspace,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- K1, the whole layer in ONE launch per pass (C <= 4) -------------------------------------------
 * The reference's own models run these layers at C = 3 (cifar10.py:253-258: mixing before every step;
 * SVHN.py:238: coupling after every step, then the skip blend :73-74); per-step launches are bound by the
 * host's launch rate there.  Here a workgroup owns all C channels of its samples (one wave per channel) and
 * applies the C x C operator in registers at the step boundaries, so the forward is the factorisation kernel
 * plus one launch, the backward one launch plus the gradient epilogue.
 * pde_adi_small_supported: 1 when (d, sweeps_per_step) can take this path (C <= 4; N = 16, 28 or 32; every
 * step x,y,x or x,y), else 0 — callers then use pde_adi_mixed_*.
 * mode as in pde_adi_mixed_forward.  skip_weight: NULL, or (mode 2 only) the device scalar of SVHN.py:36: the
 * output is sigmoid(w) u + (1 - sigmoid(w)) u_K.  states: NULL (inference), or K tensors of u's shape and
 * type that receive the sweep output of every step (the backward needs them).  steps_workspace:
 * pde_adi_steps_workspace_bytes(); kappa_*: as in pde_adi_forward. */
int pde_adi_small_supported(const PdeAdiDesc* d, int32_t sweeps_per_step);
int pde_adi_small_forward(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t mode,
                          const void* u, void* y, void* states, const float* M, const float* skip_weight,
                          const float* alpha_base, const float* beta_base,
                          const float* alpha_slope, const float* beta_slope,
                          float* kappa_max, float* kappa_max_host, void* kappa_event,
                          void* steps_workspace, size_t workspace_bytes, void* stream);
size_t pde_adi_small_backward_workspace_bytes(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t num_checkpoints);
/* Exact reverse-mode derivative of pde_adi_small_forward: gu, the four coefficient gradients, gM (C,C) and,
 * with a skip blend, *g_skip_weight; all overwritten.  ckpt_mask is relative to a step (bit i: keep the state
 * after sweep i of every step instead of rebuilding it; the call then first re-runs the forward to park them). */
int pde_adi_small_backward(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t mode,
                           const void* gy, const void* u, const void* states, const float* M, const float* skip_weight,
                           const uint64_t ckpt_mask[2], void* gu,
                           const float* alpha_base, const float* beta_base,
                           const float* alpha_slope, const float* beta_slope,
                           float* g_alpha_base, float* g_beta_base, float* g_alpha_slope, float* g_beta_slope,
                           float* gM, float* g_skip_weight, const void* steps_workspace,
                           void* workspace, size_t workspace_bytes, void* stream);

/* The trajectory of such a layer out of the SAME launches: pde_adi_small_forward / _backward without the skip blend
 * (no skip_weight / g_skip_weight) that also return the state after chosen time steps, and take an upstream gradient
 * for every one of them.  emit_mask is indexed by time step: bit k (0-based) = the state after step k, what the
 * reference's loop holds at the end of iteration k — mode 1 the step's sweep output, mode 2 the sweep output after the
 * coupling.  Only bits 0 .. K-2 may be set, K = num_sweeps / sweeps_per_step (the state after the last step is y).
 * forward_states: the emitted states go to traj[slot(k)][B][C][N][N] in io_dtype, slots in the order of the set bits; a
 * caller that wants one stacked tensor points y at the slice behind the last slot.  `states` as in the plain call (NULL:
 * inference).  With 16-bit tensors the emitting forward always goes on from the rounded sweep output of every step,
 * whether `states` is kept or not (the plain call does so only when it keeps them), so traj and y do not depend on
 * `states`, and the backward reads what the forward went on from; an emitted mode-2 state is the fp32 value rounded once.
 * backward_states: gtraj has the layout of traj and holds dL/d(state); at the top of the reverse iteration of step k the
 * adjoint gets += gtraj[slot(k)] (mode 2: before the adjoint of the coupling, mode 1: before the step's adjoint sweeps).
 * State rebuild, step-local checkpoints, masked channels, gM and the coefficient sums are those of the plain call.
 * Workspaces are those of the plain calls.  Checked on the host before any launch: traj / gtraj NULL with a non-empty
 * mask, a bit at or above K-1, or a descriptor pde_adi_small_supported refuses: PDE_E_BADARG.  An empty (or NULL) mask
 * is the plain call exactly, traj / gtraj are then not read. */
int pde_adi_small_forward_states(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t mode,
                                 const void* u, void* y, void* states, void* traj, const uint64_t emit_mask[2],
                                 const float* M,
                                 const float* alpha_base, const float* beta_base,
                                 const float* alpha_slope, const float* beta_slope,
                                 float* kappa_max, float* kappa_max_host, void* kappa_event,
                                 void* steps_workspace, size_t workspace_bytes, void* stream);
int pde_adi_small_backward_states(const PdeAdiDesc* d, int32_t sweeps_per_step, int32_t mode,
                                  const void* gy, const void* gtraj, const uint64_t emit_mask[2],
                                  const void* u, const void* states, const float* M,
                                  const uint64_t ckpt_mask[2], void* gu,
                                  const float* alpha_base, const float* beta_base,
                                  const float* alpha_slope, const float* beta_slope,
                                  float* g_alpha_base, float* g_beta_base, float* g_alpha_slope, float* g_beta_slope,
                                  float* gM, const void* steps_workspace,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- K1, layers that share an input, in ONE launch per pass ------------------------
 * cifar10.py:272-274 runs three EnhancedDiffusionLayers (5, 8 and 4 steps with their own dt/dx and their own
 * parameters) on the same x and combines them with softmax weights (:277-280); cifar_2version.py:287-288 two.
 * pde_adi_multi_forward runs up to 4 such layers (C <= 4, mode 1) inside one launch — every workgroup walks its
 * samples through layer after layer, or, while the batch alone does not fill the chip (B < 1024), the layers run side
 * by side (one layer per workgroup; the terms of `out` / `gu` meet in a small second launch, in a fixed order) — and
 * writes out = sum_i weight_i * y_i; the y_i themselves are the last of each layer's `states`.  One layer with
 * weight 1 is pde_adi_small_forward; one layer with another weight gives out = r(weight_0 * y_0) like any term.
 * How `out` is rounded (r: one rounding to io_dtype; the arithmetic is fp32; with 16-bit tensors and kept `states`
 * y_i is the rounded value the layer's last state holds):
 *   side by side (num_layers > 1, B < 1024)   t_i = r(weight_i * y_i) per layer, then out = r(((t_0 + t_1) + t_2) + t_3),
 *                                             the sum in fp32 in layer order: one rounding per term plus one of the sum
 *                                             (fp32 tensors: the L-1 fp32 additions are the roundings of the sum);
 *   one after the other (B >= 1024)           out_0 = r(weight_0 * y_0), out_i = r(fma(weight_i, y_i, out_{i-1})) with
 *                                             out_{i-1} re-read in io_dtype: L roundings of the running sum.
 * Either way |out - sum_i weight_i y_i| <= (L+1) eps sum_i |weight_i y_i| elementwise, eps = 2^-24 / 2^-8 / 2^-11 for
 * fp32 / bf16 / fp16 (plus (L+1) 2^-25 where fp16 results are subnormal).  gu = sum_i gu_i is built the same two ways.
 * The backward takes gy = dL/dout and/or per layer gys = dL/dy_i, and gives gu = sum_i gu_i, every layer's
 * parameter gradients, and g_weight = <gy, y_i>. */
typedef struct PdeSmallLayer {
    const PdeAdiDesc* desc;          /* the layer's own schedule; B, C, N, io_dtype equal across the layers  */
    int32_t sweeps_per_step;         /* equal across the layers (all Strang or all Lie)                       */
    int32_t mode;                    /* 1 | 2 as in pde_adi_mixed_forward; several layers: 1 only             */
    const float* M;                  /* (C,C)                                                                  */
    const float* skip_weight;        /* NULL | device scalar (mode 2)                                          */
    const float* alpha_base; const float* beta_base; const float* alpha_slope; const float* beta_slope;
    float weight;                    /* weight_i ...                                                           */
    const float* weight_ptr;         /* ... or, when not NULL, a device scalar holding it (no host round trip)  */
    void* states;                    /* K_i tensors (forward: NULL = inference)                                */
    float* plane_sums;               /* NULL | (B,C): forward writes sum over the plane of y_i (the adaptive average
                                        pool of cifar10.py:239 times H*W, at no extra pass)                      */
    void* steps_workspace; size_t steps_workspace_bytes;     /* pde_adi_steps_workspace_bytes(desc, sps)      */
    float* kappa_max; float* kappa_max_host;                 /* optional, as in pde_adi_forward               */
    /* backward only */
    const void* gys;                 /* NULL | dL/dy_i                                                         */
    const float* g_plane_sums;       /* NULL | (B,C) dL/d(plane_sums_i): added to every element of the plane    */
    const uint64_t* ckpt_mask;       /* relative to a step                                                     */
    float* g_alpha_base; float* g_beta_base; float* g_alpha_slope; float* g_beta_slope;
    float* gM; float* g_skip_weight; float* g_weight;        /* g_weight optional                              */
    void* workspace; size_t workspace_bytes;                 /* pde_adi_small_backward_workspace_bytes()      */
} PdeSmallLayer;
int pde_adi_multi_forward(int32_t num_layers, const PdeSmallLayer* layers, const void* u, void* out,
                          void* kappa_event, void* stream);
int pde_adi_multi_backward(int32_t num_layers, const PdeSmallLayer* layers, const void* gy, const void* u,
                           void* gu, void* stream);

/* ---- channel operators ------------------------------------------ */

/* out[b,i,p] = sum_j M[i,j] u[b,j,p]  — cifar10.py:65-72 apply_channel_mixing and
 * SVHN.py:78-86 apply_channel_coupling (both reduce to this).  M: (C,C) fp32 row-major.
 * u,out: (B,C,HW) of io_dtype; out must not alias u.  With PDE_IO_F16 (the float16 route, where M is an fp16 parameter)
 * M is expected to hold fp16 values: at C = 64 and 128 the products run on the fp16 matrix cores with M rounded to fp16,
 * as torch's fp16 matmul takes it; every other width multiplies by the fp32 values given. */
int pde_channel_mix_forward(int32_t B, int32_t C, int32_t HW, int32_t io_dtype,
                            const void* u, const float* M, void* out, void* stream);
/* gu[b,j,p] = sum_i M[i,j] gout[b,i,p];  gM[i,j] = sum_{b,p} gout[b,i,p] u[b,j,p].
 * workspace: pde_channel_mix_backward_workspace_bytes(). */
size_t pde_channel_mix_backward_workspace_bytes(int32_t B, int32_t C, int32_t HW);
int pde_channel_mix_backward(int32_t B, int32_t C, int32_t HW, int32_t io_dtype,
                             const void* u, const void* gout, const float* M,
                             void* gu, float* gM,
                             void* workspace, size_t workspace_bytes, void* stream);
/* The same with gM spread over several calls that share `workspace` (one per time step of a layer):
 * accumulate = 0 starts the partial sums, 1 adds to them; finalize = 1 reduces them into gM
 * (gM may be NULL otherwise).  The workspace's contents do not matter before the accumulate = 0 call and must stay
 * intact from there to the finalising one; gu is overwritten by every call. */
int pde_channel_mix_backward_steps(int32_t B, int32_t C, int32_t HW, int32_t io_dtype,
                                   const void* u, const void* gout, const float* M,
                                   void* gu, float* gM,
                                   void* workspace, size_t workspace_bytes,
                                   int32_t accumulate, int32_t finalize, void* stream);
/* Which kernel family pde_channel_mix_forward (backward = 0) or pde_channel_mix_backward[_steps] (backward = 1) runs
 * for these arguments; the entry points dispatch on the value this function returns.  PDE_E_BADARG for dimensions or an
 * io_dtype they refuse.  The PDE_MIX_NO_BF16_MFMA, PDE_MIX_NO_SPLIT and PDE_MIX_UNFUSED environment switches are read
 * on every call, here as there; so are PDE_RH_NO_STRIP32, PDE_RH_SPLIT and PDE_RH_NO_SPLIT of the symmetric layer
 * (pde_sym_layer_path below).
 *   code                     forward                             backward
 *   PDE_MIX_PATH_SCALAR      mix_apply_kernel                    transposed mix_apply_kernel + mix_gm_kernel
 *   PDE_MIX_PATH_MFMA_F32    mix_apply_mfma_kernel               unfused: transposed mix_apply_mfma_kernel + mix_gm_mfma_kernel
 *                            (C % 32 == 0, C <= 128, HW % 4 == 0)  (the same shapes, where no fused kernel takes them)
 *   PDE_MIX_PATH_MFMA_16     mix_apply_bf16_kernel<MixBf16|MixF16>  mix_bwd_bf16_kernel<MixBf16|MixF16>, exact products
 *                            (bf16 / fp16 tensors, C = 64 or 128, HW % 64 == 0)
 *   PDE_MIX_PATH_SPLIT3      -                                   mix_bwd_split_kernel, three bf16 pieces per operand
 *                                                                (fp32 tensors, C = 32, 64 or 96, HW % 4 == 0)
 *   PDE_MIX_PATH_FUSED       -                                   mix_bwd_fused_kernel (C = 32, 64, 96: M^T fragments in LDS;
 *                                                                C = 128: in the workspace), HW % 4 == 0
 * Every backward ends in mix_gm_reduce_kernel when finalize = 1. */
#define PDE_MIX_PATH_SCALAR   0
#define PDE_MIX_PATH_MFMA_F32 1
#define PDE_MIX_PATH_MFMA_16  2
#define PDE_MIX_PATH_SPLIT3   3
#define PDE_MIX_PATH_FUSED    4
int pde_channel_mix_path(int32_t B, int32_t C, int32_t HW, int32_t io_dtype, int32_t backward);
/* How that path spreads its work: the return value is the number of walkers — workgroups of a backward kernel (= partial
 * matrices in the workspace), workgroups of the 16-bit forward kernel, waves of the fp32-MFMA forward kernel — and
 * *chunks (optional) the number of pixel chunks they share out, chunk c going to walker c % walkers.  chunks > walkers
 * means some walkers take more than one trip of their loop.  The scalar forward kernel has no loop: walkers = chunks.
 * PDE_E_BADARG as above. */
int pde_channel_mix_splits(int32_t B, int32_t C, int32_t HW, int32_t io_dtype, int32_t backward, int64_t* chunks);

/* SVHN.py:73-74 skip connection: out = s*u0 + (1-s)*u with s = sigmoid(*skip_weight) (device scalar), n
 * elements of io_dtype, one pass.  Backward: g_u0 = s*g, g_u = (1-s)*g,
 * *g_skip_weight = s(1-s) * sum g*(u0-u) (deterministic two-stage sum). */
int pde_skip_blend_forward(int64_t n, int32_t io_dtype, const void* u0, const void* u,
                           const float* skip_weight, void* out, void* stream);
size_t pde_skip_blend_backward_workspace_bytes(int64_t n);
int pde_skip_blend_backward(int64_t n, int32_t io_dtype, const void* g, const void* u0, const void* u,
                            const float* skip_weight, void* g_u0, void* g_u, float* g_skip_weight,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- epilogue behind the shared-input layers -------------------------------------------
 * cifar10.py:270-280: features_i = y_i * gate_i[b,c] (SpatialAttention :232-244), combined = sum_i w_i features_i.
 * The gates are a small MLP of the average pool of y_i + pos_embed: the pool comes out of pde_adi_multi_forward
 * (PdeSmallLayer.plane_sums), the (B,C) MLP stays with the caller; these two calls are the passes over the full
 * tensors that remain.  ys: L <= 4 tensors (B,C,HW) of io_dtype; gates: L arrays (B,C) fp32; weights: (L) fp32 on
 * the device; HW a multiple of 4.
 *   forward : out[b,c,p]  = sum_i weights[i] gates[i][b,c] ys[i][b,c,p]
 *   backward: gys[i][b,c,p] = weights[i] gates[i][b,c] g[b,c,p];  dots[i][b,c] = sum_p g[b,c,p] ys[i][b,c,p]
 *             (dL/dgate_i = weights[i] dots[i], dL/dweights[i] = sum_bc gates[i] dots[i]). */
int pde_gate_combine_forward(int32_t L, int32_t B, int32_t C, int32_t HW, int32_t io_dtype,
                             const void* const* ys, const float* const* gates, const float* weights,
                             void* out, void* stream);
int pde_gate_combine_backward(int32_t L, int32_t B, int32_t C, int32_t HW, int32_t io_dtype, const void* g,
                              const void* const* ys, const float* const* gates, const float* weights,
                              void* const* gys, float* const* dots, void* stream);

/* ---- what follows the feature extractor in cifar10.CIFAR10PDENoConv ----------------------
 * cifar10.py:346-353: features = BatchNorm2d(combined); pooled = cat([AdaptiveAvgPool2d(4,4)(features),
 * AdaptiveMaxPool2d(4,4)(features)], dim=1).  `features` is never written: out (B,2C,4,4) fp32 comes straight from x
 * (B,C,N,N) fp32, N a multiple of 4 and <= 64.  training != 0: statistics of the batch (biased variance for the
 * normalisation; running_mean / running_var, when given, updated with `momentum` and the unbiased variance, as
 * torch.nn.BatchNorm2d does); else the running statistics.  gamma / beta may be NULL (1 / 0).  mean, invstd: (C)
 * outputs the backward needs, argmax: (B,C,4,4) int32 positions of the maxima inside their planes.
 * backward: gout (B,2C,4,4) -> gx, ggamma, gbeta (all overwritten). */
size_t pde_bn_pool_workspace_bytes(int32_t B, int32_t C);
int pde_bn_pool_forward(int32_t B, int32_t C, int32_t N, const float* x, const float* gamma, const float* beta,
                        float eps, int32_t training, float momentum, float* running_mean, float* running_var,
                        float* mean, float* invstd, float* out, int32_t* argmax,
                        void* workspace, size_t workspace_bytes, void* stream);
int pde_bn_pool_backward(int32_t B, int32_t C, int32_t N, const float* x, const float* gamma, const float* mean,
                         const float* invstd, const int32_t* argmax, const float* gout, int32_t training,
                         float* gx, float* ggamma, float* gbeta,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- K2: explicit 5-point layers --------------------------- */

/* tiny_imagenet.py:34-72: `num_steps` relaxed explicit steps (the reference's loop :44-49), each
 *   a_c = clamp(alpha_base_c, eps, max_coeff);  v = s_c u;
 *   u <- u + relax*(v + a_c*dt*Lap0(v) - u)      (Lap0: zero ghost cells, padding=1)
 * u,out: (B,C,H,W) of io_dtype (PDE_IO_F32 | PDE_IO_BF16 | PDE_IO_F16), any plane with H >= 1 and W >= 1 (H or W <= 0:
 * PDE_E_BADARG): 64x64, 32x32 and 16x16 run on the wave-per-plane kernels, every other plane on the generic kernel — in
 * float4 columns when W is a multiple of 4, in single columns otherwise (rows then start off a 16-byte boundary; this
 * variant is a correctness path and has not been timed).  states: NULL, or room for (num_steps-1) FP32 tensors of u's shape (whatever io_dtype:
 * with bf16 tensors only the layer's own input, output and gradients are bf16) that receive the inputs of steps
 * 2..num_steps (what pde_explicit5_backward needs); required for num_steps > 1 unless the plane is 64x64, 32x32 or 16x16
 * (those stay in registers over all steps, one launch); when given, all of it is written at every plane size. */
int pde_explicit5_forward(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype,
                          const void* u, const float* alpha_base, const float* channel_scaling,
                          float dt, float eps, float max_coeff, float relax,
                          int32_t num_steps, void* states, void* out, void* stream);
size_t pde_explicit5_backward_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype,
                                              int32_t num_steps);
/* gu, g_alpha_base (C), g_channel_scaling (C): overwritten.  states: as written by the forward call
 * (may be NULL when num_steps == 1). */
int pde_explicit5_backward(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype,
                           const void* u, const void* states, const void* gout,
                           const float* alpha_base, const float* channel_scaling,
                           float dt, float eps, float max_coeff, float relax, int32_t num_steps,
                           void* gu, float* g_alpha_base, float* g_channel_scaling,
                           void* workspace, size_t workspace_bytes, void* stream);

/* emotion_recognition.py:82-97: reflect-pad once, nt Jacobi updates of the interior with
 * row coefficients a_row[H] (multiplying the second difference along H) and column
 * coefficients b_col[W] (along W); the padded ring keeps its initial values.
 * u,out: (B,H,W) fp32 (the layer is single-channel), 4 <= H, W <= PDE_JACOBI_MAX_HW.  pde_jacobi_io_*: the same with
 * u, out, gout, gu of io_dtype (PDE_IO_F32 | PDE_IO_BF16 | PDE_IO_F16); the time loop stays fp32 in LDS.
 * Planes up to 64x64 run on the one-workgroup kernels (a sample's padded plane stays in the LDS of one workgroup for
 * the whole time loop); a plane with H > 64 or W > 64 runs on the tiled kernels: a workgroup owns a 64x64 tile of one
 * sample and advances it PDE_JACOBI_TILED_K steps per launch on a halo of that many cells; parked states and whatever
 * passes between launches are fp32.  The float64 entry points (pde_jacobi_f64_*) stay at H, W <= 64. */
#define PDE_JACOBI_MAX_HW 1024
#define PDE_JACOBI_TILED_K 10
/* which kernels serve an (H, W) plane: 0 none (PDE_E_BADARG), 1 the one-workgroup kernels (4 <= H, W <= 64), 2 the
 * tiled kernels (up to PDE_JACOBI_MAX_HW).  The tiled kernels advance K = PDE_JACOBI_TILED_K = 10 time steps per
 * launch: a forward of nt steps is ceil(nt / K) launches. */
int pde_jacobi_plane_path(int32_t H, int32_t W);
/* Tiled planes with nt > PDE_JACOBI_TILED_K: the launches of one forward hand the state on through two fp32 images,
 * which pde_jacobi_io_forward_ws takes as `workspace` (pde_jacobi_forward_workspace_bytes; 0 for every other call, and
 * workspace may then be NULL).  pde_jacobi_forward / pde_jacobi_io_forward are this call without a workspace: they
 * serve every plane up to nt = PDE_JACOBI_TILED_K on the tiled path and return PDE_E_WORKSPACE beyond. */
size_t pde_jacobi_forward_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t nt);
int pde_jacobi_io_forward_ws(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype,
                             const void* u, const float* a_row, const float* b_col, void* out,
                             void* workspace, size_t workspace_bytes, void* stream);
int pde_jacobi_forward(int32_t B, int32_t H, int32_t W, int32_t nt,
                       const float* u, const float* a_row, const float* b_col,
                       float* out, void* stream);
size_t pde_jacobi_backward_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t nt);
/* gu (B,H,W), g_a_row[H], g_b_col[W]: overwritten. */
int pde_jacobi_backward(int32_t B, int32_t H, int32_t W, int32_t nt,
                        const float* u, const float* gout,
                        const float* a_row, const float* b_col,
                        float* gu, float* g_a_row, float* g_b_col,
                        void* workspace, size_t workspace_bytes, void* stream);
int pde_jacobi_io_forward(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype,
                          const void* u, const float* a_row, const float* b_col, void* out, void* stream);
size_t pde_jacobi_io_backward_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype);
int pde_jacobi_io_backward(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype,
                           const void* u, const void* gout, const float* a_row, const float* b_col,
                           void* gu, float* g_a_row, float* g_b_col,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- the trajectory of the explicit layers: intermediate states of the time loop out of the plain call's launches ----
 * pde_jacobi_io_forward_ws / pde_explicit5_forward that also return the state after chosen time steps, and the backwards
 * that take an upstream gradient for every one of them.  The contract is that of pde_adi_forward_states, indexed by time
 * step: emit_mask[2] is 128 bits, bit k-1 (bit (k-1)%64 of emit_mask[(k-1)/64]) set = the state after time step k is
 * emitted, slots in the order of the set bits.  Only bits 0 .. nt-2 (num_steps-2) may be set: the state after the last
 * step is `out` itself, and a caller that wants one stacked tensor points `out` at the slice behind the last slot.
 * forward_states: the Jacobi calls write states[slot][B][H][W] (the interior of the padded plane), the explicit calls
 * traj[slot][B][C][H][W] (their `states` stays the fp32 workspace of the plain call), both in io_dtype; with 16-bit
 * tensors an emitted state is the fp32 state rounded once — the time loop goes on unrounded, so `out` and every emitted
 * state are bit for bit what the plain call of that many steps returns.
 * backward_states: gstates / gtraj has the layout of states / traj and holds dL/d(state); when the reverse walk holds the
 * adjoint of the state after step k it gets += gstates[slot(k)] on the interior cells (the frozen Jacobi ring gets
 * nothing).  Parked states, the order of the partial sums, the pgrad kernels and the fold of the reflect padding are those
 * of the plain backward; no float atomics.
 * Checked on the host before any launch, after the plain call's own argument checks: a non-empty mask with nt
 * (num_steps) > 128: PDE_E_TOO_MANY_SWEEPS; a bit at or above nt-1, or states / traj / gstates / gtraj NULL with a
 * non-empty mask: PDE_E_BADARG; then the workspace.  An empty (or NULL) mask is the plain call exactly — the same kernel
 * instantiations, states / traj / gstates / gtraj are not read; the plain entry points are these calls with a NULL mask.
 * Workspaces are those of the plain calls (the forward takes the workspace of pde_jacobi_io_forward_ws).
 * Launches are the plain call's; emission and injection add global writes and reads to them, never a launch: the
 * one-workgroup Jacobi kernels and the wave-per-plane explicit kernels (64x64, 32x32, 16x16) emit from LDS / registers
 * after the step; the tiled Jacobi forward writes the tile's own cells after the step (ceil(nt / K) launches), its
 * adjoint adds gstates[slot(n)] to G_n on every interior cell of the region still valid at that step, so neighbouring
 * tiles keep agreeing on their shared halo and no launch is cut at an emitted step; the generic explicit planes run one
 * launch per step as the plain call, the step's own launch writing traj / adding gtraj. */
int pde_jacobi_io_forward_states(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype,
                                 const void* u, const float* a_row, const float* b_col, void* out,
                                 void* states, const uint64_t emit_mask[2],
                                 void* workspace, size_t workspace_bytes, void* stream);
int pde_jacobi_io_backward_states(int32_t B, int32_t H, int32_t W, int32_t nt, int32_t io_dtype,
                                  const void* u, const void* gout, const void* gstates, const uint64_t emit_mask[2],
                                  const float* a_row, const float* b_col,
                                  void* gu, float* g_a_row, float* g_b_col,
                                  void* workspace, size_t workspace_bytes, void* stream);
int pde_explicit5_forward_states(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype,
                                 const void* u, const float* alpha_base, const float* channel_scaling,
                                 float dt, float eps, float max_coeff, float relax,
                                 int32_t num_steps, void* states, void* out,
                                 void* traj, const uint64_t emit_mask[2], void* stream);
int pde_explicit5_backward_states(int32_t B, int32_t C, int32_t H, int32_t W, int32_t io_dtype,
                                  const void* u, const void* states, const void* gout,
                                  const void* gtraj, const uint64_t emit_mask[2],
                                  const float* alpha_base, const float* channel_scaling,
                                  float dt, float eps, float max_coeff, float relax, int32_t num_steps,
                                  void* gu, float* g_alpha_base, float* g_channel_scaling,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- Ruthotto-Haber symmetric layer on the fp32 matrix cores ------------- */

/* cifar_2version.py:190-220 SymmetricLayer.forward and the residual steps built on it (ParabolicBlock :223-236,
 * HamiltonianBlock :239-258), fused:
 *     P = X K^T;  H = act(BatchNorm1d(P));  out = base + scale * (H K)
 * X, base, out, P, H: (B, D) fp32 row-major (the image batch flattened, D = C*H*W); K: (D, D) = nn.Linear weight;
 * bn_weight / bn_bias / running_mean / running_var: (D).  act: 0 identity, 1 relu, 2 tanh (cifar_2version.py:203-208).
 * training != 0: batch statistics (biased variance for normalisation; running statistics updated with `momentum`
 * and the unbiased variance, as torch.nn.BatchNorm1d does; running_* may be NULL = not tracked); training == 0:
 * running statistics.  P, H, mean[D], invstd[D] are written for the backward; base may be NULL (then out = scale*(H K)).
 * F_sym(Y) itself is base = NULL, scale = -1.  D a multiple of 64 (pde_sym_layer_supported); up to 128 batch rows the
 * statistics are the epilogue of the first product, larger batches run it by row blocks with a statistics pass beside it.
 * workspace: NULL, or pde_sym_layer_workspace_bytes(B, D) bytes of scratch (16-byte aligned; contents do not matter, no
 * two calls that share it in flight at once): with it, batches up to 128 rows run each product as 32-column strips whose
 * contraction is split over workgroups, the partial tiles added in a fixed order by a small second launch that also
 * carries the epilogue.  Without it (or where pde_sym_layer_workspace_bytes is 0): one workgroup per 16-column strip. */
int pde_sym_layer_supported(int32_t B, int32_t D);
size_t pde_sym_layer_workspace_bytes(int32_t B, int32_t D);
int pde_sym_layer_forward(int32_t B, int32_t D, int32_t act, int32_t training,
                          const float* X, const float* K, const float* bn_weight, const float* bn_bias,
                          float* running_mean, float* running_var, float momentum, float eps,
                          const float* base, float scale,
                          float* P, float* H, float* mean, float* invstd, float* out,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Backward of the above for an upstream gradient g_out (B, D) of `out` (the gradient of `base` is g_out itself and is
 * left to the caller).  dP: (B, D) scratch.  Overwritten: gX (B, D), gK (D, D) — both uses of K —, g_bn_weight[D],
 * g_bn_bias[D].  workspace: as in pde_sym_layer_forward (the same one may serve both). */
int pde_sym_layer_backward(int32_t B, int32_t D, int32_t act, int32_t training,
                           const float* g_out, float scale, const float* X, const float* K, const float* bn_weight,
                           const float* P, const float* H, const float* mean, const float* invstd,
                           float* dP, float* gX, float* gK, float* g_bn_weight, float* g_bn_bias,
                           void* workspace, size_t workspace_bytes, void* stream);
/* Which kernels pde_sym_layer_forward / _backward run for these dimensions, with (has_workspace != 0) or without a
 * workspace; the entry points and pde_sym_layer_workspace_bytes dispatch on the same function.  Returns the family, or
 * PDE_E_BADARG for what pde_sym_layer_supported refuses (the out-pointers are then left alone); each out-pointer may be
 * NULL.  The PDE_RH_NO_STRIP32, PDE_RH_SPLIT and PDE_RH_NO_SPLIT environment switches are read on every call, here as
 * there (as the PDE_MIX_* ones are), so a process can select a path between two calls.
 *   family                  products and epilogues                                        *split  *waves  *row_blocks
 *   PDE_RH_PATH_STRIP32     rh_part32_kernel + rh_fwd32_epi / rh_bwd32_epi / rh_axpy32_epi  S       2 | 4   1
 *                           (B <= 128, a workspace, S >= 2; two waves up to 64 rows)
 *   PDE_RH_PATH_STRIP16     rh_fwd_strip / rh_bwd_strip / rh_axpy_strip_kernel              0       8       1
 *                           (B <= 128 otherwise: no workspace, S < 2, PDE_RH_NO_STRIP32)
 *   PDE_RH_PATH_ROW_BLOCKS  rh_nt_strip + rh_bn_fwd / rh_bn_bwd + rh_axpy_strip_kernel      0       8       ceil(B / 128)
 * S: the slices of a strip's contraction — the largest power of two <= 8 (or <= PDE_RH_SPLIT, a power of two in 2..16)
 * with D % (64 S) == 0 and (D / 32) S <= 2048 workgroups with two waves, 1024 with four.  The workspace holds
 * (D / 32) * S * waves * 1024 floats. */
#define PDE_RH_PATH_STRIP32    0
#define PDE_RH_PATH_STRIP16    1
#define PDE_RH_PATH_ROW_BLOCKS 2
int pde_sym_layer_path(int32_t B, int32_t D, int32_t has_workspace, int32_t* split, int32_t* waves, int32_t* row_blocks);
/* The kernel of the gradient of K in pde_sym_layer_backward: PDE_RH_DK_SPLIT3 (rh_outer_split_kernel, every fp32 operand
 * as three bf16 pieces) or, under PDE_RH_NO_SPLIT, PDE_RH_DK_MFMA_F32 (rh_outer_kernel); PDE_E_BADARG as above. */
#define PDE_RH_DK_SPLIT3   0
#define PDE_RH_DK_MFMA_F32 1
int pde_sym_layer_dk_path(int32_t B, int32_t D);

/* ---- the same layer under CUDA fp16 autocast, on the fp16 matrix cores ---------------------- */

/* The rounding points of torch.autocast("cuda", torch.float16) for the layer above, r() = round to fp16 (overflow to
 * +-inf), accumulation in fp32:
 *     P = r(r(X) K16^T);  N = r(BatchNorm1d(P));  H = r(act(N));  Q = r(H K16);  out = base + r(scale Q)
 * The products by `scale` (scale Q here, scale r(g_out) in the backward) are fp32 multiplications rounded to fp32 before
 * r() rounds them again, as autocast's element-wise kernels do — not one rounding of the exact product: at scale = 0.7
 * the two differ by a 16-bit step for one element in forty.  The sign of a zero is not specified.
 * K16: (D, D) fp16 = r(K) (pde_sym_k_to_f16, once per autocast region).  X, base: (B, D) fp32.  P, H: (B, D) fp16,
 * written for the backward.  out: fp16 (B, D) = r(scale Q) when base is NULL (F_sym(Y) is scale = -1), fp32 (B, D)
 * otherwise.  Statistics, running statistics, mean and invstd as in pde_sym_layer_forward.  1 <= B <= 128 and D a
 * multiple of 64 (pde_sym_layer_f16_supported).  workspace: pde_sym_layer_f16_workspace_bytes(B, D) bytes, 16-byte
 * aligned, not NULL (the partial tiles of the split products; no two calls that share it in flight at once).
 * fp16 tensors are passed as their 16-bit patterns. */
int pde_sym_layer_f16_supported(int32_t B, int32_t D);
size_t pde_sym_layer_f16_workspace_bytes(int32_t B, int32_t D);
/* K16 = r(K), K: (D, D) fp32 */
int pde_sym_k_to_f16(int32_t D, const float* K, uint16_t* K16, void* stream);
int pde_sym_layer_f16_forward(int32_t B, int32_t D, int32_t act, int32_t training,
                              const float* X, const uint16_t* K16, const float* bn_weight, const float* bn_bias,
                              float* running_mean, float* running_var, float momentum, float eps,
                              const float* base, float scale,
                              uint16_t* P, uint16_t* H, float* mean, float* invstd, void* out,
                              void* workspace, size_t workspace_bytes, void* stream);
/* Backward for an fp32 upstream gradient g_out (B, D) of `out` (an fp16 one widened by the caller), with autocast's
 * fp16 operands: gQ = r(scale r(g_out)), dP = r(BatchNorm backward of (gQ K16^T) act'(H)) written to dP (B, D) fp16;
 * gX = dP K16, gK = dP^T r(X) + H^T gQ (D, D), g_bn_weight[D], g_bn_bias[D] in fp32.  X is the forward's fp32 input. */
int pde_sym_layer_f16_backward(int32_t B, int32_t D, int32_t act, int32_t training,
                               const float* g_out, float scale, const float* X, const uint16_t* K16, const float* bn_weight,
                               const uint16_t* P, const uint16_t* H, const float* mean, const float* invstd,
                               uint16_t* dP, float* gX, float* gK, float* g_bn_weight, float* g_bn_bias,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---- the same layer under CUDA bf16 autocast, on the bf16 matrix cores ---------------------- */

/* The fp16-autocast contract above with r() = round to nearest even to bf16 — the rounding points of
 * torch.autocast("cuda", torch.bfloat16); bf16 has fp32's exponent range, so no r() overflows:
 *     K16 = r(K);  P = r(r(X) K16^T);  N = r(BatchNorm1d(P));  H = r(act(N));  Q = r(H K16);  out = base + r(scale Q)
 * Argument lists, shapes (1 <= B <= 128, D a multiple of 64), workspace size, argument checks and error codes are those
 * of the pde_sym_layer_f16_* functions; K16, P, H, dP and a base-less `out` are bf16, passed as their 16-bit patterns.
 * Backward: gQ = r(scale r(g_out)), dP = r(...), gX = dP K16, gK = dP^T r(X) + H^T gQ, all accumulated in fp32. */
int pde_sym_layer_bf16_supported(int32_t B, int32_t D);
size_t pde_sym_layer_bf16_workspace_bytes(int32_t B, int32_t D);
/* K16 = r(K), K: (D, D) fp32 */
int pde_sym_k_to_bf16(int32_t D, const float* K, uint16_t* K16, void* stream);
int pde_sym_layer_bf16_forward(int32_t B, int32_t D, int32_t act, int32_t training,
                               const float* X, const uint16_t* K16, const float* bn_weight, const float* bn_bias,
                               float* running_mean, float* running_var, float momentum, float eps,
                               const float* base, float scale,
                               uint16_t* P, uint16_t* H, float* mean, float* invstd, void* out,
                               void* workspace, size_t workspace_bytes, void* stream);
int pde_sym_layer_bf16_backward(int32_t B, int32_t D, int32_t act, int32_t training,
                                const float* g_out, float scale, const float* X, const uint16_t* K16, const float* bn_weight,
                                const uint16_t* P, const uint16_t* H, const float* mean, const float* invstd,
                                uint16_t* dP, float* gX, float* gK, float* g_bn_weight, float* g_bn_bias,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ---- float64: the same layers computed in double end to end -----------------------------------------
 * A float64 input or parameter makes the reference's torch ops run in float64 (torch type promotion), `t` and the
 * coefficient schedule included.  These entry points are that path: every tensor is float64 (double), every scalar of
 * the schedule is a double, and the arithmetic is double with true division — the reference's own recurrences, no
 * reciprocal approximations.  Parameter gradients are summed in a fixed order: two calls give the same bits.
 * Semantics, checkpoint masks and error codes as in the float32 entry point each one names. */

typedef struct PdeSweepF64 {
    int32_t axis;       /* PDE_AXIS_X / PDE_AXIS_Y */
    int32_t pad;
    double  delta;      /* dt/2 or dt, as the reference's Python floats */
    double  h2;         /* dx**2 or dy**2 */
    double  t;          /* current_time */
} PdeSweepF64;

typedef struct PdeAdiDescF64 {
    int32_t B, C, N;            /* H = W = N, 2 <= N <= PDE_MAX_N_GENERIC                */
    int32_t io_dtype;           /* PDE_IO_F64                                            */
    int32_t num_sweeps;
    int32_t smooth3;
    int32_t has_clamp_max;
    int32_t pad;
    double  clamp_max;
    double  eps;
    PdeSweepF64 sweep[PDE_MAX_SWEEPS];
} PdeAdiDescF64;

/* pde_adi_forward / pde_adi_backward in float64 (the any-size kernels at every N: one thread per line).  kappa_max: NULL
 * or num_sweeps doubles on the device.  num_checkpoints: the number of bits set in the backward's ckpt_mask. */
size_t pde_adi_f64_forward_workspace_bytes(const PdeAdiDescF64* d);
size_t pde_adi_f64_backward_workspace_bytes(const PdeAdiDescF64* d, int32_t num_checkpoints);
int pde_adi_f64_forward(const PdeAdiDescF64* d, const double* u, double* y,
                        const double* alpha_base, const double* beta_base,
                        const double* alpha_slope, const double* beta_slope,
                        double* kappa_max, void* workspace, size_t workspace_bytes, void* stream);
int pde_adi_f64_backward(const PdeAdiDescF64* d, const double* gy, const double* y, const double* u,
                         const uint64_t ckpt_mask[2], double* gu,
                         const double* alpha_base, const double* beta_base,
                         const double* alpha_slope, const double* beta_slope,
                         double* g_alpha_base, double* g_beta_base, double* g_alpha_slope, double* g_beta_slope,
                         const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream);

/* pde_adi_forward_states / pde_adi_backward_states in float64: states, gstates (slots, B, C, N, N) doubles. */
int pde_adi_f64_forward_states(const PdeAdiDescF64* d, const double* u, double* y, double* states,
                               const uint64_t emit_mask[2],
                               const double* alpha_base, const double* beta_base,
                               const double* alpha_slope, const double* beta_slope,
                               double* kappa_max, void* workspace, size_t workspace_bytes, void* stream);
int pde_adi_f64_backward_states(const PdeAdiDescF64* d, const double* gy, const double* gstates,
                                const uint64_t emit_mask[2], const double* y, const double* u,
                                const uint64_t ckpt_mask[2], double* gu,
                                const double* alpha_base, const double* beta_base,
                                const double* alpha_slope, const double* beta_slope,
                                double* g_alpha_base, double* g_beta_base, double* g_alpha_slope, double* g_beta_slope,
                                const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream);

/* pde_channel_mix_* in float64, 1 <= C <= 128.  _steps: gM spread over calls sharing `workspace` (accumulate = 0 starts
 * the sums, 1 adds; finalize = 1 writes gM). */
int pde_channel_mix_f64_forward(int32_t B, int32_t C, int32_t HW, const double* u, const double* M, double* out,
                                void* stream);
size_t pde_channel_mix_f64_backward_workspace_bytes(int32_t B, int32_t C, int32_t HW);
int pde_channel_mix_f64_backward(int32_t B, int32_t C, int32_t HW, const double* u, const double* gout, const double* M,
                                 double* gu, double* gM, void* workspace, size_t workspace_bytes, void* stream);
int pde_channel_mix_f64_backward_steps(int32_t B, int32_t C, int32_t HW, const double* u, const double* gout,
                                       const double* M, double* gu, double* gM, void* workspace, size_t workspace_bytes,
                                       int32_t accumulate, int32_t finalize, void* stream);

/* pde_skip_blend_* in float64: s = sigmoid(*skip_weight) in double, *g_skip_weight a double. */
int pde_skip_blend_f64_forward(int64_t n, const double* u0, const double* u, const double* skip_weight, double* out,
                               void* stream);
size_t pde_skip_blend_f64_backward_workspace_bytes(int64_t n);
int pde_skip_blend_f64_backward(int64_t n, const double* g, const double* u0, const double* u, const double* skip_weight,
                                double* g_u0, double* g_u, double* g_skip_weight,
                                void* workspace, size_t workspace_bytes, void* stream);

/* pde_explicit5_* in float64, any plane size.  states: room for (num_steps-1) double tensors of u's shape, required
 * when num_steps > 1 (the inputs of steps 2..num_steps). */
int pde_explicit5_f64_forward(int32_t B, int32_t C, int32_t H, int32_t W, const double* u, const double* alpha_base,
                              const double* channel_scaling, double dt, double eps, double max_coeff, double relax,
                              int32_t num_steps, double* states, double* out, void* stream);
size_t pde_explicit5_f64_backward_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t num_steps);
int pde_explicit5_f64_backward(int32_t B, int32_t C, int32_t H, int32_t W, const double* u, const double* states,
                               const double* gout, const double* alpha_base, const double* channel_scaling,
                               double dt, double eps, double max_coeff, double relax, int32_t num_steps,
                               double* gu, double* g_alpha_base, double* g_channel_scaling,
                               void* workspace, size_t workspace_bytes, void* stream);

/* pde_jacobi_* in float64, 2 <= H, W <= 64 (the one-workgroup kernels only: no tiled path in float64). */
int pde_jacobi_f64_forward(int32_t B, int32_t H, int32_t W, int32_t nt, const double* u, const double* a_row,
                           const double* b_col, double* out, void* stream);
size_t pde_jacobi_f64_backward_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t nt);
int pde_jacobi_f64_backward(int32_t B, int32_t H, int32_t W, int32_t nt, const double* u, const double* gout,
                            const double* a_row, const double* b_col, double* gu, double* g_a_row, double* g_b_col,
                            void* workspace, size_t workspace_bytes, void* stream);

/* pde_jacobi_io_*_states / pde_explicit5_*_states in float64: states, gstates (slots, B, H, W) and traj, gtraj (slots, B,
 * C, H, W) doubles; the same contract, checks and launches (one per step for the explicit layer, the step's own launch
 * writing traj / adding gtraj; one forward launch, then recompute, adjoint and reduction for the Jacobi layer). */
int pde_explicit5_f64_forward_states(int32_t B, int32_t C, int32_t H, int32_t W, const double* u, const double* alpha_base,
                                     const double* channel_scaling, double dt, double eps, double max_coeff, double relax,
                                     int32_t num_steps, double* states, double* out,
                                     double* traj, const uint64_t emit_mask[2], void* stream);
int pde_explicit5_f64_backward_states(int32_t B, int32_t C, int32_t H, int32_t W, const double* u, const double* states,
                                      const double* gout, const double* gtraj, const uint64_t emit_mask[2],
                                      const double* alpha_base, const double* channel_scaling,
                                      double dt, double eps, double max_coeff, double relax, int32_t num_steps,
                                      double* gu, double* g_alpha_base, double* g_channel_scaling,
                                      void* workspace, size_t workspace_bytes, void* stream);
int pde_jacobi_f64_forward_states(int32_t B, int32_t H, int32_t W, int32_t nt, const double* u, const double* a_row,
                                  const double* b_col, double* out, double* states, const uint64_t emit_mask[2],
                                  void* stream);
int pde_jacobi_f64_backward_states(int32_t B, int32_t H, int32_t W, int32_t nt, const double* u, const double* gout,
                                   const double* gstates, const uint64_t emit_mask[2],
                                   const double* a_row, const double* b_col, double* gu, double* g_a_row, double* g_b_col,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- K1 on rectangular planes (H != W) -------------------------------------------------------------------
 * The reference's sweep functions read B, C, H, W = u.shape and transpose for the y direction (mnist_test.py:45,72,105;
 * cifar10.py:67,76,126,152); only its constructors fix size x size.  These entry points run the implicit time loop on
 * a (B,C,H,W) tensor with (C,H,W) parameters: an x sweep (PDE_AXIS_X) solves H lines of W unknowns with alpha, a y sweep
 * (PDE_AXIS_Y) W lines of H unknowns with beta, exactly as in the square case.  They are served by the any-size kernels
 * (one thread per line, plane in LDS — path 2 of pde_adi_line_length_path) at every shape, H == W and the fused line
 * lengths included: 2 <= H, W <= PDE_MAX_N_GENERIC, otherwise PDE_E_UNSUPPORTED_N.  There is no per-step, one-launch or
 * wide family for rectangles: a layer with a channel operator is composed per step by the caller (pde_channel_mix_* on
 * H*W pixels + one-step schedules).  With H == W == N the results are bit for bit those of pde_adi_forward /
 * pde_adi_backward at a line length N on the any-size path.  Same conventions as above: caller-owned device buffers,
 * asynchronous on `stream`, no allocation, validation on the host before anything touches the device (null pointers
 * PDE_E_BADARG, a short or misaligned workspace PDE_E_WORKSPACE). */
typedef struct PdeAdiRectDesc {
    int32_t B, C, H, W;         /* rows H (y direction, beta), columns W (x direction, alpha) */
    int32_t io_dtype;           /* PDE_IO_F32 | PDE_IO_BF16 | PDE_IO_F16 (tensor I/O; math is fp32) */
    int32_t num_sweeps;
    int32_t smooth3;            /* as PdeAdiDesc: along the solve axis                    */
    int32_t has_clamp_max;
    float   clamp_max;
    float   eps;
    PdeSweep sweep[PDE_MAX_SWEEPS];
} PdeAdiRectDesc;

/* 1 when both sides are in [2, PDE_MAX_N_GENERIC], else 0 */
int pde_adi_rect_supported(int32_t H, int32_t W);
/* scratch of the two calls below (0 for a refused descriptor); num_checkpoints: bits set in the backward's ckpt_mask */
size_t pde_adi_rect_forward_workspace_bytes(const PdeAdiRectDesc* d);
size_t pde_adi_rect_backward_workspace_bytes(const PdeAdiRectDesc* d, int32_t num_checkpoints);
/* pde_adi_kappa_max on a rectangle: the per-sweep maximum coefficient, kappa_max[num_sweeps] on the device */
int pde_adi_rect_kappa_max(const PdeAdiRectDesc* d,
                           const float* alpha_base, const float* beta_base,
                           const float* alpha_slope, const float* beta_slope,
                           float* kappa_max, void* stream);
/* pde_adi_forward on a rectangle (the time loop of mnist_test.py:44-198 / cifar10.py:74-211 on H x W planes): u, y
 * (B,C,H,W) of io_dtype, parameters (C,H,W) fp32.  kappa_max / kappa_max_host / kappa_event as in pde_adi_forward: the
 * maxima are copied to the pinned host buffer and the event is recorded behind the factorisation kernel, before the
 * sweep launch.  The workspace then holds the factorisation and may be handed to the backward as fwd_workspace. */
int pde_adi_rect_forward(const PdeAdiRectDesc* d, const void* u, void* y,
                         const float* alpha_base, const float* beta_base,
                         const float* alpha_slope, const float* beta_slope,
                         float* kappa_max, float* kappa_max_host, void* kappa_event,
                         void* workspace, size_t workspace_bytes, void* stream);
/* pde_adi_backward on a rectangle (the reference gets it from autograd): gu and the four (C,H,W) parameter gradients,
 * overwritten; ckpt_mask, u and fwd_workspace as in pde_adi_backward. */
int pde_adi_rect_backward(const PdeAdiRectDesc* d, const void* gy, const void* y, const void* u,
                          const uint64_t ckpt_mask[2], void* gu,
                          const float* alpha_base, const float* beta_base,
                          const float* alpha_slope, const float* beta_slope,
                          float* g_alpha_base, float* g_beta_base,
                          float* g_alpha_slope, float* g_beta_slope,
                          const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream);

/* pde_adi_forward_states / pde_adi_backward_states on a rectangle: states, gstates (slots, B, C, H, W) of io_dtype; the
 * same rules, the same workspaces as pde_adi_rect_forward / pde_adi_rect_backward. */
int pde_adi_rect_forward_states(const PdeAdiRectDesc* d, const void* u, void* y, void* states, const uint64_t emit_mask[2],
                                const float* alpha_base, const float* beta_base,
                                const float* alpha_slope, const float* beta_slope,
                                float* kappa_max, float* kappa_max_host, void* kappa_event,
                                void* workspace, size_t workspace_bytes, void* stream);
int pde_adi_rect_backward_states(const PdeAdiRectDesc* d, const void* gy, const void* gstates, const uint64_t emit_mask[2],
                                 const void* y, const void* u, const uint64_t ckpt_mask[2], void* gu,
                                 const float* alpha_base, const float* beta_base,
                                 const float* alpha_slope, const float* beta_slope,
                                 float* g_alpha_base, float* g_beta_base,
                                 float* g_alpha_slope, float* g_beta_slope,
                                 const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream);

/* The same in float64 (pde_adi_f64_* on a rectangle): every tensor and every scalar of the schedule a double. */
typedef struct PdeAdiRectDescF64 {
    int32_t B, C, H, W;
    int32_t io_dtype;           /* PDE_IO_F64 */
    int32_t num_sweeps;
    int32_t smooth3;
    int32_t has_clamp_max;
    double  clamp_max;
    double  eps;
    PdeSweepF64 sweep[PDE_MAX_SWEEPS];
} PdeAdiRectDescF64;

size_t pde_adi_rect_f64_forward_workspace_bytes(const PdeAdiRectDescF64* d);
size_t pde_adi_rect_f64_backward_workspace_bytes(const PdeAdiRectDescF64* d, int32_t num_checkpoints);
int pde_adi_rect_f64_kappa_max(const PdeAdiRectDescF64* d,
                               const double* alpha_base, const double* beta_base,
                               const double* alpha_slope, const double* beta_slope,
                               double* kappa_max, void* stream);
int pde_adi_rect_f64_forward(const PdeAdiRectDescF64* d, const double* u, double* y,
                             const double* alpha_base, const double* beta_base,
                             const double* alpha_slope, const double* beta_slope,
                             double* kappa_max, void* workspace, size_t workspace_bytes, void* stream);
int pde_adi_rect_f64_backward(const PdeAdiRectDescF64* d, const double* gy, const double* y, const double* u,
                              const uint64_t ckpt_mask[2], double* gu,
                              const double* alpha_base, const double* beta_base,
                              const double* alpha_slope, const double* beta_slope,
                              double* g_alpha_base, double* g_beta_base, double* g_alpha_slope, double* g_beta_slope,
                              const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream);

int pde_adi_rect_f64_forward_states(const PdeAdiRectDescF64* d, const double* u, double* y, double* states,
                                    const uint64_t emit_mask[2],
                                    const double* alpha_base, const double* beta_base,
                                    const double* alpha_slope, const double* beta_slope,
                                    double* kappa_max, void* workspace, size_t workspace_bytes, void* stream);
int pde_adi_rect_f64_backward_states(const PdeAdiRectDescF64* d, const double* gy, const double* gstates,
                                     const uint64_t emit_mask[2], const double* y, const double* u,
                                     const uint64_t ckpt_mask[2], double* gu,
                                     const double* alpha_base, const double* beta_base,
                                     const double* alpha_slope, const double* beta_slope,
                                     double* g_alpha_base, double* g_beta_base, double* g_alpha_slope, double* g_beta_slope,
                                     const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the backward of a layer whose coefficients take no gradient -----------------------------------------
 * Every implicit layer is linear in its input: gu = F^T gy, the transposed two-sided solves walked from the last sweep to
 * the first.  These entry points compute that and nothing else — for frozen coefficients, adversarial attacks, saliency
 * maps, a frozen feature extractor under a trainable head.  They read neither y nor u, rebuild no state, keep no
 * checkpoints, form no parameter-gradient sums and need no coefficient maxima: 8 bytes per element (gy in, gu out) where
 * pde_adi_backward moves 12, in a launch shaped like the forward's.  gu is bit for bit the gu of the family's
 * *_backward_states call on the same arguments (the same operations per plane in the same order).
 * The plain call is the _states call with a NULL mask.  gstates / emit_mask as in *_backward_states: dL/d(state after
 * sweep s) joins the adjoint when the reverse walk is about to enter sweep s; a non-empty mask with gstates NULL, or a
 * bit at or above num_sweeps-1: PDE_E_BADARG.  fwd_workspace: the workspace the forward call of the same descriptor and
 * coefficients left behind (its factorisation is read, not written), or NULL — the call then factorises into
 * `workspace` itself.  workspace: at least *_backward_input_workspace_bytes(d) bytes, 16-byte aligned, required either
 * way (PDE_E_WORKSPACE); the query is 0 for a descriptor the call refuses.  Descriptors, error codes and "checked on
 * the host before any launch" are those of the family's other calls, except that sweeps of one axis need not share
 * delta / h2 (that restriction of pde_adi_backward belongs to its time-weighted sums).  Nothing is allocated,
 * synchronised or waited for inside the calls.
 * pde_adi_backward_input_kernel: which kernel the square fp32 / bf16 / fp16 call runs — 0 the fused HIP kernel
 * (N = 8, 12, ..., 32; barrier-per-sweep schedule, records resident for a launch of at most three sweeps), 2 the
 * any-size kernel (one workgroup per plane); PDE_E_BADARG for a descriptor the call refuses.  The rectangle and
 * float64 families always run the any-size kernel. */
int pde_adi_backward_input_kernel(const PdeAdiDesc* d);
size_t pde_adi_backward_input_workspace_bytes(const PdeAdiDesc* d);
int pde_adi_backward_input(const PdeAdiDesc* d, const void* gy, void* gu,
                           const float* alpha_base, const float* beta_base,
                           const float* alpha_slope, const float* beta_slope,
                           const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream);
int pde_adi_backward_input_states(const PdeAdiDesc* d, const void* gy, const void* gstates, const uint64_t emit_mask[2],
                                  void* gu,
                                  const float* alpha_base, const float* beta_base,
                                  const float* alpha_slope, const float* beta_slope,
                                  const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream);

size_t pde_adi_rect_backward_input_workspace_bytes(const PdeAdiRectDesc* d);
int pde_adi_rect_backward_input(const PdeAdiRectDesc* d, const void* gy, void* gu,
                                const float* alpha_base, const float* beta_base,
                                const float* alpha_slope, const float* beta_slope,
                                const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream);
int pde_adi_rect_backward_input_states(const PdeAdiRectDesc* d, const void* gy, const void* gstates,
                                       const uint64_t emit_mask[2], void* gu,
                                       const float* alpha_base, const float* beta_base,
                                       const float* alpha_slope, const float* beta_slope,
                                       const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream);

size_t pde_adi_f64_backward_input_workspace_bytes(const PdeAdiDescF64* d);
int pde_adi_f64_backward_input(const PdeAdiDescF64* d, const double* gy, double* gu,
                               const double* alpha_base, const double* beta_base,
                               const double* alpha_slope, const double* beta_slope,
                               const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream);
int pde_adi_f64_backward_input_states(const PdeAdiDescF64* d, const double* gy, const double* gstates,
                                      const uint64_t emit_mask[2], double* gu,
                                      const double* alpha_base, const double* beta_base,
                                      const double* alpha_slope, const double* beta_slope,
                                      const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream);

size_t pde_adi_rect_f64_backward_input_workspace_bytes(const PdeAdiRectDescF64* d);
int pde_adi_rect_f64_backward_input(const PdeAdiRectDescF64* d, const double* gy, double* gu,
                                    const double* alpha_base, const double* beta_base,
                                    const double* alpha_slope, const double* beta_slope,
                                    const void* fwd_workspace, void* workspace, size_t workspace_bytes, void* stream);
int pde_adi_rect_f64_backward_input_states(const PdeAdiRectDescF64* d, const double* gy, const double* gstates,
                                           const uint64_t emit_mask[2], double* gu,
                                           const double* alpha_base, const double* beta_base,
                                           const double* alpha_slope, const double* beta_slope,
                                           const void* fwd_workspace, void* workspace, size_t workspace_bytes,
                                           void* stream);

/* The same for the one-launch C <= 4 layers (the K1 calls above and their shared-input groups): declared in
 * pdecnn_small_input.h, which this header includes below; for the layers with a channel operator above C = 4 (the
 * pde_adi_mixed_* calls, pde_channel_mix_* and pde_skip_blend_*) in pdecnn_mixed_input.h, included below as well; for
 * the explicit 5-point and the Jacobi layers (pde_explicit5_*, pde_jacobi_*) in pdecnn_explicit_input.h, the third.
 * The tangent-linear (forward-mode) passes: pdecnn_tangent.h for the implicit families, pdecnn_explicit_tangent.h for the
 * explicit 5-point and the Jacobi layers, pdecnn_tangent_fused.h for pde_adi_* on the fused solver at N = 8 .. 32. */

/* ---- utilities ------------------------------------------------------------------------- */

/* Average device time (ms) per launch of the dominant kernel of the most recent
 * pde_adi_forward / pde_adi_backward issued with timing enabled; measured with HIP
 * events recorded on the stream the kernel was launched on.  bench.py's roofline leg. */
int pde_timing_enable(int32_t on);
int pde_timing_read(double* fwd_ms_sum, int64_t* fwd_launches, double* bwd_ms_sum, int64_t* bwd_launches);

const char* pde_version(void);

#include "pdecnn_small_input.h"
#include "pdecnn_mixed_input.h"
#include "pdecnn_explicit_input.h"
#include "pdecnn_tangent.h"
#include "pdecnn_explicit_tangent.h"
#include "pdecnn_tangent_fused.h"

#ifdef __cplusplus
}
#endif
#endif /* PDECNN_H */
