/* pdecnn_tangent.h — the tangent-linear (forward-mode) pass of the implicit ADI layers (mnist_test.py:50-198,
 * cifar10.py:86-211: pde_adi_*) of libpdecnn_hip.
 * Part of the C ABI of pdecnn.h, which includes this file (inside its extern "C" block, behind the types it uses):
 * include pdecnn.h, not this file.  Error codes, io_dtype values, descriptors and the Alignment rules are those of
 * pdecnn.h. */
#ifndef PDECNN_TANGENT_H
#define PDECNN_TANGENT_H
#ifndef PDECNN_H
#error "include pdecnn.h: it includes this header"
#endif

/* One call returns y = F(theta) u and its directional derivative
 *     dy = F(theta) du + (dF/dtheta . dtheta) u
 * for the schedule of the descriptor, theta = (alpha_base, beta_base, alpha_slope, beta_slope).  Per sweep and line the
 * forward solves A(co) x = d with co = (delta/h2) smooth3(clamp(base + slope t)); the tangent of that sweep is
 *     dco  = (delta/h2) smooth3(pass . (dbase + dslope t))        pass: 1 where eps <= base + slope t <= clamp_max
 *     A dx = dd + dco_k (x_{k-1} - m_k x_k + x_{k+1})             x: the sweep's SOLVED line, m = 1 at the ends, 2 inside,
 *                                                                 a missing neighbour dropped; the same factorisation
 * (at a kink of the clamp the one-sided derivative of the pass mask above is taken: equality passes).
 *
 * All four families run on the any-size kernels (one thread per line, planes in LDS: pde_adi_gen.hip), the square fp32
 * family too at the fused sizes 8 .. 32: every N, H, W in 2 .. PDE_MAX_N_GENERIC.  Launches: gen_factor_kernel, then
 * gen_factor_tangent_kernel (dco of every sweep; skipped when all four parameter tangents are NULL), then
 * gen_tangent_kernel: one workgroup per plane, the primal and the tangent plane side by side in LDS, per sweep the primal
 * recurrences operation for operation as the any-size forward runs them, the source term, and the same recurrences on the
 * tangent.  So y is bit for bit the y of the family's forward where that runs the any-size kernels (N off the fused list,
 * rectangles, float64), dy with no parameter tangent is bit for bit that forward at du, and dy is exactly linear under a
 * scaling of all tangents by a power of two.  Where two planes exceed the LDS (float64 beyond 100 x 100) the primal plane
 * lives in a slice of `workspace` owned by the workgroup, and about one workgroup per CU walks the planes.
 * bf16 / fp16 tensors: fp32 arithmetic, y and dy rounded once on the store.  No reduction, no atomic; nothing is
 * allocated, synchronised or waited for.
 *
 * Arguments.  u, du, y, dy: [B][C][H][W] in io_dtype; the parameters and their tangents: [C][H][W] in float (double in the
 * f64 families).  du NULL: a zero input tangent.  Each parameter tangent may be NULL: zero.  All five NULL: PDE_E_BADARG
 * (nothing to differentiate: call the forward).  y may be NULL (not written); dy is required.  No output may overlap an
 * input or the other output.  Alignment: the element, for tensors and parameters alike (every access is one element wide);
 * 16 bytes for the workspace.
 *
 * Checks, their order and their codes are those of the family's forward, all on the host before the first launch: the
 * descriptor (PDE_E_BADARG, PDE_E_UNSUPPORTED_N, PDE_E_TOO_MANY_SWEEPS; io_dtype), required pointers (PDE_E_BADARG),
 * alignment (PDE_E_BADARG), then the workspace (short or not 16-byte aligned: PDE_E_WORKSPACE).
 * .._workspace_bytes: the any-size factorisation, the device copy of the schedule, dco ([S][C][H][W]) and, where the planes
 * need it, the scratch slices; 0 for a descriptor the call refuses.  The workspace is scratch: nothing in it outlives the
 * call. */
size_t pde_adi_tangent_workspace_bytes(const PdeAdiDesc* d);
int pde_adi_tangent(const PdeAdiDesc* d, const void* u, const void* du,
                    const float* alpha_base, const float* beta_base, const float* alpha_slope, const float* beta_slope,
                    const float* d_alpha_base, const float* d_beta_base, const float* d_alpha_slope,
                    const float* d_beta_slope, void* y, void* dy, void* workspace, size_t workspace_bytes, void* stream);
size_t pde_adi_f64_tangent_workspace_bytes(const PdeAdiDescF64* d);
int pde_adi_f64_tangent(const PdeAdiDescF64* d, const double* u, const double* du,
                        const double* alpha_base, const double* beta_base, const double* alpha_slope,
                        const double* beta_slope, const double* d_alpha_base, const double* d_beta_base,
                        const double* d_alpha_slope, const double* d_beta_slope, double* y, double* dy, void* workspace,
                        size_t workspace_bytes, void* stream);
size_t pde_adi_rect_tangent_workspace_bytes(const PdeAdiRectDesc* d);
int pde_adi_rect_tangent(const PdeAdiRectDesc* d, const void* u, const void* du,
                         const float* alpha_base, const float* beta_base, const float* alpha_slope, const float* beta_slope,
                         const float* d_alpha_base, const float* d_beta_base, const float* d_alpha_slope,
                         const float* d_beta_slope, void* y, void* dy, void* workspace, size_t workspace_bytes,
                         void* stream);
size_t pde_adi_rect_f64_tangent_workspace_bytes(const PdeAdiRectDescF64* d);
int pde_adi_rect_f64_tangent(const PdeAdiRectDescF64* d, const double* u, const double* du,
                             const double* alpha_base, const double* beta_base, const double* alpha_slope,
                             const double* beta_slope, const double* d_alpha_base, const double* d_beta_base,
                             const double* d_alpha_slope, const double* d_beta_slope, double* y, double* dy,
                             void* workspace, size_t workspace_bytes, void* stream);

#endif /* PDECNN_TANGENT_H */
