// One translation unit per line length: compile with -DPDE_INST_N=<N>.
#include "pde_adi_dev.h"
#include "pde_adi_launch.h"
#if PDE_INST_N == 16 || PDE_INST_N == 28 || PDE_INST_N == 32
#define PDE_INST_SMALL 1
#include "pde_adi_small.h"
#endif
#if PDE_INST_N == 28 || PDE_INST_N == 32
#define PDE_INST_WIDE 1
#include "pde_adi_wide.h"
#endif

#ifndef PDE_INST_N
#error "compile with -DPDE_INST_N=<line length>"
#endif

#define PDE_CAT2(a, b) a##b
#define PDE_CAT(a, b) PDE_CAT2(a, b)

namespace pde {
namespace {

template <typename K>
int launch(K kernel, const SweepArgs& sa, int grid, size_t lds, hipStream_t st) {
    static unsigned long long configured = 0;       // one static per kernel instantiation
    if (ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), (int)lds, configured) != PDE_OK) return PDE_E_LAUNCH;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), lds, st, sa);
    return check_launch();
}

template <typename IO>
int fwd_io(int split, int ho, const SweepArgs& sa, int grid, size_t lds, hipStream_t st) {
    constexpr int N = PDE_INST_N;
    if constexpr (N == 32 && std::is_same<IO, float>::value) {
        if (ho && split == kSplitStrang) {
            // one instantiation per set of round trips issued ahead (SweepArgs::ahead, PDE_FWD_AHEAD): a set decided at
            // run time costs the sweep loop registers it does not have
            switch (sa.ahead) {
#define PDE_CASE(AH) case AH: return launch(adi_fwd_kernel<N, kJFwd, IO, kSplitStrang, true, false, AH>, sa, grid, lds, st);
                PDE_FWD_AHEAD_LIST
#undef PDE_CASE
            }
            return PDE_E_LAUNCH;
        }
    }
    if (ho) return PDE_E_LAUNCH;
    switch (split) {
        case kSplitStrang: return launch(adi_fwd_kernel<N, kJFwd, IO, kSplitStrang>, sa, grid, lds, st);
        case kSplitLie: return launch(adi_fwd_kernel<N, kJFwd, IO, kSplitLie>, sa, grid, lds, st);
        default: return launch(adi_fwd_kernel<N, kJFwd, IO, kSplitAny>, sa, grid, lds, st);
    }
}

// the emitting variant (pde_adi_*_forward_states): barrier-per-sweep schedule at every N and I/O type.  At N = 32 the
// step-pattern bodies do not fit 128 VGPRs (the plain ones spill 3-13 registers there too): the emitting call takes the
// table-driven body, which does (110 VGPRs, no scratch) — the same arithmetic in the same order, the axis read per sweep
template <typename IO>
int fwd_emit_io(int split, const SweepArgs& sa, int grid, size_t lds, hipStream_t st) {
    constexpr int N = PDE_INST_N;
    if constexpr (N == 32) return launch(adi_fwd_kernel<N, kJFwd, IO, kSplitAny, false, true>, sa, grid, lds, st);
    else switch (split) {
        case kSplitStrang: return launch(adi_fwd_kernel<N, kJFwd, IO, kSplitStrang, false, true>, sa, grid, lds, st);
        case kSplitLie: return launch(adi_fwd_kernel<N, kJFwd, IO, kSplitLie, false, true>, sa, grid, lds, st);
        default: return launch(adi_fwd_kernel<N, kJFwd, IO, kSplitAny, false, true>, sa, grid, lds, st);
    }
}

template <bool MASKED, int SPLIT>
constexpr size_t bwd_lds() { return (size_t)(BwdStage<MASKED, SPLIT>::kFloats + kWaves * kImage) * sizeof(float); }
template <int SPLIT>
constexpr size_t bwd_lds_dual() {
    return bwd_lds<false, SPLIT>() > bwd_lds<true, kSplitAny>() ? bwd_lds<false, SPLIT>() : bwd_lds<true, kSplitAny>();
}

// grid = 2 * C * G: fast and masked variant in one launch (see adi_bwd_kernel)
template <typename IO>
int bwd_io(int split, const SweepArgs& sa, int grid, hipStream_t st) {
    constexpr int N = PDE_INST_N;
    switch (split) {
        case kSplitStrang: return launch(adi_bwd_kernel<N, kJBwd, IO, kSplitStrang>, sa, grid, bwd_lds_dual<kSplitStrang>(), st);
        case kSplitLie: return launch(adi_bwd_kernel<N, kJBwd, IO, kSplitLie>, sa, grid, bwd_lds_dual<kSplitLie>(), st);
        default: return launch(adi_bwd_kernel<N, 1, IO, kSplitAny>, sa, grid, bwd_lds_dual<kSplitAny>(), st);
    }
}

template <typename IO>
int bwd_emit_io(int split, const SweepArgs& sa, int grid, hipStream_t st) {
    constexpr int N = PDE_INST_N;
    switch (split) {
        case kSplitStrang: return launch(adi_bwd_kernel<N, kJBwd, IO, kSplitStrang, true>, sa, grid, bwd_lds_dual<kSplitStrang>(), st);
        case kSplitLie: return launch(adi_bwd_kernel<N, kJBwd, IO, kSplitLie, true>, sa, grid, bwd_lds_dual<kSplitLie>(), st);
        default: return launch(adi_bwd_kernel<N, 1, IO, kSplitAny, true>, sa, grid, bwd_lds_dual<kSplitAny>(), st);
    }
}

// the backward for the input alone (pde_adi_backward_input*): the forward's launch shape
template <typename IO, bool EMIT>
int bwd_input_io(int split, const SweepArgs& sa, int grid, size_t lds, hipStream_t st) {
    constexpr int N = PDE_INST_N;
    switch (split) {
        case kSplitStrang: return launch(adi_bwd_input_kernel<N, kJFwd, IO, kSplitStrang, EMIT>, sa, grid, lds, st);
        case kSplitLie: return launch(adi_bwd_input_kernel<N, kJFwd, IO, kSplitLie, EMIT>, sa, grid, lds, st);
        default: return launch(adi_bwd_input_kernel<N, kJFwd, IO, kSplitAny, EMIT>, sa, grid, lds, st);
    }
}

}  // namespace

int PDE_CAT(adi_launch_bwd_input_, PDE_INST_N)(int io, int split, int emit, const void* args, int grid, size_t lds,
                                               hipStream_t st) {
    const SweepArgs& sa = *static_cast<const SweepArgs*>(args);
    if (emit) {
        if (io == PDE_IO_F16) return bwd_input_io<half_t, true>(split, sa, grid, lds, st);
        return io == PDE_IO_F32 ? bwd_input_io<float, true>(split, sa, grid, lds, st)
                                : bwd_input_io<bf16_t, true>(split, sa, grid, lds, st);
    }
    if (io == PDE_IO_F16) return bwd_input_io<half_t, false>(split, sa, grid, lds, st);
    return io == PDE_IO_F32 ? bwd_input_io<float, false>(split, sa, grid, lds, st)
                            : bwd_input_io<bf16_t, false>(split, sa, grid, lds, st);
}

int PDE_CAT(adi_launch_fwd_emit_, PDE_INST_N)(int io, int split, const void* args, int grid, size_t lds, hipStream_t st) {
    const SweepArgs& sa = *static_cast<const SweepArgs*>(args);
    if (io == PDE_IO_F16) return fwd_emit_io<half_t>(split, sa, grid, lds, st);
    return io == PDE_IO_F32 ? fwd_emit_io<float>(split, sa, grid, lds, st) : fwd_emit_io<bf16_t>(split, sa, grid, lds, st);
}

int PDE_CAT(adi_launch_bwd_emit_, PDE_INST_N)(int io, int split, const void* args, int grid, hipStream_t st) {
    const SweepArgs& sa = *static_cast<const SweepArgs*>(args);
    if (io == PDE_IO_F16) return bwd_emit_io<half_t>(split, sa, grid, st);
    return io == PDE_IO_F32 ? bwd_emit_io<float>(split, sa, grid, st) : bwd_emit_io<bf16_t>(split, sa, grid, st);
}

int PDE_CAT(adi_launch_fwd_, PDE_INST_N)(int io, int split, int ho, const void* args, int grid, size_t lds, hipStream_t st) {
    const SweepArgs& sa = *static_cast<const SweepArgs*>(args);
    if (io == PDE_IO_F16) return fwd_io<half_t>(split, ho, sa, grid, lds, st);
    return io == PDE_IO_F32 ? fwd_io<float>(split, ho, sa, grid, lds, st) : fwd_io<bf16_t>(split, ho, sa, grid, lds, st);
}

int PDE_CAT(adi_launch_bwd_, PDE_INST_N)(int io, int split, const void* args, int grid, hipStream_t st) {
    const SweepArgs& sa = *static_cast<const SweepArgs*>(args);
    if (io == PDE_IO_F16) return bwd_io<half_t>(split, sa, grid, st);
    return io == PDE_IO_F32 ? bwd_io<float>(split, sa, grid, st) : bwd_io<bf16_t>(split, sa, grid, st);
}

#ifdef PDE_INST_SMALL
int PDE_CAT(adi_launch_small_fwd_, PDE_INST_N)(int io, int split, const void* args, int grid, size_t lds, hipStream_t st) {
    const SmallArgs& sa = *static_cast<const SmallArgs*>(args);
    if (io == PDE_IO_F16) return small_fwd_io<PDE_INST_N, half_t>(split, sa, grid, lds, st);
    return io == PDE_IO_F32 ? small_fwd_io<PDE_INST_N, float>(split, sa, grid, lds, st)
                            : small_fwd_io<PDE_INST_N, bf16_t>(split, sa, grid, lds, st);
}
int PDE_CAT(adi_launch_small_bwd_, PDE_INST_N)(int io, int split, const void* args, int grid, size_t lds, hipStream_t st) {
    const SmallArgs& sa = *static_cast<const SmallArgs*>(args);
    if (io == PDE_IO_F16) return small_bwd_io<PDE_INST_N, half_t>(split, sa, grid, lds, st);
    return io == PDE_IO_F32 ? small_bwd_io<PDE_INST_N, float>(split, sa, grid, lds, st)
                            : small_bwd_io<PDE_INST_N, bf16_t>(split, sa, grid, lds, st);
}
// the emitting variants (pde_adi_small_*_states): SmallArgs::traj, SmallArgs::em
int PDE_CAT(adi_launch_small_fwd_emit_, PDE_INST_N)(int io, int split, const void* args, int grid, size_t lds, hipStream_t st) {
    const SmallArgs& sa = *static_cast<const SmallArgs*>(args);
    if (io == PDE_IO_F16) return small_fwd_io<PDE_INST_N, half_t, true>(split, sa, grid, lds, st);
    return io == PDE_IO_F32 ? small_fwd_io<PDE_INST_N, float, true>(split, sa, grid, lds, st)
                            : small_fwd_io<PDE_INST_N, bf16_t, true>(split, sa, grid, lds, st);
}
int PDE_CAT(adi_launch_small_bwd_emit_, PDE_INST_N)(int io, int split, const void* args, int grid, size_t lds, hipStream_t st) {
    const SmallArgs& sa = *static_cast<const SmallArgs*>(args);
    if (io == PDE_IO_F16) return small_bwd_io<PDE_INST_N, half_t, true>(split, sa, grid, lds, st);
    return io == PDE_IO_F32 ? small_bwd_io<PDE_INST_N, float, true>(split, sa, grid, lds, st)
                            : small_bwd_io<PDE_INST_N, bf16_t, true>(split, sa, grid, lds, st);
}
// the backward for the input alone (pde_adi_small_backward_input*, pde_adi_multi_backward_input); emit != 0: with the
// emitted states' gradients
int PDE_CAT(adi_launch_small_bwd_input_, PDE_INST_N)(int io, int split, int emit, const void* args, int grid, size_t lds,
                                                     hipStream_t st) {
    const SmallArgs& sa = *static_cast<const SmallArgs*>(args);
    if (emit) {
        if (io == PDE_IO_F16) return small_bwd_input_io<PDE_INST_N, half_t, true>(split, sa, grid, lds, st);
        return io == PDE_IO_F32 ? small_bwd_input_io<PDE_INST_N, float, true>(split, sa, grid, lds, st)
                                : small_bwd_input_io<PDE_INST_N, bf16_t, true>(split, sa, grid, lds, st);
    }
    if (io == PDE_IO_F16) return small_bwd_input_io<PDE_INST_N, half_t>(split, sa, grid, lds, st);
    return io == PDE_IO_F32 ? small_bwd_input_io<PDE_INST_N, float>(split, sa, grid, lds, st)
                            : small_bwd_input_io<PDE_INST_N, bf16_t>(split, sa, grid, lds, st);
}
#endif

#ifdef PDE_INST_WIDE
int PDE_CAT(adi_launch_wide_fwd_, PDE_INST_N)(int C, int split, const void* args, int grid, hipStream_t st) {
    return wide_fwd_launch<PDE_INST_N>(C, split, *static_cast<const WideArgs*>(args), grid, st);
}
#endif

}  // namespace pde
