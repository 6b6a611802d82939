// The fused tangent-linear pass, one translation unit per line length: compile with -DPDE_INST_N=<N>.
#include "pde_adi_tangent_dev.h"
#include "pde_adi_tangent_launch.h"

#ifndef PDE_INST_N
#error "compile with -DPDE_INST_N=<line length>"
#endif

#define PDE_CAT2(a, b) a##b
#define PDE_CAT(a, b) PDE_CAT2(a, b)

namespace pde {
namespace {

template <typename K>
int launch(K kernel, const TangentArgs& ta, int grid, size_t lds, hipStream_t st) {
    static unsigned long long configured = 0;       // one static per kernel instantiation
    if (ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), (int)lds, configured) != PDE_OK) return PDE_E_LAUNCH;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), lds, st, ta);
    return check_launch();
}

template <typename IO>
int tangent_io(int par, const TangentArgs& ta, int grid, size_t lds, hipStream_t st) {
    constexpr int N = PDE_INST_N;
    return par ? launch(adi_tangent_kernel<N, kJTan, IO, true>, ta, grid, lds, st)
               : launch(adi_tangent_kernel<N, kJTan, IO, false>, ta, grid, lds, st);
}

}  // namespace

int PDE_CAT(adi_launch_factor_tangent_, PDE_INST_N)(const void* args, int grid, hipStream_t st) {
    hipLaunchKernelGGL(adi_factor_tangent_kernel<PDE_INST_N>, dim3(grid), dim3(128), 0, st,
                       *static_cast<const FactorTangentArgs*>(args));
    return check_launch();
}

int PDE_CAT(adi_launch_tangent_, PDE_INST_N)(int io, int par, const void* args, int grid, size_t lds, hipStream_t st) {
    const TangentArgs& ta = *static_cast<const TangentArgs*>(args);
    if (io == PDE_IO_F16) return tangent_io<half_t>(par, ta, grid, lds, st);
    return io == PDE_IO_F32 ? tangent_io<float>(par, ta, grid, lds, st) : tangent_io<bf16_t>(par, ta, grid, lds, st);
}

}  // namespace pde
