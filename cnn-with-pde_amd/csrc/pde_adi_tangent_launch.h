// Launch entry points of the per-N units of the fused tangent-linear pass (pde_adi_tangent_inst.hip, one object per line
// length).  Plain functions so that every unit can be compiled in parallel.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace pde {
// return 0 on success, PDE_E_LAUNCH otherwise.  args: FactorTangentArgs / TangentArgs of pde_adi_tangent_dev.h, passed by
// pointer across units.  par != 0: a parameter carries a tangent (`lds` then includes the dco ring)
#define PDE_DECLARE_N(NN)                                                                                   \
    int adi_launch_factor_tangent_##NN(const void* args, int grid, hipStream_t st);                         \
    int adi_launch_tangent_##NN(int io, int par, const void* args, int grid, size_t lds, hipStream_t st);
PDE_DECLARE_N(8) PDE_DECLARE_N(12) PDE_DECLARE_N(16) PDE_DECLARE_N(20) PDE_DECLARE_N(24) PDE_DECLARE_N(28) PDE_DECLARE_N(32)
#undef PDE_DECLARE_N
}  // namespace pde
