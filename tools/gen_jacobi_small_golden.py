"""Write tests/golden/jacobi_small_path/results.npz: the one-workgroup Jacobi kernels' results at 48x48 and 64x64, which
tests/test_gpu_jacobi_tiled.py::test_small_planes_unchanged holds bit for bit.  Talks to a libpdecnn_hip.so through
ctypes only, so it can be pointed at a library built from an older commit:

    python tools/gen_jacobi_small_golden.py [--lib path/to/libpdecnn_hip.so] [--out tests/golden/jacobi_small_path/results.npz]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "cnn-with-pde_amd", "lib", "libpdecnn_hip.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "jacobi_small_path", "results.npz"))
    args = ap.parse_args()
    from test_gpu_jacobi_tiled import small_path_case
    lib = C.CDLL(args.lib)
    lib.pde_jacobi_backward_workspace_bytes.restype = C.c_size_t
    vp = lambda t: C.c_void_p(t.data_ptr())                                                 # noqa: E731
    i32 = C.c_int32
    res = {}
    for N in (48, 64):
        u, gy, A, Bc, nt = small_path_case(N)
        u, gy, A, Bc = u.cuda(), gy.cuda(), A.cuda(), Bc.cuda()
        B = u.shape[0]
        y, gu, gA, gB = torch.empty_like(u), torch.empty_like(u), torch.empty_like(A), torch.empty_like(Bc)
        nb = lib.pde_jacobi_backward_workspace_bytes(i32(B), i32(N), i32(N), i32(nt))
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        rc = lib.pde_jacobi_forward(i32(B), i32(N), i32(N), i32(nt), vp(u), vp(A), vp(Bc), vp(y), C.c_void_p(0))
        assert rc == 0, rc
        rc = lib.pde_jacobi_backward(i32(B), i32(N), i32(N), i32(nt), vp(u), vp(gy), vp(A), vp(Bc), vp(gu), vp(gA), vp(gB),
                                     vp(ws), C.c_size_t(nb), C.c_void_p(0))
        assert rc == 0, rc
        torch.cuda.synchronize()
        for name, t in (("y", y), ("gu", gu), ("gA", gA), ("gB", gB)):
            res[f"{name}_{N}"] = t.cpu().numpy()
    np.savez(args.out, **res)
    print("wrote", args.out, {k: v.shape for k, v in res.items()})


if __name__ == "__main__":
    main()
