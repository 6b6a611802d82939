"""Write tests/golden/adi_gen_square_path/results.npz: what the any-size implicit kernels (csrc/pde_adi_gen.hip) give
behind the SQUARE entry points pde_adi_forward / pde_adi_backward at N = 30, 64 and 128 — y, gu and the four parameter
gradients of tests/rect_util.square_path_case — which tests/test_gpu_rect.py::test_square_any_size_path_did_not_move
holds bit for bit.  The committed file was written from the commit BEFORE those kernels were generalised from N to (H, W).
Talks to a libpdecnn_hip.so through ctypes only, so it can be pointed at a library built from an older commit:

    python tools/gen_adi_gen_square_golden.py [--lib path/to/libpdecnn_hip.so] [--out tests/golden/adi_gen_square_path/results.npz]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "cnn-with-pde_amd", "lib", "libpdecnn_hip.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "adi_gen_square_path", "results.npz"))
    args = ap.parse_args()
    from rect_util import SQUARE_PATH_CASES, run_entry, square_path_case
    lib = C.CDLL(args.lib)
    res = {}
    for N in SQUARE_PATH_CASES:
        for name, t in run_entry(lib, square_path_case(N), rect=False).items():
            res[f"{name}_{N}"] = t.cpu().numpy()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez(args.out, **res)
    print("wrote", args.out, {k: v.shape for k, v in res.items()})


if __name__ == "__main__":
    main()
