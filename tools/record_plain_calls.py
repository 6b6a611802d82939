#!/usr/bin/env python3
"""Record what the public functions of functional.py return for the cases of tests/plain_calls_cases.py — output, input
gradient and every parameter gradient of each plain and each trajectory call — into one .npz:

    record_plain_calls.py OUT.npz

tests/golden/plain_calls/parent.npz (a directory of its own: the .npz files directly under tests/golden are the reference's
vectors, which golden_util lists by a glob) is this run at the commit before the autograd nodes of a layer family were folded
into one (two runs in separate processes gave identical files); tests/test_gpu_plain_calls.py holds every later commit to
it bit for bit.  The kernels use no float atomics, so the same sources give the same bits on every run."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import plain_calls_cases as PC  # noqa: E402
from cnn_with_pde_amd import functional as F_  # noqa: E402


def record():
    out = {}
    for case, traj in PC.variants():
        res, _ = PC.run_case(F_, case, traj)
        for name, t in res.items():
            out[PC.key(case, traj, name, t)] = PC.to_numpy(t)
    return out


if __name__ == "__main__":
    res = record()
    np.savez_compressed(sys.argv[1], **res)
    print(f"{len(res)} tensors, {sum(v.nbytes for v in res.values())} bytes before compression -> {sys.argv[1]}")
