#!/usr/bin/env python3
"""Record what the public functions return for the cases of tests/node_calls_cases.py — every output, the input gradient
and every parameter / operator / skip-weight / weight gradient, each case run trainable, frozen and under no_grad — into
the files the case table names:

    record_node_calls.py OUTDIR

Every case runs through the native nodes (csrc/host_ext.cpp) and through the ctypes nodes (functional.py); the two must
agree bit for bit and one copy is stored.  tests/golden/node_calls/ is this run at the commit before the host glue of the
implicit-layer nodes was factored into one core per mirror (two runs in separate processes gave identical files);
tests/test_gpu_node_calls.py holds both mirrors of every later commit to it bit for bit.  The kernels use no float atomics,
so the same sources give the same bits on every run."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cnn_with_pde_amd as P  # noqa: E402
import node_calls_cases as NC  # noqa: E402
from cnn_with_pde_amd import _lib, functional  # noqa: E402,F401


def record():
    out = {f: {} for f in NC.FILES}
    for case, way in NC.variants():
        a, b = NC.both_mirrors(P, case, way)
        assert a.keys() == b.keys(), (case["name"], way, sorted(a), sorted(b))
        for name, t in a.items():
            s = b[name]
            assert t.dtype == s.dtype and t.shape == s.shape and torch.equal(t, s), (case["name"], way, name)
            out[case["file"]][NC.key(case, way, name, t)] = NC.to_numpy(t)
    return out


if __name__ == "__main__":
    os.makedirs(sys.argv[1], exist_ok=True)
    for f, res in record().items():
        path = os.path.join(sys.argv[1], f + ".npz")
        np.savez_compressed(path, **NC.pack(res))
        print(f"{len(res)} tensors, {sum(v.nbytes for v in res.values())} bytes before they are stored once each -> {path}")
