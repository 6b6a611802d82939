"""bench.py's plain run: `--steps` sets the timed steps, the JSON line holds the headline fields and nothing that only
`--full` measures, and `--dump-outputs` writes what the last timed step computed — checked against the CPU oracle on
the same seeded inputs and parameters, at a batch the oracle finishes in a second."""
import contextlib
import glob
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as G
from oracle import pde_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5


def test_plain_run_dumps_what_the_timed_step_computed(tmp_path):
    B, C, N, S = 4, 64, 32, 10
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", str(B), "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    assert (j["metric"], j["unit"], j["higher_is_better"], j["dtype"]) == ("PDE-layer fwd+bwd Msamples/s", "Msamples/s",
                                                                            True, "f32")
    assert not {"configs", "secondary", "cpu_baseline", "roofline", "hipgraph_replay", "eager_auto_policy"} & set(j)

    paths = glob.glob(str(out / "*.npy"))
    assert sum(os.path.getsize(p) for p in paths) <= 64_000_000
    got = {os.path.basename(p)[:-4]: np.load(p) for p in paths}
    names = ("alpha_base", "beta_base", "alpha_time_coeff", "beta_time_coeff")
    assert set(got) == {"y", "grad_input"} | {"grad_" + n for n in names}
    assert all(a.dtype == np.float32 for a in got.values())

    # the same inputs and parameters as the bench (its seeds), through the oracle: the layer without mixing is the
    # cifar10 layer with no operator
    sys.path.insert(0, ROOT)
    import bench
    with contextlib.redirect_stdout(io.StringIO()):
        layer = bench.build_layer(C, N, S, torch.device("cpu"), 0, mixing=False)
    params = {n: getattr(layer, n).detach() for n in names}
    g = torch.Generator().manual_seed(1234)
    u = torch.randn(B, C, N, N, generator=g)
    gy = torch.randn(B, C, N, N, generator=g)
    spec = O.AdiSpec(N, C, 0.001, 1.0, 1.0, S, "strang", False, 10.0, "none", False)
    y_ref, gu_ref, gp_ref = O.value_and_grads(lambda a, p: O.adi_forward(a, p, spec), u, params, gy)

    t = lambda k: torch.from_numpy(got[k])
    errs = {"y": G.rel_err(t("y"), y_ref), "gu": G.rel_err(t("grad_input"), gu_ref)}
    errs.update({"g_" + n: G.rel_err(t("grad_" + n), gp_ref[n]) for n in names})
    assert max(errs.values()) <= TOL, errs
