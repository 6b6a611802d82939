import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# The CPU oracle's channel products go through MKL, whose rounding depends on the code path it picks for the host CPU;
# tests/test_oracle_golden.py pins the oracle BITWISE to vectors made in MKL's reproducible mode COMPATIBLE (the same
# code path on every x86 CPU, tools/make_golden.py).  MKL reads this once, so it is set before anything loads torch.
os.environ["MKL_CBWR"] = "COMPATIBLE"


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def pytest_collection_modifyitems(config, items):
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this environment")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)
