import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "conjugate-gradient-sparse-gp_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

# MGP_TESTS_CPU_ONLY=1 (the ASan child of tests/test_sanitizers.py): the process must never initialise the GPU
# runtime, also on a machine that has a GPU, so torch reports none and every GPU-or-host choice takes the host
if os.environ.get("MGP_TESTS_CPU_ONLY") == "1":
    import torch

    torch.cuda.is_available = lambda: False


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def pytest_collection_modifyitems(config, items):
    if _has_gpu():
        return
    skip = pytest.mark.skip(reason="no GPU in this environment")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)
