import os
import shutil
import sys
import tempfile

import pytest

# Repo root on sys.path so the in-tree packages (min_tfs_client_amd, the
# tensorflow/tensorflow_serving pb2 shims, min_tfs_client alias) import
# without installation.
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: test requires an AMD GPU (MI355X); excluded by "
        "-m 'not gpu'")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="session")
def gpu_available():
    return _has_gpu()


@pytest.fixture
def sock_dir():
    """Short private directory for unix-socket paths.

    sockaddr_un.sun_path holds 107 bytes, and pytest's tmp_path (base temp
    dir + user + test name) can exceed that on its own, so sockets get a
    directory whose length does not depend on the test's name."""
    base = tempfile.gettempdir()
    if len(base) > 48:
        base = "/tmp"
    path = tempfile.mkdtemp(prefix="mtc", dir=base)
    yield path
    shutil.rmtree(path, ignore_errors=True)


def pytest_collection_modifyitems(config, items):
    if _has_gpu():
        return
    skip = pytest.mark.skip(reason="no AMD GPU in this environment")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)
