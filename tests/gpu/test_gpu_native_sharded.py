"""Native sharded Predict with device tensors: staging DMA of dim-0 slices
on the send side, parse-ahead H2D plus the device concat on the receive
side, and producer-stream ordering — against the python-orchestrated path
(``MI355X_NATIVE_SHARDED=0``) and against the input itself (echo model).
tests/integration/test_native_sharded.py holds the CPU half."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from min_tfs_client_amd.server import (  # noqa: E402
    ModelServer,
    identity_servable,
)
from min_tfs_client_amd.turbo import TurboPredictClient  # noqa: E402

DEV = "cuda:0"
TIMEOUT = 10.0


@pytest.fixture(scope="module")
def echo_address():
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="mtc", dir="/tmp")
    try:
        with ModelServer(address=f"unix://{d}/ns.sock", raw_predict=True,
                         device=DEV) as srv:
            srv.manager.load("default", identity_servable(), version=1)
            yield srv.address
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _both_paths(address, monkeypatch, inputs, shards, num_channels=4):
    outs = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("MI355X_NATIVE_SHARDED", switch)
        with TurboPredictClient(address, backend="native",
                                num_channels=num_channels) as c:
            outs[switch] = c.predict_sharded(
                "default", inputs, shards=shards, output_device=DEV,
                timeout=TIMEOUT)
    return outs["0"], outs["1"]


def _check(inputs, old, new):
    assert set(new) == set(old) == set(inputs)
    for k, x in inputs.items():
        assert new[k].device == torch.device(DEV), k
        assert new[k].dtype == x.dtype and new[k].shape == x.shape, k
        assert torch.equal(new[k], x), k
        assert torch.equal(new[k], old[k]), k


def test_multi_chunk_shards(echo_address, monkeypatch):
    """15 x 3x224x224 fp32 over 2 shards: 8 and 7 rows, 4.8 and 4.2 MB —
    each shard spans two 4 MiB staging chunks with a ragged tail, and each
    reply lands in the pinned receive pool and is device-parsed."""
    g = torch.Generator(device=DEV).manual_seed(3)
    inputs = {"images": torch.randn(15, 3, 224, 224, device=DEV,
                                    generator=g)}
    old, new = _both_paths(echo_address, monkeypatch, inputs, 2)
    _check(inputs, old, new)


def test_small_shards(echo_address, monkeypatch):
    """(5, 3) over 4 shards: every shard is far below the 1 MB pinned
    threshold, so replies are parsed by the python fallback."""
    g = torch.Generator(device=DEV).manual_seed(4)
    inputs = {"x": torch.randn(5, 3, device=DEV, generator=g)}
    old, new = _both_paths(echo_address, monkeypatch, inputs, 4)
    _check(inputs, old, new)


def test_two_inputs_uneven_shards(echo_address, monkeypatch):
    """Two inputs of different dtype/width, 33 rows over 4 shards (9,8,8,8):
    one input is device-parsed per shard, both are sliced at row offsets."""
    g = torch.Generator(device=DEV).manual_seed(5)
    inputs = {
        "images": torch.randn(33, 3, 112, 112, device=DEV, generator=g),
        "ids": torch.randint(0, 30000, (33, 7), dtype=torch.int32,
                             device=DEV, generator=g),
    }
    old, new = _both_paths(echo_address, monkeypatch, inputs, 4,
                           num_channels=8)
    _check(inputs, old, new)


def test_input_filled_on_side_stream(echo_address, monkeypatch):
    """The input is produced on a side stream and sent at once from inside
    that stream context: the call must order its DMA after the producer
    (it synchronizes the CALLER's current stream, once per request)."""
    monkeypatch.setenv("MI355X_NATIVE_SHARDED", "1")
    side = torch.cuda.Stream(device=DEV)
    with TurboPredictClient(echo_address, backend="native",
                            num_channels=4) as c:
        x = torch.zeros(15, 3, 224, 224, device=DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            # enough queued work that the fill is still running when the
            # send starts unless the call waits for it
            for i in range(20):
                x.add_(1.0)
            x.mul_(0.5).add_(torch.arange(15, device=DEV,
                                          dtype=torch.float32)
                             .view(15, 1, 1, 1))
            out = c.predict_sharded("default", {"images": x}, shards=2,
                                    output_device=DEV, timeout=TIMEOUT)
            expect = (torch.full((15, 3, 224, 224), 10.0, device=DEV)
                      + torch.arange(15, device=DEV, dtype=torch.float32)
                      .view(15, 1, 1, 1))
            assert out["images"].device == torch.device(DEV)
            assert torch.equal(out["images"], expect)
        side.synchronize()
    monkeypatch.setenv("MI355X_NATIVE_SHARDED", "0")
    with TurboPredictClient(echo_address, backend="native",
                            num_channels=4) as c:
        old = c.predict_sharded("default", {"images": x}, shards=2,
                                output_device=DEV, timeout=TIMEOUT)
    assert torch.equal(old["images"], expect)
