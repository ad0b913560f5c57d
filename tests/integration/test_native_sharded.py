"""Native sharded Predict (one C++ call per logical request) against the
python-orchestrated path it replaces, on CPU tensors.

``MI355X_NATIVE_SHARDED=0`` keeps the old per-shard python orchestration,
so every property is checked differentially: same outputs, same request
messages on the wire, same error surface. The GPU half (device regions,
stream ordering, device concat) is in tests/gpu/test_gpu_native_sharded.py.

Every RPC carries a timeout of a few seconds: a lost reply fails as
DEADLINE_EXCEEDED instead of hanging the suite.
"""
import threading
from collections import Counter

import grpc
import pytest
import torch

pytest.importorskip("min_tfs_client_amd._transport")
from min_tfs_client_amd import _transport as T  # noqa: E402
from min_tfs_client_amd.native_transport import HandlerAbort  # noqa: E402
from min_tfs_client_amd.ops import require_native  # noqa: E402
from min_tfs_client_amd.server import (  # noqa: E402
    ModelServer,
    identity_servable,
)
from min_tfs_client_amd.turbo import (  # noqa: E402
    NativeRpcError,
    TurboPredictClient,
)

native = require_native()
PREDICT = "/tensorflow.serving.PredictionService/Predict"
TIMEOUT = 5.0
BATCHES = (4, 5, 7, 33)
SHARDS = (2, 3, 4)


def _inputs(batch, seed=0):
    """One fp32 input whose larger shards cross the 64 KB region threshold
    (24000 B/row) and one small int32 input that is always inlined into
    the skeleton; row r of `tag` holds r, so a handler can tell shards
    apart."""
    g = torch.Generator().manual_seed(1000 * seed + batch)
    return {
        "images": torch.randn(batch, 3, 2000, generator=g),
        "tag": torch.arange(batch, dtype=torch.int32).reshape(batch, 1)
        .repeat(1, 16).contiguous(),
    }


@pytest.fixture(scope="module")
def echo_server():
    with ModelServer(address="127.0.0.1:0", raw_predict=True) as srv:
        srv.manager.load("default", identity_servable(), version=1)
        yield srv


@pytest.fixture(scope="module")
def reference_outputs(echo_server):
    """Outputs of the python-orchestrated path for the whole grid, computed
    once (a module fixture cannot use monkeypatch, so the switch is set
    and restored by hand)."""
    import os
    old = os.environ.get("MI355X_NATIVE_SHARDED")
    os.environ["MI355X_NATIVE_SHARDED"] = "0"
    try:
        ref = {}
        with TurboPredictClient(echo_server.address, backend="native",
                                num_channels=4) as c:
            for b in BATCHES:
                for s in SHARDS:
                    ref[(b, s)] = c.predict_sharded(
                        "default", _inputs(b), shards=s, timeout=TIMEOUT)
    finally:
        if old is None:
            del os.environ["MI355X_NATIVE_SHARDED"]
        else:
            os.environ["MI355X_NATIVE_SHARDED"] = old
    return ref


@pytest.mark.parametrize("shards", SHARDS)
@pytest.mark.parametrize("batch", BATCHES)
def test_outputs_equal_switched_off_path(echo_server, reference_outputs,
                                         monkeypatch, batch, shards):
    monkeypatch.setenv("MI355X_NATIVE_SHARDED", "1")
    inputs = _inputs(batch)
    with TurboPredictClient(echo_server.address, backend="native",
                            num_channels=4) as c:
        out = c.predict_sharded("default", inputs, shards=shards,
                                timeout=TIMEOUT)
    ref = reference_outputs[(batch, shards)]
    assert set(out) == set(ref) == set(inputs)
    for k in inputs:
        assert out[k].dtype == inputs[k].dtype
        assert torch.equal(out[k], inputs[k]), k
        assert torch.equal(out[k], ref[k]), k


class _RawServer:
    """C++ server with a python Predict handler that records every request
    message and echoes it; `hook(data, first_row)` may raise or block."""

    def __init__(self, hook=None, workers=8):
        self.received = []
        self._lock = threading.Lock()
        self._hook = hook
        self.srv = T.GrpcServer("127.0.0.1:0", workers)
        self.srv.register_handler(PREDICT, self._handle)
        self.address = self.srv.start()

    def _handle(self, view):
        data = bytes(view)
        with self._lock:
            self.received.append(data)
        if self._hook is not None:
            _spec, ins, _f = native.parse_predict_request(data, "cpu", 1)
            self._hook(int(ins["tag"][0, 0]))
        return native.echo_predict(data)

    def stop(self):
        self.srv.stop()


def test_same_request_messages_on_the_wire(monkeypatch):
    """Both paths put the same multiset of PredictRequest messages on the
    wire (shards may arrive in any order, and on any channel)."""
    srv = _RawServer()
    try:
        seen = {}
        for switch in ("0", "1"):
            monkeypatch.setenv("MI355X_NATIVE_SHARDED", switch)
            srv.received.clear()
            with TurboPredictClient(srv.address, backend="native",
                                    num_channels=4) as c:
                for b in BATCHES:
                    for s in SHARDS:
                        out = c.predict_sharded(
                            "m", _inputs(b), shards=s, timeout=TIMEOUT,
                            model_version=3, signature_name="sig")
                        assert torch.equal(out["images"],
                                           _inputs(b)["images"])
            seen[switch] = Counter(srv.received)
        assert sum(seen["1"].values()) == len(BATCHES) * sum(SHARDS)
        assert seen["0"] == seen["1"]
        # and each message is what the buffered serializer produces for
        # the same narrow() view
        ins = _inputs(5)
        view = {k: v.narrow(0, 0, 2) for k, v in ins.items()}
        expect = native.serialize_predict_request(
            "m", 3, "sig", list(view), [view[k] for k in view], 1)
        assert seen["1"][expect] >= 1
    finally:
        srv.stop()


def test_all_eight_channels_carry_streams(echo_server, monkeypatch):
    monkeypatch.setenv("MI355X_NATIVE_SHARDED", "1")
    with TurboPredictClient(echo_server.address, backend="native",
                            num_channels=8) as c:
        assert [ch.streams_started for ch in c._channels] == [0] * 8
        for i in range(8):
            out = c.predict_sharded("default", _inputs(7, seed=i), shards=4,
                                    timeout=TIMEOUT)
            assert torch.equal(out["tag"], _inputs(7, seed=i)["tag"])
        counts = [ch.streams_started for ch in c._channels]
    assert sum(counts) == 8 * 4
    assert all(n > 0 for n in counts), counts
    with pytest.raises(AttributeError):
        c._channels[0].streams_started = 0  # read-only


@pytest.mark.parametrize("bad_shard", [0, 2])
def test_one_shard_failing_surfaces_server_code(monkeypatch, bad_shard):
    """A handler that raises for one shard: the call fails with the
    server's status code once every other stream has been collected, and
    the same client keeps working. Shard 0 is sent by the calling thread,
    shard 2 by the sender pool."""
    monkeypatch.setenv("MI355X_NATIVE_SHARDED", "1")
    state = {"bad_row": -1}

    def hook(first_row):
        if first_row == state["bad_row"]:
            raise HandlerAbort(grpc.StatusCode.NOT_FOUND, "no such model")

    srv = _RawServer(hook)
    try:
        with TurboPredictClient(srv.address, backend="native",
                                num_channels=4) as c:
            ins = _inputs(8)  # shards of 2 rows: shard i starts at row 2i
            state["bad_row"] = 2 * bad_shard
            with pytest.raises(NativeRpcError) as ei:
                c.predict_sharded("m", ins, shards=4, timeout=TIMEOUT)
            assert ei.value.code() == grpc.StatusCode.NOT_FOUND
            assert "no such model" in ei.value.details()
            assert isinstance(ei.value, grpc.RpcError)
            # every shard reached the server: none was abandoned unsent
            assert len(srv.received) == 4
            state["bad_row"] = -1
            out = c.predict_sharded("m", ins, shards=4, timeout=TIMEOUT)
            assert torch.equal(out["images"], ins["images"])
    finally:
        srv.stop()


def test_one_shard_past_deadline(monkeypatch):
    """One shard's handler blocks past a 0.3 s deadline: the call raises
    DEADLINE_EXCEEDED (the stream is reset), the next call on the same
    client succeeds. The handler blocks on an event that the test sets,
    so nothing outlasts the deadline itself."""
    monkeypatch.setenv("MI355X_NATIVE_SHARDED", "1")
    release = threading.Event()
    state = {"slow_row": 4}

    def hook(first_row):
        if first_row == state["slow_row"]:
            release.wait(TIMEOUT)

    srv = _RawServer(hook)
    try:
        with TurboPredictClient(srv.address, backend="native",
                                num_channels=4) as c:
            ins = _inputs(8)
            try:
                with pytest.raises(NativeRpcError) as ei:
                    c.predict_sharded("m", ins, shards=4, timeout=0.3)
            finally:
                release.set()
            assert ei.value.code() == grpc.StatusCode.DEADLINE_EXCEEDED
            state["slow_row"] = -1
            out = c.predict_sharded("m", ins, shards=4, timeout=TIMEOUT)
            assert torch.equal(out["images"], ins["images"])
            assert torch.equal(out["tag"], ins["tag"])
    finally:
        srv.stop()


def test_concurrent_requests_do_not_cross(echo_server, monkeypatch):
    """4 threads x 20 requests x 4 shards (more shard sends than the
    sender pool has threads), every request with its own seeded input."""
    monkeypatch.setenv("MI355X_NATIVE_SHARDED", "1")
    assert T.SENDER_POOL_SIZE == 8
    errs = []
    with TurboPredictClient(echo_server.address, backend="native",
                            num_channels=8) as c:

        def worker(tid):
            try:
                for i in range(20):
                    g = torch.Generator().manual_seed(tid * 100 + i)
                    # 96 KB rows: every shard is a zero-copy host region
                    x = torch.randn(9, 3, 8192, generator=g)
                    ids = torch.randint(0, 1 << 30, (9, 5), generator=g,
                                        dtype=torch.int32)
                    out = c.predict_sharded(
                        "default", {"x": x, "ids": ids}, shards=4,
                        timeout=TIMEOUT)
                    if not (torch.equal(out["x"], x)
                            and torch.equal(out["ids"], ids)):
                        errs.append(f"mismatch thread={tid} req={i}")
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))

        threads = [threading.Thread(target=worker, args=(t,))
                   for t in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert errs == []


def test_sender_pool_restarts_after_shutdown(echo_server, monkeypatch):
    """close() of one client drains and joins the pool; the next sharded
    call (any client) starts it again."""
    monkeypatch.setenv("MI355X_NATIVE_SHARDED", "1")
    ins = _inputs(7)
    for _ in range(2):
        with TurboPredictClient(echo_server.address, backend="native",
                                num_channels=4) as c:
            out = c.predict_sharded("default", ins, shards=3,
                                    timeout=TIMEOUT)
            assert torch.equal(out["images"], ins["images"])
    T.shutdown_sender_pool()  # idempotent with nothing running
    T.shutdown_sender_pool()


def test_native_call_validates_arguments(echo_server):
    ch = T.GrpcChannel(echo_server.address)
    try:
        x = torch.zeros(4, 3)
        with pytest.raises(ValueError):
            T.predict_sharded([ch], PREDICT, "default", -1, "", ["x"],
                              [x], 5, -1, TIMEOUT)  # batch < shards
        with pytest.raises(ValueError):
            T.predict_sharded([ch], PREDICT, "default", -1, "", ["x", "y"],
                              [x, torch.zeros(3, 3)], 2, -1, TIMEOUT)
        with pytest.raises(ValueError):
            T.predict_sharded([ch], PREDICT, "default", -1, "", ["x"],
                              [torch.zeros(())], 1, -1, TIMEOUT)
        with pytest.raises(ValueError):
            T.predict_sharded([], PREDICT, "default", -1, "", ["x"], [x],
                              2, -1, TIMEOUT)
        # a non-contiguous input is made contiguous, like the old path
        xt = torch.arange(12, dtype=torch.float32).reshape(3, 4).t()
        parts = T.predict_sharded([ch], PREDICT, "default", -1, "", ["x"],
                                  [xt], 2, -1, TIMEOUT)
        got = torch.cat([native.parse_predict_response(raw, "cpu", 1)[1]["x"]
                         for _outs, raw in parts])
        assert torch.equal(got, xt)
    finally:
        ch.close()
