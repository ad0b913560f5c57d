"""Fused softmax + top-k head, CPU side: the eager twin of the kernel
(``ops.softmax_topk`` on CPU tensors), the ``Servable(postprocess=)`` output
hook, ``postprocess.TopKClassification``, the ResNet ``output_format="topk"``
mode with its ``model.json`` keys, and ``ClassificationAdapter(top_k=)``.

The order is checked against ``torch.sort(x.float(), 1, descending=True,
stable=True)``, which is the contract; scores against the fp64 softmax
gathered at those indices."""
import json

import grpc
import numpy as np
import pytest
import torch

from min_tfs_client_amd import ops
from min_tfs_client_amd.batching import BatchingServable
from min_tfs_client_amd.client import TensorServingClient
from min_tfs_client_amd.examples_adapter import (ClassificationAdapter,
                                                 examples_input)
from min_tfs_client_amd.models import resnet50_servable
from min_tfs_client_amd.postprocess import TopKClassification
from min_tfs_client_amd.repository import default_loader
from min_tfs_client_amd.server import ModelServer, Servable
from min_tfs_client_amd.tensors import tensor_proto_to_ndarray

INF, NAN = float("inf"), float("nan")
SPECIAL_ROW = [0., -0., NAN, 1., 1., -INF, INF, -0., 0.]
SPECIAL_ORDER = [2, 6, 3, 4, 0, 1, 7, 8, 5]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
U = 2.0 ** -24


def reference_order(x, k):
    return torch.sort(x.float(), dim=1, descending=True,
                      stable=True).indices[:, :k]


def reference_scores(x, order):
    return torch.softmax(x.double(), dim=1).gather(1, order)


def tied_logits(shape, dtype, seed=0):
    """randn * 4 rounded through bf16: ties are frequent in every dtype."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 4).to(torch.bfloat16).to(dtype)


# ---------------------------------------------------------------------------
# ops.softmax_topk, CPU tensors
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape,k", [((3, 1000), 5), ((2, 37), 5),
                                     ((2, 7), 7), ((2, 1), 1),
                                     ((2, 300), 64), ((4, 9), 1)], ids=str)
def test_order_and_scores_match_reference(shape, k, dtype):
    x = tied_logits(shape, dtype)
    scores, classes = ops.softmax_topk(x, k)
    assert scores.dtype == torch.float32 and classes.dtype == torch.int32
    assert tuple(scores.shape) == tuple(classes.shape) == (shape[0], k)
    assert scores.is_contiguous() and classes.is_contiguous()
    order = reference_order(x, k)
    assert torch.equal(classes.long(), order)
    ref = reference_scores(x, order)
    # torch's CPU exp and sum are not pinned to 1 ulp here: a loose relative
    # check of the formula; the GPU test holds the kernel to its derived bound
    assert bool(((scores.double() - ref).abs() <= 1e-5 * ref).all())


@pytest.mark.parametrize("k", [1, 4, 9])
def test_special_values_order(k):
    x = torch.tensor([SPECIAL_ROW])
    scores, classes = ops.softmax_topk(x, k)
    assert classes.tolist() == [SPECIAL_ORDER[:k]]
    assert torch.equal(classes.long(), reference_order(x, k))
    assert bool(torch.isnan(scores).all())      # the row holds NaN and +Inf


def test_pos_inf_row_scores_nan():
    scores, classes = ops.softmax_topk(torch.tensor([[1., INF, 2.]]), 3)
    assert classes.tolist() == [[1, 2, 0]]
    assert bool(torch.isnan(scores).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_all_equal_row_is_index_order(dtype):
    x = torch.full((2, 70), 1.5, dtype=dtype)
    scores, classes = ops.softmax_topk(x, 6)
    assert classes.tolist() == [list(range(6))] * 2
    ref = torch.full((2, 6), 1 / 70, dtype=torch.float64)
    assert bool(((scores.double() - ref).abs() <= 74 * U * ref).all())


def test_single_class():
    scores, classes = ops.softmax_topk(torch.tensor([[-3.], [7.]]), 1)
    assert classes.tolist() == [[0], [0]]
    assert scores.tolist() == [[1.0], [1.0]]


def test_neg_inf_scores_exactly_zero_and_ranks_last():
    x = torch.tensor([[1., -INF, 2., -INF, 2.]])
    scores, classes = ops.softmax_topk(x, 5)
    assert classes.tolist() == [[2, 4, 0, 1, 3]]
    assert scores[0, 3:].tolist() == [0.0, 0.0]
    assert float(scores.sum()) == pytest.approx(1.0, abs=1e-6)


def test_empty_batch():
    scores, classes = ops.softmax_topk(torch.empty((0, 16)), 4)
    assert tuple(scores.shape) == tuple(classes.shape) == (0, 4)
    assert scores.dtype == torch.float32 and classes.dtype == torch.int32


@pytest.mark.parametrize("logits,k", [
    (np.zeros((2, 8), np.float32), 2),                    # not a tensor
    ([[1.0, 2.0]], 1),
    (torch.zeros(8), 2),                                  # rank
    (torch.zeros(2, 3, 8), 2),
    (torch.zeros(2, 8, dtype=torch.float64), 2),          # dtype
    (torch.zeros(2, 8, dtype=torch.int32), 2),
    (torch.zeros(2, 16)[:, ::2], 2),                      # not contiguous
    (torch.zeros(2, 8), 0),                               # k range
    (torch.zeros(2, 8), -1),
    (torch.zeros(2, 8), 9),
    (torch.zeros(2, 100), 65),
    (torch.zeros(2, 0), 1),
    (torch.zeros(0, 8), 9),                               # also when B == 0
    (torch.zeros(2, 8), 2.0),                             # k type
    (torch.zeros(2, 8), True),
    (torch.zeros(2, 8), None),
], ids=lambda v: str(getattr(v, "shape", v)))
def test_invalid_arguments_raise_value_error(logits, k):
    with pytest.raises(ValueError):
        ops.softmax_topk(logits, k)


# ---------------------------------------------------------------------------
# Servable(postprocess=) and TopKClassification
# ---------------------------------------------------------------------------

def test_servable_applies_postprocess_to_fn_result():
    seen = []

    def post(outputs):
        seen.append(dict(outputs))
        return {"doubled": outputs["y"] * 2}

    s = Servable(lambda inputs: {"y": inputs["x"] + 1}, postprocess=post)
    out = s({"x": np.array([1.0, 2.0])})
    assert set(out) == {"doubled"} and out["doubled"].tolist() == [4.0, 6.0]
    assert len(seen) == 1 and seen[0]["y"].tolist() == [2.0, 3.0]


def test_servable_without_postprocess_is_unchanged():
    s = Servable(lambda inputs: {"y": inputs["x"]})
    assert s.postprocess is None
    x = np.array([1.0])
    assert s({"x": x})["y"] is x


def test_servable_runs_preprocess_then_fn_then_postprocess():
    s = Servable(lambda inputs: {"y": inputs["x"] + ["fn"]},
                 preprocess={"x": lambda v: v + ["pre"]},
                 postprocess=lambda o: {"y": o["y"] + ["post"]})
    assert s({"x": ["in"]})["y"] == ["in", "pre", "fn", "post"]


def test_servable_rejects_non_callable_postprocess():
    with pytest.raises(ValueError, match="postprocess"):
        Servable(lambda inputs: inputs, postprocess={"y": abs})


def test_batching_servable_gets_postprocess_from_inner():
    x = tied_logits((3, 20), torch.float32, seed=1)
    inner = Servable(lambda inputs: {"logits": inputs["x"]},
                     postprocess=TopKClassification(4))
    batched = BatchingServable(inner, max_batch_size=8,
                               batch_timeout_s=0.001)
    try:
        out = batched({"x": x})
    finally:
        batched.close()
    assert set(out) == {"scores", "classes"}
    assert torch.equal(torch.as_tensor(out["classes"]).long(),
                       reference_order(x, 4))


@pytest.mark.parametrize("as_numpy", [False, True], ids=["torch", "numpy"])
def test_topk_classification_replaces_logits(as_numpy):
    x = tied_logits((3, 50), torch.float32, seed=2)
    other = torch.arange(3)
    given = {"logits": x.numpy() if as_numpy else x, "other": other}
    out = TopKClassification(5)(given)
    assert set(out) == {"scores", "classes", "other"} and out["other"] is other
    assert set(given) == {"logits", "other"}            # not mutated
    want_scores, want_classes = ops.softmax_topk(x, 5)
    assert isinstance(out["scores"], torch.Tensor)
    assert torch.equal(out["scores"], want_scores)
    assert torch.equal(out["classes"], want_classes)


def test_topk_classification_read_only_numpy_and_bf16():
    x = tied_logits((2, 30), torch.bfloat16, seed=3)
    arr = x.float().numpy()
    arr.setflags(write=False)
    out = TopKClassification(3)({"logits": arr})
    assert torch.equal(out["classes"].long(), reference_order(x, 3))
    out = TopKClassification(3)({"logits": x})          # bf16 as it is
    assert torch.equal(out["classes"].long(), reference_order(x, 3))


def test_topk_classification_aliases():
    post = TopKClassification(2, logits="y", scores="p", classes="ids")
    out = post({"y": torch.tensor([[0., 3., 1.]])})
    assert set(out) == {"p", "ids"} and out["ids"].tolist() == [[1, 2]]


def test_topk_classification_errors():
    with pytest.raises(ValueError, match="logits"):
        TopKClassification(2)({"probs": torch.zeros(1, 4)})
    with pytest.raises(ValueError):
        TopKClassification(5)({"logits": torch.zeros(1, 4)})    # k > C
    with pytest.raises(ValueError):
        TopKClassification(2)({"logits": torch.zeros(4)})       # rank
    for k in (0, 65, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            TopKClassification(k)
    with pytest.raises(ValueError):
        TopKClassification(2, scores="a", classes="a")


def test_postprocess_value_error_is_invalid_argument(sock_dir):
    addr = f"unix://{sock_dir}/topk.sock"
    servable = Servable(lambda inputs: {"logits": inputs["x"]},
                        postprocess=TopKClassification(5))
    x = tied_logits((2, 12), torch.float32, seed=4)
    with ModelServer(address=addr, transport="grpcio") as srv:
        srv.manager.load("head", servable, version=1)
        with TensorServingClient("unix", f"//{sock_dir}/topk.sock",
                                 backend="grpcio") as client:
            resp = client.predict_request("head", {"x": x.numpy()},
                                          timeout=20)
            assert set(resp.outputs) == {"scores", "classes"}
            classes = tensor_proto_to_ndarray(resp.outputs["classes"])
            assert classes.dtype == np.int32
            assert classes.tolist() == reference_order(x, 5).tolist()
            scores = tensor_proto_to_ndarray(resp.outputs["scores"])
            assert scores.dtype == np.float32 and scores.shape == (2, 5)
            with pytest.raises(grpc.RpcError) as ei:         # C = 3 < k
                client.predict_request(
                    "head", {"x": np.zeros((2, 3), np.float32)}, timeout=20)
            assert ei.value.code() == grpc.StatusCode.INVALID_ARGUMENT


# ---------------------------------------------------------------------------
# resnet50_servable(output_format="topk") and its model.json keys
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def resnet_top3():
    return resnet50_servable(output_format="topk", top_k=3)


def test_resnet_topk_signature(resnet_top3):
    assert resnet_top3.signature["outputs"] == {
        "scores": (1, [-1, 3]), "classes": (3, [-1, 3])}
    assert resnet_top3.signature["inputs"] == {
        "images": (1, [-1, 3, 224, 224])}
    assert isinstance(resnet_top3.postprocess, TopKClassification)
    assert resnet_top3.postprocess.k == 3


def test_resnet_topk_forward(resnet_top3):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 3, 224, 224, generator=g)
    out = resnet_top3({"images": x})
    assert set(out) == {"scores", "classes"}
    scores, classes = out["scores"], out["classes"]
    assert scores.dtype == torch.float32 and tuple(scores.shape) == (1, 3)
    assert classes.dtype == torch.int32 and tuple(classes.shape) == (1, 3)
    # the head of this very model's logits
    with torch.no_grad():
        logits = resnet_top3.module(x)
    want_scores, want_classes = ops.softmax_topk(logits, 3)
    assert torch.equal(classes, want_classes)
    assert torch.equal(scores, want_scores)


def test_resnet_topk_default_is_five():
    # signature only: the postprocess is built before the model is used
    s = resnet50_servable(output_format="topk")
    assert s.signature["outputs"] == {
        "scores": (1, [-1, 5]), "classes": (3, [-1, 5])}


def test_resnet_invalid_output_arguments():
    with pytest.raises(ValueError, match="output_format"):
        resnet50_servable(output_format="probs")
    for k in (0, 65):
        with pytest.raises(ValueError, match="k must be"):
            resnet50_servable(output_format="topk", top_k=k)


def _version_dir(tmp_path, cfg):
    vdir = tmp_path / "m" / "1"
    vdir.mkdir(parents=True)
    (vdir / "model.json").write_text(json.dumps(cfg))
    return str(vdir)


def test_loader_passes_resnet_output_format_and_top_k(tmp_path):
    s = default_loader("m", _version_dir(
        tmp_path, {"family": "resnet50", "output_format": "topk",
                   "top_k": 7}))
    assert s.signature["outputs"] == {
        "scores": (1, [-1, 7]), "classes": (3, [-1, 7])}
    assert s.postprocess.k == 7


def test_loader_without_output_keys_is_unchanged(tmp_path):
    s = default_loader("m", _version_dir(tmp_path, {"family": "resnet50"}))
    assert s.signature["outputs"] == {"logits": (1, [-1, 1000])}
    assert s.postprocess is None


def test_loader_unknown_resnet_output_format_raises(tmp_path):
    with pytest.raises(ValueError, match="output_format"):
        default_loader("m", _version_dir(
            tmp_path, {"family": "resnet50", "output_format": "top5"}))


# ---------------------------------------------------------------------------
# ClassificationAdapter(top_k=)
# ---------------------------------------------------------------------------

LABELS = ["ant", "bee", "cat", "dog"]        # class 4 has no label


def _logits_servable(as_torch=False):
    def fn(features):
        x = features["x"].astype(np.float32)
        return {"scores": torch.from_numpy(x) if as_torch else x}
    return Servable(fn)


@pytest.mark.parametrize("as_torch", [False, True], ids=["numpy", "torch"])
def test_classification_adapter_top_k_order_and_labels(as_torch):
    adapter = ClassificationAdapter(_logits_servable(as_torch),
                                    labels=LABELS, top_k=3)
    rows = [[0.5, 2.0, 2.0, -1.0, 3.0], [1.0, 1.0, 1.0, 1.0, 1.0]]
    result = adapter.classify(examples_input([{"x": r} for r in rows]))
    assert len(result.classifications) == 2
    first, second = result.classifications
    assert [c.label for c in first.classes] == ["4", "bee", "cat"]
    assert [c.label for c in second.classes] == ["ant", "bee", "cat"]
    want, _ = ops.softmax_topk(torch.tensor(rows), 3)
    for cls, row in zip(result.classifications, want.tolist()):
        assert [c.score for c in cls.classes] == row
    assert [c.score for c in second.classes] == pytest.approx([0.2] * 3)


def test_classification_adapter_top_k_errors():
    for k in (0, 65, 1.5):
        with pytest.raises(ValueError):
            ClassificationAdapter(_logits_servable(), top_k=k)
    adapter = ClassificationAdapter(_logits_servable(), top_k=4)
    with pytest.raises(ValueError):                       # 2 classes < 4
        adapter.classify(examples_input([{"x": [1.0, 2.0]}]))


def test_classification_adapter_without_top_k_is_unchanged():
    rows = [[0.5, 2.0, 2.0, -1.0, 3.0], [1.0, 1.0, 1.0, 1.0, 1.0]]
    request = examples_input([{"x": r} for r in rows])
    adapter = ClassificationAdapter(_logits_servable(), labels=LABELS)
    assert adapter.top_k is None
    result = adapter.classify(request)
    for cls, row in zip(result.classifications, rows):
        assert [c.label for c in cls.classes] == LABELS + ["4"]
        assert [c.score for c in cls.classes] == row
    explicit = ClassificationAdapter(_logits_servable(), labels=LABELS,
                                     top_k=None).classify(request)
    assert explicit.SerializeToString() == result.SerializeToString()
