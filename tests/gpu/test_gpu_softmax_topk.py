"""Fused softmax + top-k head on the GPU: the softmax_topk kernel against CPU
references, then end to end through the raw server and the ResNet "topk"
output mode.

Classes are compared bit for bit with
``torch.sort(x.float(), 1, descending=True, stable=True)`` truncated to k,
on data with frequent ties (randn * 4 rounded through bf16).

Scores are checked on multiples of 1/8 in [-16, 16): exact in f32, bf16 and
f16, and every x - m is exact in fp32, so the only errors are those of the
formula. Against the fp64 softmax gathered at the reference indices:

    |out - ref| <= (C + 2E + 2) * 2**-24 * ref,    E = 1

* each expf is within E ulp (E = 1 is HIP's documented expf accuracy): the
  numerator and, at worst, the whole sum are each off by that;
* the C-term fp32 sum in any order adds at most (C - 1) u;
* the IEEE divide adds at most 1 u.

The smallest reference score on this data is about 4e-16 (exp(-32) over at
most 8193 terms), a normal fp32 number: no denormals are involved.
Largest error observed on an MI355X over the score cases of this file:
3.46 u at (2050, 8), k = 3, where the bound is 12 u; 2.52 u at C = 1000
(docs/test_matrix.md).

Each shape is the smallest that reaches a distinct path documented in the
kernel header (vector path iff base and C*sizeof(T) are multiples of 16;
rows up to 8192 classes are staged in LDS; the grid is capped at 2048
workgroups)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from min_tfs_client_amd import ops  # noqa: E402
from min_tfs_client_amd.models import resnet50_servable  # noqa: E402
from min_tfs_client_amd.postprocess import TopKClassification  # noqa: E402
from min_tfs_client_amd.server import ModelServer, Servable  # noqa: E402
from min_tfs_client_amd.turbo import TurboPredictClient  # noqa: E402

DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16,
          "f16": torch.float16}
U = 2.0 ** -24
E = 1
INF, NAN = float("inf"), float("nan")
SPECIAL_ROW = [0., -0., NAN, 1., 1., -INF, INF, -0., 0.]
SPECIAL_ORDER = [2, 6, 3, 4, 0, 1, 7, 8, 5]


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.require_native()


def tied_logits(shape, dtype, seed=0):
    """randn * 4 rounded through bf16: ties are frequent in every dtype."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 4).to(torch.bfloat16).to(dtype)


def eighths_logits(shape, dtype, seed=0):
    """Multiples of 1/8 in [-16, 16): exact in f32, bf16 and f16."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = (torch.randint(-128, 128, shape, generator=g).float() / 8).to(dtype)
    assert torch.equal(x.float() * 8, (x.float() * 8).round())
    return x


def reference_order(x, k):
    return torch.sort(x.float(), dim=1, descending=True,
                      stable=True).indices[:, :k]


def check_classes(out, x, k):
    """`out` = (scores, classes) from the device op against CPU `x`."""
    scores, classes = out
    B = x.shape[0]
    assert scores.is_cuda and classes.is_cuda
    assert scores.dtype == torch.float32 and classes.dtype == torch.int32
    assert tuple(scores.shape) == tuple(classes.shape) == (B, k)
    assert scores.is_contiguous() and classes.is_contiguous()
    order = reference_order(x, k)
    assert torch.equal(classes.cpu().long(), order)
    return order


def check_scores(out, x, k):
    order = check_classes(out, x, k)
    C = x.shape[1]
    ref = torch.softmax(x.double(), dim=1).gather(1, order)
    err = (out[0].cpu().double() - ref).abs()
    bound = (C + 2 * E + 2) * U * ref
    if err.numel():
        print(f"softmax_topk score error: shape {tuple(x.shape)} k {k} "
              f"{x.dtype}: max {float((err / (U * ref)).max()):.3f} u, "
              f"bound {C + 2 * E + 2} u, min ref {float(ref.min()):.3e}")
    assert bool((err <= bound).all())


def run(x, k):
    return ops.softmax_topk(x.to(DEV), k)


SHAPES = [
    ((3, 1000), 5),     # vector path for f32 and bf16/f16 (2000 B rows)
    ((2, 37), 5),       # scalar path, C < 64
    ((2, 7), 7),        # k == C
    ((2, 1), 1),        # single class
    ((1, 8192), 5),     # LDS threshold, staged side
    ((1, 8193), 5),     # LDS threshold, re-read side (scalar: odd C)
    ((2, 8200), 5),     # re-read side, vector path
    ((2050, 8), 3),     # more rows than the 2048-workgroup grid cap
    ((2, 300), 64),     # maximum k
]


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape,k", SHAPES, ids=str)
def test_classes_match_stable_sort(shape, k, dtype):
    x = tied_logits(shape, DTYPES[dtype])
    check_classes(run(x, k), x, k)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape,k", SHAPES, ids=str)
def test_scores_within_derived_bound(shape, k, dtype):
    x = eighths_logits(shape, DTYPES[dtype])
    check_scores(run(x, k), x, k)


@pytest.mark.parametrize("data", [tied_logits, eighths_logits],
                         ids=["tied", "eighths"])
def test_misaligned_rows_take_scalar_path(data):
    full = data((3, 1001), torch.bfloat16, seed=1).to(DEV)
    x_dev = full[1:]
    assert x_dev.is_contiguous() and x_dev.data_ptr() % 16 != 0
    out = ops.softmax_topk(x_dev, 5)
    x = x_dev.cpu()
    if data is eighths_logits:
        check_scores(out, x, 5)
    else:
        check_classes(out, x, 5)
    # the aligned copy (still the scalar path: 2002 B rows) agrees bitwise
    again = ops.softmax_topk(x_dev.clone(), 5)
    assert torch.equal(out[0], again[0]) and torch.equal(out[1], again[1])


def test_empty_batch_does_not_launch():
    x = torch.empty((0, 16), dtype=torch.bfloat16, device=DEV)
    scores, classes = ops.softmax_topk(x, 5)
    torch.cuda.synchronize()
    assert scores.is_cuda and classes.is_cuda
    assert tuple(scores.shape) == tuple(classes.shape) == (0, 5)
    assert scores.dtype == torch.float32 and classes.dtype == torch.int32


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("k", [1, 4, 9])
def test_special_values_row(k, dtype):
    x = torch.tensor([SPECIAL_ROW, SPECIAL_ROW[::-1]], dtype=DTYPES[dtype])
    scores, classes = run(x, k)
    check_classes((scores, classes), x, k)
    assert classes[0].tolist() == SPECIAL_ORDER[:k]
    assert bool(torch.isnan(scores).all())      # rows hold NaN and +Inf


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_neg_inf_scores_exactly_zero_and_ranks_last(dtype):
    x = eighths_logits((2, 40), DTYPES[dtype], seed=2)
    x[:, 3] = -INF
    x[:, 17] = -INF
    scores, classes = run(x, 40)
    check_scores((scores, classes), x, 40)
    assert classes[:, -2:].tolist() == [[3, 17]] * 2
    assert scores[:, -2:].tolist() == [[0.0, 0.0]] * 2


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("C", [70, 1000, 8193], ids=lambda c: f"C{c}")
def test_all_equal_row_is_index_order(C, dtype):
    x = torch.full((2, C), 1.5, dtype=DTYPES[dtype])
    scores, classes = run(x, 6)
    assert classes.tolist() == [list(range(6))] * 2
    check_scores((scores, classes), x, 6)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("C", [1000, 8200], ids=lambda c: f"C{c}")
def test_tie_pairs_across_thread_and_wave_boundaries(C, dtype):
    """Equal maxima at 63/64 (two waves) and 255/256 (the last thread and
    the first thread's next element): lower index first, pair by pair."""
    x = eighths_logits((2, C), DTYPES[dtype], seed=3)
    x[0, 63] = x[0, 64] = 20.0
    x[0, 255] = x[0, 256] = 18.0
    x[1, 255] = x[1, 256] = 20.0
    x[1, 63] = x[1, 64] = 18.0
    out = run(x, 5)
    check_scores(out, x, 5)
    assert out[1][:, :4].tolist() == [[63, 64, 255, 256],
                                      [255, 256, 63, 64]]


@pytest.mark.parametrize("shape,k", [((3, 1000), 5), ((1, 8193), 50)],
                         ids=str)
def test_deterministic(shape, k):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(shape, generator=g).to(torch.bfloat16).to(DEV)
    a = ops.softmax_topk(x, k)
    b = ops.softmax_topk(x, k)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_launch_uses_current_stream():
    x = eighths_logits((3, 1000), torch.bfloat16, seed=5)
    x_dev = x.to(DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        out = ops.softmax_topk(x_dev, 5)
    stream.synchronize()
    check_scores(out, x, 5)


def test_device_tensor_errors_are_value_errors():
    x = torch.zeros((2, 16), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        ops.softmax_topk(x[:, ::2], 2)                       # strided
    with pytest.raises(ValueError):
        ops.softmax_topk(x, 17)                              # k > C
    with pytest.raises(ValueError):
        ops.softmax_topk(x, 0)
    with pytest.raises(ValueError):
        ops.softmax_topk(x.double(), 2)
    with pytest.raises(ValueError):
        ops.softmax_topk(x[0], 2)


# ---------------------------------------------------------------------------
# end to end through the raw server (mirrors test_gpu_masked_mean_pool.py)
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def server(tmp_path_factory):
    sock = f"unix://{tmp_path_factory.mktemp('s')}/topk.sock"
    with ModelServer(address=sock, raw_predict=True, device=DEV) as srv:
        head = Servable(lambda inputs: {"logits": inputs["x"]},
                        postprocess=TopKClassification(5))
        srv.manager.load("head", head, version=1)
        srv.manager.load(
            "resnet_topk",
            resnet50_servable(DEV, torch.bfloat16, output_format="topk"),
            version=1)
        yield srv


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_postprocess_hook_end_to_end(server, dtype):
    x = eighths_logits((4, 1000), DTYPES[dtype], seed=6)
    with TurboPredictClient(server.address) as client:
        out = client.predict("head", {"x": x.to(DEV)}, output_device=DEV)
    assert set(out) == {"scores", "classes"}
    check_scores((out["scores"], out["classes"]), x, 5)


def test_resnet_topk_end_to_end(server):
    g = torch.Generator().manual_seed(7)
    images = torch.randn(2, 3, 224, 224, generator=g)
    with TurboPredictClient(server.address) as client:
        out = client.predict("resnet_topk", {"images": images.to(DEV)},
                             output_device=DEV)
    assert set(out) == {"scores", "classes"}
    scores, classes = out["scores"].cpu(), out["classes"].cpu()
    assert scores.dtype == torch.float32 and tuple(scores.shape) == (2, 5)
    assert classes.dtype == torch.int32 and tuple(classes.shape) == (2, 5)
    assert bool(torch.isfinite(scores).all()) and bool((scores > 0).all())
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())     # descending
    assert bool((scores.double().sum(1) <= 1.0).all())
    assert bool(((classes >= 0) & (classes < 1000)).all())
    for row in classes.tolist():
        assert len(set(row)) == 5
