"""Fused masked mean-pool head on the GPU: the masked_pool kernels against
CPU references, then end to end through the raw server and the BERT
"sentence_embedding" output mode.

Hidden states are integers in [-8, 8]: exact in bf16, f16 and f32, and every
fp32 partial sum is exact in any order (|sum| <= 8*S < 2**24). The mean is
then one correctly rounded division and must equal the CPU reference bit for
bit, whatever the kernel's reduction order. With normalize=True the result
is compared with the fp64 reference component-wise:
|out - ref| <= (H/2 + 8) * 2**-24 * |ref| (each y_i correctly rounded: 1u;
H squares summed in any order: <= (H+1)u; sqrt halves that and adds 1u; the
final division adds 1u).

Each shape is the smallest that reaches a distinct path documented in the
kernel header (tiles = ceil(H/VEC/64); S is split iff B*tiles < 1024 and
S > 16; grids are capped at 2048 workgroups)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from min_tfs_client_amd import ops  # noqa: E402
from min_tfs_client_amd.models import bert_servable  # noqa: E402
from min_tfs_client_amd.server import ModelServer  # noqa: E402
from min_tfs_client_amd.turbo import TurboPredictClient  # noqa: E402

DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16,
          "f16": torch.float16}
U = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.require_native()


def int_hidden(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).to(dtype)


def holey_mask(B, S, seed=0, dtype=torch.int32):
    """Random keep/drop per position: holes, not only a padded suffix."""
    g = torch.Generator().manual_seed(100 + seed)
    m = torch.randint(0, 2, (B, S), generator=g)
    if S:
        m[:, 0] = 1
    return m.to(dtype)


def _keep(x, mask):
    B, S, _ = x.shape
    return torch.ones(B, S, dtype=torch.bool) if mask is None else mask != 0


def mean_reference(x, mask):
    """fp32 select-sum and one division (exact for int_hidden data)."""
    keep = _keep(x, mask)
    total = torch.where(keep[..., None], x.float(), torch.zeros(())).sum(1)
    return total / keep.sum(1, keepdim=True).clamp(min=1).float()


def mean_reference64(x, mask):
    keep = _keep(x, mask)
    total = torch.where(keep[..., None], x.double(),
                        torch.zeros((), dtype=torch.float64)).sum(1)
    return total / keep.sum(1, keepdim=True).clamp(min=1).double()


def normalized_reference64(x, mask):
    y = mean_reference64(x, mask)
    return y / y.norm(dim=1, keepdim=True).clamp(min=1e-12)


def check_output(out, x, mask, normalize):
    """`out` from the device op against the CPU reference of (x, mask)."""
    B, _, H = x.shape
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
    assert tuple(out.shape) == (B, H)
    out = out.cpu()
    if normalize:
        ref = normalized_reference64(x, mask)
        bound = (H / 2 + 8) * U * ref.abs()
        assert bool(((out.double() - ref).abs() <= bound).all())
    else:
        assert torch.equal(out, mean_reference(x, mask))
    return out


def check(x, mask, normalize):
    out = ops.masked_mean_pool(
        x.to(DEV), None if mask is None else mask.to(DEV), normalize)
    return check_output(out, x, mask, normalize)


SHAPES = [
    (3, 7, 40),       # vector path: f32 rows are 160 B, bf16/f16 rows 80 B
    (2, 5, 37),       # scalar path, ragged H
    (2, 130, 768),    # S split, slices shorter than one unrolled step
    (1, 512, 768),    # small B: 32 slices of 16 rows, unrolled loop
    (4100, 2, 64),    # more work items than the 2048-workgroup grid cap
    (2, 16, 64),      # S == 16: not split
    (2, 17, 64),      # S == 17: split in two
    (1024, 40, 8),    # B*tiles == 1024: not split; unrolled loop + tail
    (1023, 40, 8),    # B*tiles == 1023: split in two
    (2, 0, 40),       # S == 0: zeros
]


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernel_matches_reference(shape, dtype, normalize):
    x = int_hidden(shape, DTYPES[dtype])
    check(x, holey_mask(shape[0], shape[1]), normalize)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_storage_offset_takes_scalar_path(dtype, normalize):
    B, S, H = 3, 7, 40
    n = B * S * H
    flat = int_hidden((n + 8,), DTYPES[dtype], seed=1).to(DEV)
    x_dev = flat[1:1 + n].view(B, S, H)
    assert x_dev.is_contiguous() and x_dev.data_ptr() % 16 != 0
    mask = holey_mask(B, S, seed=1)
    out = ops.masked_mean_pool(x_dev, mask.to(DEV), normalize)
    check_output(out, x_dev.cpu(), mask, normalize)
    # the aligned copy takes the vector path; the sums are exact on this
    # data, so both paths hand the same partials to the same finalize
    aligned = ops.masked_mean_pool(x_dev.clone(), mask.to(DEV), normalize)
    assert torch.equal(out, aligned)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("case", ["all_zero_row", "none", "bool", "uint8",
                                  "int32_values"])
def test_mask_cases(case, normalize):
    x = int_hidden((3, 40, 72), torch.bfloat16, seed=2)
    mask = holey_mask(3, 40, seed=2)
    if case == "all_zero_row":
        mask[1] = 0
        out = check(x, mask, normalize)
        assert torch.equal(out[1], torch.zeros(72))
    elif case == "none":
        out = check(x, None, normalize)
        ones = torch.ones(3, 40, dtype=torch.int32, device=DEV)
        assert torch.equal(
            out, ops.masked_mean_pool(x.to(DEV), ones, normalize).cpu())
    elif case == "bool":
        check(x, mask != 0, normalize)
    elif case == "uint8":
        check(x, (mask * 255).to(torch.uint8), normalize)
    else:
        # any non-zero int32 keeps, negative and high-bit values included
        values = torch.tensor([1, -1, 1 << 30, -(1 << 31), 256],
                              dtype=torch.int32)
        check(x, mask * values[torch.arange(40) % 5], normalize)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_nan_inf_at_masked_positions_do_not_leak(dtype, normalize):
    clean = int_hidden((3, 40, 72), DTYPES[dtype], seed=3)
    mask = holey_mask(3, 40, seed=3)
    mask[2] = 0                                  # an all-masked row too
    x = clean.clone()
    poison = torch.tensor([float("nan"), float("inf"), -float("inf")])
    for i, (b, s) in enumerate((mask == 0).nonzero().tolist()):
        x[b, s, :] = poison[i % 3]
    out = ops.masked_mean_pool(x.to(DEV), mask.to(DEV), normalize)
    assert bool(torch.isfinite(out).all())
    check_output(out, clean, mask, normalize)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", [(2, 130, 768), (1, 512, 768),
                                   (2, 5, 37)], ids=str)
def test_randn_mean_within_summation_bound(shape, dtype):
    """fp32 summation of n = cnt terms in any order:
    |out - ref| <= (cnt + 2) * 2**-24 * sum_s|x| / cnt."""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(shape, generator=g).to(DTYPES[dtype])
    mask = holey_mask(shape[0], shape[1], seed=4)
    out = ops.masked_mean_pool(x.to(DEV), mask.to(DEV)).cpu()
    keep = mask != 0
    cnt = keep.sum(1, keepdim=True).double()
    abs_sum = torch.where(keep[..., None], x.double().abs(),
                          torch.zeros((), dtype=torch.float64)).sum(1)
    bound = (cnt + 2) * U * abs_sum / cnt
    err = (out.double() - mean_reference64(x, mask)).abs()
    assert bool((err <= bound).all())


@pytest.mark.parametrize("normalize", [False, True])
def test_deterministic(normalize):
    g = torch.Generator().manual_seed(5)
    x = torch.randn((1, 512, 768), generator=g).to(torch.bfloat16).to(DEV)
    mask = holey_mask(1, 512, seed=5).to(DEV)
    a = ops.masked_mean_pool(x, mask, normalize)
    b = ops.masked_mean_pool(x, mask, normalize)
    assert torch.equal(a, b)


@pytest.mark.parametrize("normalize", [False, True])
def test_empty_batch_does_not_launch(normalize):
    x = torch.empty((0, 7, 40), dtype=torch.bfloat16, device=DEV)
    mask = torch.empty((0, 7), dtype=torch.int32, device=DEV)
    y = ops.masked_mean_pool(x, mask, normalize)
    torch.cuda.synchronize()
    assert y.is_cuda and tuple(y.shape) == (0, 40)
    assert y.dtype == torch.float32


def test_launch_uses_current_stream():
    x = int_hidden((2, 130, 768), torch.bfloat16, seed=6)
    mask = holey_mask(2, 130, seed=6)
    x_dev, m_dev = x.to(DEV), mask.to(DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        y = ops.masked_mean_pool(x_dev, m_dev, True)
    stream.synchronize()
    check_output(y, x, mask, True)


def test_device_tensor_errors_are_value_errors():
    x = torch.zeros((2, 5, 16), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        ops.masked_mean_pool(x[..., ::2])                      # strided
    with pytest.raises(ValueError):
        ops.masked_mean_pool(x, torch.ones(2, 5, dtype=torch.int32))  # CPU


# ---------------------------------------------------------------------------
# end to end through the raw server (mirrors test_gpu_image_preprocess.py)
# ---------------------------------------------------------------------------

class StubEncoder(torch.nn.Module):
    """Stands in for the encoder: a fixed integer-valued hidden state."""

    def __init__(self, hidden):
        super().__init__()
        self.hidden = hidden

    def forward(self, input_ids, attention_mask=None):
        B, S = input_ids.shape
        assert (B, S) == tuple(self.hidden.shape[:2])
        return self.hidden, torch.zeros(B, 768, device=self.hidden.device,
                                        dtype=self.hidden.dtype)


STUB_HIDDEN = int_hidden((4, 16, 768), torch.bfloat16, seed=7)


@pytest.fixture(scope="module")
def server(tmp_path_factory):
    sock = f"unix://{tmp_path_factory.mktemp('s')}/pool.sock"
    with ModelServer(address=sock, raw_predict=True, device=DEV) as srv:
        stub = bert_servable(DEV, torch.bfloat16,
                             output_format="sentence_embedding")
        stub.module = StubEncoder(STUB_HIDDEN.to(DEV))
        srv.manager.load("bert_stub", stub, version=1)
        srv.manager.load(
            "bert_embed",
            bert_servable(DEV, torch.bfloat16,
                          output_format="sentence_embedding"),
            version=1)
        yield srv


def test_stub_sentence_embedding_end_to_end(server):
    ids = torch.zeros(4, 16, dtype=torch.int32)
    mask = holey_mask(4, 16, seed=7)
    with TurboPredictClient(server.address) as client:
        out = client.predict(
            "bert_stub",
            {"input_ids": ids.to(DEV), "attention_mask": mask.to(DEV)},
            output_device=DEV)
    assert set(out) == {"sentence_embedding"}
    check_output(out["sentence_embedding"], STUB_HIDDEN, mask, True)


def test_bert_sentence_embedding_end_to_end(server):
    g = torch.Generator().manual_seed(8)
    ids = torch.randint(0, 30522, (2, 16), generator=g).to(torch.int32)
    mask = torch.ones(2, 16, dtype=torch.int32)
    mask[1, 9:] = 0
    with TurboPredictClient(server.address) as client:
        out = client.predict(
            "bert_embed",
            {"input_ids": ids.to(DEV), "attention_mask": mask.to(DEV)},
            output_device=DEV)
    assert set(out) == {"sentence_embedding"}
    emb = out["sentence_embedding"]
    assert tuple(emb.shape) == (2, 768) and emb.dtype == torch.float32
    assert bool(torch.isfinite(emb).all())
    norms = emb.double().norm(dim=1).cpu()
    assert bool(((norms - 1).abs() <= (768 / 2 + 8) * U).all())
