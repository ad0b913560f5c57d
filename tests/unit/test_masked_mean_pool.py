"""ops.masked_mean_pool on CPU, the BERT "sentence_embedding" output mode
and the model.json I/O-mode keys.

Hidden states are integers in [-8, 8]: exact in bf16, f16 and f32, and every
fp32 partial sum is exact in any order (|sum| <= 8*S < 2**24). The mean is
then one correctly rounded division, so it must equal the reference
bit for bit. With normalize=True the result is compared with the fp64
reference component-wise: |out - ref| <= (H/2 + 8) * 2**-24 * |ref| (each
y_i correctly rounded: 1u; H squares summed in any order: <= (H+1)u; sqrt
halves that and adds 1u; the final division adds 1u)."""
import json

import pytest
import torch

from min_tfs_client_amd import ops
from min_tfs_client_amd.models import bert_servable
from min_tfs_client_amd.repository import default_loader

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16,
          "f16": torch.float16}
SHAPES = [(3, 7, 40), (2, 5, 37), (1, 1, 8)]
U = 2.0 ** -24


def int_hidden(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).to(dtype)


def holey_mask(B, S, seed=0, dtype=torch.int32):
    """Random keep/drop per position: holes, not only a padded suffix."""
    g = torch.Generator().manual_seed(100 + seed)
    m = torch.randint(0, 2, (B, S), generator=g)
    m[:, 0] = 1                      # every row keeps something
    return m.to(dtype)


def mean_reference(x, mask):
    """fp32 select-sum and one division (exact for int_hidden data)."""
    B, S, _ = x.shape
    keep = torch.ones(B, S, dtype=torch.bool) if mask is None else mask != 0
    total = torch.where(keep[..., None], x.float(), torch.zeros(())).sum(1)
    return total / keep.sum(1, keepdim=True).clamp(min=1).float()


def normalized_reference64(x, mask):
    B, S, _ = x.shape
    keep = torch.ones(B, S, dtype=torch.bool) if mask is None else mask != 0
    total = torch.where(keep[..., None], x.double(),
                        torch.zeros((), dtype=torch.float64)).sum(1)
    y = total / keep.sum(1, keepdim=True).clamp(min=1).double()
    return y / y.norm(dim=1, keepdim=True).clamp(min=1e-12)


def check(x, mask, normalize, ref_mask="same"):
    ref_mask = mask if isinstance(ref_mask, str) else ref_mask
    out = ops.masked_mean_pool(x, mask, normalize)
    B, _, H = x.shape
    assert out.dtype == torch.float32 and out.is_contiguous()
    assert tuple(out.shape) == (B, H)
    if normalize:
        ref = normalized_reference64(x, ref_mask)
        bound = (H / 2 + 8) * U * ref.abs()
        assert bool(((out.double() - ref).abs() <= bound).all())
    else:
        assert torch.equal(out, mean_reference(x, ref_mask))
    return out


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_cpu_op_matches_reference(shape, dtype, normalize):
    x = int_hidden(shape, DTYPES[dtype])
    check(x, holey_mask(shape[0], shape[1]), normalize)


@pytest.mark.parametrize("normalize", [False, True])
def test_mask_none_keeps_everything(normalize):
    x = int_hidden((3, 7, 40), torch.bfloat16, seed=1)
    out = check(x, None, normalize)
    ones = torch.ones(3, 7, dtype=torch.int32)
    assert torch.equal(out, ops.masked_mean_pool(x, ones, normalize))


@pytest.mark.parametrize("normalize", [False, True])
def test_all_zero_mask_row_gives_zeros(normalize):
    x = int_hidden((3, 7, 40), torch.float32, seed=2)
    mask = holey_mask(3, 7)
    mask[1] = 0
    out = check(x, mask, normalize)
    assert torch.equal(out[1], torch.zeros(40))


@pytest.mark.parametrize("normalize", [False, True])
def test_nan_inf_at_masked_positions_do_not_leak(normalize):
    x = int_hidden((3, 7, 40), torch.float32, seed=3)
    mask = holey_mask(3, 7)
    mask[2] = 0                                  # an all-masked row too
    clean = x.clone()
    poison = torch.tensor([float("nan"), float("inf"), -float("inf")])
    drop = (mask == 0).nonzero()
    for i, (b, s) in enumerate(drop.tolist()):
        x[b, s, :] = poison[i % 3]
    out = ops.masked_mean_pool(x, mask, normalize)
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out, check(clean, mask, normalize))


def test_int64_mask_high_bits_are_kept():
    x = int_hidden((2, 5, 37), torch.float32, seed=4)
    mask = torch.tensor([[1 << 32, 0, 1, 0, 1 << 40],
                         [0, 1 << 32, 0, 0, 0]], dtype=torch.int64)
    check(x, mask, False, ref_mask=(mask != 0))
    # a plain int32 cast would have dropped 1 << 32
    assert not torch.equal(
        ops.masked_mean_pool(x, mask),
        ops.masked_mean_pool(x, mask.to(torch.int32)))


def test_bool_and_uint8_masks():
    x = int_hidden((3, 7, 40), torch.float16, seed=5)
    mask = holey_mask(3, 7)
    ref = check(x, mask, False)
    assert torch.equal(ops.masked_mean_pool(x, mask != 0), ref)
    assert torch.equal(ops.masked_mean_pool(x, mask.to(torch.uint8)), ref)


def test_non_contiguous_mask_is_accepted():
    x = int_hidden((3, 7, 40), torch.float32, seed=6)
    wide = holey_mask(3, 14)
    mask = wide[:, ::2]
    assert not mask.is_contiguous()
    assert torch.equal(ops.masked_mean_pool(x, mask),
                       mean_reference(x, mask.contiguous()))


def test_validation_raises_value_error():
    x = torch.zeros(2, 5, 8)
    ok = torch.ones(2, 5, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.masked_mean_pool([[1.0]])                       # non-tensor
    with pytest.raises(ValueError):
        ops.masked_mean_pool(torch.zeros(5, 8))             # rank 2
    with pytest.raises(ValueError):
        ops.masked_mean_pool(torch.zeros(1, 2, 5, 8))       # rank 4
    with pytest.raises(ValueError):
        ops.masked_mean_pool(x.double())                    # dtype
    with pytest.raises(ValueError):
        ops.masked_mean_pool(x.to(torch.int32))             # dtype
    with pytest.raises(ValueError):
        ops.masked_mean_pool(torch.zeros(2, 5, 16)[..., ::2])   # strided
    with pytest.raises(ValueError):
        ops.masked_mean_pool(x, torch.ones(2, 4, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.masked_mean_pool(x, torch.ones(2, 5, 1, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.masked_mean_pool(x, torch.ones(2, 5))           # float mask
    with pytest.raises(ValueError):
        ops.masked_mean_pool(x, ok.to("meta"))              # other device
    assert ops.masked_mean_pool(x, ok).shape == (2, 8)


# ---------------------------------------------------------------------------
# BERT servable output mode
# ---------------------------------------------------------------------------

class StubEncoder(torch.nn.Module):
    """Stands in for the encoder: a fixed integer-valued hidden state."""

    def __init__(self, hidden):
        super().__init__()
        self.hidden = hidden
        self.seen_mask = "unset"

    def forward(self, input_ids, attention_mask=None):
        self.seen_mask = attention_mask
        B, S = input_ids.shape
        assert (B, S) == tuple(self.hidden.shape[:2])
        return self.hidden, torch.zeros(B, 768)


@pytest.fixture(scope="module")
def embedding_servable():
    return bert_servable(output_format="sentence_embedding")


SIG_INPUTS = {"input_ids": (3, [-1, -1]), "attention_mask": (3, [-1, -1])}


def test_sentence_embedding_signature(embedding_servable):
    sig = embedding_servable.signature
    assert sig["outputs"] == {"sentence_embedding": (1, [-1, 768])}
    assert sig["inputs"] == SIG_INPUTS
    assert sig["method_name"] == "tensorflow/serving/predict"


@pytest.mark.parametrize("normalize", [False, True])
def test_sentence_embedding_with_stub_module(normalize):
    s = bert_servable(output_format="sentence_embedding",
                      normalize_embedding=normalize)
    hidden = int_hidden((4, 16, 768), torch.float32, seed=7)
    s.module = StubEncoder(hidden)
    ids = torch.zeros(4, 16, dtype=torch.int32)
    mask = holey_mask(4, 16, seed=7)

    out = s({"input_ids": ids.numpy(), "attention_mask": mask.numpy()})
    assert set(out) == {"sentence_embedding"}
    emb = out["sentence_embedding"]
    assert emb.dtype == torch.float32 and tuple(emb.shape) == (4, 768)
    assert torch.equal(s.module.seen_mask, mask)
    assert torch.equal(emb, check(hidden, mask, normalize))

    out = s({"input_ids": ids.numpy()})             # no attention_mask
    assert set(out) == {"sentence_embedding"}
    assert s.module.seen_mask is None
    assert torch.equal(out["sentence_embedding"],
                       check(hidden, None, normalize))


def test_sentence_embedding_is_normalized_by_default(embedding_servable):
    hidden = int_hidden((2, 6, 768), torch.float32, seed=8)
    real = embedding_servable.module
    embedding_servable.module = StubEncoder(hidden)
    try:
        out = embedding_servable(
            {"input_ids": torch.zeros(2, 6, dtype=torch.int32)})
    finally:
        embedding_servable.module = real
    norms = out["sentence_embedding"].double().norm(dim=1)
    assert bool(((norms - 1).abs() <= (768 / 2 + 8) * U).all())


def test_bad_output_format_raises():
    with pytest.raises(ValueError, match="output_format"):
        bert_servable(output_format="cls")


def test_default_mode_signature_and_outputs_unchanged():
    s = bert_servable()
    assert s.signature == {
        "method_name": "tensorflow/serving/predict",
        "inputs": SIG_INPUTS,
        "outputs": {"last_hidden_state": (1, [-1, -1, 768]),
                    "pooled_output": (1, [-1, 768])},
    }
    hidden = int_hidden((2, 4, 768), torch.float32, seed=9)
    s.module = StubEncoder(hidden)
    out = s({"input_ids": torch.zeros(2, 4, dtype=torch.int32)})
    assert set(out) == {"last_hidden_state", "pooled_output"}
    assert torch.equal(out["last_hidden_state"], hidden)


# ---------------------------------------------------------------------------
# model.json I/O-mode keys
# ---------------------------------------------------------------------------

def _version_dir(tmp_path, cfg):
    vdir = tmp_path / "m" / "1"
    vdir.mkdir(parents=True)
    (vdir / "model.json").write_text(json.dumps(cfg))
    return str(vdir)


def test_loader_passes_bert_output_format(tmp_path):
    s = default_loader("m", _version_dir(
        tmp_path, {"family": "bert_base",
                   "output_format": "sentence_embedding",
                   "normalize_embedding": False}))
    assert s.signature["outputs"] == {"sentence_embedding": (1, [-1, 768])}


def test_loader_passes_resnet_input_format(tmp_path):
    s = default_loader("m", _version_dir(
        tmp_path, {"family": "resnet50", "input_format": "uint8_nhwc"}))
    assert s.signature["inputs"] == {"images": (4, [-1, 224, 224, 3])}
    assert "images" in s.preprocess


def test_loader_without_mode_keys_is_unchanged(tmp_path):
    s = default_loader("m", _version_dir(tmp_path, {"family": "resnet50"}))
    assert s.signature["inputs"] == {"images": (1, [-1, 3, 224, 224])}
    assert not s.preprocess


def test_loader_unknown_mode_value_raises(tmp_path):
    with pytest.raises(ValueError, match="output_format"):
        default_loader("m", _version_dir(
            tmp_path, {"family": "bert_base", "output_format": "cls"}))
