"""Length-masked self-attention on the CPU: the eager path of
``ops.masked_self_attention`` against an fp64 reference, argument validation,
and the ``attention`` / ``dtype`` options of the BERT servable and of
``model.json`` (the kernel: tests/gpu/test_gpu_attention.py).

The eager path computes in fp32 and rounds once, so it must meet the kernel's
bound: ``2^-8 max_{j<L} |v[j,d]|`` (bf16; ``2^-11`` f16) plus half an output
ulp."""
import json

import pytest
import torch

from min_tfs_client_amd import ops
from min_tfs_client_amd.models.bert import BertConfig
from min_tfs_client_amd.preprocess import pack_ragged_tokens
from min_tfs_client_amd.repository import default_loader

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
SIGNIFICAND_BITS = {"bf16": 8, "f16": 11}


def build(heads, B, S, lengths, dtype):
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B, S, 3 * heads * 64, generator=g).to(DTYPES[dtype])
    lens = torch.tensor(lengths, dtype=torch.int32)
    qkv[torch.arange(S)[None, :] >= lens[:, None]] = float("nan")
    return qkv, lens


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("heads,B,S,lengths", [
    (2, 3, 17, [17, 1, 5]), (2, 4, 70, [70, 33, 64, 2])])
def test_eager_path_matches_reference(heads, B, S, lengths, dtype):
    qkv, lens = build(heads, B, S, lengths, dtype)
    out = ops.masked_self_attention(qkv, lens, heads)
    x = qkv.double().view(B, S, 3, heads, 64)
    for b, n in enumerate(lengths):
        for h in range(heads):
            q, k, v = (x[b, :n, i, h] for i in range(3))
            ref = torch.softmax(q @ k.T / 8.0, -1) @ v
            tol = 2.0 ** -SIGNIFICAND_BITS[dtype] * v.abs().amax(0) \
                + torch.ldexp(torch.ones_like(ref), torch.frexp(ref)[1] - 1
                              - SIGNIFICAND_BITS[dtype])
            got = out[b, :n, h * 64:(h + 1) * 64].double()
            assert bool(((got - ref).abs() <= tol).all())
        assert bool((out[b, n:] == 0).all() & ~torch.signbit(out[b, n:]).any())


@pytest.mark.parametrize("edit,message", [
    (lambda a: a.update(qkv=a["qkv"].float()), "bfloat16 or float16"),
    (lambda a: a.update(qkv=a["qkv"].transpose(0, 1)), "contiguous"),
    (lambda a: a.update(heads=4), "head_dim must be 64, got 32"),
    (lambda a: a.update(heads=2.0), "heads must be an integer"),
    (lambda a: a.update(lens=a["lens"].long()), "int32"),
    (lambda a: a.update(lens=a["lens"][:2]), "shape"),
    (lambda a: a.update(scale=float("nan")), "scale must be finite"),
])
def test_argument_errors(edit, message):
    qkv, lens = build(2, 3, 5, [5, 1, 2], "bf16")
    a = dict(qkv=qkv, lens=lens, heads=2, scale=None)
    edit(a)
    with pytest.raises(ValueError, match=message):
        ops.masked_self_attention(a["qkv"], a["lens"], a["heads"], a["scale"])


class OneLayer(BertConfig):
    vocab_size, hidden, layers, heads = 50, 128, 1, 2
    intermediate, max_pos, type_vocab = 256, 40, 2


def write_model_json(tmp_path, **keys):
    vdir = tmp_path / "1"
    vdir.mkdir(parents=True)
    (vdir / "model.json").write_text(json.dumps(
        dict(family="bert_base", **keys)))
    return str(vdir)


def test_model_json_selects_fused_attention(tmp_path, monkeypatch):
    """model.json builds BertConfig itself: shrink that to one layer."""
    for key in ("vocab_size", "hidden", "layers", "heads", "intermediate",
                "max_pos"):
        monkeypatch.setattr(BertConfig, key, getattr(OneLayer, key))
    fused, plain, exact = (
        default_loader("m", write_model_json(
            tmp_path / name, input_format="ids_ragged", **keys))
        for name, keys in (("a", dict(dtype="bfloat16", attention="fused")),
                           ("b", dict(dtype="bfloat16", attention="sdpa")),
                           ("c", dict(dtype="float32"))))
    assert fused.module.pooler.weight.dtype == torch.bfloat16
    flat, lengths = pack_ragged_tokens([[49, 3, 17, 0, 8], [4, 9], [30]])
    req = {"input_ids": flat, "sequence_lengths": lengths}
    got, want, f32 = fused(req), plain(req), exact(req)
    keep = torch.arange(5)[None, :] < torch.tensor(lengths)[:, None]
    assert tuple(got["last_hidden_state"].shape) == (3, 5, 128)
    assert bool(torch.isfinite(got["last_hidden_state"]).all())
    # both bf16 models are within the default mode's bf16-against-f32
    # difference of the f32 model, so within 2x that of each other
    for key in ("last_hidden_state", "pooled_output"):
        a, b, c = (o[key][keep] if key == "last_hidden_state" else o[key]
                   for o in (got, want, f32))
        assert float((a - b).abs().max()) <= 2 * float((b - c).abs().max())
    assert not torch.equal(got["last_hidden_state"][~keep],
                           want["last_hidden_state"][~keep])


@pytest.mark.parametrize("keys,message", [
    (dict(dtype="int8"), "dtype must be one of"),
    (dict(attention="flash"), "attention must be 'sdpa' or 'fused'"),
    (dict(attention="fused", input_format="ids_ragged"),
     "needs dtype bfloat16 or float16"),
    (dict(attention="fused", dtype="float16"),
     "needs input_format='ids_ragged'"),
    (dict(attention="fused", dtype="bfloat16", input_format="ids_fused"),
     "needs input_format='ids_ragged'"),
])
def test_servable_and_model_json_validation(tmp_path, keys, message):
    with pytest.raises(ValueError, match=message):
        default_loader("m", write_model_json(tmp_path, **keys))
