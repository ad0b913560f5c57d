"""The packed (varlen) BERT path on the CPU: the eager packed form of
``ops.masked_self_attention`` against its per-sequence contract (exact) and
an fp64 reference, ``ops.attention_tiles``, argument validation,
``ops.bert_embed_ragged(packed=True)`` and the ``attention="packed"``
servable (the kernels: tests/gpu/test_gpu_attention_packed.py).

Bound, as in test_attention.py: ``2^-8 max_{j<L} |v[j,d]|`` (bf16; ``2^-11``
f16) plus half an output ulp."""
import json

import pytest
import torch

from min_tfs_client_amd import ops
from min_tfs_client_amd.models import bert_servable
from min_tfs_client_amd.models.bert import BertConfig
from min_tfs_client_amd.preprocess import pack_ragged_tokens
from min_tfs_client_amd.repository import default_loader

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
SIGNIFICAND_BITS = {"bf16": 8, "f16": 11}


def build(lengths, dtype, heads=2):
    g = torch.Generator().manual_seed(0)
    return torch.randn(sum(lengths), 3 * heads * 64, generator=g).to(
        DTYPES[dtype])


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("lengths", [[17, 1, 5], [70, 33, 64, 2]])
def test_eager_packed_path(lengths, dtype):
    heads, qkv = 2, build(lengths, dtype)
    out = ops.masked_self_attention(qkv, None, heads,
                                    tiles=ops.attention_tiles(lengths))
    assert tuple(out.shape) == (sum(lengths), 128)
    row0 = 0
    for n in lengths:
        seq = qkv[row0:row0 + n]
        assert torch.equal(out[row0:row0 + n], ops.masked_self_attention(
            seq[None], None, heads)[0])
        for h in range(heads):
            q, k, v = (seq.double().view(n, 3, heads, 64)[:, i, h]
                       for i in range(3))
            ref = torch.softmax(q @ k.T / 8.0, -1) @ v
            tol = 2.0 ** -SIGNIFICAND_BITS[dtype] * v.abs().amax(0) \
                + torch.ldexp(torch.ones_like(ref), torch.frexp(ref)[1] - 1
                              - SIGNIFICAND_BITS[dtype])
            got = out[row0:row0 + n, h * 64:(h + 1) * 64].double()
            assert bool(((got - ref).abs() <= tol).all())
        row0 += n


def test_attention_tiles():
    lengths = [70, 33, 64, 2]
    table = ops.attention_tiles(lengths)
    assert table.dtype == torch.int32
    assert sorted(map(tuple, table.tolist())) == [
        (0, 70, 0, 0), (0, 70, 64, 0), (70, 33, 0, 1), (103, 64, 0, 2),
        (167, 2, 0, 3)]
    big = [130, 1, 64, 65, 512]
    table = ops.attention_tiles(torch.tensor(big))
    assert table.shape[0] == sum((n + 63) // 64 for n in big)
    covered = torch.zeros(sum(big), dtype=torch.int64)
    for row0, n, q0, _ in table.tolist():
        covered[row0 + q0:row0 + min(q0 + 64, n)] += 1
    assert bool((covered == 1).all())
    assert tuple(ops.attention_tiles([]).shape) == (0, 4)
    with pytest.raises(ValueError, match="sequence 1: length must be at"):
        ops.attention_tiles([3, 0])


@pytest.mark.parametrize("edit,message", [
    (lambda a: a.update(tiles=None), "needs tiles"),
    (lambda a: a.update(lens=torch.tensor([5, 1, 2], dtype=torch.int32)),
     "tiles and lengths exclude"),
    (lambda a: a.update(tiles=a["tiles"].long()), "int32"),
    (lambda a: a.update(tiles=a["tiles"][:, :3]), r"shape \[n,4\]"),
    (lambda a: a.update(qkv=a["qkv"][None]), "tiles go with a rank-2"),
    (lambda a: a.update(qkv=a["qkv"][None, None]), "got rank 4"),
])
def test_argument_errors(edit, message):
    a = dict(qkv=build([5, 1, 2], "bf16"), lens=None,
             tiles=ops.attention_tiles([5, 1, 2]))
    edit(a)
    with pytest.raises(ValueError, match=message):
        ops.masked_self_attention(a["qkv"], a["lens"], 2, tiles=a["tiles"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bert_embed_ragged_packed(dtype):
    g = torch.Generator().manual_seed(0)
    tok, pos, typ = (torch.randn(n, 64, generator=g).to(dtype)
                     for n in (50, 16, 2))
    gamma, beta = (torch.randn(64, generator=g).to(dtype) for _ in range(2))
    lengths = [1, 7, 3]
    ids = torch.randint(0, 50, (11,), generator=g, dtype=torch.int32)
    args = (lengths, tok, pos, typ, gamma, beta, 1e-12)
    hidden, mask = ops.bert_embed_ragged(ids, *args)
    packed = ops.bert_embed_ragged(ids, *args, packed=True)
    assert torch.equal(packed, hidden[mask[:, 0, 0, :] == 0])
    ids[3] = 50
    with pytest.raises(ValueError, match="sequence 1, position 2"):
        ops.bert_embed_ragged(ids, *args, packed=True)


class OneLayer(BertConfig):
    vocab_size, hidden, layers, heads = 50, 128, 1, 2
    intermediate, max_pos, type_vocab = 256, 40, 2


@pytest.mark.parametrize("kw,message", [
    (dict(attention="packed", input_format="ids_ragged"),
     "attention='packed' needs dtype"),
    (dict(attention="packed", input_format="ids", dtype=torch.bfloat16),
     "attention='packed' needs input_format"),
    (dict(attention="flash"), "attention must be 'sdpa' or 'fused'"),
])
def test_servable_rejections(kw, message):
    with pytest.raises(ValueError, match=message):
        bert_servable("cpu", config=OneLayer(), **kw)


def test_model_json_selects_packed_attention(tmp_path, monkeypatch):
    """model.json builds BertConfig itself: shrink that to one layer."""
    for key in ("vocab_size", "hidden", "layers", "heads", "intermediate",
                "max_pos"):
        monkeypatch.setattr(BertConfig, key, getattr(OneLayer, key))
    models = []
    for name, keys in (("a", dict(dtype="bfloat16", attention="packed")),
                       ("b", dict(dtype="bfloat16", attention="sdpa")),
                       ("c", dict(dtype="float32"))):
        vdir = tmp_path / name / "1"
        vdir.mkdir(parents=True)
        (vdir / "model.json").write_text(json.dumps(dict(
            family="bert_base", input_format="ids_ragged", **keys)))
        models.append(default_loader("m", str(vdir)))
    flat, lengths = pack_ragged_tokens([[49, 3, 17, 0, 8], [4, 9], [30]])
    req = {"input_ids": flat, "sequence_lengths": lengths}
    got, want, f32 = (m(req) for m in models)
    keep = torch.arange(5)[None, :] < torch.tensor(lengths)[:, None]
    assert tuple(got["last_hidden_state"].shape) == (3, 5, 128)
    padded = got["last_hidden_state"][~keep]
    assert bool((padded == 0).all()) and not bool(torch.signbit(padded).any())
    # both bf16 models are within the default mode's bf16-against-f32
    # difference of the f32 model, so within 2x that of each other
    for key in ("last_hidden_state", "pooled_output"):
        a, b, c = (o[key][keep] if key == "last_hidden_state" else o[key]
                   for o in (got, want, f32))
        assert float((a - b).abs().max()) <= 2 * float((b - c).abs().max())
