"""BERT embedding ingest on the CPU: the eager path of ``ops.bert_embed`` /
``ops.bert_embed_ragged`` against an fp64 reference, argument validation, the
``BertEncoder`` split, ``pack_ragged_tokens``, the ``model.json`` pass-through
and the fused servable modes (the kernel: tests/gpu/test_gpu_bert_embed.py).

Tolerance of the eager path: an fp32 sum of H terms in any order errs by at
most H * 2^-24 of the sum of magnitudes, which the mean, the variance and the
normalization each pass on once, so |out - ref| <= (H/2 + 16) * 2^-24 *
max|ref| per case, plus half a unit in the last place of a 16-bit output."""
import json

import numpy as np
import pytest
import torch

from min_tfs_client_amd import ops
from min_tfs_client_amd.models import bert_servable
from min_tfs_client_amd.models.bert import BertConfig, BertEncoder
from min_tfs_client_amd.preprocess import pack_ragged_tokens
from min_tfs_client_amd.repository import default_loader
from min_tfs_client_amd.server import validate_inputs_against_signature

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16,
          "f16": torch.float16}
SIGNIFICAND_BITS = {"bf16": 8, "f16": 11}
VOCAB, MAX_POS, TYPE_VOCAB, EPS = 50, 40, 2, 1e-12


def build(H, dtype, B, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    tables = [torch.randn(n, H, generator=g).to(DTYPES[dtype])
              for n in (VOCAB, MAX_POS, TYPE_VOCAB)]
    tables.append((1 + 0.1 * torch.randn(H, generator=g)).to(DTYPES[dtype]))
    tables.append((0.1 * torch.randn(H, generator=g)).to(DTYPES[dtype]))
    ids = torch.randint(0, VOCAB, (B, S), generator=g).to(torch.int32)
    types = torch.randint(0, TYPE_VOCAB, (B, S), generator=g).to(torch.int32)
    mask = torch.randint(0, 2, (B, S), generator=g).to(torch.int32) * 7
    return tables, ids, types, mask


def reference64(tables, ids, types):
    tok, pos, typ, gamma, beta = (t.double() for t in tables)
    x = tok[ids.long()] + pos[:ids.shape[1]] + typ[types.long()]
    d = x - x.mean(-1, keepdim=True)
    var = (d * d).mean(-1, keepdim=True)
    return d / torch.sqrt(var + EPS) * gamma + beta


@pytest.mark.parametrize("out", list(DTYPES))
@pytest.mark.parametrize("H,dtype,B,S", [(8, "f32", 1, 1), (520, "f16", 2, 7),
                                         (768, "bf16", 2, MAX_POS)])
def test_eager_path_matches_reference(H, dtype, B, S, out):
    tables, ids, types, mask = build(H, dtype, B, S)
    hidden, add_mask = ops.bert_embed(ids, *tables, EPS, mask, types,
                                      DTYPES[out])
    ref = reference64(tables, ids, types)
    bound = (H / 2 + 16) * 2.0 ** -24 * ref.abs().max()
    if out != "f32":                  # half an ulp: |ref| in [0.5, 1) * 2^e
        bound = bound + torch.ldexp(
            torch.ones_like(ref),
            torch.frexp(ref)[1] - 1 - SIGNIFICAND_BITS[out])
    assert bool(((hidden.double() - ref).abs() <= bound).all())
    low = torch.finfo(DTYPES[out]).min
    assert torch.equal(add_mask[:, 0, 0, :],
                       torch.where(mask != 0, 0.0, low).to(DTYPES[out]))
    empty = ops.bert_embed(ids[:0], *tables, EPS, mask[:0])
    assert (empty[0].shape, empty[1].shape) == ((0, S, H), (0, 1, 1, S))
    assert ops.bert_embed_ragged(ids[0, :0], [], *tables, EPS)[0].shape[0] == 0


def put(t, b, s, value):
    return t.index_put((torch.tensor(b), torch.tensor(s)),
                       torch.tensor(value, dtype=t.dtype))


@pytest.mark.parametrize("edit,message", [
    (lambda a: a.update(ids=a["ids"].repeat(1, 9), mask=None, types=None),
     "exceeds max_position"),
    (lambda a: a.update(ids=a["ids"][0]), "rank 2"),
    (lambda a: a.update(ids=put(a["ids"], 1, 2, VOCAB)),
     r"input_ids\[1,2\] = 50 is outside \[0, 50\)"),
    (lambda a: a.update(types=put(a["types"], 0, 4, -1)),
     r"token_type_ids\[0,4\] = -1 is outside \[0, 2\)"),
    (lambda a: a["t"].__setitem__(1, a["t"][1].half()), "share one dtype"),
    (lambda a: a.update(t=[t[..., :12].contiguous() for t in a["t"]]),
     "multiple of 8"),
])
def test_dense_argument_errors(edit, message):
    tables, ids, types, mask = build(16, "f32", 2, 5)
    a = dict(ids=ids, t=tables, mask=mask, types=types, out=None)
    edit(a)
    with pytest.raises(ValueError, match=message):
        ops.bert_embed(a["ids"], *a["t"], EPS, a["mask"], a["types"],
                       a["out"])


@pytest.mark.parametrize("lengths,kw,message", [
    ([3, MAX_POS + 1], {}, r"sequence 1: length must be in 1\.\.40.*41"),
    ([3, 8], {}, "sequence 1 ends past it"),
    ([3, 7], {"token_type_ids": torch.arange(10).int() // 6 * 2},
     r"token_type_ids of sequence 1, position 3 = 2 is outside \[0, 2\)"),
])
def test_ragged_argument_errors(lengths, kw, message):
    tables, ids, _, _ = build(16, "f32", 2, 5)
    with pytest.raises(ValueError, match=message):
        ops.bert_embed_ragged(ids.view(-1), lengths, *tables, EPS, **kw)


class OneLayer(BertConfig):
    vocab_size, hidden, layers, heads = VOCAB, 32, 1, 2
    intermediate, max_pos, type_vocab = 64, MAX_POS, TYPE_VOCAB


def test_forward_is_the_composition_of_its_parts():
    torch.manual_seed(0)
    model = BertEncoder(OneLayer()).eval()
    _, ids, types, _ = build(8, "f32", 3, 9)
    mask = (torch.arange(9)[None, :] < torch.tensor([[9], [4], [6]])).int()
    with torch.no_grad():
        x = model.embed(ids)
        parts = model.forward_embedded(x, model.additive_mask(mask, x.dtype))
        whole = model(ids, mask)
        assert all(torch.equal(w, p) for w, p in zip(whole, parts))
        assert not torch.equal(model.embed(ids, types), x)
    with pytest.raises(ValueError, match="exceeds max_position"):
        model.embed(ids.repeat(1, 5))


def test_pack_ragged_tokens_round_trip():
    seqs = [[5, 6, 7], [1], [9, 9]]
    ids, lengths = pack_ragged_tokens(seqs)
    assert [a.tolist() for a in np.split(ids, np.cumsum(lengths)[:-1])] == seqs
    assert pack_ragged_tokens([])[0].shape == (0,)


def test_loader_passes_bert_input_format(tmp_path):
    vdir = tmp_path / "1"
    vdir.mkdir()
    (vdir / "model.json").write_text(json.dumps(
        {"family": "bert_base", "input_format": "ids_ragged"}))
    s = default_loader("m", str(vdir))
    assert set(s.signature["inputs"]) == {"input_ids", "sequence_lengths",
                                          "token_type_ids"}


@pytest.mark.parametrize("output_format", ["hidden", "sentence_embedding"])
def test_fused_servable_modes_on_cpu(output_format):
    plain, fused, ragged = (
        bert_servable(config=OneLayer(), output_format=output_format,
                      input_format=mode)
        for mode in ("ids", "ids_fused", "ids_ragged"))
    seqs = [[49, 3, 17, 0, 8], [4, 9], [30, 1, 1]]
    flat, lengths = pack_ragged_tokens(seqs)
    mask = (torch.arange(5)[None, :] < torch.tensor(lengths)[:, None]).int()
    ids = torch.zeros(3, 5, dtype=torch.int32)
    ids[mask != 0] = torch.from_numpy(flat)
    req = {"input_ids": ids, "attention_mask": mask}
    want, got = plain(req), fused(req)
    packed = ragged({"input_ids": flat, "sequence_lengths": lengths})
    pair = fused(dict(req, token_type_ids=mask * (torch.arange(5) >= 2)))
    assert set(got) == set(want) == set(packed)
    for key in want:
        # fp32, one layer, O(1) activations: the two embeddings differ by a
        # few 2^-24 and the layer's two LayerNorms keep that at O(1e-6)
        assert torch.allclose(got[key], want[key], atol=1e-4)
        assert torch.equal(packed[key], got[key])
        assert not torch.equal(pair[key], got[key])
    # the optional input may be left out, a required one may not
    assert validate_inputs_against_signature(fused, req) is None
    assert validate_inputs_against_signature(
        fused, dict(req, token_type_ids=mask)) is None
    assert "Missing but required: {attention_mask}" in \
        validate_inputs_against_signature(fused, {"input_ids": ids})
    with pytest.raises(ValueError, match=r"input_ids\[1,0\] = 50"):
        fused(dict(req, input_ids=put(ids, 1, 0, 50)))
    with pytest.raises(ValueError, match="sequence 2 ends past it"):
        ragged({"input_ids": flat, "sequence_lengths": lengths + 1})
    with pytest.raises(ValueError, match="input_format"):
        bert_servable(input_format="tokens", config=OneLayer())
