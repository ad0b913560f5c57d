"""The packed (varlen) form of ``ops.masked_self_attention`` on the GPU against
an fp64 CPU reference from ``qkv`` as stored, its exact properties and
validation, ``ops.bert_embed_ragged(packed=True)``, then the
``attention="packed"`` servable through the raw server.

Tolerance, per output element, derived in test_gpu_attention.py and not
tuned: ``2^-8 * max_{j<L} |v[j,d]|`` for bf16 (``2^-11`` for f16: P is rounded
once to the operand dtype, the factor 2 covers fp32 ``exp`` and the summation
order) plus half a unit in the last place of the output dtype at the
reference value. One admitted key of a neighbour would miss it by 17x or more.

The packed ``qkv`` is a row slice of a buffer with 64 NaN rows before and
after it: a load outside every sequence breaks the bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from min_tfs_client_amd import ops  # noqa: E402
from min_tfs_client_amd.models import bert_servable  # noqa: E402
from min_tfs_client_amd.models.bert import BertConfig  # noqa: E402
from min_tfs_client_amd.preprocess import pack_ragged_tokens  # noqa: E402
from min_tfs_client_amd.server import ModelServer  # noqa: E402
from min_tfs_client_amd.turbo import TurboPredictClient  # noqa: E402

DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
SIGNIFICAND_BITS = {"bf16": 8, "f16": 11}

# (heads, lengths)
CASES = [
    (1, [1]),
    (2, [17, 1, 5]),
    (2, [70, 33, 64, 2]),
    (2, [130, 65, 129]),
    (1, [63, 47]),
    (1, [64, 16]),
    (1, [65, 15, 64]),
    (12, [40, 40]),
    (2, ([3, 1, 2] * 13334)[:40000]),     # 80 000 workgroups
]


def build(heads, lengths, dtype, seed=0):
    """Seeded randn packed qkv (T,3H) on the device, framed by NaN rows."""
    g = torch.Generator().manual_seed(seed)
    T = sum(lengths)
    framed = torch.full((T + 128, 3 * heads * 64), float("nan"),
                        dtype=DTYPES[dtype])
    framed[64:64 + T] = torch.randn(T, 3 * heads * 64, generator=g).to(
        DTYPES[dtype])
    return framed.to(DEV)[64:64 + T]


def keep_of(lengths):
    lens = torch.tensor(lengths)
    return torch.arange(int(lens.max()))[None, :] < lens[:, None]


def padded(packed, lengths):
    """(B,S,C) zeros with the packed rows at the kept positions."""
    keep = keep_of(lengths).to(packed.device)
    out = packed.new_zeros(keep.shape + packed.shape[1:])
    out[keep] = packed
    return out


def reference64(qkv, lengths, heads):
    """fp64 attention of a packed CPU qkv, packed; max_{j<L} |v[j,d]| per
    packed row."""
    keep = keep_of(lengths)
    B, S = keep.shape
    q, k, v = (t.transpose(1, 2) for t in padded(
        qkv.double(), lengths).view(B, S, 3, heads, 64).unbind(2))
    scores = (q @ k.transpose(2, 3)) / 8.0
    scores = scores.masked_fill(~keep[:, None, None, :], float("-inf"))
    ref = (torch.softmax(scores, -1) @ v).transpose(1, 2).reshape(B, S, -1)
    vmax = v.abs().amax(2).reshape(B, 1, -1).expand(B, S, -1)
    return ref[keep], vmax[keep]


def run(qkv, lengths, heads):
    return ops.masked_self_attention(
        qkv, None, heads, tiles=ops.attention_tiles(lengths, DEV))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", CASES,
                         ids=lambda c: f"{c[0]}-{c[1][:4]}-{len(c[1])}")
def test_matches_fp64_reference(case, dtype):
    heads, lengths = case
    qkv = build(heads, lengths, dtype)
    out = run(qkv, lengths, heads).cpu()
    assert tuple(out.shape) == (sum(lengths), heads * 64)
    assert bool(torch.isfinite(out).all())
    ref, vmax = reference64(qkv.cpu(), lengths, heads)
    exponent = torch.frexp(ref)[1]                # |ref| in [0.5, 1) * 2^e
    tol = 2.0 ** -SIGNIFICAND_BITS[dtype] * vmax + torch.ldexp(
        torch.ones_like(ref), exponent - 1 - SIGNIFICAND_BITS[dtype])
    err = (out.double() - ref).abs()
    print(f"heads={heads} lengths={lengths[:4]}x{len(lengths)} dtype={dtype} "
          f"max_err/tol={float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_exact_properties(dtype):
    heads, lengths = 2, [70, 33, 64, 2]
    qkv = build(heads, lengths, dtype, seed=1)
    out = run(qkv, lengths, heads)
    # the padded kernel on the same sequences, two runs, reversed neighbours
    lens = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    dense = ops.masked_self_attention(padded(qkv, lengths), lens, heads)
    assert torch.equal(out, dense[keep_of(lengths).to(DEV)])
    assert torch.equal(out, run(qkv, lengths, heads))
    parts = list(qkv.split(lengths))[::-1]
    rev = run(torch.cat(parts), lengths[::-1], heads)
    assert torch.equal(torch.cat(list(rev.split(lengths[::-1]))[::-1]), out)
    # the clamps: row0 past T, a negative q0 (tile 0), L past the end
    # (sequence 3 is the last 2 rows), q0 >= L and the int32 extremes
    top, low = (1 << 31) - 1, -(1 << 31)
    wild = torch.tensor(
        [[170, 10, 0, 9], [0, 70, -64, 0], [0, 70, 64, 0], [167, 1000, 0, 3],
         [70, 33, 64, 1], [top, top, top, 0], [low, low, low, 0]],
        dtype=torch.int32, device=DEV)
    got = ops.masked_self_attention(qkv, None, heads, tiles=wild)
    assert torch.equal(got[:70], out[:70])
    assert torch.equal(got[167:], out[167:])
    empty = ops.masked_self_attention(qkv[:0], None, heads,
                                      tiles=ops.attention_tiles([], DEV))
    assert tuple(empty.shape) == (0, 128)


@pytest.mark.parametrize("edit,message", [
    (lambda a: a.update(tiles=None), "needs tiles"),
    (lambda a: a.update(lens=torch.tensor([5, 1, 2], dtype=torch.int32,
                                          device=DEV)),
     "tiles and lengths exclude"),
    (lambda a: a.update(tiles=a["tiles"].long()), "int32"),
    (lambda a: a.update(tiles=a["tiles"][:, :3]), r"shape \[n,4\]"),
    (lambda a: a.update(tiles=a["tiles"].cpu()), "tiles is on cpu"),
])
def test_argument_errors(edit, message):
    a = dict(qkv=build(2, [5, 1, 2], "bf16"), lens=None,
             tiles=ops.attention_tiles([5, 1, 2], DEV))
    edit(a)
    with pytest.raises(ValueError, match=message):
        ops.masked_self_attention(a["qkv"], a["lens"], 2, tiles=a["tiles"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("lengths", [[1, 7, 3], [16]])
def test_bert_embed_ragged_packed(lengths, dtype):
    g = torch.Generator().manual_seed(0)
    tok, pos, typ = (torch.randn(n, 64, generator=g).to(dtype).to(DEV)
                     for n in (50, 16, 2))           # max_pos = 16
    gamma, beta = (torch.randn(64, generator=g).to(dtype).to(DEV)
                   for _ in range(2))
    ids = torch.randint(0, 50, (sum(lengths),), generator=g,
                        dtype=torch.int32).to(DEV)
    args = (lengths, tok, pos, typ, gamma, beta, 1e-12)
    hidden, mask = ops.bert_embed_ragged(ids, *args)
    packed = ops.bert_embed_ragged(ids, *args, packed=True)
    assert torch.equal(packed, hidden[mask[:, 0, 0, :] == 0])
    ids[-1] = 50
    where = f"sequence {len(lengths) - 1}, position {lengths[-1] - 1}"
    with pytest.raises(ValueError, match=where):
        ops.bert_embed_ragged(ids, *args, packed=True)


class OneLayer(BertConfig):
    vocab_size, hidden, layers, heads = 50, 128, 1, 2
    intermediate, max_pos, type_vocab = 256, 40, 2


E2E_IDS = [[49, 3, 17, 0, 8, 21, 5], [4, 9], [30, 1, 1, 12]]


@pytest.mark.parametrize("output_format", ["hidden", "sentence_embedding"])
def test_packed_attention_through_the_raw_server(sock_dir, output_format):
    """Margin: the default mode's own bf16-against-f32 difference; two bf16
    models may be 2x that apart (as in test_gpu_attention.py)."""
    flat, lengths = pack_ragged_tokens(E2E_IDS)
    req = {"input_ids": torch.from_numpy(flat).to(DEV),
           "sequence_lengths": torch.from_numpy(lengths)}
    keep = keep_of(list(lengths)).to(DEV)
    address = f"unix://{sock_dir}/packed.sock"
    with ModelServer(address=address, raw_predict=True, device=DEV) as srv:
        for name, dtype, attention in (("f32", torch.float32, "sdpa"),
                                       ("bf16", torch.bfloat16, "sdpa"),
                                       ("packed", torch.bfloat16, "packed")):
            srv.manager.load(name, bert_servable(
                DEV, dtype, input_format="ids_ragged", config=OneLayer(),
                output_format=output_format, attention=attention), version=1)
        with TurboPredictClient(address) as client:
            out = {name: client.predict(name, req, output_device=DEV)
                   for name in ("f32", "bf16", "packed")}
    for key in out["f32"]:
        f32, bf16, packed = (out[n][key] for n in ("f32", "bf16", "packed"))
        assert packed.shape == bf16.shape
        if key == "last_hidden_state":
            pad = packed[~keep]
            assert bool((pad == 0).all()) and not bool(torch.signbit(pad).any())
            f32, bf16, packed = f32[keep], bf16[keep], packed[keep]
        margin = float((bf16 - f32).abs().max())
        diff = float((packed - bf16).abs().max())
        print(f"{key}: margin={margin:.3e} packed_vs_bf16={diff:.3e}")
        assert diff <= 2 * margin
