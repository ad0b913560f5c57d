"""``ops.masked_self_attention`` on the GPU against an fp64 CPU reference from
``qkv`` as stored (per (b, head): softmax over the first L keys), its exact
properties, validation, then end to end through the raw server.

Tolerance, per output element, derived and not tuned: ``2^-8 * max_{j<L}
|v[j,d]|`` for bf16 (``2^-11`` for f16) plus half a unit in the last place of
the output dtype at the reference value. P is rounded once to the operand
dtype, so ``|sum p~_j v_j / sum p_j - ref| <= 2^-9 max|v|`` (``2^-12``); the
factor 2 covers fp32 ``exp`` and the summation order, both at least 2^10 times
smaller. One admitted padded key would miss it by 17x or more.

The kernel has one tile size, 64, for query rows and keys alike, and a wave
owns 16 rows: S = 63, 64 and 65 and lengths 15, 16, 17, 47 are the edges."""
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

# (heads, B, S, lengths)
CASES = [
    (1, 1, 1, [1]),
    (2, 3, 17, [17, 1, 5]),
    (2, 4, 70, [70, 33, 64, 2]),
    (2, 3, 130, [130, 65, 129]),
    (12, 2, 40, None),
    (2, 40000, 3, ([3, 1, 2] * 13334)[:40000]),   # > 65535 (b, head) pairs
    (1, 2, 63, [63, 47]),
    (1, 2, 64, [64, 16]),
    (1, 3, 65, [65, 15, 64]),
]


def build(heads, B, S, lengths, dtype, seed=0):
    """Seeded randn qkv, NaN at every position at or past its length."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, S, 3 * heads * 64, generator=g).to(DTYPES[dtype])
    lens = None
    if lengths is not None:
        lens = torch.tensor(lengths, dtype=torch.int32)
        qkv[torch.arange(S)[None, :] >= lens[:, None]] = float("nan")
    return qkv, lens


def reference64(qkv, lens, heads):
    """(fp64 attention, zeros at rows >= L; max_{j<L} |v[j,d]|; kept rows)"""
    B, S, H3 = qkv.shape
    q, k, v = (t.transpose(1, 2) for t in
               qkv.double().view(B, S, 3, heads, 64).unbind(2))
    n = torch.full((B,), S) if lens is None else lens.clamp(0, S)
    keep = torch.arange(S)[None, :] < n[:, None]
    rows, cols = keep[:, None, :, None], keep[:, None, None, :]
    zero = torch.zeros((), dtype=torch.float64)
    q, k, v = (torch.where(rows, t, zero) for t in (q, k, v))
    scores = (q @ k.transpose(2, 3)) / 8.0
    scores = scores.masked_fill(~cols, float("-inf"))
    p = torch.where(rows & cols, torch.softmax(scores, -1), zero)
    ref = (p @ v).transpose(1, 2).reshape(B, S, H3 // 3)
    return ref, v.abs().amax(2).reshape(B, 1, H3 // 3), keep


def half_ulp(ref, dtype):
    exponent = torch.frexp(ref)[1]                # |ref| in [0.5, 1) * 2^e
    return torch.ldexp(torch.ones_like(ref),
                       exponent - 1 - SIGNIFICAND_BITS[dtype])


def run(qkv, lens, heads):
    return ops.masked_self_attention(
        qkv.to(DEV), None if lens is None else lens.to(DEV), heads)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", CASES, ids=lambda c: str(c[:3]))
def test_matches_fp64_reference(case, dtype):
    qkv, lens = build(*case, dtype)
    out = run(qkv, lens, case[0]).cpu()
    ref, vmax, keep = reference64(qkv, lens, case[0])
    tol = 2.0 ** -SIGNIFICAND_BITS[dtype] * vmax + half_ulp(ref, dtype)
    err = (out.double() - ref).abs()
    ratio = float((err / tol)[keep].max())
    print(f"case={case[:3]} dtype={dtype} max_err/tol={ratio:.3f}")
    assert bool((err[keep] <= tol[keep]).all())
    padded = out[~keep]
    assert bool((padded == 0).all()) and not bool(torch.signbit(padded).any())


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_exact_properties(dtype):
    heads, (qkv, lens) = 2, build(2, 4, 70, [70, 33, 64, 2], dtype, seed=1)
    out = run(qkv, lens, heads)
    assert torch.equal(out, run(qkv, lens, heads))
    rows = torch.cat([run(qkv[b:b + 1], lens[b:b + 1], heads)
                      for b in range(4)])
    assert torch.equal(out, rows)
    # lengths outside 0..S are clamped on the device
    clean = torch.nan_to_num(qkv)
    wild = run(clean, torch.tensor([71, 1 << 30, -1, -(1 << 31)],
                                   dtype=torch.int32), heads)
    full = run(clean, None, heads)
    assert torch.equal(wild[:2], full[:2])
    assert bool((wild[2:] == 0).all())
    assert tuple(run(qkv[:0], lens[:0], heads).shape) == (0, 70, 128)


@pytest.mark.parametrize("edit,message", [
    (lambda a: a.update(qkv=a["qkv"].float()), "bfloat16 or float16"),
    (lambda a: a.update(qkv=a["qkv"].transpose(0, 1)), "contiguous"),
    (lambda a: a.update(heads=4), "head_dim must be 64, got 32"),
    (lambda a: a.update(lens=a["lens"].long()), "int32"),
    (lambda a: a.update(lens=a["lens"][:2]), "shape"),
    (lambda a: a.update(lens=a["lens"].cpu()), "lengths is on cpu"),
])
def test_argument_errors(edit, message):
    qkv, lens = build(2, 3, 5, [5, 1, 2], "bf16")
    a = dict(qkv=qkv.to(DEV), lens=lens.to(DEV), heads=2)
    edit(a)
    with pytest.raises(ValueError, match=message):
        ops.masked_self_attention(a["qkv"], a["lens"], a["heads"])


class OneLayer(BertConfig):
    vocab_size, hidden, layers, heads = 50, 128, 1, 2
    intermediate, max_pos, type_vocab = 256, 40, 2


E2E_IDS = [[49, 3, 17, 0, 8, 21, 5], [4, 9], [30, 1, 1, 12]]


@pytest.mark.parametrize("output_format", ["hidden", "sentence_embedding"])
def test_fused_attention_through_the_raw_server(sock_dir, output_format):
    """Margin: the default mode's own bf16-against-f32 difference; two bf16
    models may be 2x that apart (as in test_fused_mode_matches_ids_mode)."""
    flat, lengths = pack_ragged_tokens(E2E_IDS)
    req = {"input_ids": torch.from_numpy(flat).to(DEV),
           "sequence_lengths": torch.from_numpy(lengths)}
    keep = (torch.arange(7)[None, :] < torch.tensor(lengths)[:, None]).to(DEV)
    with ModelServer(address=f"unix://{sock_dir}/attn.sock", raw_predict=True,
                     device=DEV) as srv:
        for name, dtype, attention in (("f32", torch.float32, "sdpa"),
                                       ("bf16", torch.bfloat16, "sdpa"),
                                       ("fused", torch.bfloat16, "fused")):
            srv.manager.load(name, bert_servable(
                DEV, dtype, input_format="ids_ragged", config=OneLayer(),
                output_format=output_format, attention=attention), version=1)
        with TurboPredictClient(f"unix://{sock_dir}/attn.sock") as client:
            out = {name: client.predict(name, req, output_device=DEV)
                   for name in ("f32", "bf16", "fused")}
    for key in out["f32"]:
        f32, bf16, fused = (out[name][key] for name in ("f32", "bf16", "fused"))
        assert bool(torch.isfinite(fused).all())           # padded rows too
        if key == "last_hidden_state":
            assert not torch.equal(fused[~keep], bf16[~keep])
            f32, bf16, fused = f32[keep], bf16[keep], fused[keep]
        margin = float((bf16 - f32).abs().max())
        diff = float((fused - bf16).abs().max())
        print(f"{key}: margin={margin:.3e} fused_vs_bf16={diff:.3e}")
        assert diff <= 2 * margin
    for kw in (dict(input_format="ids", dtype=torch.bfloat16),
               dict(input_format="ids_ragged", dtype=torch.float32)):
        with pytest.raises(ValueError, match="attention='fused' needs"):
            bert_servable(DEV, config=OneLayer(), attention="fused", **kw)
