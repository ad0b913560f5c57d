"""Fused BERT embedding ingest on the GPU: ``ops.bert_embed`` and
``ops.bert_embed_ragged`` against an fp64 CPU reference (table values as
stored, three rows summed, biased-variance LayerNorm and affine in fp64), their
exact properties, validation, then end to end through the raw server. Tables
are tiny throughout: vocab 50, max_pos 40, type_vocab 2.

Tolerance, f32 output: per case, 4x the measured maximum error of torch's CPU
fp32 eager expression (``F.embedding`` sums + ``F.layer_norm``) against the
same reference: two correct fp32 reduction orders over at most 768 terms
differ by a few units in the last place and no more. bf16 / f16 output: plus
half a unit in the last place of the output dtype at the reference value, the
one rounding at the store, computed exactly: 2^(e-8) for bf16 and 2^(e-11) for
f16 with 2^e <= |ref| < 2^(e+1). (2^-9 |ref| is below that wherever |ref| is
no power of two: the correctly rounded exact value would miss it.) Shapes:
the smallest that reach each path of the kernel header."""
import grpc
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from min_tfs_client_amd import ops  # noqa: E402
from min_tfs_client_amd.models import bert_servable  # noqa: E402
from min_tfs_client_amd.models.bert import BertConfig  # noqa: E402
from min_tfs_client_amd.preprocess import pack_ragged_tokens  # noqa: E402
from min_tfs_client_amd.server import ModelServer  # noqa: E402
from min_tfs_client_amd.turbo import TurboPredictClient  # noqa: E402

DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16,
          "f16": torch.float16}
SIGNIFICAND_BITS = {"bf16": 8, "f16": 11}
VOCAB, MAX_POS, TYPE_VOCAB, EPS = 50, 40, 2, 1e-12

# (H, table dtype, B, S)
CASES = [
    (8, "f32", 1, 1),       # one chunk, 63 idle lanes; B*S = 1
    (8, "bf16", 1, 5),      # B*S = 5: not a multiple of the waves per group
    (8, "f32", 205, 40),    # 8200 rows > 2048 groups x 4 waves; S = max_pos
    (520, "f16", 2, 7),     # 65 chunks: ragged tail in the chunk loop
    (768, "bf16", 2, 40),   # 96 chunks: 1.5 per lane
    (768, "f32", 2, 40),    # 192 chunks: 3 per lane
]


def build(H, dtype, B, S, seed=0):
    """Seeded CPU inputs: tables, ids that include 0 and VOCAB-1, types that
    include 1, a holey mask with values other than 0 and 1."""
    g = torch.Generator().manual_seed(seed)
    tables = [torch.randn(n, H, generator=g).to(DTYPES[dtype])
              for n in (VOCAB, MAX_POS, TYPE_VOCAB)]
    tables.append((1 + 0.1 * torch.randn(H, generator=g)).to(DTYPES[dtype]))
    tables.append((0.1 * torch.randn(H, generator=g)).to(DTYPES[dtype]))
    ids = torch.randint(0, VOCAB, (B, S), generator=g).to(torch.int32)
    ids.view(-1)[0] = VOCAB - 1
    ids.view(-1)[-1] = 0
    types = torch.randint(0, TYPE_VOCAB, (B, S), generator=g).to(torch.int32)
    types.view(-1)[0] = 1
    mask = torch.randint(0, 2, (B, S), generator=g).to(torch.int32) \
        * torch.tensor([1, -3, 1 << 30, 256, 2], dtype=torch.int32)[
            torch.arange(S) % 5]
    return tables, ids, types, mask


def half_ulp(ref, out):
    """Half a unit in the last place of dtype ``out`` at ``ref`` (0: f32)."""
    if out == "f32":
        return torch.zeros_like(ref)
    exponent = torch.frexp(ref)[1]                # |ref| in [0.5, 1) * 2^e
    return torch.ldexp(torch.ones_like(ref),
                       exponent - 1 - SIGNIFICAND_BITS[out])


def reference64(tables, ids, types):
    tok, pos, typ, gamma, beta = (t.double() for t in tables)
    x = tok[ids.long()] + pos[:ids.shape[1]] + typ[types.long()]
    d = x - x.mean(-1, keepdim=True)
    var = (d * d).mean(-1, keepdim=True)
    return d / torch.sqrt(var + EPS) * gamma + beta


def eager32_error(tables, ids, types, ref):
    """Max error of torch's CPU fp32 eager expression against ``ref``."""
    tok, pos, typ, gamma, beta = (t.float() for t in tables)
    x = F.embedding(ids.long(), tok) + pos[:ids.shape[1]] \
        + F.embedding(types.long(), typ)
    y = F.layer_norm(x, x.shape[-1:], gamma, beta, EPS)
    return float((y.double() - ref).abs().max())


def run(tables, ids, mask=None, types=None, out="f32"):
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    return ops.bert_embed(dev(ids), *(t.to(DEV) for t in tables), EPS,
                          attention_mask=dev(mask), token_type_ids=dev(types),
                          out_dtype=DTYPES[out])


@pytest.mark.parametrize("out", list(DTYPES))
@pytest.mark.parametrize("case", CASES, ids=str)
def test_matches_fp64_reference(case, out):
    H, dtype, B, S = case
    tables, ids, types, mask = build(*case)
    hidden, add_mask = run(tables, ids, mask, types, out)
    ref = reference64(tables, ids, types)
    e32 = eager32_error(tables, ids, types, ref)
    err = (hidden.cpu().double() - ref).abs()
    print(f"case={case} out={out} eager_fp32_max_err={e32:.3e} "
          f"kernel_max_err={float(err.max()):.3e}")
    assert bool((err <= 4 * e32 + half_ulp(ref, out)).all())
    low = torch.finfo(DTYPES[out]).min
    want = torch.where(mask != 0, 0.0, low).to(DTYPES[out])
    assert torch.equal(add_mask.cpu(), want[:, None, None, :])
    assert not bool(torch.signbit(add_mask[add_mask == 0]).any())   # +0.0
    assert run(tables, ids, None, types, out)[1] is None


@pytest.mark.parametrize("case", CASES, ids=str)
def test_exact_properties(case):
    H, dtype, B, S = case
    tables, ids, types, mask = build(*case, seed=1)
    hidden, add_mask = run(tables, ids, mask, types, dtype)
    for other in (run(tables, ids, mask, types, dtype),
                  run(tables, ids.long(), mask.long(), types.long(), dtype)):
        assert torch.equal(hidden, other[0]) and torch.equal(add_mask, other[1])
    rows = torch.cat([run(tables, ids[b:b + 1], None, types[b:b + 1],
                          dtype)[0] for b in range(B)])
    assert torch.equal(hidden, rows)


@pytest.mark.parametrize("typed", [False, True])
@pytest.mark.parametrize("H,dtype,lengths", [
    (8, "f32", [1, 7, 3]), (520, "bf16", [1, 7, 3]),
    (768, "bf16", [MAX_POS, 2, 9]), (8, "f16", [5] * 1700)], ids=str)
def test_ragged_equals_dense(H, dtype, lengths, typed):
    B, S, pad = len(lengths), max(lengths), 3
    tables, ids, types, _ = build(H, dtype, B, S, seed=2)
    lens = torch.tensor(lengths)
    keep = torch.arange(S)[None, :] < lens[:, None]
    dense_ids = torch.where(keep, ids, pad)
    dense_types = torch.where(keep, types, 0) if typed else None
    want = run(tables, dense_ids, keep.to(torch.int32), dense_types, dtype)
    got = ops.bert_embed_ragged(
        ids[keep].to(DEV), lengths, *(t.to(DEV) for t in tables), EPS,
        token_type_ids=types[keep].to(DEV) if typed else None, pad_id=pad,
        out_dtype=DTYPES[dtype])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(got[1].cpu()[:, 0, 0, :], torch.where(
        keep, 0.0, torch.finfo(DTYPES[dtype]).min).to(DTYPES[dtype]))


@pytest.mark.parametrize("bad,message", [
    ("id", r"input_ids\[1,4\] = 50 is outside \[0, 50\)"),
    ("type", r"token_type_ids\[1,4\] = 2 is outside \[0, 2\)"),
    ("id+type", r"input_ids\[1,4\] = 50 is outside \[0, 50\)"),
    ("ragged id", r"input_ids of sequence 1, position 4 = 50 is outside"),
    ("ragged length", r"sequence 1: length must be in 1\.\.40.*got 41")])
def test_bad_values_raise_and_slot_is_reset(bad, message):
    """Only through the new ops: their kernel never indexes with a bad id."""
    tables, ids, types, mask = build(520, "bf16", 3, 7, seed=3)
    clean = run(tables, ids, mask, types, "bf16")[0]
    ids_bad, types_bad = ids.clone(), types.clone()
    if "id" in bad:
        ids_bad[1, 4], ids_bad[2, 0] = VOCAB, VOCAB + 5    # lowest row wins
    if "type" in bad:
        types_bad[1, 4] = TYPE_VOCAB
    with pytest.raises(ValueError, match=message):
        if bad.startswith("ragged"):
            ops.bert_embed_ragged(
                ids_bad.view(-1).to(DEV),
                [7, MAX_POS + 1 if "length" in bad else 7, 7],
                *(t.to(DEV) for t in tables), EPS,
                token_type_ids=types_bad.view(-1).to(DEV))
        else:
            run(tables, ids_bad, mask, types_bad, "bf16")
    # the same tensors, valid again: the error slot was reset
    assert torch.equal(run(tables, ids, mask, types, "bf16")[0], clean)


class OneLayer(BertConfig):
    vocab_size, hidden, layers, heads = VOCAB, 64, 1, 2
    intermediate, max_pos, type_vocab = 128, MAX_POS, TYPE_VOCAB


E2E_IDS = [[49, 3, 17, 0, 8, 21, 5], [4, 9], [30, 1, 1, 12]]


@pytest.fixture(scope="module")
def server(tmp_path_factory):
    sock = f"unix://{tmp_path_factory.mktemp('s')}/bert_embed.sock"
    with ModelServer(address=sock, raw_predict=True, device=DEV) as srv:
        for dtype in ("f32", "bf16"):
            for mode in ("ids", "ids_fused", "ids_ragged"):
                srv.manager.load(
                    f"{mode}_{dtype}",
                    bert_servable(DEV, DTYPES[dtype], input_format=mode,
                                  config=OneLayer()), version=1)
        with TurboPredictClient(sock) as client:
            yield srv, client


def padded_request():
    flat, lengths = pack_ragged_tokens(E2E_IDS)
    mask = (torch.arange(7)[None, :] < torch.tensor(lengths)[:, None]).int()
    ids = torch.zeros_like(mask)
    ids[mask != 0] = torch.from_numpy(flat)
    return {"input_ids": ids.to(DEV), "attention_mask": mask.to(DEV)}


def test_fused_mode_matches_ids_mode(server):
    """At the embedding, the fused kernel on the servable's own weights is
    within the f32 / bf16 tolerance above of the fp64 reference. At the final
    output the margin is the default mode's own bf16-against-f32 difference
    on the same inputs, the noise a user of this model already accepts. The
    fused f32 model may differ from the default f32 model by no more than
    that. The fused and the default bf16 model are each that far from the f32
    model, so by the triangle inequality they may be 2x that far apart."""
    srv, client = server
    req = padded_request()
    out = {name: client.predict(name, req, output_device=DEV) for name in
           ("ids_f32", "ids_bf16", "ids_fused_f32", "ids_fused_bf16")}
    ids = req["input_ids"].cpu()
    for dtype in ("f32", "bf16"):
        m = srv.manager.get(f"ids_fused_{dtype}").module
        params = [p.detach() for p in (m.tok.weight, m.pos.weight,
                                       m.typ.weight, m.ln.weight, m.ln.bias)]
        tables = [p.cpu() for p in params]
        ref = reference64(tables, ids, torch.zeros_like(ids))
        e32 = eager32_error(tables, ids, torch.zeros_like(ids), ref)
        got = ops.bert_embed(req["input_ids"], *params, m.ln.eps)[0]
        err = (got.cpu().double() - ref).abs()
        assert bool((err <= 4 * e32 + half_ulp(ref, dtype)).all())
    for key in ("last_hidden_state", "pooled_output"):
        margin = float((out["ids_bf16"][key] - out["ids_f32"][key])
                       .abs().max())
        d32 = (out["ids_fused_f32"][key] - out["ids_f32"][key]).abs().max()
        d16 = (out["ids_fused_bf16"][key] - out["ids_bf16"][key]).abs().max()
        print(f"{key}: margin={margin:.3e} fused_f32={float(d32):.3e} "
              f"fused_bf16={float(d16):.3e}")
        assert float(d32) <= margin and float(d16) <= 2 * margin


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ragged_mode_equals_fused_on_padded_input(server, dtype):
    _, client = server
    ids, lengths = pack_ragged_tokens(E2E_IDS)
    ragged = client.predict(
        f"ids_ragged_{dtype}",
        {"input_ids": torch.from_numpy(ids).to(DEV),
         "sequence_lengths": torch.from_numpy(lengths)}, output_device=DEV)
    fused = client.predict(f"ids_fused_{dtype}", padded_request(),
                           output_device=DEV)
    assert tuple(ragged["last_hidden_state"].shape) == (3, 7, 64)
    for key in fused:
        assert torch.equal(ragged[key], fused[key])


def test_token_types_reach_the_model(server):
    _, client = server
    req = padded_request()
    zeros = dict(req, token_type_ids=torch.zeros_like(req["input_ids"]))
    pair = dict(req, token_type_ids=req["attention_mask"]
                * (torch.arange(7, device=DEV) >= 3).to(torch.int32))
    plain, zero, two = (client.predict("ids_fused_f32", r, output_device=DEV)
                        ["last_hidden_state"] for r in (req, zeros, pair))
    assert torch.equal(plain, zero) and not torch.equal(zero, two)


@pytest.mark.parametrize("mode", ["ids_fused", "ids_ragged"])
def test_bad_id_is_invalid_argument(server, mode):
    _, client = server
    req = padded_request()
    req["input_ids"][2, 1] = VOCAB
    if mode == "ids_ragged":
        flat, lengths = pack_ragged_tokens([[1, 2], [3, VOCAB, 4]])
        req = {"input_ids": torch.from_numpy(flat).to(DEV),
               "sequence_lengths": torch.from_numpy(lengths)}
    with pytest.raises(grpc.RpcError) as info:
        client.predict(f"{mode}_f32", req)
    assert info.value.code() == grpc.StatusCode.INVALID_ARGUMENT
    assert "is outside [0, 50)" in info.value.details()
