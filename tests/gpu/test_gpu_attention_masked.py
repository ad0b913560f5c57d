"""Keys form of ``ops.masked_self_attention`` (arbitrary key masks) and
``ops.attention_keys`` on the GPU: fp64 reference at EVERY query row (batches,
reference and bound of tests/unit/test_attention_masked.py, the bound being
that of test_gpu_attention.py), bit identity with the length form, then
``attention="masked"`` through the raw server."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from min_tfs_client_amd import ops  # noqa: E402
from min_tfs_client_amd.models import bert_servable  # noqa: E402
from min_tfs_client_amd.server import ModelServer  # noqa: E402
from min_tfs_client_amd.turbo import TurboPredictClient  # noqa: E402
from tests.unit.test_attention_masked import (  # noqa: E402
    DTYPES, REQ, OneLayer, build, error_over_bound)

DEV = "cuda:0"


def run(qkv, mask):
    return ops.masked_self_attention(
        qkv.to(DEV), None, 2, keys=ops.attention_keys(mask.to(DEV)))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("S", [150, 17])
def test_matches_fp64_reference(S, dtype):
    qkv, mask = build(S, dtype)
    worst = error_over_bound(run(qkv, mask).cpu(), qkv, mask, dtype)
    print(f"S={S} {dtype} max_err/tol per row: {[round(w, 3) for w in worst]}")
    assert max(worst) <= 1.0


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_bit_identical_to_the_length_form(dtype):
    qkv, mask = build(150, dtype, seed=1)
    out = run(qkv, mask)
    assert torch.equal(out, run(qkv, mask))
    for b in range(6):
        kept = mask[b] != 0
        alone = ops.masked_self_attention(qkv[b, kept][None].to(DEV), None, 2)
        assert torch.equal(out[b, kept.to(DEV)], alone[0]), f"row {b}"


@pytest.mark.parametrize("S", [150, 17])
@pytest.mark.parametrize("mask_dtype", [torch.int32, torch.uint8, torch.bool,
                                        torch.int64])
def test_attention_keys(mask_dtype, S):
    mask = build(S)[1]
    m = mask.long() << 32 if mask_dtype == torch.int64 else mask.to(mask_dtype)
    index, count = ops.attention_keys(m.to(DEV))    # int64: 1 << 32 keeps
    assert index.dtype == count.dtype == torch.int32 and index.shape == m.shape
    for b in range(7):
        kept = torch.nonzero(mask[b])[:, 0]
        assert int(count[b]) == len(kept)
        assert torch.equal(index[b, :len(kept)].cpu().long(), kept)


@pytest.mark.parametrize("output_format", ["hidden", "sentence_embedding"])
def test_masked_attention_through_the_raw_server(sock_dir, output_format):
    """At ALL positions within twice the default mode's own bf16-against-f32
    difference (the criterion of test_gpu_attention.py)."""
    req = {k: v.to(DEV) for k, v in REQ.items()}
    address = f"unix://{sock_dir}/masked.sock"
    with ModelServer(address=address, raw_predict=True, device=DEV) as srv:
        for name, dtype in (("f32", torch.float32), ("sdpa", torch.bfloat16),
                            ("masked", torch.bfloat16)):
            srv.manager.load(name, bert_servable(
                DEV, dtype, config=OneLayer(), output_format=output_format,
                attention="masked" if name == "masked" else "sdpa"), version=1)
        with TurboPredictClient(address) as client:
            out = {name: client.predict(name, req, output_device=DEV)
                   for name in ("f32", "sdpa", "masked")}
    for key in out["f32"]:
        f32, bf16, masked = (out[n][key] for n in ("f32", "sdpa", "masked"))
        margin = float((bf16 - f32).abs().max())
        diff = float((masked - bf16).abs().max())
        print(f"{key}: margin={margin:.3e} masked_vs_bf16={diff:.3e}")
        assert masked.shape == bf16.shape and diff <= 2 * margin
