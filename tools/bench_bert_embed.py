#!/usr/bin/env python3
"""BERT embedding ingest: fused kernel against the eager chain, one GPU.

    python tools/bench_bert_embed.py        # JSON lines

The parent process never touches the GPU. Every case runs in a fresh child
process under its own time limit, and the tool exits non-zero on the first
case that fails or times out.

Dense cases (B x S of 1x128, 8x128, 32x384, 128x512; bf16 and f32):
``ops.bert_embed`` (one launch + the 4-byte error-slot read), the same
without that read (the bare native call with ``check=False``, which the
public op never passes: kernel time plus launch), and the eager
``BertEncoder.embed`` + ``additive_mask`` on the same BERT-base tables, in
one process, in interleaved rounds; the median round is reported. Times are
device events around ``reps`` calls after warm-up.

Ragged case: 128 sequences with seeded lengths in 16..512 through
``ops.bert_embed_ragged`` against ``ops.bert_embed`` on the same ids padded
to 512 (what a client without the ragged mode sends).

GB/s counts the bytes that must move: ids and mask in, one token row read
per position, the hidden state and the additive mask out (the position and
type rows are shared between sequences and come from cache). The share of
HBM peak uses 8.0 TB/s.
"""
import argparse
import json
import os
import subprocess
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)

SHAPES = ((1, 128), (8, 128), (32, 384), (128, 512))
CASES = [f"{b}x{s}_{d}" for b, s in SHAPES for d in ("bfloat16", "float32")]
CASES += ["ragged128_bfloat16", "ragged128_float32"]
STEP_TIMEOUT_S = 240
HBM_PEAK_GB_S = 8000.0


def time_calls(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps  # ms


def median_rounds(fns, reps, rounds=5):
    """Interleaved rounds of every callable; the median of each."""
    times = [[time_calls(fn, reps, 10) for fn in fns] for _ in range(rounds)]
    return [sorted(r[i] for r in times)[rounds // 2] for i in range(len(fns))]


def build_model(dtype):
    import torch

    from min_tfs_client_amd.models.bert import BertConfig, BertEncoder

    class EmbeddingsOnly(BertConfig):
        layers = 0

    torch.manual_seed(0)
    m = BertEncoder(EmbeddingsOnly()).to(device="cuda:0", dtype=dtype).eval()
    tables = (m.tok.weight.detach(), m.pos.weight.detach(),
              m.typ.weight.detach(), m.ln.weight.detach(),
              m.ln.bias.detach(), m.ln.eps)
    return m, tables


def moved_bytes(rows, kept_rows, H, elem):
    return rows * 8 + kept_rows * H * elem + rows * H * elem + rows * elem


def run_case(name):
    import torch

    from min_tfs_client_amd import ops

    shape, dtype_name = name.rsplit("_", 1)
    dtype = getattr(torch, dtype_name)
    elem = torch.empty((), dtype=dtype).element_size()
    dev = "cuda:0"
    native = ops.require_native()
    model, tables = build_model(dtype)
    H = tables[0].shape[1]
    g = torch.Generator().manual_seed(0)

    if shape == "ragged128":
        lengths = torch.randint(16, 513, (128,), generator=g)
        total = int(lengths.sum())
        flat = torch.randint(0, 30522, (total,), generator=g).to(torch.int32)
        keep = torch.arange(512)[None, :] < lengths[:, None]
        padded = torch.zeros(128, 512, dtype=torch.int32)
        padded[keep] = flat
        flat_d, padded_d = flat.to(dev), padded.to(dev)
        mask_d = keep.to(torch.int32).to(dev)
        lens = lengths.numpy()

        def ragged():
            return ops.bert_embed_ragged(flat_d, lens, *tables,
                                         out_dtype=dtype)

        def dense():
            return ops.bert_embed(padded_d, *tables, attention_mask=mask_d,
                                  out_dtype=dtype)

        S = int(lengths.max())
        same = torch.equal(ragged()[0], dense()[0][:, :S])
        ms_ragged, ms_dense = median_rounds((ragged, dense), 50)
        print(json.dumps({
            "case": name, "sequences": 128, "tokens": total,
            "padded_tokens": 128 * 512, "max_length": S,
            "ragged_ms": round(ms_ragged, 4),
            "padded_to_512_ms": round(ms_dense, 4),
            "request_bytes_ragged": total * 4 + 128 * 4,
            "request_bytes_padded": 128 * 512 * 8,
            "bit_identical": same}), flush=True)
        return

    B, S = (int(d) for d in shape.split("x"))
    ids = torch.randint(0, 30522, (B, S), generator=g).to(torch.int32).to(dev)
    mask = torch.ones(B, S, dtype=torch.int32, device=dev)
    mask[B // 2:, S // 2:] = 0

    def op():
        return ops.bert_embed(ids, *tables, attention_mask=mask,
                              out_dtype=dtype)

    def unchecked():
        return native.bert_embed(ids, None, B, S, mask, None, *tables, 0,
                                 dtype, False)

    @torch.no_grad()
    def eager():
        x = model.embed(ids)
        return x, model.additive_mask(mask, x.dtype)

    diff = (op()[0].float() - eager()[0].float()).abs().max().item()
    reps = 100 if B * S >= 8192 else 300
    ms_op, ms_unchecked, ms_eager = median_rounds((op, unchecked, eager), reps)
    nbytes = moved_bytes(B * S, B * S, H, elem)
    gb_s = nbytes / 1e9 / (ms_unchecked / 1e3)
    print(json.dumps({
        "case": name, "op_ms": round(ms_op, 4),
        "op_no_slot_read_ms": round(ms_unchecked, 4),
        "slot_read_ms": round(ms_op - ms_unchecked, 4),
        "eager_ms": round(ms_eager, 4),
        "eager_over_op": round(ms_eager / ms_op, 2),
        "bytes": nbytes, "no_slot_read_GB_s": round(gb_s, 1),
        "share_of_hbm_peak": round(gb_s / HBM_PEAK_GB_S, 3),
        "max_abs_diff_vs_eager": diff}), flush=True)


def run_step(args):
    """One child process under its own time limit; exit on failure."""
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        rc = subprocess.run(cmd, timeout=STEP_TIMEOUT_S).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps({"step": args, "error": "timeout",
                          "timeout_s": STEP_TIMEOUT_S}), flush=True)
        sys.exit(124)
    if rc != 0:
        print(json.dumps({"step": args, "error": "failed", "exit": rc}),
              flush=True)
        sys.exit(rc if rc > 0 else 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--case", choices=CASES, help="(child) run one case")
    a = ap.parse_args()
    if a.case:
        return run_case(a.case)
    for name in CASES:
        run_step(["--case", name])


if __name__ == "__main__":
    main()
