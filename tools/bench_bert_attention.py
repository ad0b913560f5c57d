#!/usr/bin/env python3
"""BERT self-attention: the fused length-masked MFMA kernel against what a
``BertLayer`` does by default, one GPU.

    python tools/bench_bert_attention.py        # JSON lines

The parent process never touches the GPU. Every case runs in a fresh child
process under its own time limit, and the tool exits non-zero on the first
case that fails or times out.

Both paths start from the same bf16 ``qkv`` projection (heads 12, H 768):
``ops.masked_self_attention(qkv, lengths, 12)``, one launch, against the
default layer's chain: the three transposed views,
``scaled_dot_product_attention`` with the additive ``[B,1,1,S]`` mask of
``finfo.min``, and the ``transpose(1, 2).reshape(B, S, H)`` copy. They run in
one process in interleaved rounds; times are device events around ``reps``
calls after warm-up, and the median, the fastest and the slowest of the
rounds are reported.

Cases: 128 x 512 all full length; 128 x 512 with seeded lengths uniform in
16..512; 8 x 128 with mixed lengths; 1 x 32. ``needed_tflops`` counts the
FLOPs the lengths actually ask for, 4 * 64 * heads * sum(L^2) (kept keys x
kept queries, both matmuls), over the fused kernel's time.
"""
import argparse
import json
import os
import subprocess
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)

CASES = ["128x512_full", "128x512_ragged", "8x128_mixed", "1x32_full"]
STEP_TIMEOUT_S = 240
HEADS, HEAD_DIM = 12, 64


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


def rounds_of(fns, reps, rounds=7):
    """Interleaved rounds of every callable: (median, min, max) of each."""
    times = [[time_calls(fn, reps, 10) for fn in fns] for _ in range(rounds)]
    cols = [sorted(r[i] for r in times) for i in range(len(fns))]
    return [(c[rounds // 2], c[0], c[-1]) for c in cols]


def run_case(name):
    import torch
    import torch.nn.functional as F

    from min_tfs_client_amd import ops
    from min_tfs_client_amd.models.bert import BertEncoder

    ops.require_native()
    dev = "cuda:0"
    shape, kind = name.split("_")
    B, S = (int(d) for d in shape.split("x"))
    H = HEADS * HEAD_DIM
    g = torch.Generator().manual_seed(0)
    if kind == "full":
        lengths = torch.full((B,), S)
    elif kind == "ragged":
        lengths = torch.randint(16, S + 1, (B,), generator=g)
    else:
        lengths = torch.tensor([S, S // 2, 7, S - 1, 33, 64, 65, 100][:B])
    qkv = torch.randn(B, S, 3 * H, generator=g).to(torch.bfloat16).to(dev)
    lens = lengths.to(torch.int32).to(dev)
    keep = (torch.arange(S)[None, :] < lengths[:, None]).to(dev)
    add_mask = BertEncoder.additive_mask(keep, torch.bfloat16)

    def fused():
        return ops.masked_self_attention(qkv, lens, HEADS)

    def sdpa():
        q, k, v = (t.transpose(1, 2) for t in
                   qkv.view(B, S, 3, HEADS, HEAD_DIM).unbind(2))
        attn = F.scaled_dot_product_attention(q, k, v, attn_mask=add_mask)
        return attn.transpose(1, 2).reshape(B, S, H)

    diff = (fused().float() - sdpa().float())[keep].abs().max().item()
    reps = 20 if B * S >= 8192 else 200
    (f_med, f_min, f_max), (s_med, s_min, s_max) = rounds_of((fused, sdpa),
                                                             reps)
    flops = 4.0 * HEAD_DIM * HEADS * float((lengths.double() ** 2).sum())
    print(json.dumps({
        "case": name, "tokens": int(lengths.sum()), "padded_tokens": B * S,
        "fused_ms": round(f_med, 4), "fused_min_ms": round(f_min, 4),
        "fused_max_ms": round(f_max, 4),
        "sdpa_ms": round(s_med, 4), "sdpa_min_ms": round(s_min, 4),
        "sdpa_max_ms": round(s_max, 4),
        "sdpa_over_fused": round(s_med / f_med, 2),
        "needed_gflop": round(flops / 1e9, 3),
        "needed_tflops": round(flops / 1e12 / (f_med / 1e3), 2),
        "max_abs_diff_kept": diff}), flush=True)


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
