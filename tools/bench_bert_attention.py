#!/usr/bin/env python3
"""BERT self-attention: the fused length-masked MFMA kernel against what a
``BertLayer`` does by default, one GPU.

    python tools/bench_bert_attention.py        # JSON lines
    python tools/bench_bert_attention.py --packed
    python tools/bench_bert_attention.py --masked

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

``--packed``: the packed (varlen) form against the padded fused kernel on
the full, ragged and mixed cases, in the same interleaved rounds: the op
alone (``qkv [T,3H]`` with ``ops.attention_tiles`` against ``qkv [B,S,3H]``
with ``lengths``; both table orders, sequence order and longest sequence
first, each built here from the helper's table), and one full ``BertLayer``
forward in bf16 (H 768), packed ``[T,H]`` against padded ``[B,S,H]`` with
``lengths``, which is the figure the packed path exists for.

``--masked``: the keys form (``keys=ops.attention_keys(mask)``, arbitrary
key masks, every query row computed) on the ragged case, 128 sequences of
16..512 kept tokens at S = 512, in three mask layouts (the kept tokens as a
prefix, as a suffix, scattered), in the same interleaved rounds against the
default layer's chain with the additive mask (what a dense request runs
without it), against the length form at the same counts (prefix layout only;
it computes only the kept query rows, so it is the floor) and the
``ops.attention_keys`` launch alone.
"""
import argparse
import json
import os
import subprocess
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)

CASES = ["128x512_full", "128x512_ragged", "8x128_mixed", "1x32_full"]
PACKED_CASES = CASES[:3]
MASK_LAYOUTS = ["prefix", "suffix", "scattered"]
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


def case_lengths(name, g):
    import torch

    shape, kind = name.split("_")
    B, S = (int(d) for d in shape.split("x"))
    if kind == "full":
        return B, S, torch.full((B,), S)
    if kind == "ragged":
        return B, S, torch.randint(16, S + 1, (B,), generator=g)
    return B, S, torch.tensor([S, S // 2, 7, S - 1, 33, 64, 65, 100][:B])


def stats(prefix, t):
    return {f"{prefix}_ms": round(t[0], 4), f"{prefix}_min_ms": round(t[1], 4),
            f"{prefix}_max_ms": round(t[2], 4)}


def run_packed_case(name):
    import torch

    from min_tfs_client_amd import ops
    from min_tfs_client_amd.models.bert import BertConfig, BertLayer

    ops.require_native()
    dev = "cuda:0"
    H = HEADS * HEAD_DIM
    g = torch.Generator().manual_seed(0)
    B, S, lengths = case_lengths(name, g)
    T = int(lengths.sum())
    keep = (torch.arange(S)[None, :] < lengths[:, None]).to(dev)
    lens = lengths.to(torch.int32).to(dev)
    qkv = torch.randn(B, S, 3 * H, generator=g).to(torch.bfloat16).to(dev)
    qkv_p = qkv[keep].contiguous()
    # both orders from the helper's table, whichever it emits
    table = ops.attention_tiles(lengths)
    by_seq = table[torch.argsort(table[:, 3] * (1 << 20) + table[:, 2])]
    longest = by_seq[torch.argsort(-by_seq[:, 1], stable=True)]
    by_seq, longest = by_seq.to(dev), longest.to(dev)

    def padded():
        return ops.masked_self_attention(qkv, lens, HEADS)

    def packed_seq():
        return ops.masked_self_attention(qkv_p, None, HEADS, tiles=by_seq)

    def packed_longest():
        return ops.masked_self_attention(qkv_p, None, HEADS, tiles=longest)

    same = bool(torch.equal(padded()[keep], packed_seq())) and \
        bool(torch.equal(packed_seq(), packed_longest()))
    # windows of tens of milliseconds: the differences looked for are small
    reps = 200 if B * S >= 8192 else 2000
    t_pad, t_seq, t_long = rounds_of((padded, packed_seq, packed_longest),
                                     reps)

    torch.manual_seed(0)
    layer = BertLayer(BertConfig()).to(device=dev,
                                       dtype=torch.bfloat16).eval()
    x = torch.randn(B, S, H, generator=g).to(torch.bfloat16).to(dev)
    x_p = x[keep].contiguous()
    with torch.no_grad():
        def layer_padded():
            return layer(x, None, lens)

        def layer_packed():
            return layer(x_p, None, None, by_seq)

        layer_diff = (layer_padded()[keep].float()
                      - layer_packed().float()).abs().max().item()
        l_pad, l_pack = rounds_of((layer_padded, layer_packed),
                                  40 if B * S >= 8192 else 400)
    print(json.dumps({
        "case": name, "mode": "packed", "tokens": T, "padded_tokens": B * S,
        "token_share": round(T / (B * S), 3), "bit_identical": same,
        **stats("padded", t_pad), **stats("packed_seq_order", t_seq),
        **stats("packed_longest_first", t_long),
        **stats("layer_padded", l_pad), **stats("layer_packed", l_pack),
        "layer_packed_over_padded": round(l_pack[0] / l_pad[0], 3),
        "layer_max_abs_diff_kept": layer_diff}), flush=True)


def run_masked_case(layout):
    import torch
    import torch.nn.functional as F

    from min_tfs_client_amd import ops
    from min_tfs_client_amd.models.bert import BertEncoder

    ops.require_native()
    dev = "cuda:0"
    H = HEADS * HEAD_DIM
    g = torch.Generator().manual_seed(0)
    B, S, counts = case_lengths("128x512_ragged", g)
    prefix = torch.arange(S)[None, :] < counts[:, None]
    if layout == "prefix":
        keep = prefix
    elif layout == "suffix":
        keep = prefix.flip(1)
    else:       # each row's kept positions: a seeded random subset
        rank = torch.rand(B, S, generator=g).argsort(1).argsort(1)
        keep = rank < counts[:, None]
    qkv = torch.randn(B, S, 3 * H, generator=g).to(torch.bfloat16).to(dev)
    mask = keep.to(torch.int32).to(dev)
    lens = counts.to(torch.int32).to(dev)
    add_mask = BertEncoder.additive_mask(mask, torch.bfloat16)
    keys = ops.attention_keys(mask)

    def masked():
        return ops.masked_self_attention(qkv, None, HEADS, keys=keys)

    def sdpa():
        q, k, v = (t.transpose(1, 2) for t in
                   qkv.view(B, S, 3, HEADS, HEAD_DIM).unbind(2))
        attn = F.scaled_dot_product_attention(q, k, v, attn_mask=add_mask)
        return attn.transpose(1, 2).reshape(B, S, H)

    def length_form():
        return ops.masked_self_attention(qkv, lens, HEADS)

    def key_index():
        return ops.attention_keys(mask)

    diff = (masked().float() - sdpa().float()).abs().max().item()
    same = None
    if layout == "prefix":
        kept = keep.to(dev)
        same = bool(torch.equal(masked()[kept], length_form()[kept]))
    t_m, t_s, t_l = rounds_of((masked, sdpa, length_form), 20)
    t_k, = rounds_of((key_index,), 2000)
    print(json.dumps({
        "case": "128x512_ragged", "mode": "masked", "layout": layout,
        "kept_tokens": int(counts.sum()), "padded_tokens": B * S,
        **stats("masked", t_m), **stats("sdpa", t_s),
        **stats("length_form", t_l), **stats("attention_keys", t_k),
        "sdpa_over_masked": round(t_s[0] / t_m[0], 2),
        "masked_over_length_form": round(t_m[0] / t_l[0], 2),
        "prefix_kept_rows_bit_identical": same,
        "max_abs_diff_all_rows": diff}), flush=True)


def run_case(name):
    import torch
    import torch.nn.functional as F

    from min_tfs_client_amd import ops
    from min_tfs_client_amd.models.bert import BertEncoder

    ops.require_native()
    dev = "cuda:0"
    H = HEADS * HEAD_DIM
    g = torch.Generator().manual_seed(0)
    B, S, lengths = case_lengths(name, g)
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
    ap.add_argument("--packed", action="store_true",
                    help="the packed form against the padded fused kernel")
    ap.add_argument("--masked", action="store_true",
                    help="the keys form (arbitrary key masks) against sdpa "
                         "and the length form")
    ap.add_argument("--layout", choices=MASK_LAYOUTS,
                    help="(child, with --masked) run one mask layout")
    a = ap.parse_args()
    if a.layout:
        return run_masked_case(a.layout)
    if a.masked:
        for layout in MASK_LAYOUTS:
            run_step(["--masked", "--layout", layout])
        return
    if a.case:
        return (run_packed_case if a.packed else run_case)(a.case)
    for name in PACKED_CASES if a.packed else CASES:
        run_step(["--case", name] + (["--packed"] if a.packed else []))


if __name__ == "__main__":
    main()
