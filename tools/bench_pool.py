#!/usr/bin/env python3
"""Masked mean-pool head: fused kernel against the eager chain, one GPU.

    python tools/bench_pool.py             # kernel/op timings, JSON lines
    python tools/bench_pool.py --predict   # + BERT Predict p50 per mode

The parent process never touches the GPU. Every step (one shape x dtype of
the op timings, one output mode of the Predict comparison) runs in a fresh
child process under its own time limit, and the tool exits non-zero on the
first step that fails or times out.

Op timings: ``ops.masked_mean_pool`` (public op) and the bare native call
against the eager chain

    (h * m[..., None]).sum(1) / m.sum(1, keepdim=True).clamp(min=1)

plus ``F.normalize`` when normalizing, with a full mask and with half the
positions padded. Interleaved rounds in one process, the median round is
reported. GB/s is computed from the bytes that must be read or written: the
kept rows of the hidden state, the mask and the fp32 output.

Predict p50: the real BERT-base servable (bf16) behind the raw server over
a unix socket, host tensors in and out, 8x128 tokens, "hidden" against
"sentence_embedding" mode, each from its own fresh server process.
"""
import argparse
import json
import os
import subprocess
import sys
import time

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)

OP_CASES = {
    "128x512x768_bf16": ((128, 512, 768), "bfloat16"),
    "128x512x768_f32": ((128, 512, 768), "float32"),
    "1x512x768_bf16": ((1, 512, 768), "bfloat16"),
    "1x512x768_f32": ((1, 512, 768), "float32"),
}
PREDICT_MODES = ("hidden", "sentence_embedding")
STEP_TIMEOUT_S = 240


def time_kernel(fn, reps, warmup):
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


def run_op_case(name):
    import torch
    import torch.nn.functional as F

    from min_tfs_client_amd import ops

    shape, dtype_name = OP_CASES[name]
    dtype = getattr(torch, dtype_name)
    dev = "cuda:0"
    native = ops.require_native()
    B, S, H = shape
    h = torch.randn(shape, device=dev).to(dtype)
    masks = {"full": torch.ones(B, S, dtype=torch.int32, device=dev)}
    half = masks["full"].clone()
    half[:, S // 2:] = 0
    masks["half_padded"] = half
    reps = 100 if B > 1 else 300

    for mask_name, m in masks.items():
        mf = m.to(dtype)
        kept = int(m.sum().item())
        nbytes = kept * H * h.element_size() + m.numel() * 4 + B * H * 4
        for normalize in (False, True):
            def op():
                return ops.masked_mean_pool(h, m, normalize)

            def bare():
                return native.masked_mean_pool(h, m, normalize)

            def eager():
                y = (h * mf[..., None]).sum(1) \
                    / mf.sum(1, keepdim=True).clamp(min=1)
                return F.normalize(y, dim=1) if normalize else y

            err = (op() - eager().float()).abs().max().item()
            rounds = [(time_kernel(bare, reps, 10), time_kernel(op, reps, 10),
                       time_kernel(eager, reps, 10)) for _ in range(5)]
            ms_bare, ms_op, ms_eager = (
                sorted(r[i] for r in rounds)[2] for i in range(3))
            print(json.dumps({
                "case": name, "mask": mask_name, "normalize": normalize,
                "native_ms": round(ms_bare, 4), "op_ms": round(ms_op, 4),
                "eager_ms": round(ms_eager, 4),
                "eager_over_op": round(ms_eager / ms_op, 2),
                "bytes": nbytes,
                "native_GB_s": round(nbytes / 1e9 / (ms_bare / 1e3), 1),
                "max_abs_diff_vs_eager": err}), flush=True)


def run_predict_mode(mode, batch=8, seq=128, steps=200, warmup=20):
    import tempfile

    import torch

    from min_tfs_client_amd.models import bert_servable
    from min_tfs_client_amd.server import ModelServer
    from min_tfs_client_amd.turbo import TurboPredictClient

    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 30522, (batch, seq), generator=g).to(torch.int32)
    mask = torch.ones(batch, seq, dtype=torch.int32)
    mask[batch // 2:, seq // 2:] = 0
    inputs = {"input_ids": ids, "attention_mask": mask}
    with tempfile.TemporaryDirectory() as tmp:
        sock = f"unix://{tmp}/bench_pool.sock"
        with ModelServer(address=sock, raw_predict=True, device=dev) as srv:
            srv.manager.load(
                "bert", bert_servable(dev, torch.bfloat16,
                                      output_format=mode), version=1)
            with TurboPredictClient(sock) as client:
                lat = []
                for i in range(warmup + steps):
                    t0 = time.perf_counter()
                    out = client.predict("bert", inputs)
                    if i >= warmup:
                        lat.append((time.perf_counter() - t0) * 1e3)
    lat.sort()
    print(json.dumps({
        "predict_mode": mode, "shape": [batch, seq], "steps": steps,
        "p50_ms": round(lat[len(lat) // 2], 3),
        "p99_ms": round(lat[int(len(lat) * 0.99) - 1], 3),
        "response_bytes": sum(v.numel() * v.element_size()
                              for v in out.values())}), flush=True)


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
    ap.add_argument("--predict", action="store_true",
                    help="also time BERT Predict in both output modes")
    ap.add_argument("--only-predict", action="store_true")
    ap.add_argument("--op-case", choices=sorted(OP_CASES),
                    help="(child) run one op timing case")
    ap.add_argument("--predict-mode", choices=PREDICT_MODES,
                    help="(child) run one Predict mode")
    a = ap.parse_args()
    if a.op_case:
        return run_op_case(a.op_case)
    if a.predict_mode:
        return run_predict_mode(a.predict_mode)
    if not a.only_predict:
        for name in OP_CASES:
            run_step(["--op-case", name])
    if a.predict or a.only_predict:
        for mode in PREDICT_MODES:
            run_step(["--predict-mode", mode])


if __name__ == "__main__":
    main()
