#!/usr/bin/env python3
"""Softmax + top-k head: fused kernel against the eager chain, one GPU.

    python tools/bench_topk.py             # kernel/op timings, JSON lines
    python tools/bench_topk.py --predict   # + ResNet Predict per output mode

The parent process never touches the GPU. Every step (the op timings, one
output mode of the Predict comparison) runs in a fresh child process under
its own time limit, and the tool exits non-zero on the first step that fails
or times out.

Op timings: ``ops.softmax_topk`` (public op) and the bare native call
against the eager chain on the same device

    torch.softmax(x.float(), 1).topk(k)

for B in {1, 8, 64, 256} at C=1000, k=5 (the ResNet head) and one C=32000,
k=50 case (an LM-vocabulary-sized row, past the 8192-class LDS threshold),
in bf16 and f32. Interleaved rounds in one process, the median round is
reported. GB/s is computed from the bytes that must be read or written: the
logits once, the two outputs once. The largest score difference from eager
and the number of rows whose classes differ from eager's are reported, not
asserted: eager's topk breaks ties its own way.

Predict: the real ResNet-50 servable (bf16) behind the raw server over a
unix socket, host tensors in and out, batch 8, "logits" against "topk"
mode, each from its own fresh server process; response bytes and p50.
"""
import argparse
import json
import os
import subprocess
import sys
import time

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)

OP_CASES = [(1, 1000, 5), (8, 1000, 5), (64, 1000, 5), (256, 1000, 5),
            (64, 32000, 50)]
OP_DTYPES = ("bfloat16", "float32")
PREDICT_MODES = ("logits", "topk")
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


def run_op_cases():
    import torch

    from min_tfs_client_amd import ops

    dev = "cuda:0"
    native = ops.require_native()
    for B, C, k in OP_CASES:
        for dtype_name in OP_DTYPES:
            dtype = getattr(torch, dtype_name)
            g = torch.Generator().manual_seed(0)
            x = (torch.randn((B, C), generator=g) * 4).to(dtype).to(dev)
            nbytes = x.numel() * x.element_size() + B * k * 8
            reps = 300 if C <= 1000 else 50

            def op():
                return ops.softmax_topk(x, k)

            def bare():
                return native.softmax_topk(x, k)

            def eager():
                return torch.softmax(x.float(), 1).topk(k)

            scores, classes = op()
            e_scores, e_classes = eager()
            rounds = [(time_kernel(bare, reps, 10), time_kernel(op, reps, 10),
                       time_kernel(eager, reps, 10)) for _ in range(5)]
            ms_bare, ms_op, ms_eager = (
                sorted(r[i] for r in rounds)[2] for i in range(3))
            print(json.dumps({
                "case": f"{B}x{C}_k{k}_{dtype_name}",
                "native_ms": round(ms_bare, 4), "op_ms": round(ms_op, 4),
                "eager_ms": round(ms_eager, 4),
                "eager_over_op": round(ms_eager / ms_op, 2),
                "bytes": nbytes,
                "native_GB_s": round(nbytes / 1e9 / (ms_bare / 1e3), 2),
                "max_abs_score_diff_vs_eager":
                    (scores - e_scores).abs().max().item(),
                "rows_with_other_classes_than_eager": int(
                    (classes.long() != e_classes).any(1).sum().item())}),
                flush=True)


def run_predict_mode(mode, batch=8, steps=100, warmup=20):
    import tempfile

    import torch

    from min_tfs_client_amd.models import resnet50_servable
    from min_tfs_client_amd.server import ModelServer
    from min_tfs_client_amd.turbo import TurboPredictClient

    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    inputs = {"images": torch.randn(batch, 3, 224, 224, generator=g)}
    with tempfile.TemporaryDirectory() as tmp:
        sock = f"unix://{tmp}/bench_topk.sock"
        with ModelServer(address=sock, raw_predict=True, device=dev) as srv:
            srv.manager.load(
                "resnet", resnet50_servable(dev, torch.bfloat16,
                                            output_format=mode), version=1)
            with TurboPredictClient(sock) as client:
                lat = []
                for i in range(warmup + steps):
                    t0 = time.perf_counter()
                    out = client.predict("resnet", inputs)
                    if i >= warmup:
                        lat.append((time.perf_counter() - t0) * 1e3)
    lat.sort()
    print(json.dumps({
        "predict_mode": mode, "batch": batch, "steps": steps,
        "p50_ms": round(lat[len(lat) // 2], 3),
        "p99_ms": round(lat[int(len(lat) * 0.99) - 1], 3),
        "outputs": {k: [str(v.dtype), list(v.shape)]
                    for k, v in out.items()},
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
                    help="also run ResNet Predict in both output modes")
    ap.add_argument("--only-predict", action="store_true")
    ap.add_argument("--op-cases", action="store_true",
                    help="(child) run the op timing cases")
    ap.add_argument("--predict-mode", choices=PREDICT_MODES,
                    help="(child) run one Predict mode")
    a = ap.parse_args()
    if a.op_cases:
        return run_op_cases()
    if a.predict_mode:
        return run_predict_mode(a.predict_mode)
    if not a.only_predict:
        run_step(["--op-cases"])
    if a.predict or a.only_predict:
        for mode in PREDICT_MODES:
            run_step(["--predict-mode", mode])


if __name__ == "__main__":
    main()
