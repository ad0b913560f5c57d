#!/usr/bin/env python3
"""Fused resize + crop image ingest against the eager chain, one GPU.

    python tools/bench_resize.py             # kernel/op timings, JSON lines
    python tools/bench_resize.py --predict   # + ResNet-50 Predict p50
    python tools/bench_resize.py --antialias # antialiased op timings instead

The parent process never touches the GPU. Every step (one case of the op
timings, the Predict comparison) runs in a fresh child process under its own
time limit, and the tool exits non-zero on the first step that fails or
times out.

Op timings: ``ops.image_u8_resize_to_float`` (public op), the bare native
call with its tap path chosen per tile ("lds"), the bare native call with
the direct-gather path forced ("direct"), and the eager chain on the same
device

    x.permute(0,3,1,2).float() -> F.interpolate(bilinear, antialias=False)
      -> slice -> * scale + bias -> .to(out_dtype).contiguous()

Device-event timing, warm-up then interleaved rounds in one process; the
median round is reported with the range over rounds. GB/s counts the bytes
that must move: the uint8 input read once plus the output written once.
The eager chain differs from the op by rounding only; the largest
difference is printed.

``--antialias`` times the antialiased path instead, at u8 (N,1080,1920,3)
photos -> short side 256 -> 224 centre crop and at the (N,256,341,3) points
above, N in {1, 32}: ``ops.image_u8_resize_to_float(antialias=True)``
("aa"), the eager device chain it replaces ("eager_aa": the chain above with
``antialias=True``) and the existing non-antialiased kernel ("bilinear"),
measured the same way.

Predict p50: ``resnet50_servable("cuda:0", bf16)`` in ``uint8_nhwc`` mode
with (32,224,224,3) input and in ``uint8_nhwc_resize`` mode with
(32,256,341,3) input, one raw-Predict server on a unix socket, one
``TurboPredictClient``, host tensors in and host logits out, 10 warm-up then
5 interleaved rounds x 20 requests per mode.
"""
import argparse
import json
import os
import subprocess
import sys
import time

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)

# name -> (N, size, crop, out dtype); the input is always (N,256,341,3)
HIN, WIN = 256, 341
CENTER_224 = ((256 - 224) // 2, (341 - 224) // 2, 224, 224)
OP_CASES = {}
for _n in (1, 32, 256):
    for _dt in ("float32", "bfloat16"):
        _short = "f32" if _dt == "float32" else "bf16"
        OP_CASES[f"n{_n}_full_{_short}"] = (_n, (HIN, WIN), None, _dt)
        OP_CASES[f"n{_n}_crop224_{_short}"] = (_n, (HIN, WIN), CENTER_224,
                                               _dt)
OP_CASES["n32_half_bf16"] = (32, (HIN // 2, WIN // 2), None, "bfloat16")
OP_CASES["n32_half_crop112_bf16"] = (
    32, (HIN // 2, WIN // 2), ((128 - 112) // 2, (170 - 112) // 2, 112, 112),
    "bfloat16")
# antialiased cases: name -> (N, input (H, W), size, crop, out dtype)
PHOTO = (1080, 1920)
PHOTO_SIZE = (256, 256 * 1920 // 1080)                 # short side 256
PHOTO_CROP = ((256 - 224) // 2, (PHOTO_SIZE[1] - 224) // 2, 224, 224)
AA_CASES = {}
for _n in (1, 32):
    AA_CASES[f"aa_n{_n}_photo_crop224_bf16"] = (
        _n, PHOTO, PHOTO_SIZE, PHOTO_CROP, "bfloat16")
    AA_CASES[f"aa_n{_n}_crop224_bf16"] = (
        _n, (HIN, WIN), (HIN, WIN), CENTER_224, "bfloat16")
AA_CASES["aa_n32_photo_crop224_f32"] = (
    32, PHOTO, PHOTO_SIZE, PHOTO_CROP, "float32")
AA_CASES["aa_n32_half_bf16"] = (
    32, (HIN, WIN), (HIN // 2, WIN // 2), None, "bfloat16")
STEP_TIMEOUT_S = 240
ROUNDS = 5


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


def _stats(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def run_op_case(name):
    import numpy as np
    import torch
    import torch.nn.functional as F

    from min_tfs_client_amd import ops
    from min_tfs_client_amd.preprocess import IMAGENET_MEAN, IMAGENET_STD

    N, size, crop, dtype_name = OP_CASES[name]
    dtype = getattr(torch, dtype_name)
    dev = "cuda:0"
    native = ops.require_native()
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (N, HIN, WIN, 3), dtype=torch.uint8,
                      generator=g).to(dev)
    top, left, hc, wc = crop if crop else (0, 0) + tuple(size)
    scale, bias = ops.normalization_constants(IMAGENET_MEAN, IMAGENET_STD)
    s_dev = torch.tensor(scale, device=dev).view(1, 3, 1, 1)
    b_dev = torch.tensor(bias, device=dev).view(1, 3, 1, 1)
    rh = float(np.float32(HIN / size[0]))
    rw = float(np.float32(WIN / size[1]))
    reps = 100 if N > 1 else 300

    def op():
        return ops.image_u8_resize_to_float(
            x, size, IMAGENET_MEAN, IMAGENET_STD, crop=crop, out_dtype=dtype)

    def bare(variant):
        return native.u8_nhwc_resize_normalize(
            x, rh, rw, top, left, hc, wc, scale, bias, dtype, True, variant)

    def eager():
        y = F.interpolate(x.permute(0, 3, 1, 2).float(), size=size,
                          mode="bilinear", align_corners=False,
                          antialias=False)
        y = y[:, :, top:top + hc, left:left + wc]
        return (y * s_dev + b_dev).to(dtype).contiguous()

    assert torch.equal(op(), bare(0)) and torch.equal(op(), bare(1))
    err = (op().float() - eager().float()).abs().max().item()
    fns = {"lds": lambda: bare(0), "direct": lambda: bare(1), "op": op,
           "eager": eager}
    rounds = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            rounds[k].append(time_kernel(fn, reps, 10))
    stats = {k: _stats(v) for k, v in rounds.items()}
    nbytes = x.numel() + N * 3 * hc * wc * torch.empty((), dtype=dtype
                                                       ).element_size()
    row = {"case": name, "input": [N, HIN, WIN, 3], "size": list(size),
           "crop": list(crop) if crop else None, "out": dtype_name,
           "bytes": nbytes, "max_abs_diff_vs_eager": err}
    for k, st in stats.items():
        row[f"{k}_us"] = round(st["median"] * 1e3, 2)
        row[f"{k}_us_range"] = [round(st["min"] * 1e3, 2),
                                round(st["max"] * 1e3, 2)]
    row["lds_GB_s"] = round(nbytes / 1e9 / (stats["lds"]["median"] / 1e3), 1)
    row["direct_GB_s"] = round(
        nbytes / 1e9 / (stats["direct"]["median"] / 1e3), 1)
    row["eager_over_op"] = round(
        stats["eager"]["median"] / stats["op"]["median"], 2)
    print(json.dumps(row), flush=True)


def run_aa_case(name):
    import torch
    import torch.nn.functional as F

    from min_tfs_client_amd import ops
    from min_tfs_client_amd.preprocess import IMAGENET_MEAN, IMAGENET_STD

    N, (hin, win), size, crop, dtype_name = AA_CASES[name]
    dtype = getattr(torch, dtype_name)
    dev = "cuda:0"
    ops.require_native()
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (N, hin, win, 3), dtype=torch.uint8,
                      generator=g).to(dev)
    top, left, hc, wc = crop if crop else (0, 0) + tuple(size)
    scale, bias = ops.normalization_constants(IMAGENET_MEAN, IMAGENET_STD)
    s_dev = torch.tensor(scale, device=dev).view(1, 3, 1, 1)
    b_dev = torch.tensor(bias, device=dev).view(1, 3, 1, 1)
    reps = 50 if N > 1 else 200

    def aa():
        return ops.image_u8_resize_to_float(
            x, size, IMAGENET_MEAN, IMAGENET_STD, crop=crop, out_dtype=dtype,
            antialias=True)

    def bilinear():
        return ops.image_u8_resize_to_float(
            x, size, IMAGENET_MEAN, IMAGENET_STD, crop=crop, out_dtype=dtype)

    def eager_aa():
        y = F.interpolate(x.permute(0, 3, 1, 2).float(), size=size,
                          mode="bilinear", align_corners=False,
                          antialias=True)
        y = y[:, :, top:top + hc, left:left + wc]
        return (y * s_dev + b_dev).to(dtype).contiguous()

    err = (aa().float() - eager_aa().float()).abs().max().item()
    fns = {"aa": aa, "eager_aa": eager_aa, "bilinear": bilinear}
    rounds = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            rounds[k].append(time_kernel(fn, reps, 5))
    stats = {k: _stats(v) for k, v in rounds.items()}
    nbytes = x.numel() + N * 3 * hc * wc * torch.empty((), dtype=dtype
                                                       ).element_size()
    row = {"case": name, "input": [N, hin, win, 3], "size": list(size),
           "crop": list(crop) if crop else None, "out": dtype_name,
           "bytes": nbytes, "max_abs_diff_vs_eager_aa": err}
    for k, st in stats.items():
        row[f"{k}_us"] = round(st["median"] * 1e3, 2)
        row[f"{k}_us_range"] = [round(st["min"] * 1e3, 2),
                                round(st["max"] * 1e3, 2)]
    row["eager_aa_over_aa"] = round(
        stats["eager_aa"]["median"] / stats["aa"]["median"], 2)
    row["aa_over_bilinear"] = round(
        stats["aa"]["median"] / stats["bilinear"]["median"], 2)
    print(json.dumps(row), flush=True)


def run_predict(batch=32, warmup=10, rounds=5, per_round=20):
    import tempfile

    import torch

    from min_tfs_client_amd.models import resnet50_servable
    from min_tfs_client_amd.server import ModelServer
    from min_tfs_client_amd.turbo import TurboPredictClient

    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    modes = {
        "uint8_nhwc": torch.randint(0, 256, (batch, 224, 224, 3),
                                    dtype=torch.uint8, generator=g),
        "uint8_nhwc_resize": torch.randint(0, 256, (batch, HIN, WIN, 3),
                                           dtype=torch.uint8, generator=g),
    }
    lat = {m: [] for m in modes}
    with tempfile.TemporaryDirectory() as tmp:
        sock = f"unix://{tmp}/bench_resize.sock"
        with ModelServer(address=sock, raw_predict=True, device=dev) as srv:
            for m in modes:
                srv.manager.load(
                    m, resnet50_servable(dev, torch.bfloat16, input_format=m),
                    version=1)
            with TurboPredictClient(sock) as client:
                for m, x in modes.items():
                    for _ in range(warmup):
                        client.predict(m, {"images": x})
                for _ in range(rounds):
                    for m, x in modes.items():
                        for _ in range(per_round):
                            t0 = time.perf_counter()
                            out = client.predict(m, {"images": x})
                            lat[m].append((time.perf_counter() - t0) * 1e3)
                        assert tuple(out["logits"].shape) == (batch, 1000)
    for m, x in modes.items():
        v = sorted(lat[m])
        print(json.dumps({
            "predict_mode": m, "input": list(x.shape),
            "request_bytes": x.numel(), "requests": len(v),
            "p50_ms": round(v[len(v) // 2], 3), "min_ms": round(v[0], 3),
            "p90_ms": round(v[int(len(v) * 0.9) - 1], 3)}), flush=True)


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
                    help="also time ResNet-50 Predict in both uint8 modes")
    ap.add_argument("--only-predict", action="store_true")
    ap.add_argument("--antialias", action="store_true",
                    help="time the antialiased path (and nothing else)")
    ap.add_argument("--aa-case", choices=sorted(AA_CASES),
                    help="(child) run one antialiased timing case")
    ap.add_argument("--cases", nargs="*", choices=sorted(OP_CASES),
                    help="run only these op timing cases")
    ap.add_argument("--op-case", choices=sorted(OP_CASES),
                    help="(child) run one op timing case")
    ap.add_argument("--predict-child", action="store_true",
                    help="(child) run the Predict comparison")
    a = ap.parse_args()
    if a.op_case:
        return run_op_case(a.op_case)
    if a.aa_case:
        return run_aa_case(a.aa_case)
    if a.predict_child:
        return run_predict()
    if a.antialias:
        for name in AA_CASES:
            run_step(["--aa-case", name])
        return
    if not a.only_predict:
        for name in (a.cases or OP_CASES):
            run_step(["--op-case", name])
    if a.predict or a.only_predict:
        run_step(["--predict-child"])


if __name__ == "__main__":
    main()
