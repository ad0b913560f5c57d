#!/usr/bin/env python3
"""Fused YUV 4:2:0 ingest against the RGB kernel and the two-step path, one
GPU.

    python tools/bench_yuv.py             # kernel/op timings, JSON lines
    python tools/bench_yuv.py --predict   # + ResNet-50 Predict p50
    python tools/bench_yuv.py --antialias # the antialiased op instead

The parent process never touches the GPU. Every step (one case of the op
timings, the Predict comparison) runs in a fresh child process under its own
time limit, and the tool exits non-zero on the first step that fails or
times out.

Op timings, on uint8 frames (N,256,342) stored [N,384,342] (the (256,341)
photo of the other tools, with the even width 4:2:0 needs) -> 224 centre
crop of the frame at its own size, NCHW:

* "yuv": ``ops.image_yuv420_resize_to_float``, one launch, taps from LDS;
* "yuv_direct": the same native call with the direct-gather path forced;
* "rgb": the existing RGB kernel (``ops.image_u8_resize_to_float``) on the
  already converted [N,256,342,3] tensor, which reads twice the bytes;
* "two_step": ``ops.yuv420_to_rgb_u8`` on the device (torch integer ops)
  followed by the RGB kernel, what a server without the fused kernel runs.

All four give the same bits (asserted). Device-event timing, warm-up then
interleaved rounds in one process; the median round is reported with the
range over rounds. GB/s counts the bytes that must move: the input read once
plus the output written once.

``--antialias`` times ``ops.image_yuv420_resize_to_float(...,
antialias=True)``, u8 -> bf16 NCHW, NV12, in the same way: "yuv" (taps from
LDS) and "yuv_direct" against "rgb", the antialiased RGB op alone on the
already converted tensor, and "two_step", ``ops.yuv420_to_rgb_u8`` on the
device followed by the antialiased RGB op. Shapes: (32,1080,1920) and
(1,1080,1920) frames -> (256,455) with the 224 centre crop, and (32,256,342)
-> (128,170). All four give the same bits (asserted).

Predict p50: ``resnet50_servable("cuda:0", bf16)`` in ``nv12_resize`` mode
with (32,384,342) frames and in ``uint8_nhwc_resize`` mode with the
converted (32,256,342,3) pixels, one raw-Predict server on a unix socket,
one ``TurboPredictClient``, host tensors in and host logits out, 10 warm-up
then 5 interleaved rounds x 20 requests per mode. Both modes hand the model
the same bits (tests/gpu/test_gpu_image_yuv420.py); the logits are not
compared here, since the model's convolutions are not bit-reproducible from
call to call at their default, fastest settings.
"""
import argparse
import json
import os
import subprocess
import sys
import time

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)

HIN, WIN = 256, 342
CENTER_224 = ((HIN - 224) // 2, (WIN - 224) // 2, 224, 224)
# name -> (N, chroma, out dtype)
OP_CASES = {}
for _n in (1, 32, 256):
    for _dt, _short in (("float32", "f32"), ("bfloat16", "bf16")):
        OP_CASES[f"n{_n}_nv12_crop224_{_short}"] = (_n, "nv12", _dt)
OP_CASES["n32_i420_crop224_bf16"] = (32, "i420", "bfloat16")
OP_CASES["n256_i420_crop224_bf16"] = (256, "i420", "bfloat16")
# name -> (N, H, W, resized size, crop)
AA_CASES = {
    "aa_n32_1080p_256x455_crop224": (32, 1080, 1920, (256, 455),
                                     (16, 115, 224, 224)),
    "aa_n1_1080p_256x455_crop224": (1, 1080, 1920, (256, 455),
                                    (16, 115, 224, 224)),
    "aa_n32_256x342_128x170": (32, 256, 342, (128, 170), None),
}
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


def _frames(n, seed=0, h=HIN, w=WIN):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h * 3 // 2, w), dtype=torch.uint8,
                         generator=g)


def run_op_case(name):
    import torch

    from min_tfs_client_amd import ops
    from min_tfs_client_amd.preprocess import IMAGENET_MEAN, IMAGENET_STD

    N, chroma, dtype_name = OP_CASES[name]
    dtype = getattr(torch, dtype_name)
    dev = "cuda:0"
    ops.require_native()
    x = _frames(N).to(dev)
    rgb_dev = ops.yuv420_to_rgb_u8(x, chroma)
    size, crop = (HIN, WIN), CENTER_224
    reps = 100 if N > 1 else 300

    def yuv(variant=0):
        return ops.image_yuv420_resize_to_float(
            x, size, IMAGENET_MEAN, IMAGENET_STD, crop=crop, out_dtype=dtype,
            _variant=variant, chroma=chroma)

    def rgb():
        return ops.image_u8_resize_to_float(
            rgb_dev, size, IMAGENET_MEAN, IMAGENET_STD, crop=crop,
            out_dtype=dtype)

    def two_step():
        return ops.image_u8_resize_to_float(
            ops.yuv420_to_rgb_u8(x, chroma), size, IMAGENET_MEAN,
            IMAGENET_STD, crop=crop, out_dtype=dtype)

    want = rgb()
    assert torch.equal(yuv(), want) and torch.equal(yuv(1), want)
    assert torch.equal(two_step(), want)
    fns = {"yuv": yuv, "yuv_direct": lambda: yuv(1), "rgb": rgb,
           "two_step": two_step}
    rounds = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            rounds[k].append(time_kernel(fn, reps, 10))
    stats = {k: _stats(v) for k, v in rounds.items()}
    out_bytes = want.numel() * want.element_size()
    row = {"case": name, "frames": [N, HIN, WIN], "chroma": chroma,
           "crop": list(crop), "out": dtype_name,
           "yuv_bytes": x.numel() + out_bytes,
           "rgb_bytes": rgb_dev.numel() + out_bytes}
    for k, st in stats.items():
        row[f"{k}_us"] = round(st["median"] * 1e3, 2)
        row[f"{k}_us_range"] = [round(st["min"] * 1e3, 2),
                                round(st["max"] * 1e3, 2)]
    row["yuv_GB_s"] = round(
        row["yuv_bytes"] / 1e9 / (stats["yuv"]["median"] / 1e3), 1)
    row["rgb_GB_s"] = round(
        row["rgb_bytes"] / 1e9 / (stats["rgb"]["median"] / 1e3), 1)
    row["two_step_over_yuv"] = round(
        stats["two_step"]["median"] / stats["yuv"]["median"], 2)
    row["yuv_over_rgb"] = round(
        stats["yuv"]["median"] / stats["rgb"]["median"], 2)
    print(json.dumps(row), flush=True)


def run_aa_case(name):
    import torch

    from min_tfs_client_amd import ops
    from min_tfs_client_amd.preprocess import IMAGENET_MEAN, IMAGENET_STD

    N, H, W, size, crop = AA_CASES[name]
    dtype, chroma, dev = torch.bfloat16, "nv12", "cuda:0"
    ops.require_native()
    x = _frames(N, h=H, w=W).to(dev)
    rgb_dev = ops.yuv420_to_rgb_u8(x, chroma)
    reps = 50 if N > 1 else 200

    def yuv(variant=0):
        return ops.image_yuv420_resize_to_float(
            x, size, IMAGENET_MEAN, IMAGENET_STD, crop=crop, out_dtype=dtype,
            _variant=variant, chroma=chroma, antialias=True)

    def rgb():
        return ops.image_u8_resize_to_float(
            rgb_dev, size, IMAGENET_MEAN, IMAGENET_STD, crop=crop,
            out_dtype=dtype, antialias=True)

    def two_step():
        return ops.image_u8_resize_to_float(
            ops.yuv420_to_rgb_u8(x, chroma), size, IMAGENET_MEAN,
            IMAGENET_STD, crop=crop, out_dtype=dtype, antialias=True)

    want = rgb()
    assert torch.equal(yuv(), want) and torch.equal(yuv(1), want)
    assert torch.equal(two_step(), want)
    fns = {"yuv": yuv, "yuv_direct": lambda: yuv(1), "rgb": rgb,
           "two_step": two_step}
    rounds = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            rounds[k].append(time_kernel(fn, reps, 5))
    stats = {k: _stats(v) for k, v in rounds.items()}
    row = {"case": name, "frames": [N, H, W], "chroma": chroma,
           "size": list(size), "crop": list(crop) if crop else None,
           "out": "bfloat16", "antialias": True}
    for k, st in stats.items():
        row[f"{k}_us"] = round(st["median"] * 1e3, 2)
        row[f"{k}_us_range"] = [round(st["min"] * 1e3, 2),
                                round(st["max"] * 1e3, 2)]
    row["direct_over_yuv"] = round(
        stats["yuv_direct"]["median"] / stats["yuv"]["median"], 2)
    row["two_step_over_yuv"] = round(
        stats["two_step"]["median"] / stats["yuv"]["median"], 2)
    row["yuv_over_rgb"] = round(
        stats["yuv"]["median"] / stats["rgb"]["median"], 2)
    print(json.dumps(row), flush=True)


def run_predict(batch=32, warmup=10, rounds=5, per_round=20):
    import tempfile

    import torch

    from min_tfs_client_amd import ops
    from min_tfs_client_amd.models import resnet50_servable
    from min_tfs_client_amd.server import ModelServer
    from min_tfs_client_amd.turbo import TurboPredictClient

    dev = "cuda:0"
    frames = _frames(batch)
    modes = {"nv12_resize": frames,
             "uint8_nhwc_resize": ops.yuv420_to_rgb_u8(frames, "nv12")}
    lat = {m: [] for m in modes}
    with tempfile.TemporaryDirectory() as tmp:
        sock = f"unix://{tmp}/bench_yuv.sock"
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
                    help="also time ResNet-50 Predict, NV12 against RGB")
    ap.add_argument("--only-predict", action="store_true")
    ap.add_argument("--antialias", action="store_true",
                    help="time the antialiased op on its own shapes instead")
    ap.add_argument("--aa-case", choices=sorted(AA_CASES),
                    help="(child) run one antialiased op timing case")
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
