#!/usr/bin/env python3
"""Ragged uint8 image batches (N photos of N sizes, one launch) against the
per-image loop of dense calls they replace, one GPU.

    python tools/bench_ragged.py             # op timings, JSON lines
    python tools/bench_ragged.py --predict   # + ResNet-50 Predict comparison
    python tools/bench_ragged.py --antialias # op timings, antialiased filter

The parent process never touches the GPU. Every step (one N of the op
timings, the Predict comparison) runs in a fresh child process under its own
time limit, and the tool exits non-zero on the first step that fails or
times out.

Op timings, u8 -> bf16 NCHW, short side 256 then the 224 centre crop, N in
{1, 32}; the photos have seeded mixed sizes, H in 256..512 and W in 341..683:

* ``ragged``: ``ops.image_u8_ragged_resize_to_float`` on the packed photos,
  shapes given on the host. This is the whole op: argument checks, the
  per-image table built on the host, its pinned copy, one launch.
* ``ragged_kernel``: the bare native call on a table that is already on the
  device, i.e. ``ragged`` without the host-side table work.
* ``ragged_dev_shapes``: ``ragged`` with ``shapes`` as a device tensor, which
  adds the synchronizing D2H copy of the shapes.
* ``loop``: the reference the op replaces: a Python loop of N dense
  ``ops.image_u8_resize_to_float`` calls, one per photo, plus ``torch.cat``.
* ``dense``: the dense op on N images of ONE size (384,512), and
  ``ragged_same``: the ragged op on the same N images, to show what the
  per-image table costs when it is not needed.

``ragged`` and ``loop`` are checked for equality first. Device-event timing,
warm-up then interleaved rounds in one process; the median round is reported
with the range over rounds. ``host_us`` is the host clock per ``ragged``
call without a device wait (what the calling thread spends).

``--antialias`` times the same set with ``antialias=True`` everywhere (rows
are tagged ``"antialias": true``): ``ragged`` is the whole antialiased op,
``ragged_kernel`` the native entry on a pre-built HOST table (the entry
derives the row ranges and ships its own device table, so that work is
inside the number), ``loop`` the N dense antialiased calls plus ``torch.cat``
the op replaces, ``dense`` the dense antialiased kernels on N images of one
size.

``--predict``: ``resnet50_servable("cuda:0", bf16)`` on one raw-Predict
server on a unix socket, one ``TurboPredictClient``, host tensors in and
host logits out: one ``uint8_ragged`` Predict of the 32 mixed photos against
32 single-image ``uint8_nhwc_resize`` Predicts of the same photos, 5 warm-up
then 5 interleaved rounds x 10 repetitions; the time is for all 32 images.
"""
import argparse
import json
import os
import subprocess
import sys
import time

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)

OP_NS = (1, 32)
SAME_SIZE = (384, 512)
STEP_TIMEOUT_S = 240
ROUNDS = 5


def photo_shapes(n, seed=0):
    import numpy as np

    rng = np.random.RandomState(seed)
    return [(int(rng.randint(256, 513)), int(rng.randint(341, 684)))
            for _ in range(n)]


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


def time_host(fn, reps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return dt / reps * 1e3  # ms


def _stats(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def run_op_case(n, antialias=False):
    import numpy as np
    import torch

    from min_tfs_client_amd import ops
    from min_tfs_client_amd.preprocess import (IMAGENET_MEAN, IMAGENET_STD,
                                               ImagePreprocess)

    dev = "cuda:0"
    dtype = torch.bfloat16
    native = ops.require_native()
    rule = ImagePreprocess(IMAGENET_MEAN, IMAGENET_STD, resize=256,
                           center_crop=224)
    g = torch.Generator().manual_seed(0)

    def make(shapes):
        images = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8,
                                generator=g).to(dev) for h, w in shapes]
        sizes = [rule.resized_size(h, w) for h, w in shapes]
        origins = [rule.crop_window(*s)[:2] for s in sizes]
        flat = torch.cat([im.reshape(-1) for im in images])
        return images, flat, np.array(sizes), np.array(origins)

    shapes = photo_shapes(n)
    images, flat, sizes, origins = make(shapes)
    batched = [im.unsqueeze(0) for im in images]
    shapes_np = np.array(shapes, dtype=np.int32)
    shapes_dev = torch.from_numpy(shapes_np).to(dev)
    same_shapes = [SAME_SIZE] * n
    _, same_flat, same_sizes, same_origins = make(same_shapes)
    same_x = same_flat.view(n, SAME_SIZE[0], SAME_SIZE[1], 3)
    same_np = np.array(same_shapes, dtype=np.int32)
    scale, bias = ops.normalization_constants(IMAGENET_MEAN, IMAGENET_STD)

    def ragged(s=shapes_np):
        return ops.image_u8_ragged_resize_to_float(
            flat, s, sizes, (224, 224), IMAGENET_MEAN, IMAGENET_STD,
            origins=origins, out_dtype=dtype, antialias=antialias)

    # the table exactly as the op builds it, kept on the device
    offsets = np.zeros(n, dtype=np.int64)
    np.cumsum((shapes_np[:-1, 0].astype(np.int64) * shapes_np[:-1, 1] * 3),
              out=offsets[1:])
    t = np.zeros((n, 8), dtype=np.int32)
    t[:, 0:2] = offsets.astype("<i8").view("<i4").reshape(n, 2)
    t[:, 2:4] = shapes_np
    t[:, 4:6] = origins
    t[:, 6:8] = (shapes_np.astype(np.int64) / sizes).astype(
        np.float32).view(np.int32)
    table_host = torch.from_numpy(t)
    table_dev = table_host.to(dev)

    def ragged_kernel():
        if antialias:
            return native.u8_ragged_resize_aa_normalize(
                flat, table_host, 3, 224, 224, scale, bias, dtype, True)
        return native.u8_ragged_resize_normalize(
            flat, table_dev, 3, 224, 224, scale, bias, dtype, True)

    def loop():
        return torch.cat([ops.image_u8_resize_to_float(
            x, tuple(int(v) for v in sizes[i]), IMAGENET_MEAN, IMAGENET_STD,
            crop=(int(origins[i][0]), int(origins[i][1]), 224, 224),
            out_dtype=dtype, antialias=antialias)
            for i, x in enumerate(batched)])

    def dense():
        return ops.image_u8_resize_to_float(
            same_x, tuple(int(v) for v in same_sizes[0]), IMAGENET_MEAN,
            IMAGENET_STD,
            crop=(int(same_origins[0][0]), int(same_origins[0][1]), 224, 224),
            out_dtype=dtype, antialias=antialias)

    def ragged_same():
        return ops.image_u8_ragged_resize_to_float(
            same_flat, same_np, same_sizes, (224, 224), IMAGENET_MEAN,
            IMAGENET_STD, origins=same_origins, out_dtype=dtype,
            antialias=antialias)

    assert torch.equal(ragged(), loop())
    assert torch.equal(ragged(), ragged_kernel())
    assert torch.equal(ragged(shapes_dev), loop())
    assert torch.equal(ragged_same(), dense())
    fns = {"ragged": ragged, "ragged_kernel": ragged_kernel,
           "ragged_dev_shapes": lambda: ragged(shapes_dev), "loop": loop,
           "dense": dense, "ragged_same": ragged_same}
    reps = 100 if n > 1 else 300
    rounds = {k: [] for k in fns}
    host = []
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            rounds[k].append(time_kernel(fn, reps, 10))
        host.append(time_host(ragged, reps))
    row = {"case": f"n{n}", "antialias": antialias, "images": n,
           "input_bytes": flat.numel(),
           "out": "bfloat16", "crop": 224,
           "shapes": shapes if n <= 4 else shapes[:4] + ["..."]}
    for k, v in rounds.items():
        st = _stats(v)
        row[f"{k}_us"] = round(st["median"] * 1e3, 2)
        row[f"{k}_us_range"] = [round(st["min"] * 1e3, 2),
                                round(st["max"] * 1e3, 2)]
    st = _stats(host)
    row["host_us"] = round(st["median"] * 1e3, 2)
    row["host_us_range"] = [round(st["min"] * 1e3, 2),
                            round(st["max"] * 1e3, 2)]
    row["loop_over_ragged"] = round(row["loop_us"] / row["ragged_us"], 2)
    row["ragged_same_over_dense"] = round(
        row["ragged_same_us"] / row["dense_us"], 2)
    print(json.dumps(row), flush=True)


def run_predict(batch=32, warmup=5, rounds=5, per_round=10):
    import tempfile

    import torch

    from min_tfs_client_amd.models import resnet50_servable
    from min_tfs_client_amd.preprocess import pack_ragged_images
    from min_tfs_client_amd.server import ModelServer
    from min_tfs_client_amd.turbo import TurboPredictClient

    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    images = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8,
                            generator=g) for h, w in photo_shapes(batch)]
    data, shapes = pack_ragged_images([im.numpy() for im in images])
    ragged_inputs = {"images": torch.from_numpy(data),
                     "image_shapes": torch.from_numpy(shapes)}
    singles = [im.unsqueeze(0).contiguous() for im in images]
    lat = {"uint8_ragged": [], "uint8_nhwc_resize": []}
    with tempfile.TemporaryDirectory() as tmp:
        sock = f"unix://{tmp}/bench_ragged.sock"
        with ModelServer(address=sock, raw_predict=True, device=dev) as srv:
            for m in lat:
                srv.manager.load(
                    m, resnet50_servable(dev, torch.bfloat16, input_format=m),
                    version=1)
            with TurboPredictClient(sock) as client:
                def one_ragged():
                    out = client.predict("uint8_ragged", ragged_inputs)
                    assert tuple(out["logits"].shape) == (batch, 1000)

                def all_singles():
                    for x in singles:
                        out = client.predict("uint8_nhwc_resize",
                                             {"images": x})
                    assert tuple(out["logits"].shape) == (1, 1000)

                modes = {"uint8_ragged": one_ragged,
                         "uint8_nhwc_resize": all_singles}
                for fn in modes.values():
                    for _ in range(warmup):
                        fn()
                for _ in range(rounds):
                    for m, fn in modes.items():
                        for _ in range(per_round):
                            t0 = time.perf_counter()
                            fn()
                            lat[m].append((time.perf_counter() - t0) * 1e3)
    for m, v in lat.items():
        v = sorted(v)
        print(json.dumps({
            "predict_mode": m, "images": batch,
            "requests_per_repetition": 1 if m == "uint8_ragged" else batch,
            "request_bytes_total": int(data.size), "repetitions": len(v),
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
                    help="also compare one ragged Predict of 32 images with "
                         "32 single-image Predicts")
    ap.add_argument("--only-predict", action="store_true")
    ap.add_argument("--antialias", action="store_true",
                    help="time the antialiased ragged op against the loop of "
                         "dense antialiased calls and the dense kernels")
    ap.add_argument("--op-case", type=int, choices=OP_NS,
                    help="(child) run the op timings at this N")
    ap.add_argument("--predict-child", action="store_true",
                    help="(child) run the Predict comparison")
    a = ap.parse_args()
    if a.op_case:
        return run_op_case(a.op_case, a.antialias)
    if a.predict_child:
        return run_predict()
    if not a.only_predict:
        for n in OP_NS:
            run_step(["--op-case", str(n)] +
                     (["--antialias"] if a.antialias else []))
    if a.predict or a.only_predict:
        run_step(["--predict-child"])


if __name__ == "__main__":
    main()
