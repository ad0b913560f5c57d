#!/usr/bin/env python3
"""ViT patch embedding from uint8 pixels: the fused MFMA kernel against the
composed chain a user would run without it, one GPU.

    python tools/bench_patch_embed.py          # JSON lines
    python tools/bench_patch_embed.py --yuv    # NV12 / I420 input, see below
    python tools/bench_patch_embed.py --resize # resize + crop input, see below
    python tools/bench_patch_embed.py --ragged # mixed sizes, one launch

The parent process never touches the GPU; the timings run in one fresh child
process under a time limit, and the tool exits non-zero if it fails.

Fused: ``ops.image_u8_patch_embed`` (one launch). Baseline, four passes:

    ImagePreprocess (u8 NHWC -> normalized NCHW, model dtype)
    -> F.conv2d(P x P, stride P) -> flatten/transpose
    -> cat class token -> + pos_embed

ViT-B/16 shapes: 224x224, D = 768, batch 1, 8, 32 and 128, model dtype bf16
and fp32 (the fused projection is bf16 x bf16 -> fp32 in both; the baseline
convolves in the model dtype). Interleaved rounds in one process, the median
round is reported. ``fused_GB_s`` counts the bytes the fused op must move:
pixels in, tokens out, weights once (15.7 MB for 32 images in bf16, 1.2 MB
of it weights).
``max_abs_diff`` against the baseline is reported, not asserted: the
baseline rounds the normalized pixel and the weights differently.

``--yuv``: ``ops.image_yuv420_patch_embed`` on NV12 and I420 frames, bf16
output, the same shapes and batches, per tile (rule, small, large):

    (a) ``yuv_*_ms``       the fused YUV op
    (b) ``rgb_*_ms``       the RGB kernel on an already converted tensor, the
                           floor: (a)/(b) is the cost of converting inside
    (c) ``two_step_*_ms``  what a user runs without it: ``yuv420_to_rgb_u8``
                           on the device, then the RGB kernel

with the ratios (a)/(b) and (c)/(a), and ``identical``: whether (a) and (c)
gave the same bits.

``--resize``: ``ops.image_u8_resize_patch_embed`` (shorter side to 256,
centre crop 224) from 480x640 and 1080x1920 images, batch 1, 8 and 32, bf16
and fp32, per tile, against ``two_step_ms``, what a user runs without it:
``ops.image_u8_resize_to_float`` then ``VisionTransformer.embed``. The
224x224 rows are the identity-size call against ``image_u8_patch_embed``
(``rgb_*_ms``): the cost of the second MFMA piece and the bf16 tile.
``max_over_min_round`` is the largest spread of one timing over the rounds.

``--ragged``: ``ops.image_u8_ragged_resize_patch_embed`` on N = 1, 8 and 32
seeded photos of mixed sizes (256..512 x 341..683, both orientations, shorter
side to 256, centre crop 224, bf16), per tile (``ragged_*_ms``, the whole
Python op: checks, table, pinned copy, launch) and ``kernel_rule_ms``, the
launch alone on a device-resident table, against what a user runs without it:
``loop_ms``, N dense batch-1 ``image_u8_resize_patch_embed`` calls plus
``torch.cat``, and ``two_step_ms``, ``ops.image_u8_ragged_resize_to_float``
then ``VisionTransformer.embed``. The ``uniform_*`` columns are the control
on N images of ONE size (384x512): the ragged launch on a device-resident
table against the dense resampling kernel on the stacked batch, per forced
tile, which is what the per-row geometry costs. ``identical``: whether the
ragged op and the loop (uniform: the dense kernel) gave the same bits.
"""
import json
import os
import subprocess
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)

BATCHES = (1, 8, 32, 128)
DTYPES = ("bfloat16", "float32")
TILES = {"rule": 0, "small": 1, "large": 2}
TIMEOUT_S = 300


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


def run_cases():
    import torch
    import torch.nn.functional as F

    from min_tfs_client_amd import ops
    from min_tfs_client_amd.preprocess import (IMAGENET_MEAN, IMAGENET_STD,
                                               ImagePreprocess)

    dev, P, D, S = "cuda:0", 16, 768, 224
    T = (S // P) ** 2 + 1
    g = torch.Generator().manual_seed(0)
    w = torch.randn((D, 3, P, P), generator=g) * 0.02
    b = torch.randn(D, generator=g) * 0.02
    pos = (torch.randn((T, D), generator=g) * 0.02).to(dev)
    cls = (torch.randn(D, generator=g) * 0.02).to(dev)
    wk, bias_f = (t.to(dev) for t in ops.patch_embed_fold(
        w, b, IMAGENET_MEAN, IMAGENET_STD))
    for dtype_name in DTYPES:
        dtype = getattr(torch, dtype_name)
        pre = ImagePreprocess(IMAGENET_MEAN, IMAGENET_STD, out_dtype=dtype)
        w_m, b_m = w.to(dev, dtype), b.to(dev, dtype)
        pos_m, cls_m = pos.to(dtype).view(1, T, D), cls.to(dtype).view(1, 1, D)
        for N in BATCHES:
            x = torch.randint(0, 256, (N, S, S, 3), dtype=torch.uint8,
                              generator=g).to(dev)

            def fused(tile=0):
                return ops._image_u8_patch_embed(
                    x, wk, bias_f, P, pos, cls, dtype, tile)

            def baseline():
                y = F.conv2d(pre(x), w_m, b_m, stride=P)
                y = y.flatten(2).transpose(1, 2)
                return torch.cat((cls_m.expand(N, -1, -1), y), 1) + pos_m

            diff = (fused().float() - baseline().float()).abs().max().item()
            reps = 200 if N <= 32 else 50
            fns = [lambda t=t: fused(t) for t in TILES.values()] + [baseline]
            rounds = [[time_kernel(f, reps, 10) for f in fns]
                      for _ in range(5)]
            ms = [sorted(r[i] for r in rounds)[2] for i in range(len(fns))]
            nbytes = x.numel() + N * T * D * x.new_empty(
                0, dtype=dtype).element_size() + wk.numel() * 2
            row = {"case": f"{N}x{S}x{S}_{dtype_name}", "bytes": nbytes}
            for name, t in zip(TILES, ms):
                row[f"fused_{name}_ms"] = round(t, 4)
            row.update({
                "baseline_ms": round(ms[-1], 4),
                "baseline_over_fused": round(ms[-1] / ms[0], 2),
                "fused_GB_s": round(nbytes / 1e9 / (ms[0] / 1e3), 1),
                "max_abs_diff": diff})
            print(json.dumps(row), flush=True)


def run_yuv_cases():
    import torch

    from min_tfs_client_amd import ops
    from min_tfs_client_amd.preprocess import IMAGENET_MEAN, IMAGENET_STD

    dev, P, D, S = "cuda:0", 16, 768, 224
    T = (S // P) ** 2 + 1
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(0)
    w = torch.randn((D, 3, P, P), generator=g) * 0.02
    b = torch.randn(D, generator=g) * 0.02
    pos = (torch.randn((T, D), generator=g) * 0.02).to(dev)
    cls = (torch.randn(D, generator=g) * 0.02).to(dev)
    wk, bias_f = (t.to(dev) for t in ops.patch_embed_fold(
        w, b, IMAGENET_MEAN, IMAGENET_STD))
    for chroma in ops.YUV_CHROMA_LAYOUTS:
        for N in BATCHES:
            x = torch.randint(0, 256, (N, S * 3 // 2, S), dtype=torch.uint8,
                              generator=g).to(dev)
            rgb = ops.yuv420_to_rgb_u8(x, chroma)

            def yuv(tile):
                return ops._image_yuv420_patch_embed(
                    x, wk, bias_f, P, pos, cls, dtype, tile, chroma=chroma)

            def floor(tile):
                return ops._image_u8_patch_embed(
                    rgb, wk, bias_f, P, pos, cls, dtype, tile)

            def two_step(tile):
                return ops._image_u8_patch_embed(
                    ops.yuv420_to_rgb_u8(x, chroma), wk, bias_f, P, pos, cls,
                    dtype, tile)

            same = all(torch.equal(yuv(t), two_step(t))
                       for t in TILES.values())
            reps = 200 if N <= 32 else 50
            fns = [lambda f=f, t=t: f(t) for t in TILES.values()
                   for f in (yuv, floor, two_step)]
            rounds = [[time_kernel(f, reps, 10) for f in fns]
                      for _ in range(5)]
            ms = [sorted(r[i] for r in rounds)[2] for i in range(len(fns))]
            row = {"case": f"{N}x{S}x{S}_{chroma}_bfloat16",
                   "identical": same}
            for i, name in enumerate(TILES):
                a, fl, c = ms[3 * i:3 * i + 3]
                row.update({
                    f"yuv_{name}_ms": round(a, 4),
                    f"rgb_{name}_ms": round(fl, 4),
                    f"two_step_{name}_ms": round(c, 4),
                    f"yuv_over_rgb_{name}": round(a / fl, 2),
                    f"two_step_over_yuv_{name}": round(c / a, 2)})
            print(json.dumps(row), flush=True)


def run_resize_cases():
    import torch

    from min_tfs_client_amd import ops
    from min_tfs_client_amd.models import vit_b16
    from min_tfs_client_amd.preprocess import IMAGENET_MEAN, IMAGENET_STD

    dev, P, S = "cuda:0", 16, 224
    torch.manual_seed(0)
    model = vit_b16().to(dev).eval()
    wk, bias_f = ops.patch_embed_fold(
        model.patch_embed.weight, model.patch_embed.bias, IMAGENET_MEAN,
        IMAGENET_STD)
    pos = model.pos_embed.detach().float()[0].contiguous()
    cls = model.cls_token.detach().float().reshape(-1)
    g = torch.Generator().manual_seed(0)
    for dtype_name in DTYPES:
        dtype = getattr(torch, dtype_name)
        m = model.to(dtype)
        # the identity size is the cost of the second piece and the bf16 tile
        for hw in ((480, 640), (1080, 1920), (S, S)):
            Hr, Wr = (256, 256 * hw[1] // hw[0]) if hw[0] != S else hw
            crop = ((Hr - S) // 2, (Wr - S) // 2, S, S)
            for N in (1, 8, 32):
                x = torch.randint(0, 256, (N, *hw, 3), dtype=torch.uint8,
                                  generator=g).to(dev)

                def fused(tile=0):
                    return ops._image_u8_resize_patch_embed(
                        x, (Hr, Wr), wk, bias_f, P, crop, pos, cls, dtype,
                        tile)

                @torch.no_grad()
                def two_step():
                    return m.embed(ops.image_u8_resize_to_float(
                        x, (Hr, Wr), IMAGENET_MEAN, IMAGENET_STD, crop=crop,
                        out_dtype=dtype))

                def rgb(tile=0):
                    return ops._image_u8_patch_embed(
                        x, wk, bias_f, P, pos, cls, dtype, tile)

                other = two_step if hw[0] != S else rgb
                diff = (fused().float() - other().float()).abs().max().item()
                fns = [lambda t=t: fused(t) for t in TILES.values()] + [other]
                if hw[0] == S:
                    fns += [lambda: rgb(1), lambda: rgb(2)]
                rounds = [[time_kernel(f, 100, 10) for f in fns]
                          for _ in range(5)]
                ms = [sorted(r[i] for r in rounds)[2]
                      for i in range(len(fns))]
                spread = max(max(r[i] for r in rounds) /
                             min(r[i] for r in rounds)
                             for i in range(len(fns)))
                row = {"case": f"{N}x{hw[0]}x{hw[1]}_{dtype_name}"}
                for name, t in zip(TILES, ms):
                    row[f"fused_{name}_ms"] = round(t, 4)
                if hw[0] != S:
                    row["two_step_ms"] = round(ms[3], 4)
                    row["two_step_over_fused"] = round(ms[3] / ms[0], 2)
                else:
                    for name, t in zip(TILES, ms[3:]):
                        row[f"rgb_{name}_ms"] = round(t, 4)
                    row["fused_over_rgb"] = round(ms[0] / ms[3], 2)
                row.update({"max_over_min_round": round(spread, 2),
                            "max_abs_diff": diff})
                print(json.dumps(row), flush=True)


def run_ragged_cases():
    import numpy as np
    import torch

    from min_tfs_client_amd import ops
    from min_tfs_client_amd.models import vit_b16
    from min_tfs_client_amd.preprocess import IMAGENET_MEAN, IMAGENET_STD

    dev, P, S, dtype = "cuda:0", 16, 224, torch.bfloat16
    native = ops.require_native()
    torch.manual_seed(0)
    model = vit_b16().to(dev).eval()
    wk, bias_f = ops.patch_embed_fold(
        model.patch_embed.weight, model.patch_embed.bias, IMAGENET_MEAN,
        IMAGENET_STD)
    pos = model.pos_embed.detach().float()[0].contiguous()
    cls = model.cls_token.detach().float().reshape(-1)
    m = model.to(dtype)
    g = torch.Generator().manual_seed(0)
    rng = np.random.default_rng(0)

    def geometry(shapes):
        """shorter side to 256, centre crop 224: sizes, origins, table"""
        sizes = [(256, 256 * w // h) if h <= w else (256 * h // w, 256)
                 for h, w in shapes]
        origins = [((hr - S) // 2, (wr - S) // 2) for hr, wr in sizes]
        shp = np.array(shapes, dtype=np.int64)
        nbytes = shp[:, 0] * shp[:, 1] * 3
        offsets = np.concatenate(([0], np.cumsum(nbytes[:-1])))
        table = ops._ragged_table(
            shp, np.array(sizes), np.array(origins), offsets, True).to(dev)
        return sizes, origins, [int(o) for o in offsets], table

    for N in (1, 8, 32):
        # photos of mixed sizes and both orientations, and the uniform control
        mixed = [(int(rng.integers(256, 513)), int(rng.integers(341, 684)))
                 [::int(rng.choice((1, -1)))] for _ in range(N)]
        row = {"case": f"{N}_mixed_bfloat16"}
        spreads = []
        for label, shapes in (("", mixed), ("uniform_", [(384, 512)] * N)):
            sizes, origins, offs, table = geometry(shapes)
            data = torch.randint(
                0, 256, (sum(h * w * 3 for h, w in shapes),),
                dtype=torch.uint8, generator=g).to(dev)
            views = [data[o:o + h * w * 3].view(1, h, w, 3)
                     for o, (h, w) in zip(offs, shapes)]

            def ragged(tile=0):
                return ops._image_u8_ragged_resize_patch_embed(
                    data, shapes, sizes, (S, S), wk, bias_f, P, origins, pos,
                    cls, dtype, tile)

            def kernel(tile=0):       # the launch alone, table on the device
                return native.u8_ragged_resize_patch_embed(
                    data, table, S, S, wk, bias_f, P, pos, cls, dtype, tile)

            def loop():
                return torch.cat([ops._image_u8_resize_patch_embed(
                    v, sz, wk, bias_f, P, (*o, S, S), pos, cls, dtype, 0)
                    for v, sz, o in zip(views, sizes, origins)])

            @torch.no_grad()
            def two_step():
                return m.embed(ops.image_u8_ragged_resize_to_float(
                    data, shapes, sizes, (S, S), IMAGENET_MEAN, IMAGENET_STD,
                    origins=origins, out_dtype=dtype))

            def dense(tile=0):        # uniform sizes only
                return ops._image_u8_resize_patch_embed(
                    data.view(N, *shapes[0], 3), sizes[0], wk, bias_f, P,
                    (*origins[0], S, S), pos, cls, dtype, tile)

            if label:
                names = [f"{k}_{t}" for t in ("small", "large")
                         for k in ("kernel", "dense")]
                fns = [lambda f=f, t=t: f(t) for t in (1, 2)
                       for f in (kernel, dense)]
                same = all(torch.equal(kernel(t), dense(t)) for t in (1, 2))
            else:
                names = [f"ragged_{t}" for t in TILES] + [
                    "kernel_rule", "loop", "two_step"]
                fns = [lambda t=t: ragged(t) for t in TILES.values()] + [
                    kernel, loop, two_step]
                same = torch.equal(ragged(), loop())
                row["max_abs_diff_two_step"] = (
                    ragged().float() - two_step().float()).abs().max().item()
            rounds = [[time_kernel(f, 100, 10) for f in fns]
                      for _ in range(5)]
            for i, name in enumerate(names):
                ts = sorted(r[i] for r in rounds)
                row[f"{label}{name}_ms"] = round(ts[2], 4)
                spreads.append(ts[-1] / ts[0])
            row[f"{label}identical"] = same
        row.update({
            "loop_over_ragged": round(row["loop_ms"] / row["ragged_rule_ms"],
                                      2),
            "two_step_over_ragged": round(
                row["two_step_ms"] / row["ragged_rule_ms"], 2),
            "uniform_kernel_over_dense_small": round(
                row["uniform_kernel_small_ms"] / row["uniform_dense_small_ms"],
                2),
            "uniform_kernel_over_dense_large": round(
                row["uniform_kernel_large_ms"] / row["uniform_dense_large_ms"],
                2),
            "max_over_min_round": round(max(spreads), 2)})
        print(json.dumps(row), flush=True)


def main():
    if sys.argv[1:] == ["--cases"]:
        return run_cases()
    if sys.argv[1:] == ["--yuv-cases"]:
        return run_yuv_cases()
    if sys.argv[1:] == ["--resize-cases"]:
        return run_resize_cases()
    if sys.argv[1:] == ["--ragged-cases"]:
        return run_ragged_cases()
    child = {"--yuv": "--yuv-cases", "--resize": "--resize-cases",
             "--ragged": "--ragged-cases"}.get(
        " ".join(sys.argv[1:]), "--cases")
    cmd = [sys.executable, os.path.abspath(__file__), child]
    try:
        rc = subprocess.run(cmd, timeout=TIMEOUT_S).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": "timeout", "timeout_s": TIMEOUT_S}),
              flush=True)
        sys.exit(124)
    if rc != 0:
        print(json.dumps({"error": "failed", "exit": rc}), flush=True)
        sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
