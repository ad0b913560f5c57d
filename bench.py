#!/usr/bin/env python3
"""Flagship serving benchmark: Predict req/s + p50 round-trip.

Headline config (BASELINE.json): 32x3x224x224 fp32 PredictRequest per GPU
per step against a local loopback PredictionService, full round trip —
HIP/staging pack of the device tensor into wire bytes, gRPC over a unix
socket to a separate server process, C++ parse + echo, response unpacked
back to HBM. For --gpus N > 1 (torchrun, one rank per GPU) the step is the
data-parallel config 4: rank 0 scatters the global batch over RCCL/xGMI,
each rank round-trips its shard, responses are all-gathered.

Contract: rank 0 prints ONE JSON line; value is the WHOLE-JOB req/s
aggregate; timing brackets exactly K steps between barrier+synchronize
pairs; MAX elapsed over ranks.

Usage:
  python bench.py                         # 1 GPU (or CPU fallback), quick
  python bench.py --gpus 8 --steps 64     # under torch.distributed.run
  python bench.py --bench-config bert     # BASELINE config 3
  python bench.py --encoding proto        # python-protobuf client (A/B)
  python bench.py --dump-outputs DIR      # last timed step's outputs as .npy

Inputs are seeded, so two runs with the same arguments send identical
requests and their --dump-outputs files can be compared array for array.
"""
from __future__ import annotations

import argparse
import json
import multiprocessing
import os
import statistics
import sys
import time

_ROOT = os.path.dirname(os.path.abspath(__file__))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _server_proc(address: str, ready, stop, servable: str = "echo",
                 device: str = "cpu", shm_dir: str = ""):
    """Loopback PredictionService in its own process (own GIL)."""
    if _ROOT not in sys.path:
        sys.path.insert(0, _ROOT)
    from min_tfs_client_amd.server import ModelServer, identity_servable
    with ModelServer(address=address, raw_predict=True, max_workers=16,
                     device=device, shm_handshake_dir=shm_dir or None) as srv:
        if servable == "echo":
            srv.manager.load("default", identity_servable(), version=1)
        elif servable == "resnet50":
            from min_tfs_client_amd.models import resnet50_servable
            srv.manager.load("default", resnet50_servable(device), version=1)
        elif servable == "bert":
            from min_tfs_client_amd.models import bert_servable
            srv.manager.load("default", bert_servable(device), version=1)
        else:
            raise ValueError(f"unknown servable {servable}")
        ready.set()
        stop.wait()


def make_inputs(cfg: str, device, batch_override=None):
    # seeded CPU generator: identical inputs from run to run on any device
    g = torch.Generator(device="cpu").manual_seed(0)
    if cfg == "resnet50":
        b = batch_override or 32
        return {"images": torch.randn(b, 3, 224, 224, generator=g,
                                      dtype=torch.float32).to(device)}
    if cfg == "bert":
        b = batch_override or 128
        ids = torch.randint(0, 30522, (b, 512), generator=g,
                            dtype=torch.int32).to(device)
        mask = torch.ones(b, 512, dtype=torch.int32, device=device)
        return {"input_ids": ids, "attention_mask": mask}
    if cfg == "scalar":
        return {"x": torch.zeros((), dtype=torch.float32, device=device)}
    if cfg in ("bf16pack", "fused"):
        b = batch_override or 32
        return {"images": torch.randn(b, 3, 224, 224, generator=g,
                                      dtype=torch.bfloat16).to(device)}
    raise ValueError(f"unknown bench config {cfg}")


_DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(outs, out_dir: str) -> None:
    """Write each output of one step as out_dir/<name>.npy: float32 for
    float dtypes up to 32 bits, float64 otherwise (exact for int32). The
    64 MB budget is split evenly; a larger array is stored as a fixed,
    seeded sample of its flattened elements."""
    os.makedirs(out_dir, exist_ok=True)
    budget = _DUMP_BUDGET_BYTES // max(1, len(outs))
    for name in sorted(outs):
        v = outs[name]
        if isinstance(v, torch.Tensor):
            wide = (not v.dtype.is_floating_point) or v.element_size() > 4
            arr = v.detach().to("cpu").to(
                torch.float64 if wide else torch.float32).numpy()
        else:
            arr = np.asarray(v)
            arr = arr.astype(np.float32 if arr.dtype.kind == "f"
                             and arr.itemsize <= 4 else np.float64)
        if arr.nbytes > budget:
            idx = np.random.default_rng(0).choice(
                arr.size, budget // arr.itemsize, replace=False)
            arr = arr.reshape(-1)[np.sort(idx)]
        np.save(os.path.join(out_dir, f"{name}.npy"), arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int,
                    default=int(os.environ.get("WORLD_SIZE", "1")))
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--bench-config", default="resnet50",
                    choices=["resnet50", "bert", "scalar", "bf16pack",
                             "fused"],
                    help="fused = BASELINE config 5: bf16 NCHW input, "
                         "fused cast+NCHW->NHWC CDNA4 kernel before "
                         "serialize, fp32 NHWC on the wire")
    ap.add_argument("--encoding", default="turbo",
                    choices=["turbo", "proto"],
                    help="turbo = C++ codec raw-bytes path; proto = "
                         "python-protobuf client (reference-style)")
    ap.add_argument("--grpc-impl", default="native",
                    choices=["native", "grpcio"],
                    help="gRPC stack for the turbo path: native = the "
                         "C++ HTTP/2 transport (~2 copies/hop); grpcio = "
                         "python gRPC (round-1 baseline, A/B)")
    ap.add_argument("--copy-mode", type=int, default=1,
                    help="0 = pinned-staged pipelined copies, 1 = direct "
                         "pageable hipMemcpy (A/B)")
    ap.add_argument("--streaming", default="auto",
                    choices=["auto", "on", "off"],
                    help="skeleton+regions send (device DMA chunks "
                         "overlap DATA frames; host regions zero-copy "
                         "iovec). auto = on for the native transport "
                         "(A/B with off)")
    ap.add_argument("--transport", default="unix",
                    choices=["unix", "tcp", "shm"],
                    help="unix/tcp = gRPC; shm = shared-memory local "
                         "transport (same wire bytes, ~2 copies per hop)")
    ap.add_argument("--servable", default="echo",
                    choices=["echo", "resnet50", "bert"],
                    help="what the loopback server runs: echo (the codec/"
                         "transport benchmark) or a real model family")
    ap.add_argument("--shards", type=int, default=-1,
                    help="split each logical request along dim 0 into this "
                         "many parallel rpcs over separate channels "
                         "(default: 4 for gRPC transports — measured to "
                         "more than halve p50 — and 1 for shm, where the "
                         "copies are the only cost and sharding adds "
                         "thread overhead)")
    ap.add_argument("--servers", type=int, default=1,
                    help="loopback server processes per rank; the python "
                         "gRPC server caps ~9 GB/s per process, so >1 "
                         "raises the per-GPU ceiling (requests spread "
                         "across instances)")
    ap.add_argument("--pipeline", type=int, default=-1,
                    help="in-flight requests per rank (1 = sequential; "
                         ">1 overlaps serialize/transport/parse of "
                         "consecutive requests). Default: 4 single-rank "
                         "over gRPC (measured peak with shards 4), 1 "
                         "multi-rank/shm")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the outputs of the "
                         "last timed step to DIR/<name>.npy (float32/"
                         "float64, at most 64 MB in all)")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline "
                         "figure; this benchmark has none (the A/B "
                         "matrices and per-stage breakdowns are separate "
                         "programs under tools/), so the flag is accepted "
                         "and changes nothing")
    args = ap.parse_args()
    if args.shards < 0:
        args.shards = 1 if args.transport == "shm" else 4

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    if args.pipeline < 0:
        args.pipeline = (4 if world_size == 1 and args.transport != "shm"
                         and args.encoding == "turbo" else 1)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n_gpus = max(args.gpus, world_size)

    has_gpu = torch.cuda.is_available()
    if has_gpu:
        torch.cuda.set_device(local_rank)
        device = torch.device(f"cuda:{local_rank}")
    else:
        device = torch.device("cpu")

    dist = None
    if world_size > 1:
        import torch.distributed as dist_mod
        dist = dist_mod
        backend = "nccl" if has_gpu else "gloo"
        dist.init_process_group(backend=backend)

    # ---- per-rank loopback server fleet -------------------------------
    ctx = multiprocessing.get_context("spawn")
    server_device = f"cuda:{local_rank}" if has_gpu else "cpu"
    addresses, procs, stop = [], [], ctx.Event()
    readies = []
    shm_dirs = []
    for si in range(max(1, args.servers)):
        shm_dir = ""
        if args.transport == "shm":
            shm_dir = f"/tmp/mi355x_shm_{os.getpid()}_{rank}_{si}"
            shm_dirs.append(shm_dir)
        if args.transport in ("unix", "shm"):
            address = (f"unix:///tmp/mi355x_bench_{os.getpid()}_"
                       f"{rank}_{si}.sock")
        else:
            import socket as _socket
            s = _socket.socket()
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
            s.close()
            address = f"127.0.0.1:{port}"
        ready = ctx.Event()
        proc = ctx.Process(target=_server_proc,
                           args=(address, ready, stop, args.servable,
                                 server_device, shm_dir),
                           daemon=True)
        proc.start()
        addresses.append(address)
        readies.append(ready)
        procs.append(proc)
    # fresh boxes: first torch import in the children can take minutes;
    # poll so a crashed server child fails the bench fast instead of
    # hanging for the full window.
    import time as _time
    for ready, proc in zip(readies, procs):
        deadline = _time.monotonic() + 300
        while not ready.wait(2):
            if not proc.is_alive():
                raise RuntimeError(
                    "bench server process died during startup "
                    f"(exitcode={proc.exitcode})")
            if _time.monotonic() > deadline:
                raise RuntimeError("bench server failed to start (timeout)")
    address = addresses[0] if len(addresses) == 1 else addresses

    # ---- client ------------------------------------------------------
    inputs = make_inputs(args.bench_config, device)
    per_rank_batch = next(iter(inputs.values())).shape[0] \
        if next(iter(inputs.values())).dim() > 0 else 1

    if args.transport == "shm":
        if args.encoding != "turbo" or args.pipeline > 1:
            raise SystemExit("--transport shm requires turbo encoding and "
                             "no pipelining (open more connections "
                             "instead)")
        from min_tfs_client_amd.shm import ShmPredictClient

        class _ShmFleet:
            """shards parallel connections over the server fleet."""

            def __init__(self, dirs, conns):
                from concurrent.futures import ThreadPoolExecutor
                self.clients = [
                    ShmPredictClient(dirs[i % len(dirs)],
                                     slot_bytes=96 << 20)
                    for i in range(conns)]
                self.pool = ThreadPoolExecutor(max_workers=conns)

            def close(self):
                for c in self.clients:
                    c.close()

        fleet = _ShmFleet(shm_dirs, max(1, args.shards))
        client = fleet.clients[0]

        def step_fn(step_inputs):
            out_dev = f"cuda:{local_rank}" if has_gpu else "cpu"
            ncl = len(fleet.clients)
            keys = list(step_inputs.keys())
            batch = (step_inputs[keys[0]].shape[0]
                     if step_inputs[keys[0]].dim() > 0 else 1)
            if ncl == 1 or batch < ncl or any(
                    step_inputs[k].dim() == 0 or
                    step_inputs[k].shape[0] != batch for k in keys):
                return client.predict("default", step_inputs,
                                      output_device=out_dev,
                                      copy_mode=args.copy_mode)
            base, rem = divmod(batch, ncl)
            sizes = [base + (1 if i < rem else 0) for i in range(ncl)]
            futs, off = [], 0
            for i, nrows in enumerate(sizes):
                shard = {k: step_inputs[k].narrow(0, off, nrows)
                         for k in keys}
                futs.append(fleet.pool.submit(
                    fleet.clients[i].predict, "default", shard,
                    output_device=out_dev, copy_mode=args.copy_mode))
                off += nrows
            parts = [f.result() for f in futs]
            return {k: torch.cat([p[k] for p in parts], dim=0)
                    for k in parts[0]}
    elif args.encoding == "turbo":
        from min_tfs_client_amd.turbo import TurboPredictClient
        client = TurboPredictClient(
            address,
            num_channels=min(8, max(min(args.pipeline, 8), args.shards,
                                    args.servers,
                                    args.shards * (2 if args.pipeline > 1
                                                   else 1))),
            backend=args.grpc_impl)

        transform = ({"images": ("nhwc", torch.float32)}
                     if args.bench_config == "fused" else None)

        stream_arg = (None if args.streaming == "auto"
                      else args.streaming == "on")

        def step_fn(step_inputs):
            out_dev = f"cuda:{local_rank}" if has_gpu else "cpu"
            if args.shards > 1 and transform is None:
                return client.predict_sharded(
                    "default", step_inputs, shards=args.shards,
                    output_device=out_dev, copy_mode=args.copy_mode,
                    streaming=stream_arg)
            return client.predict("default", step_inputs,
                                  output_device=out_dev,
                                  copy_mode=args.copy_mode,
                                  transform=transform,
                                  streaming=stream_arg)
    else:
        from min_tfs_client_amd.client import TensorServingClient
        if args.transport == "unix":
            raise SystemExit("--encoding proto requires --transport tcp")
        addr0 = address if isinstance(address, str) else address[0]
        host, port = addr0.split(":")
        client = TensorServingClient(host, int(port))

        def step_fn(step_inputs):
            resp = client.predict_request("default", step_inputs)
            from min_tfs_client_amd.tensors import tensor_proto_to_ndarray
            return {k: tensor_proto_to_ndarray(v)
                    for k, v in resp.outputs.items()}

    # ---- one data-parallel step --------------------------------------
    # world_size > 1 (config 4): rank 0 holds the GLOBAL batch
    # (per_rank_batch * N rows); each step scatters the real dim-0 chunks
    # over RCCL/xGMI, each rank round-trips its shard, responses are
    # all-gathered.
    keys = sorted(inputs.keys())
    if dist is not None and rank == 0:
        global_inputs = {
            k: torch.cat([inputs[k]] * world_size, dim=0).contiguous()
            if inputs[k].dim() > 0 else inputs[k]
            for k in keys}
    else:
        global_inputs = None

    def dp_step():
        step_inputs = {}
        if dist is not None:
            for k in keys:
                shard = torch.empty_like(inputs[k])
                if rank == 0:
                    full = global_inputs[k]
                    n = inputs[k].shape[0] if inputs[k].dim() > 0 else 1
                    scatter_list = list(full.split(n, dim=0)) \
                        if full.dim() > 0 else [full] * world_size
                else:
                    scatter_list = None
                dist.scatter(shard, scatter_list, src=0)
                step_inputs[k] = shard
        else:
            step_inputs = inputs
        outs = step_fn(step_inputs)
        if dist is not None:
            for k, v in outs.items():
                if isinstance(v, torch.Tensor) and v.dim() > 0:
                    gathered = [torch.empty_like(v)
                                for _ in range(world_size)]
                    dist.all_gather(gathered, v.contiguous())
        return outs

    def sync():
        if has_gpu:
            torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()

    if args.pipeline > 1 and world_size > 1:
        raise SystemExit("--pipeline > 1 is single-rank only")
    if args.pipeline > 1 and args.encoding != "turbo":
        raise SystemExit("--pipeline > 1 requires --encoding turbo")

    def run_pipelined(nsteps):
        """Sliding window of `pipeline` in-flight requests; returns
        per-request submit->complete latencies and the outputs of the
        last request. With --shards > 1 each in-flight request is itself
        shard-parallel (thread pool of `pipeline` sharded calls)."""
        out_dev = f"cuda:{local_rank}" if has_gpu else "cpu"
        lat_local = []
        inflight = []
        submitted = 0
        last = None
        if args.shards > 1:
            from concurrent.futures import ThreadPoolExecutor
            pool = ThreadPoolExecutor(max_workers=args.pipeline)
            try:
                while submitted < min(args.pipeline, nsteps):
                    inflight.append((pool.submit(step_fn, inputs),
                                     time.perf_counter()))
                    submitted += 1
                done = 0
                while done < nsteps:
                    fut, ts = inflight.pop(0)
                    outs = fut.result()
                    lat_local.append(time.perf_counter() - ts)
                    done += 1
                    if done == nsteps:
                        last = outs
                    del outs
                    if submitted < nsteps:
                        inflight.append((pool.submit(step_fn, inputs),
                                         time.perf_counter()))
                        submitted += 1
            finally:
                pool.shutdown(wait=True)
            return lat_local, last
        while submitted < min(args.pipeline, nsteps):
            fut, dec = client.predict_future("default", inputs)
            inflight.append((fut, dec, time.perf_counter()))
            submitted += 1
        done = 0
        while done < nsteps:
            fut, dec, ts = inflight.pop(0)
            outs = dec(fut.result(), output_device=out_dev)
            lat_local.append(time.perf_counter() - ts)
            done += 1
            if done == nsteps:
                last = outs
            del outs
            if submitted < nsteps:
                fut, dec = client.predict_future("default", inputs)
                inflight.append((fut, dec, time.perf_counter()))
                submitted += 1
        return lat_local, last

    # ---- warmup ------------------------------------------------------
    if args.pipeline > 1:
        run_pipelined(args.warmup)
    else:
        for _ in range(args.warmup):
            dp_step()
    sync()

    # ---- timed region ------------------------------------------------
    lat = []
    last_outs = None
    t0 = time.perf_counter()
    if args.pipeline > 1:
        lat, last_outs = run_pipelined(args.steps)
    else:
        for i in range(args.steps):
            s0 = time.perf_counter()
            outs = dp_step()
            lat.append(time.perf_counter() - s0)
            if i == args.steps - 1:
                last_outs = outs
            del outs
    sync()
    t1 = time.perf_counter()

    elapsed = t1 - t0
    if dist is not None:
        e = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if has_gpu else "cpu")
        dist.all_reduce(e, op=dist.ReduceOp.MAX)
        elapsed = float(e.item())

    # whole-job aggregate: one request per rank per step
    reqs_per_s = n_gpus * args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1e3
    lat.sort()
    p50_ms = statistics.median(lat) * 1e3
    p99_ms = lat[min(len(lat) - 1, int(0.99 * len(lat)))] * 1e3

    if rank == 0 and args.dump_outputs:
        dump_outputs(last_outs, args.dump_outputs)

    if rank == 0:
        result = {
            "metric": "predict_req_per_s",
            "value": round(reqs_per_s, 3),
            "unit": "req/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "p50_ms_rtt": round(p50_ms, 3),
            "p99_ms_rtt": round(p99_ms, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": ("bf16" if args.bench_config in ("bf16pack", "fused")
                      else "int32" if args.bench_config == "bert"
                      else "fp32"),
            "data": "synthetic",
            "config": {
                "model": (f"identity-echo[{args.bench_config}]"
                          if args.servable == "echo"
                          else f"{args.servable}[{args.bench_config}]"),
                "global_batch": per_rank_batch * n_gpus,
                "seq_len": 512 if args.bench_config == "bert" else None,
                "shape_per_request": list(
                    next(iter(inputs.values())).shape),
                "parallelism": f"dp{n_gpus}",
                "pipeline": args.pipeline,
                "shards": args.shards,
                "encoding": args.encoding,
                "grpc_impl": args.grpc_impl,
                "copy_mode": args.copy_mode,
                "streaming": args.streaming,
                "transport": args.transport,
                "servers_per_rank": args.servers,
                "gpu": has_gpu,
            },
        }
        print(json.dumps(result))

    stop.set()
    for proc in procs:
        proc.join(timeout=10)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
