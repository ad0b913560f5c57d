#!/usr/bin/env python3
"""Where a sharded Predict's wall time goes, per phase, for both
orchestrations of TurboPredictClient.predict_sharded.

  --path python   the per-shard python orchestration
                  (MI355X_NATIVE_SHARDED=0), re-enacted here step for step
                  with time.perf_counter around each phase: serialize,
                  producer sync, submit -> send-start latency, send, wait,
                  merge
  --path native   the single C++ call; phases come from its own trace
                  (MI355X_SHARDED_TRACE): plan, producer sync, send-start
                  latency, send, wait, merge

Both report the per-channel stream counts (GrpcChannel.streams_started) and
the time device sends blocked in the staging pool (acquire_ms of
MI355X_STAGING_TRACE). Same workload as the headline benchmark: 32x3x224x224
fp32 echo over a unix socket, 8 channels, --shards 4, --pipeline N request
threads. Prints one JSON object.

  python tools/bench_sharded_breakdown.py --path python --pipeline 4
"""
from __future__ import annotations

import argparse
import json
import multiprocessing
import os
import statistics
import sys
import tempfile
import threading
import time

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)


def _med(xs):
    return round(statistics.median(xs), 4) if xs else None


def _p99(xs):
    xs = sorted(xs)
    return round(xs[min(len(xs) - 1, int(0.99 * len(xs)))], 4) if xs else None


def python_request(client, inputs, shards, dev, parse_dev, rec):
    """TurboPredictClient.predict_sharded's python orchestration, timed."""
    import torch
    pc = time.perf_counter
    t_req = pc()
    keys = list(inputs)
    batch = inputs[keys[0]].shape[0]
    base, rem = divmod(batch, shards)
    sizes = [base + (1 if i < rem else 0) for i in range(shards)]
    views, off = [], 0
    for n in sizes:
        views.append({k: inputs[k].narrow(0, off, n) for k in keys})
        off += n
    submitted = [0.0] * shards

    def send_shard(i):
        t0 = pc()
        stub = client._stubs[i % len(client._stubs)]
        names = list(views[i])
        blob, regions, keep = client._native.serialize_predict_streaming(
            True, "default", -1, "", names, [views[i][k] for k in names])
        t1 = pc()
        if any(r[3] for r in regions):
            torch.cuda.current_stream().synchronize()
        t2 = pc()
        if parse_dev >= 0:
            fut = stub.future_streaming_parsed(blob, regions, parse_dev, 60.0)
        else:
            fut = stub.future_streaming(blob, regions, 60.0)
        t3 = pc()
        return fut, (t0 - submitted[i], t1 - t0, t2 - t1, t3 - t2)

    sends = []
    for i in range(shards):
        submitted[i] = pc()
        sends.append(client._send_pool.submit(send_shard, i))
    results = [s.result() for s in sends]
    t_sent = pc()
    parts = []
    for fut, _ in results:
        if parse_dev >= 0:
            outs, raw = fut.result_parsed()
            if outs is None:
                _s, outs, _ = client._native.parse_predict_response(
                    raw, dev, 1)
        else:
            _s, outs, _ = client._native.parse_predict_response(
                fut.result(), dev, 1)
        parts.append(outs)
    t_wait = pc()
    merged = {k: torch.cat([p[k] for p in parts], dim=0) for k in parts[0]}
    t_done = pc()
    with rec["lock"]:
        for _, (lat, ser, sync, send) in results:
            rec["send_start_latency_ms"].append(lat * 1e3)
            rec["serialize_ms"].append(ser * 1e3)
            rec["sync_ms"].append(sync * 1e3)
            rec["send_ms"].append(send * 1e3)
        rec["all_sends_done_ms"].append((t_sent - t_req) * 1e3)
        rec["wait_ms"].append((t_wait - t_sent) * 1e3)
        rec["merge_ms"].append((t_done - t_wait) * 1e3)
        rec["total_ms"].append((t_done - t_req) * 1e3)
    return merged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", choices=["python", "native"], required=True)
    ap.add_argument("--pipeline", type=int, default=4)
    ap.add_argument("--shards", type=int, default=4)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=32)
    args = ap.parse_args()

    tmp = tempfile.mkdtemp(prefix="mtcbd", dir="/tmp")
    staging_trace = os.path.join(tmp, "staging.jsonl")
    sharded_trace = os.path.join(tmp, "sharded.jsonl")
    os.environ["MI355X_STAGING_TRACE"] = staging_trace
    os.environ["MI355X_SHARDED_TRACE"] = sharded_trace
    os.environ["MI355X_NATIVE_SHARDED"] = (
        "1" if args.path == "native" else "0")

    import torch

    import bench
    from min_tfs_client_amd.turbo import TurboPredictClient

    has_gpu = torch.cuda.is_available()
    dev = "cuda:0" if has_gpu else "cpu"
    ctx = multiprocessing.get_context("spawn")
    address = f"unix://{tmp}/bd.sock"
    ready, stop = ctx.Event(), ctx.Event()
    env_trace = os.environ.pop("MI355X_STAGING_TRACE")  # client side only
    proc = ctx.Process(target=bench._server_proc,
                       args=(address, ready, stop, "echo", dev, ""),
                       daemon=True)
    proc.start()
    os.environ["MI355X_STAGING_TRACE"] = env_trace
    if not ready.wait(300):
        raise SystemExit("server failed to start")

    inputs = bench.make_inputs("resnet50", torch.device(dev))
    parse_dev = 0 if has_gpu else -1
    rec = {k: [] for k in (
        "send_start_latency_ms", "serialize_ms", "sync_ms", "send_ms",
        "all_sends_done_ms", "wait_ms", "merge_ms", "total_ms")}
    rec["lock"] = threading.Lock()
    client = TurboPredictClient(address, num_channels=args.channels,
                                backend="native")

    def one_request():
        if args.path == "python":
            return python_request(client, inputs, args.shards, dev,
                                  parse_dev, rec)
        t0 = time.perf_counter()
        out = client.predict_sharded("default", inputs, shards=args.shards,
                                     output_device=dev)
        with rec["lock"]:
            rec["total_ms"].append((time.perf_counter() - t0) * 1e3)
        return out

    def run(n):
        counter = {"left": n}
        lock = threading.Lock()

        def worker():
            while True:
                with lock:
                    if counter["left"] <= 0:
                        return
                    counter["left"] -= 1
                one_request()

        ts = [threading.Thread(target=worker) for _ in range(args.pipeline)]
        t0 = time.perf_counter()
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        if has_gpu:
            torch.cuda.synchronize()
        return time.perf_counter() - t0

    run(args.warmup)
    for k, v in rec.items():
        if k != "lock":
            v.clear()
    for p in (staging_trace, sharded_trace):
        if os.path.exists(p):
            os.remove(p)
    before = [ch.streams_started for ch in client._channels]
    elapsed = run(args.steps)
    after = [ch.streams_started for ch in client._channels]

    result = {
        "path": args.path, "pipeline": args.pipeline, "shards": args.shards,
        "channels": args.channels, "steps": args.steps, "gpu": has_gpu,
        "req_per_s": round(args.steps / elapsed, 2),
        "streams_per_channel": [a - b for a, b in zip(after, before)],
        "phases_median_ms": {}, "phases_p99_ms": {},
    }
    if args.path == "native" and os.path.exists(sharded_trace):
        with open(sharded_trace) as f:
            lines = [json.loads(x) for x in f if x.strip()]
        rec["plan_ms"] = [x["plan_ms"] for x in lines]
        rec["sync_ms"] = [x["sync_ms"] for x in lines]
        rec["send_start_latency_ms"] = [
            s - (x["plan_ms"] + x["sync_ms"])
            for x in lines for s in x["send_start_ms"]]
        rec["send_ms"] = [s for x in lines for s in x["send_ms"]]
        rec["all_sends_done_ms"] = [x["sends_done_ms"] for x in lines]
        rec["wait_ms"] = [x["wait_ms"] for x in lines]
        rec["merge_ms"] = [x["merge_ms"] for x in lines]
        rec["native_total_ms"] = [x["total_ms"] for x in lines]
    for k, v in rec.items():
        if k != "lock" and v:
            result["phases_median_ms"][k] = _med(v)
            result["phases_p99_ms"][k] = _p99(v)
    if os.path.exists(staging_trace):
        with open(staging_trace) as f:
            acq = [json.loads(x).get("acquire_ms", 0.0)
                   for x in f if x.strip()]
        result["staging_acquire_ms"] = {
            "sends": len(acq), "median": _med(acq), "p99": _p99(acq),
            "max": round(max(acq), 4) if acq else None,
            "blocked_over_0.1ms": sum(1 for a in acq if a > 0.1)}
    print(json.dumps(result))

    client.close()
    stop.set()
    proc.join(timeout=10)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
