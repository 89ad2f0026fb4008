"""Frames/s of sassd.stream.FrameStream next to the two ways a frame could be run before it, in ONE process, alternating
within every repeat (so the blocks share the box, the clocks and the minute):

  A      the in-flight loop of bench.py rebuilt from public calls: three InferencePlan(overlap=False), one stream each,
         run_graph round-robin on device clouds, nothing read back (the detections stay in HBM)
  C      one plan (two-branch), run_graph + results() per frame: detections on the host, a host sync after every frame
  S      FrameStream(inflight=3).map(...) on host clouds: detections on the host, in order, status checked per frame
  S-dev  the same on device clouds

    python tools/bench_stream.py --steps 200 --warmup 20 --repeats 5 [--config multi] [--out profiles/frame_stream_bench.json]

Prints one JSON line: per block the frames/s of every repeat, their median and min-max; S/A and S/C; the per-frame host time
of submit and of collect in S (time.perf_counter around the calls of an explicit submit / collect loop); csrc_hash.  Every
block runs `--steps` batches between torch.cuda.synchronize() on both sides, after `--warmup` untimed ones."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sassd  # noqa: E402,F401
import bench  # noqa: E402
from sassd import _C  # noqa: E402
from sassd.pipeline import InferencePlan  # noqa: E402
from sassd.stream import FrameStream  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="car", choices=["car", "multi"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=16, help="distinct seeded clouds the batches cycle through")
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model, w = bench.build_model(0, dev, a.config)
    sd = model.state_dict()
    B, S = w["batch"], a.inflight
    kw = dict(batch_size=B, anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev, **w["plan"])
    host = [np.ascontiguousarray(w["frame"](i)) for i in range(max(a.frames, B))]
    devc = [torch.from_numpy(p).to(dev) for p in host]

    def batch_of(src, i):
        return [src[(i * B + j) % len(src)] for j in range(B)]

    # ---- A: bench.py's in-HBM loop --------------------------------------------------------------------------------------
    A_PLANS = 3                                  # the published recipe, whatever --inflight gives the stream
    a_plans = [InferencePlan(sd, overlap=False, **kw) for _ in range(A_PLANS)]
    a_streams = [torch.cuda.Stream(device=dev) for _ in range(A_PLANS)]
    for pl, st in zip(a_plans, a_streams):
        with torch.cuda.stream(st):
            pl.capture(w["points_cap"])
    # ---- C: one plan, results() per frame ---------------------------------------------------------------------------------
    c_plan = InferencePlan(sd, **kw)
    c_plan.capture(w["points_cap"])
    # ---- S / S-dev ----------------------------------------------------------------------------------------------------------
    fs = FrameStream(sd, inflight=S, points_cap=w["points_cap"], **kw)
    torch.cuda.synchronize()

    def run_a(n):
        for i in range(n):
            with torch.cuda.stream(a_streams[i % A_PLANS]):
                a_plans[i % A_PLANS].run_graph(batch_of(devc, i))

    def run_c(n):
        k = 0
        for i in range(n):
            c_plan.run_graph(batch_of(devc, i))
            k += sum(r[0] is not None for r in c_plan.results())
        return k

    def run_s(n, src):
        k = 0
        for _, dets in fs.map(batch_of(src, i) for i in range(n)):
            k += sum(r[0] is not None for r in dets)
        return k

    host_us = dict(submit=[], collect=[])

    def run_s_timed(n):
        """The loop of FrameStream.map written out, with perf_counter around submit and collect."""
        pending, ts, tc = [], 0.0, 0.0
        for i in range(n):
            if len(pending) == S:
                t0 = time.perf_counter()
                fs.collect(pending.pop(0))
                tc += time.perf_counter() - t0
            clouds = batch_of(host, i)
            t0 = time.perf_counter()
            pending.append(fs.submit(clouds))
            ts += time.perf_counter() - t0
        for t in pending:
            t0 = time.perf_counter()
            fs.collect(t)
            tc += time.perf_counter() - t0
        host_us["submit"].append(ts / n * 1e6)
        host_us["collect"].append(tc / n * 1e6)

    blocks = [("A", lambda n: run_a(n)), ("C", run_c), ("S", lambda n: run_s(n, host)), ("S-dev", lambda n: run_s(n, devc))]
    fps = {name: [] for name, _ in blocks}
    for rep in range(a.repeats):
        for name, fn in blocks:
            fn(a.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(a.steps)
            torch.cuda.synchronize()
            fps[name].append(a.steps * B / (time.perf_counter() - t0))
        run_s_timed(a.steps)
        torch.cuda.synchronize()
    for pl in a_plans + [c_plan] + fs.plans:
        st = int(pl.status.item())
        assert st == 0, "pipeline status 0x%x" % st
    fs.close()

    def stat(v):
        return dict(fps=[round(x, 1) for x in v], median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))

    out = {name: stat(v) for name, v in fps.items()}
    s_med, a_med, c_max = out["S"]["median"], out["A"]["median"], out["C"]["max"]
    rec = dict(tool="tools/bench_stream.py", config=a.config, batch=B, inflight=S,
               block_A="%d InferencePlan(overlap=False), one stream each" % A_PLANS, steps=a.steps, warmup=a.warmup,
               repeats=a.repeats, unit="frames/s", blocks=out, S_over_A=round(s_med / a_med, 4),
               S_over_C_max=round(s_med / c_max, 4), required_S_median_above_C_max=bool(s_med > c_max),
               aim_S_median_at_least_0p95_A_median=bool(s_med >= 0.95 * a_med),
               host_us_per_frame=dict(submit=round(float(np.median(host_us["submit"])), 1),
                                      collect_including_the_wait=round(float(np.median(host_us["collect"])), 1)),
               record_bytes=int(fs.plans[0].record.numel()), csrc_hash=_C.csrc_hash(),
               device=torch.cuda.get_device_name(0), hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", "runtime default"))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
