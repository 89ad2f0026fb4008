"""Frames/s of FrameStream(raw_cap=...) -- raw 360-degree sweeps cropped to the camera frustum inside the captured frame --
next to the two ways the same sweeps can be run without it, in ONE process, alternating within every repeat (so the blocks
share the box, the clocks and the minute).  car_cfg, batch 1, host clouds, `--inflight` frames in flight:

  R   the sweeps' REDUCED clouds (cut to the frustum beforehand, velodyne_reduced/) through a stream without raw_cap
  H   the raw sweeps reduced per frame on the host with numpy -- the same six planes, float64 -- then submitted to R's stream:
      what feeding raw sweeps costs without raw_cap
  X   the raw sweeps through a stream with raw_cap: the crop is two kernels at the head of the frame

R and X run the same frames behind the crop, so X/R prices the crop's two nodes plus the larger host-to-device copy.  The
sweeps are 64 beams x 2083 azimuths all around the sensor (seed 0: 121 746 rows, 14 986 of them inside the frustum of
tests/augment_synth.calib_matrices() at image shape 375 x 1242): raw_cap 122 880, points_cap 16 384 for all three blocks.

    python tools/bench_stream_crop.py --steps 200 --warmup 20 --repeats 5 [--out profiles/frame_stream_crop.json]

Prints one JSON line: per block the frames/s of every repeat, their median and min-max; X/R and X/H; the per-frame host time
of submit and of collect in R and in X (time.perf_counter around the calls of an explicit submit / collect loop: the host
copies every cloud into the slot's pinned block inside submit, 1.9 MB for a raw sweep); csrc_hash.  Every block runs `--steps`
frames between torch.cuda.synchronize() on both sides, after `--warmup` untimed ones."""
import argparse
import json
import os
import sys

import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sassd  # noqa: E402,F401
import bench  # noqa: E402
import augment_synth  # noqa: E402
from sassd import _C, synth  # noqa: E402
from sassd.stream import FrameStream, frustum_of  # noqa: E402

RAW_CAP, POINTS_CAP, IMG_SHAPE = 122880, 16384, (375, 1242)


def raw_sweep(seed):
    az = np.deg2rad(np.linspace(-180, 180, 2083, endpoint=False))
    return synth._ray_cloud(seed, (2.0, -24.8), az, (5.0, 70.0), 80.0, (-80, -80, -3, 80, 80, 3))


def reduce_on_host(pts, pl):
    """The crop's test in numpy: float64, products and sums rounded one by one, then a boolean index."""
    x, y, z = (pts[:, i].astype(np.float64) for i in range(3))
    out = np.zeros(len(pts), bool)
    for k in range(6):
        out |= ((x * pl[k, 0] + y * pl[k, 1]) + z * pl[k, 2]) + pl[k, 3] >= 0
    return pts[~out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8, help="distinct seeded sweeps the frames cycle through")
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model, w = bench.build_model(0, dev, "car")
    sd = model.state_dict()
    S = a.inflight
    kw = dict(batch_size=1, anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev, precision=a.precision, **w["plan"])
    planes = frustum_of(augment_synth.calib_matrices(), IMG_SHAPE)
    raw = [raw_sweep(i) for i in range(a.frames)]
    red = [np.ascontiguousarray(reduce_on_host(p, planes)) for p in raw]
    assert max(len(p) for p in raw) <= RAW_CAP and max(len(p) for p in red) <= POINTS_CAP
    fs_r = FrameStream(sd, inflight=S, points_cap=POINTS_CAP, **kw)
    fs_x = FrameStream(sd, inflight=S, points_cap=POINTS_CAP, raw_cap=RAW_CAP, **kw)
    torch.cuda.synchronize()

    def count(stream, batches):
        k = 0
        for _, dets in stream.map(batches):
            k += sum(0 if r[0] is None else len(r[0]) for r in dets)
        return k

    def run_r(n):
        return count(fs_r, ([red[i % len(red)]] for i in range(n)))

    def run_h(n):
        return count(fs_r, ([reduce_on_host(raw[i % len(raw)], planes)] for i in range(n)))

    def run_x(n):
        return count(fs_x, (([raw[i % len(raw)]], [planes]) for i in range(n)))

    # the three blocks detect the same boxes (the tests hold them to bit equality; here a count guards the measurement)
    n_check = len(raw)
    dets = [fn(n_check) for fn in (run_r, run_h, run_x)]
    assert dets[0] == dets[1] == dets[2] and dets[0] > 0, dets

    host_us = {"R": dict(submit=[], collect=[]), "X": dict(submit=[], collect=[])}

    def run_timed(name, stream, batch, n):
        """The loop of FrameStream.map written out, with perf_counter around submit and collect."""
        pending, ts, tc = [], 0.0, 0.0
        for i in range(n):
            if len(pending) == S:
                t0 = time.perf_counter()
                stream.collect(pending.pop(0))
                tc += time.perf_counter() - t0
            args = batch(i)
            t0 = time.perf_counter()
            pending.append(stream.submit(*args))
            ts += time.perf_counter() - t0
        for t in pending:
            t0 = time.perf_counter()
            stream.collect(t)
            tc += time.perf_counter() - t0
        host_us[name]["submit"].append(ts / n * 1e6)
        host_us[name]["collect"].append(tc / n * 1e6)

    blocks = [("R", run_r), ("H", run_h), ("X", run_x)]
    fps = {name: [] for name, _ in blocks}
    for rep in range(a.repeats):
        for name, fn in blocks:
            fn(a.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(a.steps)
            torch.cuda.synchronize()
            fps[name].append(a.steps / (time.perf_counter() - t0))
        run_timed("R", fs_r, lambda i: ([red[i % len(red)]],), a.steps)
        run_timed("X", fs_x, lambda i: ([raw[i % len(raw)]], [planes]), a.steps)
        torch.cuda.synchronize()
    for pl in fs_r.plans + fs_x.plans:
        st = int(pl.status.item())
        assert st == 0, "pipeline status 0x%x" % st
    fs_r.close()
    fs_x.close()

    def stat(v):
        return dict(fps=[round(x, 1) for x in v], median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))

    out = {name: stat(v) for name, v in fps.items()}
    r_med, h_med, x_med = (out[k]["median"] for k in ("R", "H", "X"))
    rec = dict(tool="tools/bench_stream_crop.py", config="car", batch=1, inflight=S, precision=a.precision, steps=a.steps,
               warmup=a.warmup, repeats=a.repeats, unit="frames/s", raw_cap=RAW_CAP, points_cap=POINTS_CAP,
               sweeps=dict(distinct=len(raw), raw_points=[len(p) for p in raw], kept_points=[len(p) for p in red]),
               detections_per_pass=dets[0], blocks=out, X_over_R=round(x_med / r_med, 4), X_over_H=round(x_med / h_med, 4),
               X_below_0p9_R=bool(x_med < 0.9 * r_med),
               host_us_per_frame={k: dict(submit=round(float(np.median(v["submit"])), 1),
                                          collect_including_the_wait=round(float(np.median(v["collect"])), 1))
                                  for k, v in host_us.items()}, csrc_hash=_C.csrc_hash(), device=torch.cuda.get_device_name(0),
               hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", "runtime default"))
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
