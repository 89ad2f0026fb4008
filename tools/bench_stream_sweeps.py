"""Frames/s of FrameStream(sweeps=S) -- the multi-sweep cloud merged from a device ring inside the captured frame -- next to
the same frames merged on the host with numpy and submitted whole, in ONE process, alternating within every repeat (so the
blocks share the box, the clocks and the minute).  car_cfg weights with a 5-feature input layer (x, y, z, intensity, time lag),
batch 1, `--inflight` frames in flight, S = `--sweeps` sweeps of the K21 size: one static K21 scene seen from a swaying sensor.

  A   sassd.stream.merge_sweeps_host per frame on the submitting thread (S - 1 float64 transforms of a sweep, one
      concatenation), then a plain FrameStream(ndim=5): S x 21500 rows of 5 floats cross the bus per frame
  B   FrameStream(ndim=4, sweeps=S, time_feature=True): the new sweep alone crosses the bus, sassd_merge_sweeps_dev merges

A process's HIP streams share the runtime's hardware queues in the order they were created, and that place has moved a
stream's rate by 15 % (README, FrameStream(annos=True)).  So both creation orders are measured, each in a fresh child
process (`--order AB`, `--order BA`); `--order both`, the default, starts the two children and reports both records.

    python tools/bench_stream_sweeps.py --steps 200 --warmup 20 --repeats 5 [--out profiles/frame_stream_sweeps.json]

Prints one JSON line: per order and block the frames/s of every repeat, their median and min-max; B/A; the host time per frame
inside submit() and, for A, in the merge in front of it (time.perf_counter around those calls alone); the merge kernel's time
from HIP events (mean over back-to-back launches on the descriptors of a real frame); the H2D bytes per frame; csrc_hash.
Every block runs `--steps` frames between torch.cuda.synchronize() on both sides, after `--warmup` untimed ones.  No gain is
assumed and no figure is a pass criterion: the record says what was measured."""
import argparse
from collections import deque
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rigid_pose(yaw, t):
    out = np.eye(4)
    out[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    out[:3, 3] = t
    return out


def sway(n):
    """n sensor-to-world poses of a closed path -- the sensor sways +-2 m along x, +-1 m along y and +-0.05 rad in yaw -- so
    that a stream can run it round and round as ONE sequence and every measured frame has all its sweeps behind it"""
    phi = 2 * np.pi * np.arange(n) / n
    return [rigid_pose(0.05 * np.sin(f), [2 * np.sin(f), np.cos(f), 0.0]) for f in phi]


def measure(a, order):
    import torch
    import sassd  # noqa: F401
    from sassd import _C, kernels as K, synth
    from sassd.stream import FrameStream, merge_sweeps_host, stage_layout, sweep_transform
    dev = torch.device("cuda:0")
    S, inflight = a.sweeps, a.inflight
    w = dict(synth.workload("car"), overrides=dict(backbone=dict(num_input_features=5), neck=dict(num_input_features=5)))
    model, _ = synth.build_detector_for(w, 0)

    # the sequence: a static K21 scene, every sweep all of it in the sensor frame of its pose (so a merged frame fills the
    # voxels of one K21 frame S times over and the frame behind the merge is the bench workload's)
    n_seq, dt = a.frames, 0.05
    poses = sway(n_seq)
    scene = np.ascontiguousarray(w["frame"](0))
    sweeps = []
    for p in poses:
        m = sweep_transform(p, poses[0])
        s = scene.copy()
        s[:, :3] = (scene[:, :3].astype(np.float64) @ m[:, :3].T + m[:, 3]).astype(np.float32)
        sweeps.append(s)
    sweep_cap, points_cap = w["points_cap"], S * w["points_cap"]

    def entries(i):
        """frame i of the endless sequence: sweep i % n_seq at time i * dt, behind it the S - 1 sweeps before it"""
        return [(sweeps[i % n_seq], None, 0.0)] + [
            (sweeps[j % n_seq], sweep_transform(poses[i % n_seq], poses[j % n_seq]), np.float32(i * dt - j * dt))
            for j in range(i - 1, max(0, i - S + 1) - 1, -1)]

    synth.calibrate_cls_head_on_device(model, w, dev, merge_sweeps_host(entries(S - 1), True), target_count=200)
    sd = model.state_dict()
    kw = dict(batch_size=1, anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev, **w["plan"])
    make = dict(A=lambda: FrameStream(sd, inflight=inflight, points_cap=points_cap, ndim=5, **kw),
                B=lambda: FrameStream(sd, inflight=inflight, points_cap=points_cap, ndim=4, sweeps=S, sweep_cap=sweep_cap,
                                      time_feature=True, **kw))
    fs = {}
    for name in order:                                  # the creation order under measurement
        fs[name] = make[name]()
    torch.cuda.synchronize()
    host = dict(A_merge=[], A_submit=[], B_submit=[])

    at = dict(A=0, B=0)                                 # the next frame of each block's sequence

    def run(name, n, keep=None):
        """the next n frames of the block's sequence -> detections in all"""
        stream, k, pending = fs[name], 0, deque()
        t_merge = t_submit = 0.0

        def collect():
            d = stream.collect(pending.popleft())
            if keep is not None:
                keep.append(d)
            return 0 if d[0][0] is None else len(d[0][0])

        for i in range(at[name], at[name] + n):
            if len(pending) == inflight:
                k += collect()
            if name == "A":
                t0 = time.perf_counter()
                cloud = merge_sweeps_host(entries(i), True)
                t1 = time.perf_counter()
                pending.append(stream.submit([cloud]))
                t2 = time.perf_counter()
                t_merge, t_submit = t_merge + (t1 - t0), t_submit + (t2 - t1)
            else:
                t1 = time.perf_counter()
                pending.append(stream.submit([sweeps[i % n_seq]], sweeps=[dict(pose=poses[i % n_seq], time=i * dt, first=i == 0)]))
                t_submit += time.perf_counter() - t1
        while pending:
            k += collect()
        at[name] += n
        if name == "A":
            host["A_merge"].append(t_merge / n * 1e6)
        host[name + "_submit"].append(t_submit / n * 1e6)
        return k

    # both blocks return the same detections, frame for frame (the tests hold this; here it guards the measurement)
    got = dict(A=[], B=[])
    n_check = n_seq + S
    check = {name: run(name, n_check, got[name]) for name in "AB"}
    assert check["A"] == check["B"] and check["A"] > 0, check
    for da, db in zip(got["A"], got["B"]):
        assert all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(da[0], db[0]))
    for v in host.values():
        del v[:]

    fps = dict(A=[], B=[])
    for rep in range(a.repeats):
        for name in order:
            run(name, a.warmup)
            del host[name + "_submit"][-1:]
            if name == "A":
                del host["A_merge"][-1:]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, a.steps)
            torch.cuda.synchronize()
            fps[name].append(a.steps / (time.perf_counter() - t0))

    # the merge kernel alone, HIP events around back-to-back launches on the descriptors the last frame left behind
    plan = fs["B"].plans[0]
    n_k = 200
    args = (plan.sw_ring[0], plan.sw_slot[0], plan.sw_count[0], plan.sw_xform[0], plan.sw_T[0], plan.sw_dt[0], True,
            plan.pts_in[0], plan.npts[0:1], plan.status)
    merged_rows = int(plan.npts[0].item())
    for _ in range(20):
        K.merge_sweeps(*args)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n_k):
        K.merge_sweeps(*args)
    e1.record()
    torch.cuda.synchronize()
    kernel_us = e0.elapsed_time(e1) * 1e3 / n_k
    for stream in fs.values():
        for pl in stream.plans:
            st = int(pl.status.item())
            assert st == 0, "pipeline status 0x%x" % st
        stream.close()

    def stat(v):
        return dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))

    res = {name: dict(fps=[round(x, 1) for x in v], **stat(v)) for name, v in fps.items()}
    block_a, block_b = stage_layout(1, seal=True)["total"], stage_layout(1, seal=True, sweeps=S)["total"]
    return dict(build_order=list(order), blocks=res, B_over_A=round(res["B"]["median"] / res["A"]["median"], 4),
                host_us_per_frame={k: stat(v) for k, v in host.items()},
                merge_kernel_us=dict(mean_of_back_to_back_launches=round(kernel_us, 2), launches=n_k, merged_rows=merged_rows),
                h2d_bytes_per_frame=dict(A=S * len(scene) * 5 * 4 + block_a, B=len(scene) * 4 * 4 + block_b,
                                         note="a full frame of the sequence: S sweeps merged"),
                detections_per_frame=round(check["A"] / n_check, 2), csrc_hash=_C.csrc_hash(),
                device=torch.cuda.get_device_name(0), hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", "runtime default"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8, help="sweeps of the closed path the sequence runs round")
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--order", default="both", choices=["both", "AB", "BA"])
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    if a.order == "both":                   # a fresh process per creation order; this one never opens the GPU
        runs = []
        for order in ("AB", "BA"):
            cmd = [sys.executable, os.path.abspath(__file__), "--order", order] + [
                "--%s=%d" % (k, getattr(a, k)) for k in ("steps", "warmup", "repeats", "frames", "inflight", "sweeps")]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True).stdout
            runs.append(json.loads(out.strip().splitlines()[-1])["orders"][0])
    else:
        runs = [measure(a, a.order)]
    rec = dict(tool="tools/bench_stream_sweeps.py", config="car, 5-feature input layer", batch=1, inflight=a.inflight,
               sweeps=a.sweeps, sweep_points=21500, steps=a.steps, warmup=a.warmup, repeats=a.repeats, unit="frames/s",
               frames=a.frames, orders=runs)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
