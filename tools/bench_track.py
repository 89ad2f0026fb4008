"""What tracking costs (FrameStream(track=...); include/sassd.h "Tracking"), on one MI355X, in ONE process per stream-creation
order.  car_cfg weights, batch 1, the 4 seeded car frames.

  (a) the kernel: sassd_track_step alone.  HIP events around `--launches` back-to-back calls of the C entry point, 5 blocks of
      each configuration, alternating; the median block.  Three configurations: the detection list a real car frame leaves
      behind against roughly 20 live tracks (the tracks that list itself gives birth to) and against roughly 200 (180 more
      parked around it, which never die), both with cap = 256; and the worst case the interface admits for the car plan,
      D = capD detections (512) against as many live tracks (cap = 512), every detection matched in every call.  The state moves
      on from call to call as it does in a stream; the descriptor is the identity with dt = 0.1 s.
  (b) the stream: frames/s with `--inflight` frames in flight without (P) and with (PT) track=, alternating within every
      repeat; the median of `--repeats` blocks of `--steps` frames.  The base is the stream without track= of the same build.

A process's HIP streams share the runtime's hardware queues in the order they were created, and that place has moved a
stream's rate by 10-15 % (README).  So two creation orders are measured, each in a fresh child process (`--order fwd`,
`--order rev`); `--order both`, the default, starts the two children, reports both records, and compares the tracked
stream with the plain one at the SAME place in the creation order (`tracked_over_plain_same_place`): within one process the
place alone decides more than tracking does.

    python tools/bench_track.py --steps 200 --warmup 20 --repeats 5 [--out profiles/track.json]

Prints one JSON line.  No figure is assumed and none is a pass criterion: the record says what was measured, on one box, in
one run."""
import argparse
from collections import deque
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCKS = ("P", "PT")
SPEC = dict(max_dist=2.0, max_age=3, alpha=0.5, cap=256, birth_score=0.0)


def measure(a, order):
    import torch
    import bench
    import sassd  # noqa: F401
    from sassd import _C, track as T
    from sassd.pipeline import InferencePlan
    from sassd.stream import FrameStream
    dev = torch.device("cuda:0")
    model, w = bench.build_model(0, dev, "car")
    sd = model.state_dict()
    frames = [np.ascontiguousarray(w["frame"](i)) for i in range(4)]
    kw = dict(inflight=a.inflight, points_cap=w["points_cap"], anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev,
              batch_size=1, **w["plan"])
    names = BLOCKS if order == "fwd" else BLOCKS[::-1]
    fs = {name: FrameStream(sd, **(dict(track=SPEC) if name == "PT" else {}), **kw) for name in names}   # the order measured
    torch.cuda.synchronize()
    clock = [0]

    def run(name, n):
        """n frames through the block -> (detections, detections with a track) in all"""
        stream, k, m, pending = fs[name], 0, 0, deque()

        def take():
            nonlocal k, m
            d = stream.collect(pending.popleft())
            k += 0 if d[0][0] is None else len(d[0][0])
            if name == "PT":
                m += int((d[0][3]["ids"] >= 0).sum())
        for i in range(n):
            if len(pending) == a.inflight:
                take()
            if name == "PT":
                clock[0] += 1
                pending.append(stream.submit([frames[i % 4]], track=[dict(time=0.1 * clock[0])]))
            else:
                pending.append(stream.submit([frames[i % 4]]))
        while pending:
            take()
        return k, m

    dets = {name: run(name, 4) for name in names}           # the 4 frames once: the detection counts
    fps = {name: [] for name in names}
    for rep in range(a.repeats):
        for name in (names if rep % 2 == 0 else names[::-1]):       # alternate: no drift favours one block
            run(name, a.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, a.steps)
            torch.cuda.synchronize()
            fps[name].append(a.steps / (time.perf_counter() - t0))
    for stream in fs.values():
        for pl in stream.plans:
            st = int(pl.status.item())
            assert st == 0, "pipeline status 0x%x" % st
        stream.close()

    # (a) the kernel alone: HIP events around back-to-back launches of the C entry point, alternating blocks
    def block_us(fn, n_k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_k):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n_k

    plan = InferencePlan(sd, anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev, batch_size=1, **w["plan"])
    counts = []
    for p in frames:
        plan.run_from_points([torch.from_numpy(p).to(dev)])
        torch.cuda.synchronize()
        counts.append(int(plan.out["counts"][0].item()))
    plan.run_from_points([torch.from_numpy(frames[int(np.argmax(counts))]).to(dev)])
    torch.cuda.synchronize()
    car = {k: v.clone() for k, v in plan.out.items()}
    cap_d = plan.capD
    g = np.arange(cap_d)
    grid = np.zeros((1, cap_d, 7), np.float32)
    grid[0, :, 0], grid[0, :, 1] = 2.0 + 3.0 * (g % 24), -34.0 + 3.0 * (g // 24)
    grid[0, :, 2:] = [-1.0, 1.6, 3.9, 1.56, 0.0]
    crowd = dict(boxes=torch.from_numpy(grid).to(dev), scores=torch.full((1, cap_d), 0.8, device=dev),
                 labels=torch.zeros(1, cap_d, dtype=torch.int32, device=dev),
                 counts=torch.full((1,), cap_d, dtype=torch.int32, device=dev))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    L = _C.lib()
    configs = {}
    for name, det, cap, parked in (("car_20", car, 256, 0), ("car_200", car, 256, 180), ("worst_%d" % cap_d, crowd, min(cap_d, T.MAX_CAP), 0)):
        trk = T.Tracker(1, cap_d, dev, **dict(SPEC, cap=cap))
        if parked:                                          # tracks of the detections' label around the scene; they never die
            st = trk.state()
            f = T.slot_fields(st["slots"][0])
            rng = np.random.default_rng(0)
            for i in range(cap - parked, cap):
                f["id"][i], f["label"][i], f["hits"][i], f["misses"][i] = 100000 + i, 0, 5, -(1 << 30)
                f["box"][i] = [rng.uniform(0, 70), rng.uniform(-40, 40), -1.0, 1.6, 3.9, 1.56, 0.0]
            trk.load_state(st)
        desc = T.identity_desc(1, reset=False)
        desc["dt"][:] = 0.1
        trk.desc.copy_(torch.from_numpy(T.pack_desc(desc)))
        p = trk.params
        md = (ctypes.c_float * len(p["max_dist"]))(*p["max_dist"])
        args = [_C.ptr(det[k]) for k in ("boxes", "scores", "labels", "counts")] + [
            1, cap_d, _C.ptr(trk.seq), _C.ptr(status), _C.ptr(trk.desc), _C.ptr(trk.slots), _C.ptr(trk.next_id), cap, md,
            len(p["max_dist"]), p["max_age"], p["alpha"], p["birth_score"], _C.ptr(trk.record), trk.record_bytes, _C.stream()]

        def step(args=args):
            assert L.sassd_track_step(*args) == 0
        block_us(step, 20)
        configs[name] = dict(step=step, trk=trk, det=det, cap=cap, us=[])
    for rep in range(5):
        for name in (list(configs) if rep % 2 == 0 else list(configs)[::-1]):
            configs[name]["us"].append(block_us(configs[name]["step"], a.launches))
    kernels = {}
    for name, c in configs.items():
        rec = T.decode_track_record(c["trk"].record.cpu().numpy(), 1, cap_d, c["cap"])
        ids = T.slot_fields(rec["slots"][0])["id"]
        kernels[name] = dict(detections=int(rec["count"][0]), matched=int((rec["det_hits"][0] >= 2).sum()),
                             live_tracks=int((ids >= 0).sum()), cap=c["cap"], cap_d=cap_d, dropped=int(rec["dropped"][0]),
                             track_step_us=round(float(np.median(c["us"])), 2), blocks_us=[round(x, 2) for x in c["us"]],
                             launches=a.launches, blocks=5)

    def stat(v):
        return dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))
    res = {name: dict(fps=[round(x, 1) for x in v], **stat(v)) for name, v in fps.items()}
    med = {name: res[name]["median"] for name in res}
    return dict(build_order=list(names), blocks=res, tracked_over_plain=round(med["PT"] / med["P"], 4),
                us_per_frame_added=round(1e6 / med["PT"] - 1e6 / med["P"], 2), kernels=kernels,
                detections_over_4_frames={k: v[0] for k, v in dets.items()}, tracked_detections_over_4_frames=dets["PT"][1],
                csrc_hash=_C.csrc_hash(), device=torch.cuda.get_device_name(0),
                hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", "runtime default"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--order", default="both", choices=["both", "fwd", "rev"])
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    if a.order == "both":                   # a fresh process per creation order; this one never opens the GPU
        runs = []
        for order in ("fwd", "rev"):
            cmd = [sys.executable, os.path.abspath(__file__), "--order", order] + [
                "--%s=%d" % (k, getattr(a, k)) for k in ("steps", "warmup", "repeats", "inflight", "launches")]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True).stdout
            runs.append(json.loads(out.strip().splitlines()[-1])["orders"][0])
    else:
        runs = [measure(a, a.order)]
    rec = dict(tool="tools/bench_track.py", config="car", batch=1, inflight=a.inflight, steps=a.steps, warmup=a.warmup,
               repeats=a.repeats, track=SPEC, unit="frames/s; kernels in microseconds", note="one box, one run", orders=runs)
    if len(runs) == 2:                      # the same place in the creation order, across the two processes
        med = [{k: v["median"] for k, v in r["blocks"].items()} for r in runs]
        rec["tracked_over_plain_same_place"] = dict(created_first=round(med[1]["PT"] / med[0]["P"], 4),
                                                    created_second=round(med[0]["PT"] / med[1]["P"], 4))
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
