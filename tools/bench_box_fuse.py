"""What box fusion costs (InferencePlan / FrameStream(fuse_iou=...); include/sassd.h "Box fusion"), on one MI355X, in ONE process per
stream-creation order.  car_cfg weights, batch 1, the 4 seeded car frames.

  (a) the kernel: sassd_box_fuse next to sassd_rescore_nms -- the kernel it follows, the yardstick -- on the candidate lists a
      real frame leaves behind, for the plain frame and for the pooled lists of T2 (identity + flip) and T4 (+ rotations of
      +-pi/8).  HIP events around 200 back-to-back calls of the C entry points, 5 blocks of each, alternating; the median block.
  (b) the stream: frames/s with `--inflight` frames in flight for plain, T2 and T4 streams without (P, T2, T4) and with
      (PF, T2F, T4F) fuse_iou, alternating within every repeat; the median of `--repeats` blocks of `--steps` frames.

A process's HIP streams share the runtime's hardware queues in the order they were created, and that place has moved a
stream's rate by 11-15 % (README).  So two creation orders are measured, each in a fresh child process (`--order fwd`,
`--order rev`); `--order both`, the default, starts the two children and reports both records.

    python tools/bench_box_fuse.py --steps 200 --warmup 20 --repeats 5 [--out profiles/box_fuse.json]

Prints one JSON line.  No figure is assumed and none is a pass criterion: the record says what was measured, on one box, in
one run."""
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

ID, FLIP = (0, 0.0, 1.0), (1, 0.0, 1.0)
VIEWS = {1: None, 2: [ID, FLIP], 4: [ID, FLIP, (0, np.pi / 8, 1.0), (0, -np.pi / 8, 1.0)]}
BLOCKS = ("P", "PF", "T2", "T2F", "T4", "T4F")


def measure(a, order):
    import torch
    import bench
    import sassd  # noqa: F401
    from sassd import _C, kernels as K
    from sassd.pipeline import InferencePlan
    from sassd.stream import FrameStream
    dev = torch.device("cuda:0")
    model, w = bench.build_model(0, dev, "car")
    sd = model.state_dict()
    frames = [np.ascontiguousarray(w["frame"](i)) for i in range(4)]
    kw = dict(inflight=a.inflight, points_cap=w["points_cap"], anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev,
              batch_size=1, **w["plan"])

    def make(name):
        V = 1 if name[0] == "P" else int(name[1])
        return FrameStream(sd, **({} if V == 1 else dict(tta=VIEWS[V])), **(dict(fuse_iou=a.fuse_iou) if name[-1] == "F" else {}),
                           **kw)
    names = BLOCKS if order == "fwd" else BLOCKS[::-1]
    fs = {name: make(name) for name in names}               # the creation order under measurement
    torch.cuda.synchronize()

    def run(name, n):
        """n frames through the block -> detections in all"""
        stream, k, pending = fs[name], 0, deque()
        for i in range(n):
            if len(pending) == a.inflight:
                d = stream.collect(pending.popleft())
                k += 0 if d[0][0] is None else len(d[0][0])
            pending.append(stream.submit([frames[i % 4]]))
        while pending:
            d = stream.collect(pending.popleft())
            k += 0 if d[0][0] is None else len(d[0][0])
        return k

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

    # (a) the kernel next to rescore / NMS on the lists a real frame leaves behind (eager plans, the frame with the most
    # candidates of the four), HIP events around back-to-back launches, alternating blocks
    def block_us(fn, n_k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_k):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n_k
    pkw = dict(anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev, batch_size=1, **w["plan"])
    kernels = {}
    for V in (1, 2, 4):
        plan = InferencePlan(sd, fuse_iou=a.fuse_iou, **({} if V == 1 else dict(tta=VIEWS[V])), **pkw)
        rows = []
        for p in frames:
            plan.run_from_points([torch.from_numpy(p).to(dev)])
            torch.cuda.synchronize()
            cand = plan.df if plan.tta is None else plan.pool
            rows.append(int(cand["counts"][0].item()))
        plan.run_from_points([torch.from_numpy(frames[int(np.argmax(rows))]).to(dev)])
        torch.cuda.synchronize()
        cand = plan.df if plan.tta is None else plan.pool
        args = (cand["guided"], plan.logits if plan.tta is None else cand["logits"], cand["labels"], cand["counts"])
        n_det = int(plan.det["counts"][0].item())
        moved = int((plan.fused[0, :n_det] != plan.det["boxes"][0, :n_det]).any(-1).sum().item())

        # the C entry points themselves (ctypes, arguments built once): the host's part of a launch stays below the kernels'
        L = _C.lib()
        wsb = L.sassd_rescore_nms_workspace_bytes(1, int(cand["guided"].shape[1]))
        ws = K.workspace("rescore_nms", wsb, dev)
        ptrs = [_C.ptr(t) for t in args]
        det_ptrs = [_C.ptr(plan.det[k]) for k in ("boxes", "scores", "labels", "counts")]
        cap_k, stream = int(cand["guided"].shape[1]), _C.stream()
        nms_args = ptrs + [1, cap_k, float(plan.score_thr), float(plan.iou_thr)] + det_ptrs + [plan.capD, _C.ptr(plan.status),
                                                                                              _C.ptr(ws), wsb, stream]
        fuse_args = ptrs + [1, cap_k, float(plan.score_thr), float(plan.fuse_iou), det_ptrs[0], det_ptrs[2], det_ptrs[3],
                            plan.capD, _C.ptr(plan.fused), stream]

        def nms():
            assert L.sassd_rescore_nms(*nms_args) == 0

        def fuse():
            assert L.sassd_box_fuse(*fuse_args) == 0
        for fn in (nms, fuse):
            block_us(fn, 20)
        t = dict(nms=[], fuse=[])
        for rep in range(5):
            for key, fn in ((("nms", nms), ("fuse", fuse)) if rep % 2 == 0 else (("fuse", fuse), ("nms", nms))):
                t[key].append(block_us(fn, a.launches))
        med = {k: float(np.median(v)) for k, v in t.items()}
        kernels["plain" if V == 1 else "T%d" % V] = dict(
            candidates=max(rows), candidates_per_frame=rows, cap_rows=int(cand["guided"].shape[1]), detections=n_det,
            boxes_moved=moved, rescore_nms_us=round(med["nms"], 2), box_fuse_us=round(med["fuse"], 2),
            rescore_nms_blocks_us=[round(x, 2) for x in t["nms"]], box_fuse_blocks_us=[round(x, 2) for x in t["fuse"]],
            fuse_over_nms=round(med["fuse"] / med["nms"], 4), launches=a.launches, blocks=5)

    def stat(v):
        return dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))
    res = {name: dict(fps=[round(x, 1) for x in v], **stat(v)) for name, v in fps.items()}
    med = {name: res[name]["median"] for name in res}
    return dict(build_order=list(names), blocks=res,
                fused_over_unfused={k: round(med[k + "F"] / med[k], 4) for k in ("P", "T2", "T4")},
                us_per_frame_added={k: round(1e6 / med[k + "F"] - 1e6 / med[k], 2) for k in ("P", "T2", "T4")},
                kernels=kernels, detections_over_4_frames=dets, csrc_hash=_C.csrc_hash(), device=torch.cuda.get_device_name(0),
                hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", "runtime default"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--fuse-iou", dest="fuse_iou", type=float, default=0.7)
    ap.add_argument("--order", default="both", choices=["both", "fwd", "rev"])
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    if a.order == "both":                   # a fresh process per creation order; this one never opens the GPU
        runs = []
        for order in ("fwd", "rev"):
            cmd = [sys.executable, os.path.abspath(__file__), "--order", order, "--fuse-iou", repr(a.fuse_iou)] + [
                "--%s=%d" % (k, getattr(a, k)) for k in ("steps", "warmup", "repeats", "inflight", "launches")]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True).stdout
            runs.append(json.loads(out.strip().splitlines()[-1])["orders"][0])
    else:
        runs = [measure(a, a.order)]
    rec = dict(tool="tools/bench_box_fuse.py", config="car", batch=1, inflight=a.inflight, steps=a.steps, warmup=a.warmup,
               repeats=a.repeats, fuse_iou=a.fuse_iou, unit="frames/s; kernels in microseconds",
               views={"T%d" % V: [list(v) for v in VIEWS[V]] for V in (2, 4)}, note="one box, one run", orders=runs)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
