"""Frames/s of FrameStream(tta=views) -- test-time augmentation inside the captured frame -- next to a plain stream and next to
the same views done on the host, in ONE process, alternating within every repeat (so the blocks share the box, the clocks and
the minute).  car_cfg weights, batch 1, `--inflight` frames in flight, the 4 seeded car frames round and round.

  P    a plain FrameStream: one view, the rate README publishes
  T2   FrameStream(tta=identity + flip)
  T4   FrameStream(tta=identity + flip + rotations of +-pi/8)
  H2   the views of T2 on the host: sassd.tta.views_host per frame on the submitting thread, a plain batch-2 stream, the V
       result sets pulled to the host, sassd.tta.unview_boxes, one iou3d_utils.nms_gpu over all of them
  H4   the same for the views of T4 on a plain batch-4 stream

A process's HIP streams share the runtime's hardware queues in the order they were created, and that place has moved a
stream's rate by 11-15 % (README).  So two creation orders are measured, each in a fresh child process (`--order fwd`,
`--order rev`); `--order both`, the default, starts the two children and reports both records.

    python tools/bench_tta.py --steps 200 --warmup 20 --repeats 5 [--out profiles/tta.json]

Prints one JSON line: per order and block the frames/s of every repeat, their median and min-max; T/H and T x V / P per view
count; the HIP-event time of the two new kernels (mean over back-to-back launches on the buffers a real frame left behind);
the post stage and rescore / NMS alone for four per-view candidate lists against one pooled list (HIP events, eager plans);
the detection counts over the 4 frames, plain against T2 / T4; csrc_hash.  Every block runs `--steps` frames between
torch.cuda.synchronize() on both sides, after `--warmup` untimed ones.  No rate is assumed and no figure is a pass criterion:
the record says what was measured, on one box, in one run."""
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
VIEWS = {2: [ID, FLIP], 4: [ID, FLIP, (0, np.pi / 8, 1.0), (0, -np.pi / 8, 1.0)]}
BLOCKS = ("P", "T2", "T4", "H2", "H4")


def measure(a, order):
    import torch
    import bench
    import sassd  # noqa: F401
    from sassd import _C, iou3d_utils, kernels as K, tta as T
    from sassd.stream import FrameStream
    dev = torch.device("cuda:0")
    model, w = bench.build_model(0, dev, "car")
    sd = model.state_dict()
    frames = [np.ascontiguousarray(w["frame"](i)) for i in range(4)]
    kw = dict(inflight=a.inflight, points_cap=w["points_cap"], anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev,
              **w["plan"])
    make = dict(P=lambda: FrameStream(sd, batch_size=1, **kw),
                T2=lambda: FrameStream(sd, batch_size=1, tta=VIEWS[2], **kw), T4=lambda: FrameStream(sd, batch_size=1, tta=VIEWS[4], **kw),
                H2=lambda: FrameStream(sd, batch_size=2, **kw), H4=lambda: FrameStream(sd, batch_size=4, **kw))
    names = BLOCKS if order == "fwd" else BLOCKS[::-1]
    fs = {name: make[name]() for name in names}             # the creation order under measurement
    torch.cuda.synchronize()
    iou_thr = fs["P"].plans[0].iou_thr
    params = {v: T.view_params(VIEWS[v]) for v in VIEWS}

    def host_pool(dets, V):
        """V result sets of one cloud's views -> pooled detections: the numpy inverse, one NMS over all of them"""
        p = params[V]
        boxes, scores, labels = [], [], []
        for v, (b, s, l) in enumerate(dets):
            if b is None:
                continue
            boxes.append(b if v == 0 else T.unview_boxes(b, p["flip"][v], p["sin"][v], p["cos"][v], p["scale"][v], p["angle"][v]))
            scores.append(s)
            labels.append(l)
        if not boxes:
            return 0
        boxes, scores = torch.from_numpy(np.concatenate(boxes)).to(dev), torch.from_numpy(np.concatenate(scores)).to(dev)
        keep = iou3d_utils.nms_gpu(iou3d_utils.boxes3d_to_bev_torch(boxes).contiguous(), scores, iou_thr)
        return int(keep.numel())

    host_us = {name: [] for name in ("H2", "H4")}

    def run(name, n):
        """n frames through the block -> detections in all"""
        stream, k, pending, t_host = fs[name], 0, deque(), 0.0
        V = int(name[1]) if name[0] == "H" else 0

        def collect():
            nonlocal t_host
            d = stream.collect(pending.popleft())
            if V:
                t0 = time.perf_counter()
                got = host_pool(d, V)
                t_host += time.perf_counter() - t0
                return got
            return 0 if d[0][0] is None else len(d[0][0])

        for i in range(n):
            if len(pending) == a.inflight:
                k += collect()
            if V:
                t0 = time.perf_counter()
                clouds = T.views_host(frames[i % 4], VIEWS[V])
                t_host += time.perf_counter() - t0
                pending.append(stream.submit(clouds))
            else:
                pending.append(stream.submit([frames[i % 4]]))
        while pending:
            k += collect()
        if V:
            host_us[name].append(t_host / n * 1e6)
        return k

    dets = {name: run(name, 4) for name in names}           # the 4 frames once: the detection counts
    for v in host_us.values():
        del v[:]
    fps = {name: [] for name in names}
    for rep in range(a.repeats):
        for name in (names if rep % 2 == 0 else names[::-1]):       # alternate: no drift favours one block
            run(name, a.warmup)
            if name in host_us:
                del host_us[name][-1:]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, a.steps)
            torch.cuda.synchronize()
            fps[name].append(a.steps / (time.perf_counter() - t0))

    # the two new kernels alone, HIP events around back-to-back launches on the buffers the last frame left behind
    def kernel_us(fn, n_k=200):
        for _ in range(20):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_k):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) * 1e3 / n_k, 2)
    kernels = {}
    for V in (2, 4):
        pl = fs["T%d" % V].plans[0]
        cnt = [pl.npts_views[0, v:v + 1] for v in range(V - 1)]
        kernels["T%d" % V] = dict(
            views_us=kernel_us(lambda: K.tta_views(pl.pts_in[0], pl.npts[0:1], pl.tta, pl.pts_views[0], cnt)),
            pool_us=kernel_us(lambda: K.tta_pool(pl.df["guided"], pl.logits, pl.df["labels"], pl.df["counts"], pl.tta, pl.capP,
                                                 out=pl.pool, status=pl.status)),
            points=int(pl.npts[0].item()), pooled_rows=int(pl.pool["counts"][0].item()), launches=200)
    # where the frame's time goes behind PSWarp: the post stage (HIP events per stage, eager plans) and rescore / NMS alone, for
    # four lists of one view's candidates (the plain batch-4 plan on views_host clouds) against one pooled list (the tta plan)
    from sassd.pipeline import InferencePlan
    pkw = dict(anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev, **w["plan"])
    post = {}
    for name, plan, clouds in (
            ("plain_batch4", InferencePlan(sd, batch_size=4, **pkw), [torch.from_numpy(v).to(dev) for v in T.views_host(frames[1], VIEWS[4])]),
            ("tta_V4", InferencePlan(sd, batch_size=1, tta=VIEWS[4], **pkw), [torch.from_numpy(frames[1]).to(dev)])):
        for _ in range(5):
            plan.run_from_points(clouds)
        torch.cuda.synchronize()
        plan.prof = {}
        for _ in range(30):
            plan.run_from_points(clouds)
        torch.cuda.synchronize()
        post[name] = {k + "_us": round(float(np.median([e0.elapsed_time(e1) for e0, e1 in v])) * 1e3, 1)
                      for k, v in plan.prof.items() if k in ("voxelize", "sparse", "heads", "post")}
        plan.prof = None
        cand = plan.df if plan.tta is None else plan.pool
        args = (cand["guided"], plan.logits if plan.tta is None else cand["logits"], cand["labels"], cand["counts"])
        post[name]["rescore_nms_us"] = kernel_us(lambda: K.rescore_nms(*args, plan.score_thr, plan.iou_thr, plan.capD, plan.det,
                                                                       plan.status), 100)
        post[name]["candidates"] = [int(c) for c in cand["counts"].cpu()]
    for stream in fs.values():
        for pl in stream.plans:
            st = int(pl.status.item())
            assert st == 0, "pipeline status 0x%x" % st
        stream.close()

    def stat(v):
        return dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))
    res = {name: dict(fps=[round(x, 1) for x in v], **stat(v)) for name, v in fps.items()}
    med = {name: res[name]["median"] for name in res}
    return dict(build_order=list(names), blocks=res,
                T_over_H={"V%d" % V: round(med["T%d" % V] / med["H%d" % V], 4) for V in (2, 4)},
                TxV_over_P={"V%d" % V: round(med["T%d" % V] * V / med["P"], 4) for V in (2, 4)},
                host_us_per_frame={k: stat(v) for k, v in host_us.items()}, kernels=kernels, post_stage=post,
                detections_over_4_frames=dict(plain=dets["P"], T2=dets["T2"], T4=dets["T4"], H2=dets["H2"], H4=dets["H4"],
                                              note="H pools the per-view NMS survivors, T the candidates: not the same set"),
                csrc_hash=_C.csrc_hash(), device=torch.cuda.get_device_name(0),
                hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", "runtime default"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--order", default="both", choices=["both", "fwd", "rev"])
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    if a.order == "both":                   # a fresh process per creation order; this one never opens the GPU
        runs = []
        for order in ("fwd", "rev"):
            cmd = [sys.executable, os.path.abspath(__file__), "--order", order] + [
                "--%s=%d" % (k, getattr(a, k)) for k in ("steps", "warmup", "repeats", "inflight")]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True).stdout
            runs.append(json.loads(out.strip().splitlines()[-1])["orders"][0])
    else:
        runs = [measure(a, a.order)]
    rec = dict(tool="tools/bench_tta.py", config="car", batch=1, inflight=a.inflight, steps=a.steps, warmup=a.warmup,
               repeats=a.repeats, unit="frames/s", views={"T%d" % V: [list(v) for v in VIEWS[V]] for V in VIEWS},
               note="one box, one run", orders=runs)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
