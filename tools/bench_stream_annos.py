"""Frames/s of FrameStream(annos=True) -- the KITTI result annotation computed inside the captured frame -- next to the same
frames with the annotation built on the host, in ONE process, alternating within every repeat (so the blocks share the box,
the clocks and the minute).  car_cfg, batch 1, host clouds, `--inflight` frames in flight, the bench workload's frames:

  H   a stream without annos; every collected frame goes through model.result_annos (kitti_common.kitti_bbox2results:
      a dozen small numpy calls) on the thread that submits and collects
  D   a stream with annos=True; every collected frame goes through kitti_common.result_anno_from_cam (indexing only)
  H2  the control: a SECOND stream of form H, built after D.  The streams are built in the order H, D, H2, and a process's
      HIP streams share the runtime's hardware queues in the order they were created: where H2 runs like D and not like H,
      the difference between H and D is the place in that order, not the annotation

    python tools/bench_stream_annos.py --steps 200 --warmup 20 --repeats 5 [--out profiles/frame_stream_annos.json]

Prints one JSON line: per block the frames/s of every repeat, their median and min-max; D/H; the host time per frame spent
turning a collected frame into its annotation (time.perf_counter around that call alone, in a loop of its own over frames
collected beforehand); the annotation kernel's time from HIP events (mean over back-to-back launches on the detections of a
real frame); detections and annotation rows per frame; csrc_hash.  Every block runs `--steps` frames between
torch.cuda.synchronize() on both sides, after `--warmup` untimed ones.  No gain is assumed: the record says what was
measured."""
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
from sassd import _C, kernels as K, kitti_common as kc  # noqa: E402
from sassd.stream import FrameStream  # noqa: E402

IMG_SHAPE = (375, 1242)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8, help="distinct frames of the bench workload the stream cycles through")
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model, w = bench.build_model(0, dev, "car")
    model.class_names = ["Car"]
    sd = model.state_dict()
    S = a.inflight
    kw = dict(batch_size=1, anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev, precision=a.precision, **w["plan"])
    calib = kc.Calibration(matrices=augment_synth.calib_matrices())
    cal = [dict(calib=calib, img_shape=IMG_SHAPE)]
    meta = [dict(calib=calib, img_shape=IMG_SHAPE, sample_idx=0)]
    frames = [np.ascontiguousarray(w["frame"](i)) for i in range(a.frames)]
    fs_h = FrameStream(sd, inflight=S, points_cap=w["points_cap"], **kw)
    fs_d = FrameStream(sd, inflight=S, points_cap=w["points_cap"], annos=True, **kw)
    fs_h2 = FrameStream(sd, inflight=S, points_cap=w["points_cap"], **kw)
    torch.cuda.synchronize()

    def anno_h(dets):
        return model.result_annos(dets, meta)[0]

    def anno_d(dets):
        b, s, l, cam = dets[0]
        return kc.result_anno_from_cam(cam, s, l, 0, model.class_names)

    def run_h(n, fs=fs_h):
        k = r = 0
        for _, dets in fs.map([frames[i % len(frames)]] for i in range(n)):
            k += 0 if dets[0][0] is None else len(dets[0][0])
            r += len(anno_h(dets)["name"])
        return k, r

    def run_h2(n):
        return run_h(n, fs_h2)

    def run_d(n):
        k = r = 0
        for _, dets in fs_d.map(([frames[i % len(frames)]], None, cal) for i in range(n)):
            k += 0 if dets[0][0] is None else len(dets[0][0])
            r += len(anno_d(dets)["name"])
        return k, r

    # both blocks detect the same number of boxes and annotate the same number of them (the tests hold the values to
    # their bars; here two counts guard the measurement)
    check = [fn(len(frames)) for fn in (run_h, run_d, run_h2)]
    assert check[0] == check[1] == check[2] and check[0][0] > 0, check

    # host time of the conversion alone, on frames collected beforehand (fresh copies: kitti_bbox2results wraps yaw in place)
    got_h = [d for _, d in fs_h.map([p] for p in frames)]
    got_d = [d for _, d in fs_d.map(([p], None, cal) for p in frames)]

    def time_conv(fn, got, n):
        copies = [[tuple(None if x is None else (dict(x) if isinstance(x, dict) else x.copy()) for x in got[i % len(got)][0])]
                  for i in range(n)]
        t0 = time.perf_counter()
        for d in copies:
            fn(d)
        return (time.perf_counter() - t0) / n * 1e6

    conv_us = dict(H=[], D=[])
    blocks = [("H", run_h), ("D", run_d), ("H2", run_h2)]
    fps = {name: [] for name, _ in blocks}
    for rep in range(a.repeats):
        for name, fn in blocks:
            fn(a.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(a.steps)
            torch.cuda.synchronize()
            fps[name].append(a.steps / (time.perf_counter() - t0))
        conv_us["H"].append(time_conv(anno_h, got_h, a.steps))
        conv_us["D"].append(time_conv(anno_d, got_d, a.steps))

    # the annotation kernel alone, HIP events around back-to-back launches on the detections the last frame left behind
    plan = fs_d.plans[0]
    out = torch.empty(K.frame_annos_bytes(plan.B, plan.capD), dtype=torch.uint8, device=dev)
    n_k = 200
    for _ in range(20):
        K.frame_annos(plan.det, plan.calib, out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n_k):
        K.frame_annos(plan.det, plan.calib, out)
    e1.record()
    torch.cuda.synchronize()
    kernel_us = e0.elapsed_time(e1) * 1e3 / n_k

    for pl in fs_h.plans + fs_d.plans + fs_h2.plans:
        st = int(pl.status.item())
        assert st == 0, "pipeline status 0x%x" % st
    fs_h.close()
    fs_d.close()
    fs_h2.close()

    def stat(v):
        return dict(fps=[round(x, 1) for x in v], median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))

    res = {name: stat(v) for name, v in fps.items()}
    rec = dict(tool="tools/bench_stream_annos.py", config="car", batch=1, inflight=S, precision=a.precision, steps=a.steps,
               warmup=a.warmup, repeats=a.repeats, unit="frames/s", frames=len(frames), cap_d=int(plan.capD),
               detections_per_frame=round(check[0][0] / len(frames), 2), annotation_rows_per_frame=round(check[0][1] / len(frames), 2),
               blocks=res, build_order=["H", "D", "H2"], D_over_H=round(res["D"]["median"] / res["H"]["median"], 4),
               D_over_H2=round(res["D"]["median"] / res["H2"]["median"], 4),
               host_us_per_frame_building_the_annotation={k: dict(median=round(float(np.median(v)), 1), min=round(min(v), 1),
                                                                  max=round(max(v), 1)) for k, v in conv_us.items()},
               annos_kernel_us=dict(mean_of_back_to_back_launches=round(kernel_us, 2), launches=n_k),
               csrc_hash=_C.csrc_hash(), device=torch.cuda.get_device_name(0),
               hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", "runtime default"))
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
