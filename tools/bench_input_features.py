"""What a wider sparse input layer costs: the kernels of csrc/spconv_in.hip (3..8 features per voxel) against the 4-channel
kernels the KITTI paths keep, in one process.

1. forward     SubMConv3d(Cin, 16, 3) + folded BatchNorm + ReLU on the level-0 rulebook of a K21 frame: the existing (4, 16)
               kernel, then the input-layer kernel at Cin 4, 5 and 8, each with the fp32 and the bf16 store.
2. wgrad       the input-layer weight gradient at Cin 5 and 8 against the existing (4, 16) one on the level-0 rulebook of two
               K21 frames (the training batch of the bench workload).
3. frames/s    a Cin = 5 plan against a Cin = 4 plan of otherwise equal seeded weights (the fifth weight slice and the fifth
               point column are seeded additions): the captured frame replayed with a host wait per frame, and three frames
               in flight through FrameStream.

Kernels run in alternating blocks, `--repeats` blocks each, after `--warmup` untimed launches; a block is `--iters`
back-to-back launches between two HIP events, its figure the mean per launch; median and min..max over the blocks.  The
byte model beside each kernel: 4 P Cin gathered + 108 n rulebook + 64 n (32 n bf16) stored + the weight image, P pairs, n rows.
One JSON record; no target.

    python tools/bench_input_features.py [--iters 200] [--warmup 20] [--repeats 5] [--out profiles/input_features.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sassd import _C, kernels as K, synth  # noqa: E402
from sassd.pipeline import INPUT_WEIGHT_KEY, InferencePlan  # noqa: E402
from sassd.stream import FrameStream  # noqa: E402


def _spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), n=len(v))


def _blocks(work, iters, warmup, repeats):
    """{name: launch} -> {name: [us per launch of each block]}, the blocks of the kernels alternating"""
    for fn in work.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in work}
    for _ in range(repeats):
        for name, fn in work.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / iters)
    return us


def _rulebook(sd, w, dev, clouds):
    """level-0 submanifold rulebook of `clouds` (one batch) from a plan's own voxelizer and pyramid: (nbr, n_ptr, n, cap, pairs)"""
    plan = InferencePlan(sd, batch_size=len(clouds), anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev, **w["plan"])
    plan.run_from_points([torch.from_numpy(c).to(dev) for c in clouds])
    torch.cuda.synchronize()
    assert int(plan.status.item()) == 0
    n = int(plan.n[0].item())
    nbr = plan.nbr["subm0"].clone()
    return nbr, plan.n[0].clone(), n, plan.caps[0], int((nbr[:n] >= 0).sum().item())


def _five(pts, seed):
    return np.ascontiguousarray(np.concatenate([pts, np.random.default_rng(seed).random((len(pts), 1), dtype=np.float32)], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200, help="frames per frames/s block")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    import bench
    model, w = bench.build_model(0, dev)
    sd4 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    rec = dict(workload="sparse input layer, K21 frames (synthetic lidar64, 21500 points)", iters=a.iters, warmup=a.warmup,
               repeats=a.repeats, csrc_hash=_C.csrc_hash(), device=torch.cuda.get_device_name(0))

    # ---- 1. forward on the frame's level-0 rulebook ------------------------------------------------------------------
    nbr, nptr, n, cap, pairs = _rulebook(sd4, w, dev, [synth.k21(0)])
    scale, shift = (torch.rand(16, generator=g) + 0.5).to(dev), (torch.randn(16, generator=g) * 0.1).to(dev)
    work, model_bytes = {}, {}
    for cin in (4, 5, 8):
        x = torch.randn(cap, cin, generator=g).to(dev)
        wt = (torch.randn(27, cin, 16, generator=g) * 0.2).to(dev)
        wp = K.spconv_in_pack_weight(wt)
        for bf in (False, True):
            y = torch.empty(cap, 16, dtype=torch.bfloat16 if bf else torch.float32, device=dev)
            name = "in_cin%d_%s" % (cin, "bf16" if bf else "fp32")
            work[name] = (lambda x=x, wp=wp, cin=cin, y=y, bf=bf:
                          K.spconv_in_fwd(x, nbr, nptr, cap, wp, 27, cin, 16, scale, shift, True, y, y_bf16=bf))
            model_bytes[name] = 4 * pairs * cin + 108 * n + (32 if bf else 64) * n + 4 * wp.numel()
        if cin == 4:
            y32 = torch.empty(cap, 16, device=dev)
            y16 = torch.empty(cap, 16, dtype=torch.bfloat16, device=dev)
            wp16 = K.spconv_bf16_pack_weight(wt)
            work["existing_4_16_fp32"] = (lambda x=x, wp=wp, y=y32: K.spconv_fwd(x, nbr, nptr, cap, wp, 27, 4, 16, scale, shift,
                                                                                  True, y, cfg=0))
            work["existing_4_16_bf16"] = (lambda x=x, wp=wp16, y=y16: K.spconv_fwd_bf16(x, nbr, nptr, cap, wp, 27, 4, 16, scale,
                                                                                        shift, True, y))
            model_bytes["existing_4_16_fp32"] = 16 * pairs + 108 * n + 64 * n + 4 * wp.numel()
            model_bytes["existing_4_16_bf16"] = 16 * pairs + 108 * n + 32 * n + 4 * wp.numel()
    us = _blocks(work, a.iters, a.warmup, a.repeats)
    base = {s: statistics.median(us["existing_4_16_" + s]) for s in ("fp32", "bf16")}
    rec["forward"] = dict(rows=n, pairs=pairs, results={
        k: dict(us=_spread(v), model_bytes=model_bytes[k], model_bytes_vs_4_16=round(model_bytes[k] / model_bytes["existing_4_16_" + k[-4:]], 3),
                time_vs_4_16=round(statistics.median(v) / base[k[-4:]], 3)) for k, v in us.items()})
    for k, r in rec["forward"]["results"].items():
        print("forward %-20s %7.2f us [%.2f..%.2f]  %.2fx the (4,16) kernel, byte model %.2fx" % (
            k, r["us"]["median"], r["us"]["min"], r["us"]["max"], r["time_vs_4_16"], r["model_bytes_vs_4_16"]), flush=True)

    # ---- 2. weight gradient at the training batch's row count -------------------------------------------------------------
    nbr2, nptr2, n2, cap2, pairs2 = _rulebook(sd4, w, dev, [synth.k21(0), synth.k21(1)])
    dy = torch.randn(cap2, 16, generator=g).to(dev)
    work = {}
    for cin in (4, 5, 8):
        x = torch.randn(cap2, cin, generator=g).to(dev)
        dw = torch.empty(27, cin, 16, device=dev)
        if cin == 4:
            work["existing_4_16"] = lambda x=x, dw=dw: K.spconv_bwd_weight(x, dy, nbr2, nptr2, cap2, 4, 16, dw=dw, cfg=0)
        work["in_cin%d" % cin] = lambda x=x, dw=dw, cin=cin: K.spconv_in_bwd_weight(x, dy, nbr2, nptr2, cap2, cin, 16, dw=dw)
    us = _blocks(work, a.iters, a.warmup, a.repeats)
    b = statistics.median(us["existing_4_16"])
    rec["wgrad"] = dict(rows=n2, pairs=pairs2, results={k: dict(us=_spread(v), time_vs_4_16=round(statistics.median(v) / b, 3))
                                                         for k, v in us.items()})
    for k, r in rec["wgrad"]["results"].items():
        print("wgrad   %-20s %7.2f us [%.2f..%.2f]  %.2fx the (4,16) kernel" % (
            k, r["us"]["median"], r["us"]["min"], r["us"]["max"], r["time_vs_4_16"]), flush=True)

    # ---- 3. frames/s: a Cin = 5 plan against the Cin = 4 plan --------------------------------------------------------------
    sd5 = dict(sd4)
    w4 = sd4[INPUT_WEIGHT_KEY]
    extra = (torch.randn(3, 3, 3, 1, 16, generator=g) * float(w4.std())).to(w4)
    sd5[INPUT_WEIGHT_KEY] = torch.cat([w4, extra], 3).contiguous()
    frames4 = [synth.k21(100 + i) for i in range(8)]
    frames = {4: frames4, 5: [_five(p, i) for i, p in enumerate(frames4)]}
    sds = {4: sd4, 5: sd5}
    kw = dict(anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev, **w["plan"])
    fps = {"cin%d_%s" % (c, m): [] for c in (4, 5) for m in ("sequential", "inflight3")}
    plans, streams = {}, {}
    for c in (4, 5):
        plans[c] = InferencePlan(sds[c], batch_size=1, **kw)
        plans[c].capture(w["points_cap"], ndim=c)
        streams[c] = FrameStream(sds[c], inflight=3, points_cap=w["points_cap"], ndim=c, **kw)
    dev_frames = {c: [torch.from_numpy(p).to(dev) for p in frames[c]] for c in (4, 5)}
    ndet = {}
    try:
        for rep in range(a.repeats + 1):                     # block 0 warms up
            for c in (4, 5):
                t0 = time.perf_counter()
                for i in range(a.frames):
                    plans[c].run_graph([dev_frames[c][i % 8]])
                    torch.cuda.synchronize()
                t1 = time.perf_counter()
                got = 0
                for _, dets in streams[c].map([frames[c][i % 8]] for i in range(a.frames)):
                    got += 0 if dets[0][0] is None else len(dets[0][0])
                t2 = time.perf_counter()
                ndet[c] = got
                if rep:
                    fps["cin%d_sequential" % c].append(a.frames / (t1 - t0))
                    fps["cin%d_inflight3" % c].append(a.frames / (t2 - t1))
    finally:
        for s in streams.values():
            s.close()
    rec["frames_per_s"] = dict(frames=a.frames, detections_per_block=ndet, results={k: _spread(v) for k, v in fps.items()})
    for m in ("sequential", "inflight3"):
        r4, r5 = rec["frames_per_s"]["results"]["cin4_" + m], rec["frames_per_s"]["results"]["cin5_" + m]
        print("frames/s %-11s Cin 4: %.1f [%.1f..%.1f]   Cin 5: %.1f [%.1f..%.1f]   ratio %.3f" % (
            m, r4["median"], r4["min"], r4["max"], r5["median"], r5["min"], r5["max"], r5["median"] / r4["median"]), flush=True)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
