"""What GT-sampling at another width costs: sassd_paste_objects_nd (3..8 floats per point) against the 4-column
sassd_paste_objects the KITTI path keeps, and a whole PointAugmentor.augment_frame call on 5-wide clouds against the same
call on 4-wide ones, in one process.

1. paste     15 sampled objects, a few thousand rows (80..400 points each, what a close KITTI car returns): the existing
             4-column kernel, then the nd kernel at W = 3, 4, 5, 8, lowered as the road-plane recipe does.  The byte model
             beside each: 8 W bytes per row read + written, plus the 15 objects' tables; time proportional to W at best.
             The nd kernel's W = 4 output is compared with the 4-column kernel's, byte for byte, before anything is timed.
2. frames    augment_frame (car config of tests/augment_synth.py, the three synthetic frames in turn, database resident)
             at W = 4 twice (series a and b of the same code: their difference is the run-to-run spread) and at W = 5 on
             the widened database and frames, from the same random seed per block.  Host wall clock around a block that ends
             in a device synchronise; the call reads results back itself.

Kernels run in alternating blocks, `--repeats` blocks each, after `--warmup` untimed launches; a block is `--iters`
back-to-back launches between two HIP events, its figure the mean per launch; median and min..max over the blocks.
One JSON record; no target.

    python tools/bench_gt_sampling_width.py [--iters 200] [--warmup 20] [--repeats 5] [--out profiles/gt_sampling_width.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import augment_synth as S  # noqa: E402
import wide_cloud_cases as W  # noqa: E402
from sassd import _C, kitti_common as kc, point_augmentor as PA  # noqa: E402

HBM_MEASURED_TBS = 6.29             # float4 copy on an MI355X


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


def _paste_inputs(width, dev, n_obj=15):
    """n_obj sampled objects of 80..400 points out of a 60-object database; the same objects and shifts at every width"""
    r = np.random.default_rng(11)
    db_counts = r.integers(80, 400, 60)
    db_start = np.concatenate([[0], np.cumsum(db_counts)])
    pick = r.permutation(60)[:n_obj]
    counts = db_counts[pick].astype(np.int64)
    out_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    shift = np.stack([r.uniform(4, 66, n_obj), r.uniform(-34, 34, n_obj), r.uniform(-1.9, -1.3, n_obj)], 1)
    lower = r.uniform(-0.4, 0.4, n_obj)
    db = np.random.default_rng(12).uniform(-3, 3, (int(db_start[-1]), 8)).astype(np.float32)[:, :width]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n_out = int(out_start[-1])
    return dict(db=t(db), src=t(db_start[pick].astype(np.int64)), ostart=t(out_start), shift=t(shift), lower=t(lower),
                out=torch.empty(n_out, width, device=dev), n_obj=n_obj, n_out=n_out, width=width)


def _paste_launch(x, entry):
    lib, p = _C.lib(), _C.ptr
    if entry == "four":
        return lambda: _C.check(lib.sassd_paste_objects(p(x["db"]), p(x["src"]), p(x["ostart"]), x["n_obj"], x["n_out"],
                                                        p(x["shift"]), p(x["lower"]), p(x["out"]), _C.stream()), "paste")
    return lambda: _C.check(lib.sassd_paste_objects_nd(p(x["db"]), x["width"], p(x["src"]), p(x["ostart"]), x["n_obj"],
                                                       x["n_out"], p(x["shift"]), p(x["lower"]), p(x["out"]), _C.stream()),
                            "paste_nd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=30, help="augment_frame calls per block")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = dict(workload="GT-sampling paste, 15 objects; augment_frame on the synthetic car frames", iters=a.iters,
               warmup=a.warmup, repeats=a.repeats, csrc_hash=_C.csrc_hash(), device=torch.cuda.get_device_name(0))

    # ---- 1. the paste kernels ---------------------------------------------------------------------------------------------
    inputs = {w: _paste_inputs(w, dev) for w in (3, 4, 5, 8)}
    four = dict(inputs[4], out=torch.empty_like(inputs[4]["out"]))
    _paste_launch(four, "four")()
    _paste_launch(inputs[4], "nd")()
    torch.cuda.synchronize()
    same = bool(torch.equal(four["out"].view(torch.int32), inputs[4]["out"].view(torch.int32)))
    assert same, "sassd_paste_objects_nd at 4 columns differs from sassd_paste_objects"
    work = {"existing_4": _paste_launch(four, "four")}
    for w in (3, 4, 5, 8):
        work["nd_w%d" % w] = _paste_launch(inputs[w], "nd")
    us = _blocks(work, a.iters, a.warmup, a.repeats)
    n_out, n_obj = inputs[4]["n_out"], inputs[4]["n_obj"]
    model = lambda w: 8 * w * n_out + n_obj * (8 + 8 + 24 + 8)
    base = statistics.median(us["existing_4"])
    res = {}
    for k, v in us.items():
        w = 4 if k == "existing_4" else int(k[4:])
        med = statistics.median(v)
        res[k] = dict(us=_spread(v), model_bytes=model(w), gb_per_s=round(model(w) / med * 1e-3, 2),
                      share_of_hbm=round(model(w) / med * 1e-3 / (HBM_MEASURED_TBS * 1e3), 5),
                      time_vs_existing_4=round(med / base, 3), model_bytes_vs_4=round(model(w) / model(4), 3))
    t3, t8 = res["nd_w3"]["us"]["median"], res["nd_w8"]["us"]["median"]
    # 8/3 of the bytes: a stream bound by bytes takes 2.67 x as long; a launch that waits on its first loads takes the same
    bound = "latency" if t8 / t3 < 1.5 and res["nd_w8"]["share_of_hbm"] < 0.1 else "bandwidth"
    rec["paste"] = dict(rows=n_out, objects=n_obj, nd_w4_equals_existing=same, results=res, w8_over_w3=round(t8 / t3, 3),
                        bound=bound)
    for k, r in res.items():
        print("paste %-11s %7.2f us [%.2f..%.2f]  %.2fx the 4-column kernel, byte model %.2fx, %.1f GB/s" % (
            k, r["us"]["median"], r["us"]["min"], r["us"]["max"], r["time_vs_existing_4"], r["model_bytes_vs_4"],
            r["gb_per_s"]), flush=True)
    print("paste: W 8 takes %.2fx the time of W 3 for 2.67x the bytes -> %s-bound" % (t8 / t3, bound), flush=True)

    # ---- 2. augment_frame ----------------------------------------------------------------------------------------------------
    cfg = S.AUGMENTOR_CONFIGS["car"]
    calib = kc.Calibration(matrices=S.calib_matrices())
    db4 = S.make_database()
    augs, clouds = {}, {}
    frames = [S.frame(f) for f in range(3)]
    for name, width in (("w4_a", 4), ("w4_b", 4), ("w5", 5)):
        root = tempfile.mkdtemp()
        S.write_database(W.widen_database(db4, width), root)
        np.random.seed(0)
        augs[name] = PA.PointAugmentor(root_path=root, info_path=os.path.join(root, "kitti_dbinfos_train.pkl"), device=dev,
                                       **cfg)
        clouds[name] = [torch.from_numpy(W.widen_points(p, width, f)).to(dev) for f, (p, _, _) in enumerate(frames)]
    ms = {k: [] for k in augs}
    rows_out = {}
    for rep in range(a.repeats + 1):                          # block 0 warms up
        for name, aug in augs.items():
            np.random.seed(100 + rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = 0
            for i in range(a.frames):
                f = i % 3
                out = aug.augment_frame(clouds[name][f], frames[f][1].copy(), frames[f][2], cfg["sample_classes"], None, calib)
                got += int(out[0].shape[0])
            torch.cuda.synchronize()
            if rep:
                ms[name].append((time.perf_counter() - t0) / a.frames * 1e3)
            rows_out[name] = got // a.frames
    assert rows_out["w4_a"] == rows_out["w4_b"] == rows_out["w5"], rows_out
    m = {k: statistics.median(v) for k, v in ms.items()}
    rec["augment_frame"] = dict(frames_per_block=a.frames, rows_out_mean=rows_out["w5"],
                                ms_per_frame={k: _spread(v) for k, v in ms.items()},
                                w4_b_over_w4_a=round(m["w4_b"] / m["w4_a"], 4), w5_over_w4_a=round(m["w5"] / m["w4_a"], 4))
    for k, v in ms.items():
        s = _spread(v)
        print("augment_frame %-5s %.3f ms [%.3f..%.3f]" % (k, s["median"], s["min"], s["max"]), flush=True)
    print("augment_frame: W 5 / W 4 = %.3f; the same W 4 code twice = %.3f" % (m["w5"] / m["w4_a"], m["w4_b"] / m["w4_a"]),
          flush=True)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
