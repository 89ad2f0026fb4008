"""BEV conv0 fed from the sparse tensor against the dense map, on the same weights, in one process
(InferencePlan(dense_entry=False / True)).

bench.py always builds the default plan, so it cannot run both forms; this builds both from the bench model
(bench.build_model) and measures them in turn, `--repeats` times each, the order alternating:
  * sequential frames/s: one two-branch frame graph replayed `--steps` times back to back;
  * host-synced frames/s: the same graph with a device synchronisation after every frame;
  * frames in flight: three one-branch plans on three streams (bench.py's headline form).
One JSON record: every value, median and min..max per figure, the sparse / dense ratios of the medians, and whether the
detections of the two forms on the same seeded frames are equal bit for bit.

    python tools/bench_conv0_entry.py [--steps 200] [--warmup 20] [--repeats 5] [--workloads car]
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

import bench  # noqa: E402
from sassd.pipeline import InferencePlan  # noqa: E402
from bench_precision import _fps_sequential, _fps_inflight  # noqa: E402

FORMS = {"sparse_entry": False, "dense_entry": True}


def _plan(sd, w, dev, form, overlap=True):
    return InferencePlan(sd, batch_size=w["batch"], anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev,
                         overlap=overlap, dense_entry=FORMS[form], **w["plan"])


def _fps_synced(plan, batch_of, steps, warmup):
    for i in range(warmup):
        plan.run_graph(batch_of(i))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        plan.run_graph(batch_of(i))
        torch.cuda.synchronize()
    return steps * plan.B / (time.perf_counter() - t0)


def _spread(v):
    return dict(values=v, median=statistics.median(v), min=min(v), max=max(v))


def measure(config, dev, steps, warmup, repeats):
    model, w = bench.build_model(0, dev, config)
    sd = model.state_dict()
    B = w["batch"]
    clouds = [torch.from_numpy(w["frame"](i)).to(dev) for i in range(max(8, B))]

    def batch_of(i):
        return [clouds[(i * B + j) % len(clouds)] for j in range(B)]
    forms = tuple(FORMS)
    seq = {f: _plan(sd, w, dev, f) for f in forms}
    fly = {f: [_plan(sd, w, dev, f, overlap=False) for _ in range(3)] for f in forms}
    assert seq["sparse_entry"].sparse_entry and not seq["dense_entry"].sparse_entry
    streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
    for f in forms:
        cap = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(cap):
            seq[f].capture(w["points_cap"])
        for pl, st in zip(fly[f], streams):
            with torch.cuda.stream(st):
                pl.capture(w["points_cap"])
    torch.cuda.synchronize()
    equal = True
    for i in range(4):
        res = {}
        for f in forms:
            seq[f].run_graph(batch_of(i))
            torch.cuda.synchronize()
            res[f] = seq[f].results()
        for (ba, sa, la), (bb, sb, lb) in zip(res["sparse_entry"], res["dense_entry"]):
            equal &= (ba is None) == (bb is None)
            if ba is not None and bb is not None:
                equal &= bool(np.array_equal(ba, bb) and np.array_equal(sa, sb) and np.array_equal(la, lb))
    figs = {f: dict(seq=[], synced=[], inflight=[]) for f in forms}
    for r in range(repeats):
        for f in (forms if r % 2 == 0 else forms[::-1]):            # alternate the order: no drift favours one side
            figs[f]["seq"].append(_fps_sequential(seq[f], batch_of, steps, warmup))
            figs[f]["synced"].append(_fps_synced(seq[f], batch_of, steps, warmup))
            figs[f]["inflight"].append(_fps_inflight(fly[f], streams, batch_of, steps, warmup))
    out = dict(workload=config, batch=B, repeats=repeats, steps=steps, detections_bit_equal=bool(equal))
    for f in forms:
        out[f] = dict(fps_sequential=_spread(figs[f]["seq"]), fps_host_synced=_spread(figs[f]["synced"]),
                      fps_inflight3=_spread(figs[f]["inflight"]))
    out["sparse_over_dense"] = {k: out["sparse_entry"][k]["median"] / out["dense_entry"][k]["median"]
                                for k in ("fps_sequential", "fps_host_synced", "fps_inflight3")}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workloads", default="car")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    rec = dict(tool="bench_conv0_entry", device=torch.cuda.get_device_name(0),
               results=[measure(c, dev, a.steps, a.warmup, a.repeats) for c in a.workloads.split(",")])
    print(json.dumps(rec, default=float))


if __name__ == "__main__":
    main()
