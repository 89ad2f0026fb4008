"""bf16 against fp32 inference on the same weights, in one process (InferencePlan(precision=..., sparse_precision=...)).

For each workload (car batch 1, multi_cfg batch 8) four plans are built from the bench model (bench.build_model) -- fp32, bf16 dense
convs, bf16 dense convs + bf16 sparse backbone, fp32 dense convs + bf16 sparse backbone (PLANS) -- and measured in turn,
`--repeats` times each:
  * sequential frames/s: one plan's captured frame (two-branch graph) replayed `--steps` times back to back;
  * frames in flight: three one-branch plans on three streams (bench.py's form);
  * the BEV stage: per-layer events of plan.prof (bev_conv0..7) and the heads (fused SSD head + both part-sensitive convs), on
    eager frames;
  * the sparse stage: the `sparse` segment of plan.prof (rulebook pyramid waits + 14 sparse convs), and each sparse conv on its
    own (sparse_conv0..13, plan.prof_sparse_layers: events between the launches, on separate eager frames).
One JSON record: median and min..max over the repeats per figure, the bf16 / fp32 ratios, and the largest difference per detection
field between the two plans on the same seeded frames (count, boxes, scores, labels of the detections both plans keep).

    python tools/bench_precision.py [--steps 200] [--warmup 20] [--repeats 5] [--workloads car,multi]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from sassd.pipeline import InferencePlan  # noqa: E402


# plan name -> (precision, sparse_precision): the dense convs and the sparse backbone choose independently
PLANS = {"fp32": ("fp32", "fp32"), "bf16": ("bf16", "fp32"), "bf16_sparse": ("bf16", "bf16"), "fp32_dense_bf16_sparse": ("fp32", "bf16")}


def _plan(sd, w, dev, name, overlap=True):
    precision, sparse_precision = PLANS[name]
    return InferencePlan(sd, batch_size=w["batch"], anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev,
                         overlap=overlap, precision=precision, sparse_precision=sparse_precision, **w["plan"])


def _spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v))


def _fps_sequential(plan, batch_of, steps, warmup):
    for i in range(warmup):
        plan.run_graph(batch_of(i))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        plan.run_graph(batch_of(i))
    e1.record()
    torch.cuda.synchronize()
    return steps * plan.B / (e0.elapsed_time(e1) / 1e3)


def _fps_inflight(plans, streams, batch_of, steps, warmup):
    S = len(plans)

    def step(i):
        with torch.cuda.stream(streams[i % S]):
            plans[i % S].run_graph(batch_of(i))
    for i in range(max(warmup, S)):
        step(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in streams:
        s.wait_event(e0)
    for i in range(steps):
        step(i)
    for s in streams:
        torch.cuda.current_stream().wait_stream(s)
    e1.record()
    torch.cuda.synchronize()
    return steps * plans[0].B / (e0.elapsed_time(e1) / 1e3)


def _stage_ms(plan, batch, frames=10):
    """per-segment milliseconds (median over `frames` eager frames) from plan.prof"""
    plan.prof = {}
    for _ in range(frames):
        plan.run_from_points(batch)
    torch.cuda.synchronize()
    out = {k: statistics.median(a.elapsed_time(b) for a, b in v) for k, v in plan.prof.items()}
    # the sparse segment (rulebook waits included) on frames without per-layer events, then each sparse conv on its own
    plan.prof_sparse_layers = True
    for _ in range(frames):
        plan.run_from_points(batch)
    torch.cuda.synchronize()
    out.update({k: statistics.median(a.elapsed_time(b) for a, b in v) for k, v in plan.prof.items() if k.startswith("sparse_conv")})
    plan.prof, plan.prof_sparse_layers = None, False
    out["bev"] = sum(v for k, v in out.items() if k.startswith("bev_conv"))
    out["bev+heads"] = out["bev"] + out.get("heads", 0.0)
    out["sparse_convs"] = sum(v for k, v in out.items() if k.startswith("sparse_conv") and k != "sparse_convs")
    return out


def _detections(plan):
    torch.cuda.synchronize()
    return plan.results()


def _det_diff(a, b):
    """largest difference per field between two per-sample detection lists, over detections matched by order"""
    d = dict(count=0, boxes=np.zeros(7), scores=0.0, labels_differ=0, samples=len(a))
    for (ba, sa, la), (bb, sb, lb) in zip(a, b):
        na, nb = (0 if ba is None else len(ba)), (0 if bb is None else len(bb))
        d["count"] = max(d["count"], abs(na - nb))
        n = min(na, nb)
        if n:
            d["boxes"] = np.maximum(d["boxes"], np.abs(ba[:n].astype(np.float64) - bb[:n]).max(0))
            d["scores"] = max(d["scores"], float(np.abs(sa[:n].astype(np.float64) - sb[:n]).max()))
            d["labels_differ"] += int((la[:n] != lb[:n]).sum())
    d["boxes"] = [float(x) for x in d["boxes"]]
    return d


def measure(config, dev, steps, warmup, repeats):
    model, w = bench.build_model(0, dev, config)
    sd = model.state_dict()
    B = w["batch"]
    clouds = [torch.from_numpy(w["frame"](i)).to(dev) for i in range(max(8, B))]

    def batch_of(i):
        return [clouds[(i * B + j) % len(clouds)] for j in range(B)]
    precs = tuple(PLANS)
    seq = {p: _plan(sd, w, dev, p) for p in precs}
    fly = {p: [_plan(sd, w, dev, p, overlap=False) for _ in range(3)] for p in precs}
    eager = {p: _plan(sd, w, dev, p) for p in precs}
    streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
    for p in precs:
        cap = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(cap):
            seq[p].capture(w["points_cap"])
        for pl, st in zip(fly[p], streams):
            with torch.cuda.stream(st):
                pl.capture(w["points_cap"])
    torch.cuda.synchronize()
    # detections of the two plans on the same seeded frames
    diffs, counts = [], {p: 0 for p in precs}
    for i in range(4):
        res = {}
        for p in precs:
            eager[p].run_from_points(batch_of(i))
            res[p] = _detections(eager[p])
            assert int(eager[p].status.item()) == 0, (p, "status 0x%x" % int(eager[p].status.item()))
            counts[p] += sum(0 if r[0] is None else len(r[0]) for r in res[p])
        diffs.append({p: _det_diff(res["fp32"], res[p]) for p in precs if p != "fp32"})

    def det_of(p):
        d_ = [d[p] for d in diffs]
        return dict(count=max(d["count"] for d in d_), boxes=list(np.max([d["boxes"] for d in d_], 0)),
                    scores=max(d["scores"] for d in d_), labels_differ=sum(d["labels_differ"] for d in d_),
                    detections=dict(fp32=counts["fp32"], **{p: counts[p]}), frames=4 * B)
    figs = {p: dict(seq=[], inflight=[], bev=[], bev_heads=[], sparse=[], sparse_convs=[], layers={}) for p in precs}
    for r in range(repeats):
        for p in (precs if r % 2 == 0 else precs[::-1]):          # alternate the order: no drift favours one side
            f = figs[p]
            st = _stage_ms(eager[p], batch_of(r))
            f["bev"].append(st["bev"])
            f["bev_heads"].append(st["bev+heads"])
            f["sparse"].append(st["sparse"])
            f["sparse_convs"].append(st["sparse_convs"])
            for k, v in st.items():
                if k.startswith("bev_conv") or k.startswith("sparse_conv") or k in ("heads", "densify"):
                    f["layers"].setdefault(k, []).append(v)
            f["seq"].append(_fps_sequential(seq[p], batch_of, steps, warmup))
            f["inflight"].append(_fps_inflight(fly[p], streams, batch_of, steps, warmup))
    out = dict(workload=config, batch=B, repeats=repeats, steps=steps)
    for p in precs:
        f = figs[p]
        out[p] = dict(precision=PLANS[p][0], sparse_precision=PLANS[p][1], fps_sequential=_spread(f["seq"]),
                      fps_inflight3=_spread(f["inflight"]), bev_ms=_spread(f["bev"]), bev_heads_ms=_spread(f["bev_heads"]),
                      sparse_ms=_spread(f["sparse"]), sparse_convs_ms=_spread(f["sparse_convs"]),
                      layers_ms={k: statistics.median(v) for k, v in sorted(f["layers"].items())})
    med = lambda p, k: out[p][k]["median"]      # noqa: E731
    out["bf16_over_fp32"] = dict(bev_speedup=med("fp32", "bev_ms") / med("bf16", "bev_ms"),
                                 bev_heads_speedup=med("fp32", "bev_heads_ms") / med("bf16", "bev_heads_ms"),
                                 fps_sequential=med("bf16", "fps_sequential") / med("fp32", "fps_sequential"),
                                 fps_inflight3=med("bf16", "fps_inflight3") / med("fp32", "fps_inflight3"))
    # the bf16 sparse backbone against the fp32 one, on plans whose dense convs are the same
    for p, base in (("bf16_sparse", "bf16"), ("fp32_dense_bf16_sparse", "fp32")):
        out["%s_over_%s" % (p, base)] = dict(
            sparse_speedup=med(base, "sparse_ms") / med(p, "sparse_ms"),
            sparse_convs_speedup=med(base, "sparse_convs_ms") / med(p, "sparse_convs_ms"),
            fps_sequential=med(p, "fps_sequential") / med(base, "fps_sequential"),
            fps_inflight3=med(p, "fps_inflight3") / med(base, "fps_inflight3"),
            layer_speedup={"sparse_conv%d" % i: out[base]["layers_ms"]["sparse_conv%d" % i] / out[p]["layers_ms"]["sparse_conv%d" % i]
                           for i in range(14)})
    out["detections_bf16_vs_fp32"] = det_of("bf16")
    out["detections_bf16_sparse_vs_fp32"] = det_of("bf16_sparse")
    out["detections_fp32_dense_bf16_sparse_vs_fp32"] = det_of("fp32_dense_bf16_sparse")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workloads", default="car,multi")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    rec = dict(tool="bench_precision", device=torch.cuda.get_device_name(0),
               results=[measure(c, dev, a.steps, a.warmup, a.repeats) for c in a.workloads.split(",")])
    print(json.dumps(rec, default=float))


if __name__ == "__main__":
    main()
