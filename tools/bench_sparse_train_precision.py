"""The bf16 sparse training mode (train_cfg['sparse_precision'] = 'bf16') against the fp32 sparse backbone, in one process.

car_cfg batch 2 training (the workload of tests/det_train.py and tools/bench_determinism.py), fp32 and bf16 dense convolutions, each
with the fp32 and the bf16 sparse backbone.  Per dense precision one model per sparse precision; the two are stepped in alternating
blocks of `--steps` steps, `--repeats` blocks each, after `--warmup` steps.  A step is timed with stream events around
train.train_one_iter.  Then, in `--profile-steps` separate steps per model, every sparse launch is bracketed by its own pair of
HIP events (sparse forward, data gradient, weight gradient, the sparse BatchNorm + ReLU) and the peak allocated memory of a step is
read.  One JSON record: per combination the median and min..max over the blocks of the per-block median step time, the summed
event times per step and category, the peak memory, and the bf16 / fp32 ratios.

`--trajectory N` also records an N-step loss trajectory of bf16 sparse + bf16 dense (tests/analysis/train_trajectory.py's seeded
workload) and compares the mean of its last 20 steps with the spread of the recorded fp32 runs (`--fp32-trajectory`).

    python tools/bench_sparse_train_precision.py [--steps 20] [--warmup 5] [--repeats 5] [--trajectory 200] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "analysis"))

from sassd import _C, autograd as AG, kernels as K  # noqa: E402
from bench_determinism import Trainer, _spread  # noqa: E402

# wrapper name -> category; the raw bf16 kernel serves forward and data gradient: told apart by whether autograd is running a backward
CATEGORIES = dict(spconv_fwd="sparse_fwd", spconv_bwd_data="sparse_dgrad", spconv_bwd_weight="sparse_wgrad",
                  spconv_fwd_bf16_raw=None, spconv_bwd_weight_bf16="sparse_wgrad", bn_relu_fwd="sparse_bn", bn_relu_bwd="sparse_bn")


class EventProfile:
    """`with EventProfile() as p:` brackets every sparse launch made through sassd.kernels with a pair of stream events"""

    def __enter__(self):
        self.events, self.saved = [], {}
        for name, cat in CATEGORIES.items():
            fn = getattr(K, name)
            self.saved[name] = fn
            setattr(K, name, self._wrap(fn, cat))
        return self

    def _wrap(self, fn, cat):
        def call(*a, **kw):
            c = cat or ("sparse_dgrad" if torch._C._current_graph_task_id() >= 0 else "sparse_fwd")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **kw)
            e1.record()
            self.events.append((c, e0, e1))
            return out
        return call

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(K, name, fn)
        return False

    def totals_ms(self):
        torch.cuda.synchronize()
        out = {}
        for c, e0, e1 in self.events:
            out[c] = out.get(c, 0.0) + e0.elapsed_time(e1)
        return out


def make_trainer(dev, sparse):
    """bench_determinism's Trainer (default, non-deterministic step) with the sparse precision in the detector's train_cfg"""
    with AG.sparse_precision_scope(sparse):                   # the optimizer's PackPlan is built for the mode
        t = Trainer(dev, False)
    t.model.train_cfg['sparse_precision'] = sparse
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--precisions", default="fp32,bf16", help="dense precisions")
    ap.add_argument("--trajectory", type=int, default=0)
    ap.add_argument("--fp32-trajectory", default=os.path.join(ROOT, "profiles", "r06_train_trajectory.json"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = dict(workload="car_cfg batch 2 training, K21 frames + 8 synthetic car boxes, adam_onecycle, grad clip 10",
               steps=a.steps, warmup=a.warmup, repeats=a.repeats, profile_steps=a.profile_steps, csrc_hash=_C.csrc_hash(),
               device=torch.cuda.get_device_name(0), results={})
    prev = AG.bev_precision()
    try:
        for dense in a.precisions.split(","):
            AG.set_bev_precision(dense)
            tr = {sp: make_trainer(dev, sp) for sp in ("fp32", "bf16")}
            for t in tr.values():
                for _ in range(a.warmup):
                    t.step()
            blocks = {sp: [] for sp in tr}
            for _ in range(a.repeats):
                for sp, t in tr.items():
                    blocks[sp].append(statistics.median(t.step() for _ in range(a.steps)))
            res = {}
            for sp, t in tr.items():
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                t.step()
                peak = torch.cuda.max_memory_allocated()
                with EventProfile() as p:
                    for _ in range(a.profile_steps):
                        t.step()
                ev = {c: v / a.profile_steps for c, v in p.totals_ms().items()}
                ev["sparse_total"] = sum(ev.values())
                res[sp + "_sparse"] = dict(step_ms=_spread(blocks[sp]), sparse_event_ms_per_step=ev, peak_allocated_mib=peak / 2 ** 20)
            f, b = res["fp32_sparse"], res["bf16_sparse"]
            res["bf16_over_fp32"] = dict(
                step=b["step_ms"]["median"] / f["step_ms"]["median"],
                peak_allocated=b["peak_allocated_mib"] / f["peak_allocated_mib"],
                **{c: b["sparse_event_ms_per_step"][c] / v for c, v in f["sparse_event_ms_per_step"].items()
                   if c in b["sparse_event_ms_per_step"] and v > 0})
            rec["results"][dense + "_dense"] = res
            for sp in ("fp32_sparse", "bf16_sparse"):
                s = res[sp]["step_ms"]
                print("%s dense, %s: %.3f ms [%.3f..%.3f]  events %s  peak %.0f MiB" % (
                    dense, sp, s["median"], s["min"], s["max"],
                    {c: round(v, 3) for c, v in res[sp]["sparse_event_ms_per_step"].items()}, res[sp]["peak_allocated_mib"]), flush=True)
            del tr
        if a.trajectory:
            import numpy as np
            import train_trajectory as TT
            AG.set_sparse_precision("bf16")
            try:
                curves = TT.run("bf16", a.trajectory, dev)
            finally:
                AG.set_sparse_precision("fp32")
            tail = TT.summary(curves)
            traj = dict(steps=a.trajectory, tail_mean_last_20_steps=tail, loss=curves["loss"],
                        finite=bool(np.isfinite(curves["loss"]).all()))
            if os.path.exists(a.fp32_trajectory):
                ref = json.load(open(a.fp32_trajectory))["tail_mean_last_20_steps"]
                lo, hi = sorted((ref["fp32"]["loss"], ref["fp32_again"]["loss"]))
                traj["fp32_runs_tail_loss"] = [lo, hi]
                traj["bf16_dense_fp32_sparse_tail_loss"] = ref["bf16"]["loss"]
                traj["inside_fp32_spread"] = bool(lo <= tail["loss"] <= hi)
                traj["distance_to_fp32_spread"] = float(max(lo - tail["loss"], tail["loss"] - hi, 0.0))
                traj["fp32_spread_width"] = hi - lo
            rec["trajectory_bf16_sparse_bf16_dense"] = traj
            print("trajectory:", {k: v for k, v in traj.items() if k != "loss"}, flush=True)
    finally:
        AG.set_bev_precision(prev)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
