"""The deterministic training mode against the default step, in one process (train_cfg['deterministic']).

car_cfg batch 2 training (the workload of tests/det_train.py: K21 frames + 8 synthetic car boxes each, adam_onecycle, grad
clip on), fp32 and bf16 BEV convolutions.  Per precision one model trains with the mode off and one with it on; the two are
stepped in alternating blocks of `--steps` steps, `--repeats` blocks each, after `--warmup` steps.  A step is timed with
stream events around train.train_one_iter (forward, backward, exchange, update; the batch is built before the first event).
One JSON record: per precision and mode the median and min..max over the blocks of the per-block median step time, and the
on / off ratio.

    python tools/bench_determinism.py [--steps 20] [--warmup 5] [--repeats 5] [--out profiles/bench_determinism.json]
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
from sassd import _C, autograd as AG, synth, train  # noqa: E402


class Trainer:
    def __init__(self, dev, deterministic, seed=0, batch=2, frames=8):
        w = synth.workload("car")
        torch.manual_seed(seed)
        model, cfg = synth.build_detector_for(w, seed, train=True, cls_bias=-3.0)
        self.model = model.to(dev)
        self.model.train_cfg['deterministic'] = bool(deterministic)
        self.anchors = dict(Car=torch.from_numpy(w["anchors"]).to(dev))
        self.anchors_bv = dict(Car=torch.from_numpy(w["anchors_bv"]).to(dev))
        self.opt = train.build_optimizer(self.model, cfg.optimizer, 1)
        assert self.opt.deterministic == bool(deterministic)
        self.sched = train.build_scheduler(self.opt, 10 ** 6, 1, cfg.optimizer, cfg.lr_config)
        self.sync = train.GradSync(self.opt.flat)
        host = [w["frame"](i) for i in range(frames)]
        self.clouds = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in host]
        self.gts = [torch.from_numpy(bench.synth_gt_on_points(p, i, 8, "car")).to(dev) for i, p in enumerate(host)]
        self.types = [np.array(["Car"] * 8) for _ in range(frames)]
        self.cal, self.batch, self.frames, self.it = w["cal"], batch, frames, 0

    def step(self):
        ids = [(self.it * self.batch + j) % self.frames for j in range(self.batch)]
        cal = self.cal
        b = train.device_batch([self.clouds[k] for k in ids], [self.gts[k] for k in ids], [self.types[k] for k in ids],
                               ["Car"], self.anchors, self.anchors_bv, cal["voxel_size"], cal["pc_range"],
                               max_points=cal["max_points"], max_voxels=cal["max_voxels"], model=self.model)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        train.train_one_iter(self.model, self.opt, self.sched, self.sync, b, self.it)
        e1.record()
        e1.synchronize()
        self.it += 1
        return e0.elapsed_time(e1)


def _spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = dict(workload="car_cfg batch 2 training, K21 frames + 8 synthetic car boxes, adam_onecycle, grad clip 10",
               steps=a.steps, warmup=a.warmup, repeats=a.repeats, csrc_hash=_C.csrc_hash(), device=torch.cuda.get_device_name(0),
               results={})
    prev = AG.bev_precision()
    try:
        for prec in a.precisions.split(","):
            AG.set_bev_precision(prec)
            tr = {False: Trainer(dev, False), True: Trainer(dev, True)}
            for t in tr.values():
                for _ in range(a.warmup):
                    t.step()
            blocks = {False: [], True: []}
            for _ in range(a.repeats):
                for mode in (False, True):
                    blocks[mode].append(statistics.median(tr[mode].step() for _ in range(a.steps)))
            off, on = _spread(blocks[False]), _spread(blocks[True])
            rec["results"][prec] = dict(default_ms=off, deterministic_ms=on, ratio=on["median"] / off["median"])
            print(prec, "default %.3f ms [%.3f..%.3f]  deterministic %.3f ms [%.3f..%.3f]  ratio %.4f" % (
                off["median"], off["min"], off["max"], on["median"], on["min"], on["max"], on["median"] / off["median"]),
                flush=True)
            del tr
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
