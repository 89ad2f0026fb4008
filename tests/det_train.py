#!/usr/bin/env python
"""The training workload of the deterministic-mode tests (tests/test_gpu_determinism.py) and of
tools/bench_determinism.py: car_cfg, K21 frames with 8 synthetic car boxes each, adam_onecycle with the config's
gradient clip, everything seeded (model init, frames, boxes, batch order) -- the workload of
tests/analysis/train_trajectory.py.  `run()` returns every step's loss and loss terms and, at the end, the flat
parameters and both Adam moments, so that two runs can be compared with torch.equal.

As a script it runs the same workload with the gradient exchange forced through a one-rank `nccl` (RCCL) communicator
(a process group needs a process of its own) and saves the result with torch.save:

    python tests/det_train.py --rccl --steps 30 --precision fp32 --out result.pt
"""
import argparse
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import sassd  # noqa: E402,F401
from sassd import autograd as AG, synth, train  # noqa: E402
import bench  # noqa: E402


@contextlib.contextmanager
def torch_deterministic(on):
    """torch.use_deterministic_algorithms(on) for the block (warn_only: a torch op without a deterministic
    implementation warns instead of raising -- the bit comparison of the tests is the arbiter), the previous setting
    restored afterwards."""
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(on, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=prev_warn)


def run(dev, steps=30, precision="fp32", deterministic=True, workload="car", batch=2, frames=8, seed=0, sync_force=False,
        first_grad=False, timing=False):
    """-> dict(loss=[steps tensors], terms={name: [steps tensors]}, params, exp_avg, exp_avg_sq[, grad0][, step_ms]).
    deterministic: True / False sets train_cfg['deterministic']; None leaves the key out (the torch flag decides).
    first_grad: also return the flat gradient of the first backward (before the exchange and the update)."""
    prev = AG.bev_precision()
    AG.set_bev_precision(precision)
    try:
        torch.manual_seed(seed)
        w = synth.workload(workload)
        model, cfg = synth.build_detector_for(w, seed, train=True, cls_bias=-3.0)
        model = model.to(dev)
        if deterministic is not None:
            model.train_cfg['deterministic'] = bool(deterministic)
        anchors = dict(Car=torch.from_numpy(w["anchors"]).to(dev))
        anchors_bv = dict(Car=torch.from_numpy(w["anchors_bv"]).to(dev))
        opt = train.build_optimizer(model, cfg.optimizer, 1)
        sched = train.build_scheduler(opt, max(steps, 1), 1, cfg.optimizer, cfg.lr_config)
        sync = train.GradSync(opt.flat, force=sync_force)
        if sync_force:
            assert sync.on
        host = [w["frame"](i) for i in range(frames)]
        clouds = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in host]
        gts = [torch.from_numpy(bench.synth_gt_on_points(p, i, 8, "car")).to(dev) for i, p in enumerate(host)]
        types = [np.array(["Car"] * 8) for _ in range(frames)]
        cal = w["cal"]
        out = dict(loss=[], terms={})
        ms = []
        for it in range(steps):
            ids = [(it * batch + j) % frames for j in range(batch)]
            b = train.device_batch([clouds[k] for k in ids], [gts[k] for k in ids], [types[k] for k in ids], ["Car"],
                                   anchors, anchors_bv, cal["voxel_size"], cal["pc_range"], max_points=cal["max_points"],
                                   max_voxels=cal["max_voxels"], model=model)
            if first_grad and it == 0:
                opt.zero_grad()
                loss0, _ = train.parse_losses(model(**b))
                loss0.backward()
                opt.flat.collect(0, len(opt.flat.params))
                out["grad0"] = opt.flat._grad.detach().clone()
            if timing:
                ev = [torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)]
                ev[0].record()
            loss, terms = train.train_one_iter(model, opt, sched, sync, b, it)
            if timing:
                ev[1].record()
                ev[1].synchronize()
                ms.append(ev[0].elapsed_time(ev[1]))
            out["loss"].append(loss.detach().clone())
            for k, v in terms.items():
                out["terms"].setdefault(k, []).append(v.detach().clone())
        torch.cuda.synchronize()
        out["params"] = opt.flat.data.detach().clone()
        out["exp_avg"] = opt.exp_avg.detach().clone()
        out["exp_avg_sq"] = opt.exp_avg_sq.detach().clone()
        out["deterministic"] = opt.deterministic
        if timing:
            out["step_ms"] = ms
        return out
    finally:
        AG.set_bev_precision(prev)


def to_cpu(r):
    def cp(v):
        if torch.is_tensor(v):
            return v.cpu()
        if isinstance(v, dict):
            return {k: cp(x) for k, x in v.items()}
        if isinstance(v, list):
            return [cp(x) for x in v]
        return v
    return cp(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rccl", action="store_true", help="gradients through a one-rank nccl communicator (GradSync force)")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    if a.rccl:
        from sassd import dist as D
        _, _, world = D.init("nccl", force_single=True)
        assert world == 1
    r = run(dev, steps=a.steps, precision=a.precision, deterministic=True, sync_force=a.rccl)
    torch.save(to_cpu(r), a.out)
    if a.rccl:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
