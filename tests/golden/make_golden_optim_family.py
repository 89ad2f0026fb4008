"""Generate tests/golden/optim_family_ref.npz by running the reference's own optimizer stack on the CPU (build container
only): tools/train_utils/optimization/__init__.py -- build_optimizer('adam' | 'sgd') + build_scheduler('cosine' |
'step', with the cosine warm-up in front) + clip_grad_norm_ and the warm-up / main switch exactly as train_one_epoch has
them (tools/train_utils/__init__.py:39-61) -- on the tiny Linear/BatchNorm model of make_golden_optim.py with seeded
synthetic gradients, every third step scaled to be clipped, 20 iterations.

Per pair (adam | sgd) x (cosine | step [8, 14]): per-step parameters and lr, and `fp64_dist`, the maximum distance between
the reference's fp32 trajectory and its own float64 run of the same steps (the error the reference's arithmetic carries:
the GPU test's bar is held against it).  `lr_nowarm/<policy>`: the lr of the 20 iterations without the warm-up.
Resume cases, as arrays only: the optimizer.state_dict() contents of a reference 'adam_onecycle' run after 8 steps (per
index exp_avg / exp_avg_sq / step, the group index lists), the model_state key order, parameters after steps 7..15; the
same for 'sgd' (momentum_buffer; its continuation is the (sgd, cosine) trajectory itself).

    python tests/golden/make_golden_optim_family.py
"""
import collections
import collections.abc
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch
from torch import nn
from torch.nn.utils import clip_grad_norm_

collections.Iterable = collections.abc.Iterable          # the reference predates python 3.10
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = "/root/reference/tools/train_utils/optimization"
ITERS, RESUME_AT, RESUME_END = 20, 8, 16


class AttrDict(dict):
    __getattr__ = dict.__getitem__


def tiny_model():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(6, 5), nn.BatchNorm1d(5), nn.ReLU(), nn.Linear(5, 3, bias=False))


def gradients(model):
    """grads[it][name], fp32: the same stream for every run"""
    g = torch.Generator().manual_seed(1)
    out = []
    for it in range(ITERS):
        scale = 40.0 if it % 3 == 0 else 0.5                          # every third step exceeds max_norm -> clipped
        out.append({n: torch.randn(p.shape, generator=g) * scale for n, p in model.named_parameters()})
    return out


def cur_lr(opt):
    try:
        return float(opt.lr)
    except Exception:
        return float(opt.param_groups[0]['lr'])


def run(ro, ocfg, lcfg, grads, dtype=torch.float32, stop=ITERS, step_optimizer=True):
    """the loop of train_one_epoch -> (per-step {name: parameter}, per-step lr, optimizer, model)"""
    model = tiny_model().to(dtype)
    opt = ro.build_optimizer(model, ocfg)
    sched, warm = ro.build_scheduler(opt, total_iters_each_epoch=5, total_epochs=4, last_epoch=-1, optim_cfg=ocfg,
                                     lr_cfg=lcfg)
    params, lrs = [], []
    for it in range(stop):
        cur = warm if warm is not None and it <= warm.T_max else sched
        cur.step(it)
        lrs.append(cur_lr(opt))
        if not step_optimizer:
            continue
        opt.zero_grad()
        for n, p in model.named_parameters():
            p.grad = grads[it][n].to(dtype).clone()
        clip_grad_norm_(model.parameters(), **ocfg.grad_clip)
        opt.step()
        params.append({n: p.detach().clone() for n, p in model.named_parameters()})
    return params, lrs, opt, model


def main():
    warnings.filterwarnings("ignore", category=UserWarning)           # scheduler.step(epoch) is deprecated, not gone
    spec = importlib.util.spec_from_file_location("ref_optimization", os.path.join(PKG, "__init__.py"),
                                                  submodule_search_locations=[PKG])
    ro = importlib.util.module_from_spec(spec)
    sys.modules["ref_optimization"] = ro
    spec.loader.exec_module(ro)

    model = tiny_model()
    names = [n for n, _ in model.named_parameters()]
    grads = gradients(model)
    out = {"init/" + n: p.detach().clone().numpy() for n, p in model.named_parameters()}
    for it in range(ITERS):
        for n in names:
            out["grad%d/%s" % (it, n)] = grads[it][n].numpy()
    out["names"] = np.array(names)
    out["model_state_keys"] = np.array(list(model.state_dict().keys()))

    clip = AttrDict(max_norm=10, norm_type=2)
    ocfgs = dict(adam=AttrDict(type="adam", lr=0.01, weight_decay=0.01, grad_clip=clip),
                 sgd=AttrDict(type="sgd", lr=0.01, weight_decay=0.01, momentum=0.9, grad_clip=clip))
    warm = dict(warmup=True, warmup_iters=4, warmup_ratio=0.1)
    lcfgs = dict(cosine=AttrDict(policy="cosine", **warm), step=AttrDict(policy="step", step=[8, 14], **warm))
    for oname, ocfg in ocfgs.items():
        for lname, lcfg in lcfgs.items():
            pair = "%s_%s" % (oname, lname)
            p32, lrs, _, _ = run(ro, ocfg, lcfg, grads)
            p64, lrs64, _, _ = run(ro, ocfg, lcfg, grads, dtype=torch.float64)
            assert lrs == lrs64
            for it in range(ITERS):
                for n in names:
                    out["%s/step%d/%s" % (pair, it, n)] = p32[it][n].numpy()
            out[pair + "/lr"] = np.array(lrs)
            out[pair + "/fp64_dist"] = np.array(max(float((p32[it][n].double() - p64[it][n]).abs().max())
                                                    for it in range(ITERS) for n in names))
            print(pair, "fp32 - fp64 max distance %.3g" % out[pair + "/fp64_dist"], "lr", lrs[:6])
    for lname, lcfg in lcfgs.items():
        nowarm = AttrDict({k: v for k, v in lcfg.items() if not k.startswith("warmup")})
        out["lr_nowarm/" + lname] = np.array(run(ro, ocfgs["sgd"], nowarm, grads, step_optimizer=False)[1])

    def record_state(tag, opt, keys):
        sd = opt.state_dict()
        for gi, g in enumerate(sd["param_groups"]):
            out["%s/group%d" % (tag, gi)] = np.array(g["params"], dtype=np.int64)
        out[tag + "/n_groups"] = np.array(len(sd["param_groups"]))
        for idx, entry in sd["state"].items():
            for k in keys:
                out["%s/%s/%d" % (tag, k, idx)] = entry[k].detach().clone().numpy()
            if "step" in entry:
                out["%s/step/%d" % (tag, idx)] = np.array(int(entry["step"]))

    # resume, 'adam_onecycle' (the configuration of make_golden_optim.py): the state after 8 steps, the run to step 15
    ocfg = AttrDict(type="adam_onecycle", lr=0.003, weight_decay=0.01, grad_clip=clip)
    lcfg = AttrDict(policy="onecycle", moms=[0.95, 0.85], div_factor=10, pct_start=0.4)
    _, _, opt, _ = run(ro, ocfg, lcfg, grads, stop=RESUME_AT)
    record_state("resume_onecycle", opt, ("exp_avg", "exp_avg_sq"))
    p32, lrs, _, _ = run(ro, ocfg, lcfg, grads, stop=RESUME_END)
    for it in range(RESUME_AT - 1, RESUME_END):
        for n in names:
            out["resume_onecycle/step%d/%s" % (it, n)] = p32[it][n].numpy()
    out["resume_onecycle/lr"] = np.array(lrs)
    # resume, 'sgd': the state of the (sgd, cosine) run after 8 steps; its continuation is recorded above
    _, _, opt, _ = run(ro, ocfgs["sgd"], lcfgs["cosine"], grads, stop=RESUME_AT)
    record_state("resume_sgd", opt, ("momentum_buffer",))

    np.savez_compressed(os.path.join(HERE, "optim_family_ref.npz"), **out)
    print("optim_family_ref.npz", len(out), "arrays")


if __name__ == "__main__":
    main()
