"""Shared by test_optim_family_cpu.py and test_gpu_optim_family.py: the recorded runs of the reference's optimizer stack
(tests/golden/make_golden_optim_family.py -> optim_family_ref.npz), the tiny model they ran on, the configurations, and
a reference-format checkpoint rebuilt from the recorded arrays."""
import collections
import os

import numpy as np
import torch

O = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_family_ref.npz"))
NAMES = [str(n) for n in O["names"]]
ITERS = 20
CLIP = dict(max_norm=10, norm_type=2)
OPTIM = dict(adam=dict(type="adam", lr=0.01, weight_decay=0.01, grad_clip=CLIP),
             sgd=dict(type="sgd", lr=0.01, weight_decay=0.01, momentum=0.9, grad_clip=CLIP),
             adam_onecycle=dict(type="adam_onecycle", lr=0.003, weight_decay=0.01, grad_clip=CLIP))
WARM = dict(warmup=True, warmup_iters=4, warmup_ratio=0.1)
LR = dict(cosine=dict(policy="cosine"), step=dict(policy="step", step=[8, 14]),
          onecycle=dict(policy="onecycle", moms=[0.95, 0.85], div_factor=10, pct_start=0.4))
STATE_KEYS = dict(resume_onecycle=("exp_avg", "exp_avg_sq"), resume_sgd=("momentum_buffer",))
# where each resume case starts from (parameters after step 7) and what it must follow (steps 8..15)
RESUME = dict(resume_onecycle=("adam_onecycle", "onecycle", "resume_onecycle"), resume_sgd=("sgd", "cosine", "sgd_cosine"))


def tiny_model(params=None):
    """the model of the golden runs; parameters from O['init/*'] or from `params` {name: array}"""
    model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.BatchNorm1d(5), torch.nn.ReLU(),
                                torch.nn.Linear(5, 3, bias=False))
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.from_numpy(params[n] if params is not None else O["init/" + n]))
    return model


def lr_cfg(policy, warm=True):
    return dict(LR[policy], **(WARM if warm and policy != "onecycle" else {}))


def params_after(run, it):
    return {n: O["%s/step%d/%s" % (run, it, n)] for n in NAMES}


def torch_state(tag, swap_groups=False, prefix=""):
    """(optimizer_state, model_state) of a reference checkpoint after 8 steps, rebuilt from the recorded arrays: the
    torch optimizer format {'state': {index: {...}}, 'param_groups': [{'params': [...]}, ...]} and an ordered model_state
    in the recorded key order (parameters after step 7; buffers from a fresh model)."""
    n_groups = int(O[tag + "/n_groups"])
    groups = [dict(params=[int(i) for i in O["%s/group%d" % (tag, g)]], lr=0.0) for g in range(n_groups)]
    if swap_groups:
        groups = groups[::-1]
    state = {}
    for g in groups:
        for i in g["params"]:
            entry = {k: torch.from_numpy(O["%s/%s/%d" % (tag, k, i)].copy()) for k in STATE_KEYS[tag]}
            if "%s/step/%d" % (tag, i) in O:
                entry["step"] = torch.tensor(float(O["%s/step/%d" % (tag, i)]))      # a 0-d tensor, as torch >= 1.12 keeps it
            state[i] = entry
    start = params_after(RESUME[tag][2], 7)
    fresh = tiny_model().state_dict()
    model_state = collections.OrderedDict()
    for k in O["model_state_keys"]:
        k = str(k)
        model_state[prefix + k] = torch.from_numpy(start[k].copy()) if k in start else fresh[k].clone()
    return dict(state=state, param_groups=groups), model_state


def write_checkpoint(path, tag, **kw):
    ost, mst = torch_state(tag, **kw)
    torch.save(dict(epoch=1, it=8, model_state=mst, optimizer_state=ost, version="none"), str(path))
    return ost, mst
