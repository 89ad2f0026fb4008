"""Without a GPU: the optimizer family around its kernels -- build_optimizer('adam' | 'sgd' | 'adam_onecycle'),
build_scheduler('onecycle' | 'cosine' | 'step') with the warm-up in front, the C ABI's argument checks, flat state
round trips, and the mapping of a reference checkpoint's torch optimizer state onto the flat buffers (recorded runs of
the reference's own stack: tests/golden/make_golden_optim_family.py)."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import _C, train

import optim_family_cases as F

O = F.O
EINVAL = -1


def _lrs(policy, warm):
    class Opt:
        lr = F.OPTIM["sgd"]["lr"]
    opt, cfg = Opt(), F.lr_cfg(policy, warm)
    sched = train.build_scheduler(opt, 5, 4, F.OPTIM["sgd"], cfg)
    warmup = train.build_warmup_scheduler(opt, F.OPTIM["sgd"], cfg)
    assert (warmup is not None) == warm
    out = []
    for it in range(F.ITERS):
        (warmup if warmup is not None and it <= warmup.T_max else sched).step(it)       # runner.train_one_epoch's switch
        out.append(opt.lr)
    return np.array(out)


@pytest.mark.parametrize("policy", ["cosine", "step"])
def test_lr_values(policy):
    """every one of the 20 iterations, with and without the warm-up, to 1e-12 relative of the reference's lr"""
    for warm, ref in ((True, O["sgd_%s/lr" % policy]), (False, O["lr_nowarm/" + policy])):
        got = _lrs(policy, warm)
        assert ref.shape == (F.ITERS,) and np.all(ref > 0)
        assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref)), (policy, warm, got, ref)
    assert np.array_equal(O["adam_%s/lr" % policy], O["sgd_%s/lr" % policy])            # the schedule does not see the optimizer


def test_dispatch():
    kinds = dict(adam=train.Adam, sgd=train.SGD, adam_onecycle=train.AdamOneCycle)
    for typ, cls in kinds.items():
        opt = train.build_optimizer(F.tiny_model(), F.OPTIM[typ])
        assert type(opt) is cls and isinstance(opt, train.FlatOptimizer) and opt.type == typ
        assert opt.lr == F.OPTIM[typ]["lr"] and opt.max_norm == 10.0 and opt.pack_plan is None
        for policy in ("cosine", "step") + (("onecycle",) if typ == "adam_onecycle" else ()):
            sched = train.build_scheduler(opt, 5, 4, F.OPTIM[typ], F.lr_cfg(policy))
            sched.step(3)
            assert opt.lr > 0
    sgd = train.build_optimizer(F.tiny_model(), F.OPTIM["sgd"])
    assert sgd.momentum == 0.9 and train.build_optimizer(F.tiny_model(), F.OPTIM["adam"]).betas == (0.9, 0.999)
    with pytest.raises(ValueError):                    # 'onecycle' drives a momentum these optimizers do not have
        train.build_scheduler(sgd, 5, 4, F.OPTIM["sgd"], F.lr_cfg("onecycle"))
    with pytest.raises(NotImplementedError):
        train.build_optimizer(F.tiny_model(), dict(F.OPTIM["adam"], type="rmsprop"))
    with pytest.raises(NotImplementedError):
        train.build_scheduler(sgd, 5, 4, F.OPTIM["sgd"], dict(policy="poly"))


def test_abi_argument_checks():
    L = _C.lib()
    null, p16, p20 = None, C.c_void_p(16), C.c_void_p(20)
    adam = lambda p, g, m, v, n=10, step=1: L.sassd_adam_l2_step(p, g, m, v, n, null, 1e-3, 0.9, 0.999, 1e-8, 0.01, step,  # noqa: E731
                                                                 10.0, 1.0, null)
    sgd = lambda p, g, b, n=10: L.sassd_sgd_step(p, g, b, n, null, 1e-3, 0.9, 0.01, 10.0, 1.0, null)  # noqa: E731
    assert adam(null, null, null, null) == EINVAL
    for k in range(4):                                  # each pointer in turn: NULL, then not 16-byte aligned
        for bad in (null, p20):
            a = [p16] * 4
            a[k] = bad
            assert adam(*a) == EINVAL, (k, bad)
    assert adam(p16, p16, p16, p16, n=-1) == EINVAL
    assert adam(p16, p16, p16, p16, step=0) == EINVAL   # step counts from 1
    assert sgd(null, null, null) == EINVAL
    for k in range(3):
        for bad in (null, p20):
            a = [p16] * 3
            a[k] = bad
            assert sgd(*a) == EINVAL, (k, bad)
    assert sgd(p16, p16, p16, n=-1) == EINVAL


def _flat_views(opt, key):
    """{parameter name: the slice of the flat state `key` at that parameter's offset, shaped like it}"""
    out = {}
    for n, p, o in zip(F.NAMES, opt.flat.params, opt.flat.offsets):     # FlatParams keeps model.parameters() order = NAMES
        out[n] = getattr(opt, key)[o:o + p.numel()].view(p.shape)
    return out


def _expected(tag):
    """{state key: {parameter name: recorded tensor}} by the reference's own grouping: index i of group g is the i-th
    parameter of (non-BatchNorm leaves | BatchNorm leaves) for two groups, of model.parameters() for one"""
    bn = [n for n in F.NAMES if n.startswith("1.")]
    order = [n for n in F.NAMES if n not in bn] + bn if int(O[tag + "/n_groups"]) == 2 else F.NAMES
    return {k: {n: O["%s/%s/%d" % (tag, k, i)] for i, n in enumerate(order)} for k in F.STATE_KEYS[tag]}


@pytest.mark.parametrize("tag,prefix", [("resume_onecycle", ""), ("resume_onecycle", "module."), ("resume_sgd", "")])
def test_torch_state_maps_onto_the_flat_buffers(tmp_path, tag, prefix):
    typ = F.RESUME[tag][0]
    F.write_checkpoint(tmp_path / "ref.pth", tag, prefix=prefix)
    model = F.tiny_model()
    opt = train.build_optimizer(model, F.OPTIM[typ])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                 # a loaded state warns about nothing
        epoch, it = train.load_checkpoint(model, opt, str(tmp_path / "ref.pth"))
    assert (epoch, it) == (1, 8)
    want = _expected(tag)
    assert int(O[tag + "/n_groups"]) == (2 if typ == "adam_onecycle" else 1)
    for k, per_name in want.items():
        got = _flat_views(opt, k)
        for n in F.NAMES:
            assert got[n].shape == per_name[n].shape, (k, n)
            assert np.array_equal(got[n].numpy(), per_name[n]), (k, n)                   # bit for bit, at the parameter's offset
        inside = torch.zeros(opt.flat.numel, dtype=torch.bool)
        for o, p in zip(opt.flat.offsets, opt.flat.params):
            inside[o:o + p.numel()] = True
        assert float(getattr(opt, k)[~inside].abs().sum()) == 0.0                        # the alignment padding stays zero
    if typ == "adam_onecycle":
        assert opt.steps == 8 and isinstance(opt.steps, int)
    for n, p in model.named_parameters():              # and the model came along
        assert np.array_equal(p.detach().numpy(), F.params_after(F.RESUME[tag][2], 7)[n])


def _untouched(opt):
    return opt.steps == 0 and all(float(getattr(opt, k).abs().max()) == 0.0 for k in opt.state_keys)


def test_group_order_is_honoured(tmp_path):
    """the BatchNorm group is the SECOND group of an 'adam_onecycle' state: index 2 is the last Linear's weight, not the
    BatchNorm weight that registration order would put there; a file with the two groups swapped does not give the
    recorded placement (its groups no longer match the model's: nothing is loaded)"""
    assert [int(i) for i in O["resume_onecycle/group0"]] == [0, 1, 2] and [int(i) for i in O["resume_onecycle/group1"]] == [3, 4]
    assert O["resume_onecycle/exp_avg/2"].shape == (3, 5) and O["resume_onecycle/exp_avg/3"].shape == (5,)
    F.write_checkpoint(tmp_path / "swapped.pth", "resume_onecycle", swap_groups=True)
    model = F.tiny_model()
    opt = train.build_optimizer(model, F.OPTIM["adam_onecycle"])
    with pytest.warns(UserWarning, match="starts fresh"):
        train.load_checkpoint(model, opt, str(tmp_path / "swapped.pth"))
    assert _untouched(opt)
    got = _flat_views(opt, "exp_avg")
    assert not np.array_equal(got["3.weight"].numpy(), O["resume_onecycle/exp_avg/2"])


def test_mismatched_states_are_not_loaded(tmp_path):
    # one tensor of the wrong shape
    ost, mst = F.torch_state("resume_onecycle")
    ost["state"][4]["exp_avg_sq"] = torch.zeros(7)
    torch.save(dict(epoch=1, it=8, model_state=mst, optimizer_state=ost), str(tmp_path / "shape.pth"))
    # an SGD state offered to an Adam optimizer (and the other way round)
    F.write_checkpoint(tmp_path / "sgd.pth", "resume_sgd")
    F.write_checkpoint(tmp_path / "onecycle.pth", "resume_onecycle")
    # a parameter count that does not match the mapping; something that is no optimizer state at all
    ost2, mst2 = F.torch_state("resume_sgd")
    ost2["param_groups"][0]["params"] = ost2["param_groups"][0]["params"][:-1]
    torch.save(dict(epoch=1, it=8, model_state=mst2, optimizer_state=ost2), str(tmp_path / "count.pth"))
    torch.save(dict(epoch=1, it=8, model_state=mst2, optimizer_state=dict(foo=1)), str(tmp_path / "unknown.pth"))
    cases = [("shape.pth", "adam_onecycle"), ("sgd.pth", "adam"), ("sgd.pth", "adam_onecycle"), ("onecycle.pth", "sgd"),
             ("count.pth", "sgd"), ("unknown.pth", "sgd")]
    for fname, typ in cases:
        opt = train.build_optimizer(F.tiny_model(), F.OPTIM[typ])
        with pytest.warns(UserWarning, match="starts fresh"):
            train.load_checkpoint(F.tiny_model(), opt, str(tmp_path / fname))
        assert _untouched(opt), (fname, typ)


def test_differing_step_counts_warn_once(tmp_path):
    ost, mst = F.torch_state("resume_onecycle")
    ost["state"][1]["step"] = 5                         # an int beside 0-d tensors
    del ost["state"][3]                                 # a parameter that never received a gradient: zeros
    torch.save(dict(epoch=1, it=8, model_state=mst, optimizer_state=ost), str(tmp_path / "steps.pth"))
    model = F.tiny_model()
    opt = train.build_optimizer(model, F.OPTIM["adam_onecycle"])
    with pytest.warns(UserWarning, match="step counts") as rec:
        train.load_checkpoint(model, opt, str(tmp_path / "steps.pth"))
    assert len([w for w in rec if "step counts" in str(w.message)]) == 1 and opt.steps == 8
    got = _flat_views(opt, "exp_avg")
    assert float(got["1.weight"].abs().max()) == 0.0 and np.array_equal(got["1.bias"].numpy(), O["resume_onecycle/exp_avg/4"])


def test_state_dict_round_trips(tmp_path):
    g = torch.Generator().manual_seed(3)
    made = {}
    for typ in ("adam", "sgd", "adam_onecycle"):
        opt = train.build_optimizer(F.tiny_model(), F.OPTIM[typ])
        for k in opt.state_keys:
            getattr(opt, k).copy_(torch.rand(opt.flat.numel, generator=g))
        opt.steps, opt.lr = 11, 0.00123
        sd = opt.state_dict()
        assert sd.get("type", "adam_onecycle") == typ and set(opt.state_keys) <= set(sd)
        if typ == "adam_onecycle":                      # its keys are what they were
            assert set(sd) == {"exp_avg", "exp_avg_sq", "steps", "lr", "mom"}
        made[typ] = (opt, sd)
        other = train.build_optimizer(F.tiny_model(), F.OPTIM[typ])
        other.load_state_dict(sd)
        assert other.steps == 11 and other.lr == 0.00123
        for k in opt.state_keys:
            assert torch.equal(getattr(other, k), getattr(opt, k)) and getattr(other, k) is not sd[k]
        # and through a checkpoint file of this tree
        model = F.tiny_model()
        train.save_checkpoint(train.checkpoint_state(model, opt, 2, 11), str(tmp_path / typ))
        third = train.build_optimizer(model, F.OPTIM[typ])
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert train.load_checkpoint(model, third, str(tmp_path / (typ + ".pth"))) == (2, 11)
        assert third.steps == 11 and all(torch.equal(getattr(third, k), getattr(opt, k)) for k in opt.state_keys)
    for src in made:
        for dst in made:
            if src != dst:
                opt = train.build_optimizer(F.tiny_model(), F.OPTIM[dst])
                with pytest.raises(ValueError, match=src):
                    opt.load_state_dict(made[src][1])
                assert _untouched(opt)
