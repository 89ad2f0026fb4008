"""-m gpu: optimizer types 'adam' and 'sgd' (sassd_adam_l2_step / sassd_sgd_step) behind build_optimizer /
build_scheduler / build_warmup_scheduler, against the recorded runs of the reference's own optimizer stack
(tests/golden/make_golden_optim_family.py -> optim_family_ref.npz: 20 iterations, every third one clipped), the two
kernels at their edges against a float64 statement of their documented rules, and the resume from a reference
checkpoint's torch optimizer state.

The trajectory bar is the one of tests/test_gpu_optim.py: every parameter within 2e-6 * max(1, |ref|max) after every step.
The reference's own fp32 run sits 1.6e-7 .. 3.7e-7 from its float64 run of the same steps (`<pair>/fp64_dist` in the
golden file), so the bar leaves about 5x room; should a regenerated golden file ever record a distance above 1e-6 for a
pair, that pair's bar is twice that distance (_bar).  test_kernel_edges also holds sassd_adam_step, the kernel of the default
'adam_onecycle' type, to its rule."""
import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import kernels as K
from sassd import train

import optim_family_cases as F

pytestmark = pytest.mark.gpu
O = F.O
EPS = float(np.finfo(np.float32).eps)


def _bar(run, ref):
    dist = float(O[run + "/fp64_dist"]) if run + "/fp64_dist" in O else 0.0
    return (2e-6 if dist <= 1e-6 else 2 * dist) * max(1.0, float(np.abs(ref).max()))


def _build(dev, typ, policy, params=None, **kw):
    model = F.tiny_model(params).to(dev)
    cfg = F.lr_cfg(policy)
    opt = train.build_optimizer(model, F.OPTIM[typ], **kw)
    sched = train.build_scheduler(opt, 5, 4, F.OPTIM[typ], cfg)
    return model, opt, sched, train.build_warmup_scheduler(opt, F.OPTIM[typ], cfg)


def _follow(dev, model, opt, sched, warm, run, its, grad_mul=1.0):
    """train_one_epoch's schedule switch + the recorded gradients; -> the largest error / bar over steps and parameters"""
    params = dict(model.named_parameters())
    assert sorted(params) == sorted(F.NAMES)
    worst = 0.0
    for it in its:
        (warm if warm is not None and it <= warm.T_max else sched).step(it)
        if run + "/lr" in O:
            assert abs(opt.lr - float(O[run + "/lr"][it])) <= 1e-12 * float(O[run + "/lr"][it]), (run, it, opt.lr)
        opt.zero_grad()
        for n in F.NAMES:
            params[n].grad = torch.from_numpy(O["grad%d/%s" % (it, n)] * np.float32(grad_mul)).to(dev)
        opt.step()
        for n in F.NAMES:
            ref = O["%s/step%d/%s" % (run, it, n)]
            err = float(np.abs(params[n].detach().cpu().numpy() - ref).max())
            worst = max(worst, err / _bar(run, ref))
    return worst


@pytest.mark.parametrize("typ,policy", [("adam", "cosine"), ("adam", "step"), ("sgd", "cosine"), ("sgd", "step")])
def test_trajectory(dev, typ, policy):
    run = "%s_%s" % (typ, policy)
    assert float(O[run + "/fp64_dist"]) > 0
    worst = _follow(dev, *_build(dev, typ, policy), run, range(F.ITERS))
    print("%s: worst error / bar = %.3f (reference fp32 - fp64: %.2e)" % (run, worst, float(O[run + "/fp64_dist"])))
    assert worst <= 1.0, (run, worst)


def test_world_size(dev):
    """the all-reduced SUM of two ranks' gradients with world_size 2: grad_scale inside the clip and the update"""
    worst = _follow(dev, *_build(dev, "sgd", "cosine", world_size=2), "sgd_cosine", range(F.ITERS), grad_mul=2.0)
    print("sgd_cosine, world_size 2: worst error / bar = %.3f" % worst)
    assert worst <= 1.0, worst


# ---- the kernels at their edges ------------------------------------------------------------------------------------------
def _f(x):
    return float(np.float32(x))            # a scalar as the C ABI receives it


def _coef(sumsq, max_norm, grad_scale):
    if sumsq is None or max_norm <= 0:
        return _f(grad_scale)
    return _f(grad_scale) * min(1.0, _f(max_norm) / (np.sqrt(float(sumsq)) * _f(grad_scale) + _f(1e-6)))


def sgd_rule(p, g, b, sumsq, lr, momentum, wd, max_norm, grad_scale):
    """include/sassd.h, sassd_sgd_step, in float64 -> (p', buf', |update|, the magnitudes buf' is summed from)"""
    gc = g * _coef(sumsq, max_norm, grad_scale)
    g1 = gc + _f(wd) * p
    b1 = _f(momentum) * b + g1
    return p - _f(lr) * b1, b1, np.abs(b1), np.abs(_f(momentum) * b) + np.abs(gc) + np.abs(_f(wd) * p)


def adam_l2_rule(p, g, m, v, sumsq, lr, b1, b2, eps, wd, step, max_norm, grad_scale):
    """include/sassd.h, sassd_adam_l2_step, in float64 -> (p', m', v', |update|, the magnitudes m' and v' are summed from)"""
    gc = g * _coef(sumsq, max_norm, grad_scale)
    g1 = gc + _f(wd) * p
    gsum = np.abs(gc) + np.abs(_f(wd) * p)
    m1 = _f(b1) * m + (1 - _f(b1)) * g1
    v1 = _f(b2) * v + (1 - _f(b2)) * g1 * g1
    upd = (m1 / (1 - _f(b1) ** step)) / (np.sqrt(v1) / np.sqrt(1 - _f(b2) ** step) + _f(eps))
    return (p - _f(lr) * upd, m1, v1, np.abs(upd), np.abs(_f(b1) * m) + (1 - _f(b1)) * gsum,
            np.abs(_f(b2) * v) + (1 - _f(b2)) * gsum * gsum)


def adam_rule(p, g, m, v, sumsq, lr, b1, b2, eps, wd, step, max_norm, grad_scale):
    """include/sassd.h, sassd_adam_step ('adam_onecycle': decoupled decay, csrc/optim.hip adam_one<false>), in float64 ->
    (p', m', v', |update|, the magnitudes m' and v' are summed from).  The decay scales the parameter, p *= 1 - wd * lr, and
    never joins the gradient: the moments see the clipped gradient alone."""
    gc = g * _coef(sumsq, max_norm, grad_scale)
    p0 = p * (1 - _f(wd) * _f(lr))
    m1 = _f(b1) * m + (1 - _f(b1)) * gc
    v1 = _f(b2) * v + (1 - _f(b2)) * gc * gc
    upd = (m1 / (1 - _f(b1) ** step)) / (np.sqrt(v1) / np.sqrt(1 - _f(b2) ** step) + _f(eps))
    return (p0 - _f(lr) * upd, m1, v1, np.abs(upd), np.abs(_f(b1) * m) + (1 - _f(b1)) * np.abs(gc),
            np.abs(_f(b2) * v) + (1 - _f(b2)) * gc * gc)


EDGE_N = (1, 3, 4, 5, 1023, 2_097_159)     # the last: one float4 beyond the 2048 x 256 x 4 grid -> a second stride iteration + a 3-element tail
PAD = 9                                     # elements past n in every buffer: they must come back untouched


def _buffers(dev, n, seed, positive=()):
    """gradient and state: standard normal (|.| for a second moment).  Parameters: random sign, magnitude uniform in
    [0.5, 1.5) -- the parameter bar 4 eps (|p| + lr |update|) has no term for cancellation INSIDE the update (momentum * buf
    against g, beta1 * m against (1 - beta1) g): where the update cancels to a fraction of its operands and p is ~1e-4 as
    well, the rounding of those operands alone (any correctly rounded fp32 evaluation of the rule, 3..8 elements of 2 M
    standard normal ones) exceeds it.  The cancelling sums themselves are held to bounds that carry their operands."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = {}
    for k in ("p", "g", "s0", "s1"):
        t = torch.randn(n + PAD, generator=g)
        if k == "p":
            t = torch.sign(t) * (0.5 + torch.rand(n + PAD, generator=g))
        out[k] = (t.abs() if k in positive else t).to(dev)
    return out


def _check(tag, got, want, bound, n):
    got, want = got.double().cpu().numpy(), np.asarray(want)
    ratio = float((np.abs(got[:n] - want) / bound).max())
    assert ratio <= 1.0, (tag, ratio, int(np.argmax(np.abs(got[:n] - want) / bound)))
    return ratio


@pytest.mark.parametrize("n", EDGE_N)
@pytest.mark.parametrize("kernel", ["sgd", "adam_l2", "adam"])
def test_kernel_edges(dev, kernel, n):
    """One step from random state against the documented rule in float64 (scalars as the fp32 values the ABI receives, the
    square sum as the device holds it).  Parameter bar: |err| <= 4 eps (|p| + lr |update|): the result is a handful of
    correctly rounded fp32 operations on the update and one subtraction from p (see _buffers for the state this holds on).
    The momentum buffer and the moments are sums of products that may cancel: 4 eps of the summed magnitudes of their
    operands, |momentum buf| + |g'| + |wd p|; |beta1 m| + (1 - beta1)(|g'| + |wd p|); beta2 v + (1 - beta2)(|g'| + |wd p|)^2.
    "adam" is sassd_adam_step, the default OneCycle optimizer's kernel (decoupled decay): the same bars, without the wd p terms
    in its moments (the decay scales the parameter: one more rounding of p, inside 4 eps |p|)."""
    lr, worst = 0.01, 0.0
    cases = [(clip, wd, mom) for clip in (False, True) for wd in (0.0, 0.01) for mom in ((0.9, 0.0) if kernel == "sgd" else (0.9,))]
    for ci, (clip, wd, mom) in enumerate(cases):
        t = _buffers(dev, n, 100 + ci, positive=("s1",))
        before = {k: v.clone() for k, v in t.items()}
        h = {k: v[:n].double().cpu().numpy() for k, v in t.items()}
        sumsq, ssq, max_norm = None, None, 0.0
        if clip:
            sumsq = K.grad_sumsq(t["g"][:n])
            ssq = float(sumsq.item())
            max_norm = 0.5 * float(np.sqrt(ssq))                       # the clip halves the gradient
            assert ssq > 0
        p, g, s0, s1 = (t[k][:n] for k in ("p", "g", "s0", "s1"))
        tag = (kernel, n, clip, wd, mom)
        if kernel == "sgd":
            K.sgd_step(p, g, s0, sumsq, lr, mom, wd, max_norm, 0.5)
            p1, b1, upd, bsum = sgd_rule(h["p"], h["g"], h["s0"], ssq, lr, mom, wd, max_norm, 0.5)
            worst = max(worst, _check(tag + ("buf",), t["s0"], b1, 4 * EPS * bsum, n))
            assert torch.equal(t["s1"], before["s1"])
        else:
            step = 1 + ci
            step_fn, rule = (K.adam_l2_step, adam_l2_rule) if kernel == "adam_l2" else (K.adam_step, adam_rule)
            step_fn(p, g, s0, s1, sumsq, lr, 0.9, 0.999, 1e-8, wd, step, max_norm, 0.5)
            p1, m1, v1, upd, msum, vsum = rule(h["p"], h["g"], h["s0"], h["s1"], ssq, lr, 0.9, 0.999, 1e-8, wd, step, max_norm, 0.5)
            worst = max(worst, _check(tag + ("exp_avg",), t["s0"], m1, 4 * EPS * msum, n))
            worst = max(worst, _check(tag + ("exp_avg_sq",), t["s1"], v1, 4 * EPS * vsum, n))
        worst = max(worst, _check(tag + ("param",), t["p"], p1, 4 * EPS * (np.abs(h["p"]) + _f(lr) * upd), n))
        assert float((t["p"][:n] - before["p"][:n]).abs().max()) > 0                    # the step moved something
        for k in t:                                                                     # nothing past n was touched
            assert torch.equal(t[k][n:], before[k][n:]), tag + (k,)
        assert torch.equal(t["g"], before["g"])
    print("%s n=%d: worst error / bar = %.3f" % (kernel, n, worst))


# ---- resume from a reference checkpoint ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["resume_onecycle", "resume_sgd"])
def test_resume_from_a_reference_checkpoint(dev, tmp_path, tag):
    """steps 8..15 after loading the reference's torch optimizer state stay within the trajectory bar; the same
    continuation from a fresh optimizer does not (so the state was used)"""
    typ, policy, run = F.RESUME[tag]
    F.write_checkpoint(tmp_path / "ref.pth", tag)
    model, opt, sched, warm = _build(dev, typ, policy)
    assert train.load_checkpoint(model, opt, str(tmp_path / "ref.pth")) == (1, 8)
    if typ == "adam_onecycle":
        assert opt.steps == 8
    assert all(float(getattr(opt, k).abs().max()) > 0 for k in opt.state_keys)
    worst = _follow(dev, model, opt, sched, warm, run, range(8, 16))
    print("%s: resumed, worst error / bar = %.3f" % (tag, worst))
    assert worst <= 1.0, (tag, worst)
    model, opt, sched, warm = _build(dev, typ, policy, params=F.params_after(run, 7))
    fresh = _follow(dev, model, opt, sched, warm, run, range(8, 16))
    print("%s: fresh optimizer, worst error / bar = %.1f" % (tag, fresh))
    assert fresh > 1.0, (tag, fresh)


# ---- determinism, and the existing kernel beside the new ones -------------------------------------------------------------
def _five_steps(dev, typ):
    model, opt, sched, warm = _build(dev, typ, "cosine", deterministic=True)
    assert opt.deterministic
    _follow(dev, model, opt, sched, warm, "%s_cosine" % typ, range(5))
    return [opt.flat.data.clone()] + [getattr(opt, k).clone() for k in opt.state_keys]


@pytest.mark.parametrize("typ", ["sgd", "adam"])
def test_deterministic_runs_are_bit_identical(dev, typ):
    a, b = _five_steps(dev, typ), _five_steps(dev, typ)
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _adam_onecycle_20(dev):
    """the 20 steps of test_gpu_optim.py::test_adam_onecycle_trajectory, on sassd_adam_step's arguments"""
    n = 1023
    g = torch.Generator().manual_seed(5)
    p, m, v = torch.randn(n, generator=g).to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    sumsq = torch.zeros(1, device=dev)
    for it in range(20):
        grad = (torch.randn(n, generator=g) * (4.0 if it % 3 == 0 else 0.05)).to(dev)
        K.grad_sumsq(grad, sumsq, deterministic=True)
        K.adam_step(p, grad, m, v, sumsq, 0.003 * (1 + it) / 20, 0.95 - 0.005 * it, 0.99, 1e-8, 0.01, it + 1, 10.0, 1.0)
    return p, m, v


def test_adam_onecycle_unmoved_by_the_new_kernels(dev):
    """the kernels share no state: sassd_adam_step gives the same bits before and after an 'sgd' optimizer was built and
    stepped in the same process"""
    before = _adam_onecycle_20(dev)
    _follow(dev, *_build(dev, "sgd", "cosine"), "sgd_cosine", range(3))
    after = _adam_onecycle_20(dev)
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert float((before[0] - torch.randn(1023, generator=torch.Generator().manual_seed(5)).to(dev)).abs().max()) > 0
