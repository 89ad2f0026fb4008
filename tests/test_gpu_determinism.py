"""-m gpu: the deterministic training mode (include/sassd.h "Deterministic training").  The four `_det` kernels against
the summation-order contract (numpy models that sum in the same order bit for bit), then whole training steps: two
independent runs with train_cfg['deterministic'] must agree bit for bit in every loss term, every parameter and both
Adam moments, in fp32 and bf16, through the torch flag, through the one-rank RCCL exchange and at Waymo scale."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sassd  # noqa: F401
from sassd import kernels as K
from sassd.autograd import PSWarpFn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import det_train  # noqa: E402
from test_determinism_cpu import interp_grad_model  # noqa: E402

pytestmark = pytest.mark.gpu


def _interp_case(rng, n, m, c):
    """idx [n,3] with empty rows (rows >= m - 50 never drawn, nor 1..9), row 0 the neighbour j = 0 of EVERY point."""
    idx = rng.integers(10, m - 50, size=(n, 3)).astype(np.int32)
    idx[:, 0] = 0
    w = rng.random((n, 3)).astype(np.float32)
    w /= w.sum(1, keepdims=True)
    g = rng.standard_normal((n, c)).astype(np.float32)
    init = rng.standard_normal((m, c)).astype(np.float32)
    return idx, w, g, init


@pytest.mark.parametrize("c,n", [(32, 4000), (64, 65536)])
def test_three_interpolate_grad_det_is_the_ordered_sum(dev, c, n):
    rng = np.random.default_rng(c + n)
    m = max(200, n // 8)
    idx, w, g, init = _interp_case(rng, n, m, c)
    ref = interp_grad_model(g, idx, w, init)
    ti, tw, tg = (torch.from_numpy(a).to(dev) for a in (idx, w, g))
    outs = []
    for _ in range(5):
        gp = torch.from_numpy(init).to(dev)
        K.three_interpolate_grad(tg, ti, tw, m, deterministic=True, grad_points=gp)
        outs.append(gp.cpu().numpy())
    for o in outs[1:]:
        assert np.array_equal(o.view(np.uint32), outs[0].view(np.uint32)), "launches differ"
    assert np.array_equal(outs[0].view(np.uint32), ref.view(np.uint32)), \
        "not the ordered fp32 sum: %d of %d entries differ" % (int((outs[0] != ref).sum()), ref.size)
    assert np.array_equal(outs[0][m - 50:], init[m - 50:]) and np.array_equal(outs[0][1:10], init[1:10])   # empty rows
    # float64: the ordinary rows within 1e-6 of the largest |sum|; row 0 (n terms, sequential) within the a-priori bound
    # of a sequential fp32 sum, (L + 1) u sum |terms|
    ref64 = init.astype(np.float64).copy()
    np.add.at(ref64, idx.reshape(-1), (g.astype(np.float64)[:, None, :] * w.astype(np.float64)[:, :, None]).reshape(-1, c))
    err = np.abs(outs[0].astype(np.float64) - ref64)
    assert err[1:].max() <= 1e-6 * np.abs(ref64).max(), err[1:].max()
    abs0 = np.abs(init[0].astype(np.float64)) + (np.abs(g.astype(np.float64)) * w[:, :1]).sum(0)
    assert (err[0] <= (n + 1) * 2.0 ** -24 * abs0).all()


def test_aux_head_bwd_det(dev):
    """Feature gradients bit-equal over launches and close to the atomic kernel's; dw1 / dw2 bit-identical to it."""
    g = torch.Generator().manual_seed(7)
    n, M = 30000, [9000, 4000, 1500]
    feats = [torch.randn(m, c, generator=g).to(dev) for m, c in zip(M, (32, 64, 64))]
    nn_idx = []
    for m in M:
        r = torch.randint(0, m, (n, 3), generator=g, dtype=torch.int32)
        r[::7, 1] = 3                                          # a hot voxel: the nearest neighbour of many points
        nn_idx.append(r.to(dev))
    w1 = (torch.randn(64, 160, generator=g) * 0.1).to(dev)
    w2 = (torch.randn(4, 64, generator=g) * 0.1).to(dev)
    wgt = torch.rand(n, 9, generator=g)
    wgt = (wgt.view(n, 3, 3) / wgt.view(n, 3, 3).sum(2, keepdim=True)).reshape(n, 9).contiguous().to(dev)
    h = torch.randn(n, 64, generator=g).to(dev)
    gout = torch.randn(n, 4, generator=g).to(dev)
    gs = torch.tensor([0.7, 1.3]).to(dev)
    base = K.aux_head_bwd(feats, nn_idx, w1, w2, wgt, h, gout, gs)
    runs = [K.aux_head_bwd(feats, nn_idx, w1, w2, wgt, h, gout, gs, deterministic=True) for _ in range(3)]
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r[0], runs[0][0]))
    gf, dw1, dw2 = runs[0]
    assert torch.equal(dw1, base[1]) and torch.equal(dw2, base[2])
    for a, b in zip(gf, base[0]):
        assert (a - b).abs().max().item() <= 1e-5 * max(1.0, b.abs().max().item())


def _piled_boxes(g, k):
    boxes = torch.zeros(k, 7)
    boxes[:, 0] = 30.0 + torch.rand(k, generator=g) * 2.0          # a few hundred boxes within a couple of metres
    boxes[:, 1] = -1.0 + torch.rand(k, generator=g) * 2.0
    boxes[:, 2] = -1.0
    boxes[:, 3] = 1.6 + torch.rand(k, generator=g)
    boxes[:, 4] = 3.9 + torch.rand(k, generator=g)
    boxes[:, 5] = 1.5
    boxes[:, 6] = (torch.rand(k, generator=g) - 0.5) * 6.3
    return boxes


def test_pswarp_sample_bwd_det_is_the_ordered_sum(dev):
    g = torch.Generator().manual_seed(11)
    k = 300
    feat = torch.randn(1, 28, 200, 176, generator=g)
    boxes = _piled_boxes(g, k)
    dl = torch.randn(k, generator=g)
    fd, bd, dld = feat.to(dev), boxes.to(dev).view(1, k, 7).contiguous(), dl.to(dev).view(1, k).contiguous()
    cnt = torch.tensor([k], dtype=torch.int32, device=dev)
    off = (0.0, 40.0)
    df, dg = K.pswarp_sample_bwd(fd, bd, cnt, k, off, 2.5, dld, deterministic=True)
    df2, dg2 = K.pswarp_sample_bwd(fd, bd, cnt, k, off, 2.5, dld, deterministic=True)
    assert torch.equal(df, df2) and torch.equal(dg, dg2)
    # each box alone: one contributor per pixel, so its map is exact; then the ascending-box fp32 sum
    one = torch.ones(1, dtype=torch.int32, device=dev)
    ref = torch.zeros_like(fd)
    for i in range(k):
        d1, _ = K.pswarp_sample_bwd(fd, bd[:, i:i + 1].contiguous(), one, 1, off, 2.5, dld[:, i:i + 1].contiguous(),
                                    deterministic=True)
        ref = ref + d1
    assert int((df != ref).sum()) == 0, "not the ascending-box sum at %d pixels" % int((df != ref).sum())
    assert int(((ref != 0).sum(1) > 0).sum()) > 0
    _, dga = K.pswarp_sample_bwd(fd, bd, cnt, k, off, 2.5, dld)
    assert torch.equal(dg, dga), "dguided must be the atomic kernel's, bit for bit"
    # against torch grid_sample autograd in float64 (the bar of test_pswarp_backward_vs_grid_sample): the sampling grid is
    # formed in fp32 as there (and in the kernel) -- fp32 coordinates of ~75 pixels move the bilinear weights by ~1e-5
    # on their own -- and the sampling and its gradient then run in float64
    fr, br = feat.double().clone().requires_grad_(), boxes
    ct, st = torch.cos(br[:, 6]).view(k, 1, 1), torch.sin(br[:, 6]).view(k, 1, 1)
    xx = torch.linspace(-.5, .5, 4).view(1, 4, 1) * br[:, 3].view(k, 1, 1)
    yy = torch.linspace(-.5, .5, 7).view(1, 1, 7) * br[:, 4].view(k, 1, 1)
    sx = (xx * ct + yy * st + br[:, 0].view(k, 1, 1) + 0.0) * 2.5
    sy = (yy * ct - xx * st + br[:, 1].view(k, 1, 1) + 40.0) * 2.5
    grid = torch.stack([sx.reshape(k, 28).t() / 175, sy.reshape(k, 28).t() / 199], -1).view(28, k, 1, 2) * 2 - 1
    out = F.grid_sample(fr[0].unsqueeze(1), grid.double(), align_corners=True).mean(0).view(-1)
    out.backward(dl.double())
    rel = ((df.cpu().double() - fr.grad).norm() / fr.grad.norm()).item()
    assert rel < 1e-5, rel
    # through the autograd function, flag on
    fa = fd.clone().requires_grad_()
    PSWarpFn.apply(fa, boxes.to(dev), off, 2.5, True).backward(dl.to(dev))
    assert torch.equal(fa.grad, df)


def test_grad_sumsq_det(dev):
    from sassd import synth, train
    w = synth.workload("car")
    model, _ = synth.build_detector_for(w, 0, train=True)
    n_model = train.FlatParams(model.to(dev)).numel
    g = torch.Generator().manual_seed(3)
    for n in (n_model, 1_000_003, 1):
        x = torch.randn(n, generator=g)
        xd = x.to(dev)
        a = K.grad_sumsq(xd, deterministic=True)
        b = K.grad_sumsq(xd, deterministic=True)
        assert torch.equal(a, b)
        ref = float((x.double() ** 2).sum())
        assert abs(a.item() - ref) <= 1e-6 * ref, (n, a.item(), ref)


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a["loss"], b["loss"])):
        assert torch.equal(x, y), "%s: loss differs at step %d: %r vs %r" % (what, i, x.item(), y.item())
    assert a["terms"].keys() == b["terms"].keys()
    for k in a["terms"]:
        for i, (x, y) in enumerate(zip(a["terms"][k], b["terms"][k])):
            assert torch.equal(x, y), "%s: %s differs at step %d" % (what, k, i)
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(a[k], b[k]), "%s: %s differ (max %g)" % (what, k, (a[k] - b[k]).abs().max().item())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_deterministic_training_is_bit_reproducible(dev, precision):
    a = det_train.run(dev, 30, precision)
    b = det_train.run(dev, 30, precision)
    assert a["deterministic"] and len(a["loss"]) == 30
    _same(a, b, precision + " config switch")
    if precision == "fp32":
        with det_train.torch_deterministic(True):
            c = det_train.run(dev, 30, precision, deterministic=None)
        assert not torch.are_deterministic_algorithms_enabled()
        assert c["deterministic"]
        _same(a, c, "torch flag")


def test_deterministic_training_through_rccl(dev, tmp_path):
    a = det_train.run(dev, 30, "fp32")
    out = str(tmp_path / "rccl.pt")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "det_train.py"), "--rccl", "--steps", "30",
                        "--out", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    _same(det_train.to_cpu(a), torch.load(out), "one-rank RCCL")


def test_deterministic_training_waymo_scale(dev):
    a = det_train.run(dev, 3, "fp32", workload="waymo", batch=4, frames=4)
    b = det_train.run(dev, 3, "fp32", workload="waymo", batch=4, frames=4)
    _same(a, b, "waymo batch 4")


def test_deterministic_mode_changes_only_the_summation_order(dev):
    """The forward pass is the same in both modes: the first step's loss terms are equal; the first flat gradient agrees
    within the step tolerance of the existing training tests."""
    a = det_train.run(dev, 1, "fp32", deterministic=True, first_grad=True)
    b = det_train.run(dev, 1, "fp32", deterministic=False, first_grad=True)
    assert a["deterministic"] and not b["deterministic"]
    assert torch.equal(a["loss"][0], b["loss"][0])
    for k in a["terms"]:
        assert torch.equal(a["terms"][k][0], b["terms"][k][0]), k
    ga, gb = a["grad0"], b["grad0"]
    assert ((ga - gb).norm() / gb.norm()).item() < 1e-4
