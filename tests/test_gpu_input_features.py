"""-m gpu: the sparse input layer at 3..8 features per voxel (csrc/spconv_in.hip, include/sassd.h "Sparse input layer") -- the
kernels on a hand-sized rulebook against the CPU oracle (oracle.nets.sparse_conv is generic in Cin; the reference cannot run a
width other than 4) and, at width 4, bit for bit against the kernel the 4-feature paths keep; the spconv facade and PackPlan;
InferencePlan in its four precision forms, its captured graph and FrameStream on a 5-column frame.

Bars: forward 2e-4 * max(1, |ref|max) and weight gradient 2e-4 * max(1, |dw|max), the per-layer bars of test_spconv_layer /
test_spconv_backward (tests/test_gpu_kernels.py); the plan at the bars tests/test_gpu_pipeline.py holds the 4-feature plan to
(sparse features 1e-5 and BEV features 2e-5 of the map maximum, boxes and scores 1e-4 absolute at safe thresholds).  Everything
that replays the same kernels on the same inputs is held to equality."""
import contextlib
import os

import numpy as np
import pytest
import torch
from torch import nn

import sassd  # noqa: F401
from sassd import anchors as A, kernels as K, synth
from sassd.config import Config
from sassd.detector import VxNet, build_detector
from sassd.pipeline import InferencePlan
from sassd.stream import FrameStream
from oracle import clib, nets as onets, rulebook as orb
import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 12345.0


# ---- geometry of the kernel cases ----------------------------------------------------------------------------------------------
def _pattern(origin=(0, 0, 0)):
    """(z, y, x) voxels inside a (6, 12, 12) cell at `origin`: one full 4x4x4 block (inner voxels have all 27 neighbours), a row
    on two faces of the cell (neighbours outside the grid when the cell sits on the grid's faces), 24 isolated voxels (the centre
    offset only)."""
    z, y, x = np.meshgrid(np.arange(1, 5), np.arange(2, 6), np.arange(2, 6), indexing="ij")
    block = np.stack([z.ravel(), y.ravel(), x.ravel()], 1)
    rows = np.array([(0, 0, i) for i in range(12)] + [(5, 11, i) for i in range(12)])
    iso = np.array([(zz, yy, xx) for zz in (1, 3) for yy in (7, 9) for xx in range(0, 12, 2)])
    return np.concatenate([block, rows, iso]) + np.asarray(origin)


def _geometry(grid=(6, 12, 12), origins=((0, 0, 0),), seed=0):
    """[n, 4] int32 (b, z, y, x) rows in a seeded random order, batch 2: the pattern, and in the second batch element the same
    pattern shifted by one voxel along x (a cross-batch neighbour would show as a pair the oracle does not have)."""
    out = []
    for b in range(2):
        for o in origins:
            p = _pattern(o) + np.array([0, 0, b])
            p = p[(p < np.asarray(grid)).all(1)]
            out.append(np.concatenate([np.full((len(p), 1), b), p], 1))
    idx = np.unique(np.concatenate(out), axis=0).astype(np.int32)
    return idx[np.random.default_rng(seed).permutation(len(idx))]


_BOOK = {}


def _book(dev):
    """the hand-sized rulebook of the kernel cases, built once: n rows (not a multiple of 16), capacity n + 37"""
    if not _BOOK:
        idx = _geometry()
        _, nbr = orb.subm_rulebook(idx, (6, 12, 12))
        n = len(idx)
        assert n % 16 != 0 and n > 128, n
        full = (nbr >= 0).sum(1)
        assert full.max() == 27 and (full == 1).sum() >= 24, "the geometry lost its full / isolated voxels"
        oo, kk = np.nonzero(nbr >= 0)
        assert (idx[oo, 0] == idx[nbr[oo, kk], 0]).all(), "oracle pairs cross the batch"
        cap = n + 37
        nb = torch.full((cap, 27), -1, dtype=torch.int32, device=dev)
        nb[:n] = torch.from_numpy(nbr).to(dev)
        _BOOK.update(idx=idx, nbr=nbr, n=n, cap=cap, nb=nb, nptr=torch.tensor([n], dtype=torch.int32, device=dev))
    return _BOOK


def _layer_inputs(cin, seed_off=0):
    g = torch.Generator().manual_seed(cin * 100 + 16 + seed_off)
    n = _BOOK["n"]
    x = torch.randn(n, cin, generator=g)
    w = torch.randn(27, cin, 16, generator=g) * 0.2
    scale = torch.rand(16, generator=g) + 0.5
    shift = torch.randn(16, generator=g) * 0.1
    return x, w, scale, shift


def _padded(x, cap, dev):
    xd = torch.zeros(cap, x.shape[1], device=dev)
    xd[:x.shape[0]] = x.to(dev)
    return xd


# ---- forward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", [3, 5, 6, 7, 8])
def test_forward_matches_the_oracle(dev, cin):
    bk = _book(dev)
    n, cap = bk["n"], bk["cap"]
    x, w, scale, shift = _layer_inputs(cin)
    raw = onets.sparse_conv(x, bk["nbr"], w)
    ref = torch.relu(raw * scale + shift)
    bar = 2e-4 * max(1.0, ref.abs().max().item())
    xd = _padded(x, cap, dev)
    wp = K.spconv_pack_weight(w.to(dev))                        # routed to the input-layer pack
    assert wp.numel() == 27 * ((cin + 3) // 4 * 4) * 16
    y = torch.full((cap, 16), SENTINEL, device=dev)
    out = K.spconv_fwd(xd, bk["nb"], bk["nptr"], cap, wp, 27, cin, 16, scale.to(dev), shift.to(dev), True, y)
    assert out is y
    e = (y[:n].cpu() - ref).abs().max().item()
    print("Cin %d: epilogue max |y - oracle| = %.2e (bar %.2e)" % (cin, e, bar))
    assert e < bar, e
    assert bool((y[n:] == SENTINEL).all()), "rows n..cap-1 were written"
    y2 = torch.full((cap, 16), SENTINEL, device=dev)
    K.spconv_fwd(xd, bk["nb"], bk["nptr"], cap, wp, 27, cin, 16, y=y2)
    e2 = (y2[:n].cpu() - raw).abs().max().item()
    print("Cin %d: raw max |y - oracle| = %.2e (bar %.2e)" % (cin, e2, bar))
    assert e2 < bar, e2
    assert bool((y2[n:] == SENTINEL).all())
    # the bf16 store: the fp32 result rounded to nearest even, bit for bit
    yb = K.spconv_in_fwd(xd, bk["nb"], bk["nptr"], cap, wp, 27, cin, 16, scale.to(dev), shift.to(dev), True, y_bf16=True)
    assert yb.dtype == torch.bfloat16
    assert torch.equal(yb[:n].view(torch.int16), y[:n].to(torch.bfloat16).view(torch.int16))
    # the bf16-sparse wrappers route the same layer
    wpb = K.spconv_bf16_pack_weight(w.to(dev))
    yb2 = K.spconv_fwd_bf16(xd, bk["nb"], bk["nptr"], cap, wpb, 27, cin, 16, scale.to(dev), shift.to(dev), True)
    assert torch.equal(yb2[:n].view(torch.int16), yb[:n].view(torch.int16))


def test_width4_equals_the_existing_kernel_bit_for_bit(dev):
    bk = _book(dev)
    n, cap = bk["n"], bk["cap"]
    x, w, scale, shift = _layer_inputs(4)
    xd, wd, sc, sh = _padded(x, cap, dev), w.to(dev), scale.to(dev), shift.to(dev)
    wp_old = K.spconv_pack_weight(wd)
    wp_new = K.spconv_in_pack_weight(wd)
    assert torch.equal(wp_old, wp_new)
    for args in ((None, None, False), (sc, sh, True), (sc, None, False), (None, sh, True)):
        old = K.spconv_fwd(xd, bk["nb"], bk["nptr"], cap, wp_old, 27, 4, 16, *args)
        new = K.spconv_in_fwd(xd, bk["nb"], bk["nptr"], cap, wp_new, 27, 4, 16, *args)
        assert torch.equal(new[:n], old[:n]), args
    old16 = K.spconv_fwd_bf16(xd, bk["nb"], bk["nptr"], cap, K.spconv_bf16_pack_weight(wd), 27, 4, 16, sc, sh, True)
    new16 = K.spconv_in_fwd(xd, bk["nb"], bk["nptr"], cap, wp_new, 27, 4, 16, sc, sh, True, y_bf16=True)
    assert torch.equal(new16[:n].view(torch.int16), old16[:n].view(torch.int16))


def test_zero_fifth_column_equals_width4(dev):
    """Cin = 5 with the fifth feature zero and arbitrary finite fifth weight rows: fmaf(0, w, acc) leaves acc, so the result
    is the width-4 result of the first four columns and weight rows."""
    bk = _book(dev)
    n, cap = bk["n"], bk["cap"]
    x5, w5, scale, shift = _layer_inputs(5)
    x5[:, 4] = 0.0
    w5[:, 4] = torch.randn(27, 16, generator=torch.Generator().manual_seed(9)) * 1e3
    sc, sh = scale.to(dev), shift.to(dev)
    y5 = K.spconv_fwd(_padded(x5, cap, dev), bk["nb"], bk["nptr"], cap, K.spconv_pack_weight(w5.to(dev)), 27, 5, 16, sc, sh, True)
    x4, w4 = x5[:, :4].contiguous(), w5[:, :4].contiguous()
    y4 = K.spconv_fwd(_padded(x4, cap, dev), bk["nb"], bk["nptr"], cap, K.spconv_pack_weight(w4.to(dev)), 27, 4, 16, sc, sh, True)
    assert torch.equal(y5[:n], y4[:n])
    r5 = K.spconv_fwd(_padded(x5, cap, dev), bk["nb"], bk["nptr"], cap, K.spconv_pack_weight(w5.to(dev)), 27, 5, 16)
    r4 = K.spconv_fwd(_padded(x4, cap, dev), bk["nb"], bk["nptr"], cap, K.spconv_pack_weight(w4.to(dev)), 27, 4, 16)
    assert torch.equal(r5[:n], r4[:n])


@pytest.mark.parametrize("cin", [3, 5, 8])
def test_empty_input_launches_cleanly(dev, cin):
    bk = _book(dev)
    cap = bk["cap"]
    x, w, scale, shift = _layer_inputs(cin)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    y = torch.full((cap, 16), SENTINEL, device=dev)
    K.spconv_fwd(_padded(x, cap, dev), bk["nb"], zero, cap, K.spconv_pack_weight(w.to(dev)), 27, cin, 16, y=y)
    dw = K.spconv_bwd_weight(_padded(x, cap, dev), torch.ones(cap, 16, device=dev), bk["nb"], zero, cap, cin, 16)
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())
    assert not bool(dw.any())


# ---- weight gradient -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", [3, 5, 8])
def test_weight_gradient_matches_autograd_through_the_oracle(dev, cin):
    bk = _book(dev)
    n, cap = bk["n"], bk["cap"]
    x, w, _, _ = _layer_inputs(cin, 7)
    w.requires_grad_(True)
    dy = torch.randn(n, 16, generator=torch.Generator().manual_seed(cin))
    onets.sparse_conv(x, bk["nbr"], w).backward(dy)
    xd, dyd = _padded(x, cap, dev), _padded(dy, cap, dev)
    dyd[n:] = 7.0                                             # rows past n must not be read into the sum
    dw = K.spconv_bwd_weight(xd, dyd, bk["nb"], bk["nptr"], cap, cin, 16)
    bar = 2e-4 * max(1.0, w.grad.abs().max().item())
    e = (dw.cpu() - w.grad).abs().max().item()
    print("Cin %d: max |dw - autograd| = %.2e (bar %.2e)" % (cin, e, bar))
    assert e < bar, e
    dw2 = K.spconv_bwd_weight(xd, dyd, bk["nb"], bk["nptr"], cap, cin, 16, dw=dw.clone(), accumulate=True)
    assert torch.allclose(dw2, 2 * dw, rtol=1e-5, atol=1e-4 * max(1.0, dw.abs().max().item()))
    again = K.spconv_bwd_weight(xd, dyd, bk["nb"], bk["nptr"], cap, cin, 16)
    assert torch.equal(again, dw)


def test_weight_gradient_width4_agrees_with_the_existing_kernel(dev):
    bk = _book(dev)
    n, cap = bk["n"], bk["cap"]
    x, _, _, _ = _layer_inputs(4, 7)
    dy = torch.randn(n, 16, generator=torch.Generator().manual_seed(4))
    xd, dyd = _padded(x, cap, dev), _padded(dy, cap, dev)
    old = K.spconv_bwd_weight(xd, dyd, bk["nb"], bk["nptr"], cap, 4, 16)
    new = K.spconv_in_bwd_weight(xd, dyd, bk["nb"], bk["nptr"], cap, 4, 16)
    assert (new - old).abs().max().item() < 2e-4 * max(1.0, old.abs().max().item())


def test_weight_gradient_over_several_workgroups(dev):
    """more rows than one 128-row workgroup and one staging step: the partials of several workgroups meet in the reduction"""
    idx = _geometry((16, 32, 32), ((0, 0, 0), (8, 16, 16), (0, 16, 0), (8, 0, 16)))[:-5]     # a ragged last workgroup
    _, nbr = orb.subm_rulebook(idx, (16, 32, 32))
    n = len(idx)
    assert n > 3 * 128 and n % 128 != 0
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, 5, generator=g)
    w = torch.zeros(27, 5, 16, requires_grad=True)
    dy = torch.randn(n, 16, generator=g)
    onets.sparse_conv(x, nbr, w).backward(dy)
    nb = torch.from_numpy(nbr).to(dev)
    nptr = torch.tensor([n], dtype=torch.int32, device=dev)
    dw = K.spconv_bwd_weight(x.to(dev), dy.to(dev), nb, nptr, n, 5, 16)
    e = (dw.cpu() - w.grad).abs().max().item()
    assert e < 2e-4 * max(1.0, w.grad.abs().max().item()), e
    assert torch.equal(K.spconv_bwd_weight(x.to(dev), dy.to(dev), nb, nptr, n, 5, 16), dw)


# ---- the spconv facade ---------------------------------------------------------------------------------------------------------
def _facade_geometry():
    return _geometry((16, 32, 32), ((0, 0, 0), (8, 16, 16), (0, 16, 0), (8, 0, 16))), (16, 32, 32)


def test_facade_layer_weight_gradient(dev):
    from sassd import spconv
    idx, shape = _facade_geometry()
    _, nbr = orb.subm_rulebook(idx, shape)
    n = len(idx)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, 5, generator=g)
    gout = torch.randn(n, 16, generator=g)
    seq = spconv.SparseSequential(spconv.SubMConv3d(5, 16, 3, bias=False, indice_key="subm0"),
                                  nn.BatchNorm1d(16, eps=1e-3, momentum=0.01), nn.ReLU()).to(dev).train()
    w0 = seq[0].weight.detach().cpu().clone()
    out = seq(spconv.SparseConvTensor(x.to(dev), torch.from_numpy(idx).to(dev), shape, 2))
    (out.features * gout.to(dev)).sum().backward()
    w = w0.reshape(27, 5, 16).clone().requires_grad_(True)
    bn = nn.BatchNorm1d(16, eps=1e-3, momentum=0.01).train()
    (torch.relu(bn(onets.sparse_conv(x, nbr, w))) * gout).sum().backward()
    got = seq[0].weight.grad.cpu().reshape(27, 5, 16)
    bar = 2e-4 * max(1.0, w.grad.abs().max().item())
    e = (got - w.grad).abs().max().item()
    print("facade: max |weight.grad - oracle| = %.2e (bar %.2e)" % (e, bar))
    assert e < bar, e
    # the input layer has no data gradient; the error no longer speaks of four channels
    xg = x.to(dev).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="the input layer has none"):
        seq(spconv.SparseConvTensor(xg, torch.from_numpy(idx).to(dev), shape, 2)).features.sum().backward()


def _vxnet_step(dev, seed=0):
    from sassd import spconv
    idx, shape = _facade_geometry()
    torch.manual_seed(seed)
    net = VxNet(5).to(dev).train()
    x = torch.randn(len(idx), 5, generator=torch.Generator().manual_seed(5)).to(dev)
    out, middle = net(spconv.SparseConvTensor(x, torch.from_numpy(idx).to(dev), shape, 2))
    assert out.features.shape[0] > 0 and all(m.features.shape[0] > 0 for m in middle)
    out.features_f32().float().square().mean().backward()
    torch.cuda.synchronize()
    return net


def test_vxnet5_training_step_gradients_are_finite(dev):
    net = _vxnet_step(dev)
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert float(net.conv0[0].weight.grad.abs().max()) > 0.0


def test_vxnet5_training_step_bf16_sparse(dev):
    from sassd import autograd as AG
    with AG.sparse_precision_scope("bf16"):
        net = _vxnet_step(dev)
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert float(net.conv0[0].weight.grad.abs().max()) > 0.0


def test_pack_plan_refreshes_the_input_layer_image(dev):
    from sassd import train, weight_images as WI
    torch.manual_seed(0)
    net = VxNet(5).to(dev).train()
    opt = train.build_optimizer(net, dict(type="adam_onecycle", lr=0.003, weight_decay=0.01,
                                          grad_clip=dict(max_norm=10, norm_type=2)), 1)
    assert opt.pack_plan is not None
    before = net.conv0[0].weight.detach().clone()
    opt.flat.grad.normal_(0, 1e-2)
    opt.lr = 1e-2
    opt.step()
    torch.cuda.synchronize()
    conv = net.conv0[0]
    assert not torch.equal(conv.weight.detach(), before)
    fresh = K.spconv_pack_weight(conv.weight.detach().reshape(27, 5, 16).contiguous())
    assert fresh.numel() == 27 * 8 * 16
    assert torch.equal(WI.peek(conv.weight, "spconv"), fresh)
    assert conv.packed_weight() is WI.peek(conv.weight, "spconv")


# ---- InferencePlan / FrameStream on a 5-column frame ---------------------------------------------------------------------------
CFG = dict(voxel_size=synth.KITTI_VOXEL, pc_range=synth.KITTI_RANGE, max_points=5, max_voxels=20000,
           sparse_shape=(40, 1600, 1408), grid_xyz=(1408, 1600, 40))


def _anchors():
    an = A.AnchorGeneratorStride(sizes=[1.6, 3.9, 1.56], anchor_strides=[.4, .4, 1.], anchor_offsets=[.2, -39.8, -1.78],
                                 rotations=[0, 1.57])([1, 200, 176]).reshape(-1, 7)
    return an, A.rbbox2d_to_near_bbox(an[:, [0, 1, 3, 4, 6]]).astype(np.float32)


def _five_columns(pts, seed):
    """a seeded fifth column in [0, 1) behind x, y, z, intensity"""
    extra = np.random.default_rng(seed).random((len(pts), 1), dtype=np.float32)
    return np.ascontiguousarray(np.concatenate([pts, extra], 1), np.float32)


@contextlib.contextmanager
def _oracle_at_width5():
    """tests/helpers.py walks the oracle at the KITTI width: oracle_params cuts the input layer's weight by the first row of
    sassd.pipeline.VXNET and oracle_features takes clib.voxel_mean's default of four means.  Inside this block both say five;
    nothing else of the helpers changes."""
    from sassd import pipeline
    rows, mean = pipeline.VXNET, clib.voxel_mean
    pipeline.VXNET = [rows[0][:3] + (5,) + rows[0][4:]] + list(rows[1:])
    clib.voxel_mean = lambda v, n, nfeat=5: mean(v, n, nfeat)
    try:
        yield
    finally:
        pipeline.VXNET, clib.voxel_mean = rows, mean


_CASE = {}


def _case():
    """seeded weights with a [3, 3, 3, 5, 16] input layer, the k21 frame with a fifth column, the oracle's whole path on it"""
    if not _CASE:
        c = Config.fromfile(os.path.join(ROOT, "configs", "car_cfg.py"))
        c.model["backbone"]["num_input_features"] = 5
        c.model["neck"]["num_input_features"] = 5
        model = H.randomize_detector(build_detector(c.model, c.train_cfg, c.test_cfg).eval(), 0)
        an, bv = _anchors()
        cloud = _five_columns(H.frame("k21"), 21)
        with _oracle_at_width5():
            H.calibrate_cls_head(model, _five_columns(H.frame("small", 11), 11), bv, CFG)
            sd = {k: v.clone() for k, v in model.state_dict().items()}
            assert tuple(sd["neck.backbone.conv0.0.weight"].shape) == (3, 3, 3, 5, 16)
            ref, rpn_thr, score_thr = H.oracle_forward_safe(sd, [cloud], an, bv, CFG)
        _CASE.update(sd=sd, an=an, bv=bv, cloud=cloud, ref=ref, thr=dict(rpn_thr=rpn_thr, score_thr=score_thr))
    return _CASE


def _plan(dev, **kw):
    cs = _case()
    return InferencePlan(cs["sd"], batch_size=1, anchors=cs["an"], anchors_bv=cs["bv"], device=dev, **dict(cs["thr"], **kw))


def _det_state(plan):
    k = int(plan.det["counts"][0].item())
    c = int(plan.df["counts"][0].item())
    return [t.clone() for t in (plan.det["counts"], plan.det["boxes"][0, :k], plan.det["scores"][0, :k], plan.det["labels"][0, :k],
                                plan.df["counts"], plan.df["guided"][0, :c], plan.logits[0, :c], plan.mask, plan.x, plan.conv6)]


def test_plan_vs_oracle_and_graph_replay(dev):
    cs = _case()
    ref = cs["ref"]
    plan = _plan(dev)
    assert plan.cin == 5 and tuple(plan.mean.shape) == (plan.caps[0], 5) and plan.sp[0][1] == 5
    pts = torch.from_numpy(cs["cloud"]).to(dev)
    plan.run_from_points([pts])
    torch.cuda.synchronize()
    assert int(plan.status.item()) == 0
    n0 = int(plan.n[0].item())
    assert n0 == len(ref["coors"]) and np.array_equal(plan.idx[0][:n0].cpu().numpy(), ref["coors"])
    assert np.array_equal(plan.mean[:n0].cpu().numpy(), ref["feats"]) and ref["feats"].shape[1] == 5
    n3 = int(plan.n[3].item())
    assert n3 == len(ref["idx3"]) and np.array_equal(plan.idx[3][:n3].cpu().numpy(), ref["idx3"])
    e = (plan.sp_out[:n3].cpu() - ref["x3"]).abs().max().item()
    m3 = max(1.0, ref["x3"].abs().max().item())
    print("sparse features: max |x3 - oracle| = %.2e = %.1e of the maximum %.1f (bar 1e-5)" % (e, e / m3, m3))
    assert e < 1e-5 * m3, (e, m3)
    for name, got in (("conv6", plan.conv6), ("x", plan.x)):
        r = ref[name]
        e = (got.cpu() - r).abs().max().item()
        m = max(1.0, r.abs().max().item())
        print("BEV %s: max |got - oracle| = %.2e = %.1e of the maximum %.1f (bar 2e-5)" % (name, e, e / m, m))
        assert e < 2e-5 * m, (name, e, m)
    assert np.array_equal(plan.mask.cpu().numpy().astype(bool), ref["masks"])
    res = plan.results()
    d = ref["dets"][0]
    assert d is not None and res[0][0] is not None and len(res[0][0]) == len(d[0]) >= 1
    eb, es = np.abs(res[0][0] - d[0]).max(), np.abs(res[0][1] - d[1]).max()
    print("detections: %d, max |box - oracle| = %.2e, max |score - oracle| = %.2e (bars 1e-4 absolute)" % (len(d[0]), eb, es))
    assert eb <= 1e-4 and es <= 1e-4 and np.array_equal(res[0][2], d[2])
    # the captured frame replays to the eager frame
    want = _det_state(plan)
    graph_plan = _plan(dev)
    graph_plan.capture(len(cs["cloud"]) + 64, ndim=5)
    for _ in range(2):
        graph_plan.run_graph([pts])
        torch.cuda.synchronize()
        assert int(graph_plan.status.item()) == 0
        for j, (got, w) in enumerate(zip(_det_state(graph_plan), want)):
            assert got.shape == w.shape and torch.equal(got, w), j
    # a too narrow staging width is refused before anything is captured; so are voxel features of another width
    fresh = _plan(dev)
    with pytest.raises(ValueError, match="ndim=4"):
        fresh.capture(1024, ndim=4)
    assert fresh.graph is None and not hasattr(fresh, "pts_in")
    with pytest.raises(ValueError, match="5 features per voxel"):
        fresh.load_voxels(torch.zeros(3, 4, device=dev), torch.zeros(3, 4, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="ndim=4"):
        FrameStream(cs["sd"], inflight=1, points_cap=1024, anchors=cs["an"], anchors_bv=cs["bv"], device=dev, ndim=4)


@pytest.mark.parametrize("precision,sparse_precision", [("fp32", "bf16"), ("bf16", "fp32"), ("bf16", "bf16")])
def test_bf16_plan_forms_run_the_frame(dev, precision, sparse_precision):
    cs = _case()
    plan = _plan(dev, precision=precision, sparse_precision=sparse_precision)
    plan.run_from_points([torch.from_numpy(cs["cloud"]).to(dev)])
    torch.cuda.synchronize()
    assert int(plan.status.item()) == 0
    boxes, scores, labels = plan.results()[0]
    assert boxes is not None and len(boxes) >= 1
    assert np.isfinite(boxes).all() and np.isfinite(scores).all()
    if sparse_precision == "bf16":
        assert plan.sp_out.dtype == torch.bfloat16 and plan.sp[0][4].numel() * 2 == 27 * 8 * 16 * 4     # the fp32 image, as int16


def test_frame_stream_returns_the_plans_detections(dev):
    cs = _case()
    frames = [cs["cloud"], _five_columns(H.frame("small", 3), 3), cs["cloud"][::2].copy()]
    eager = _plan(dev, overlap=False)
    want = []
    for p in frames:
        eager.run_from_points([torch.from_numpy(p).to(dev)])
        want.append(eager.results())
    assert any(w[0][0] is not None for w in want)
    with FrameStream(cs["sd"], inflight=2, points_cap=len(cs["cloud"]) + 64, anchors=cs["an"], anchors_bv=cs["bv"], device=dev,
                     ndim=5, **cs["thr"]) as fs:
        tickets = [fs.submit([p]) for p in frames]
        got = [fs.collect(t) for t in tickets]
        with pytest.raises(ValueError, match=r"expected \[N, 5\]"):
            fs.submit([frames[0][:, :4].copy()])
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) == 1
        if w[0][0] is None:
            assert g[0][0] is None, i
            continue
        for j, (a, r) in enumerate(zip(g[0], w[0])):
            assert a.dtype == r.dtype and a.shape == r.shape and a.tobytes() == r.tobytes(), (i, j)


# ---- a whole training step of a 5-feature detector -----------------------------------------------------------------------------
_TRAIN = {}


def _train_case(dev):
    """car_cfg with num_input_features = 5, batch 2 of 5-column K21 frames through train.device_batch"""
    if not _TRAIN:
        import bench
        from sassd import train
        w = dict(synth.workload("car"), overrides=dict(backbone=dict(num_input_features=5), neck=dict(num_input_features=5)))
        model, cfg = synth.build_detector_for(w, 0, train=True, cls_bias=-2.0)
        model = model.to(dev).train()
        assert tuple(model.neck.backbone.conv0[0].weight.shape) == (3, 3, 3, 5, 16)
        anchors = dict(Car=torch.from_numpy(w["anchors"]).to(dev))
        anchors_bv = dict(Car=torch.from_numpy(w["anchors_bv"]).to(dev))
        clouds = [torch.from_numpy(_five_columns(synth.k21(i), i)).to(dev) for i in range(2)]
        gts = [torch.from_numpy(bench.synth_gt_on_points(synth.k21(i), i)).to(dev) for i in range(2)]
        types = [np.array(["Car"] * int(g.shape[0])) for g in gts]
        batch = train.device_batch(clouds, gts, types, ["Car"], anchors, anchors_bv, synth.KITTI_VOXEL, synth.KITTI_RANGE,
                                   model=model)
        assert batch["voxels"][0].shape[2] == 5
        _TRAIN.update(model=model, batch=batch)
    return _TRAIN["model"], _TRAIN["batch"]


def _step(model, batch):
    model.zero_grad(set_to_none=True)
    losses = model(**batch)
    total = sum(v.sum() for v in losses.values())
    total.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    total = total.detach()
    assert np.isfinite(float(total))
    for n, g in grads.items():
        assert bool(torch.isfinite(g).all()), n
    assert float(grads["neck.backbone.conv0.0.weight"].abs().max()) > 0.0
    return float(total), grads


@pytest.mark.parametrize("mode", ["fp32", "bf16_dense", "bf16_sparse", "deterministic"])
def test_training_step_of_a_5_feature_detector(dev, mode):
    from sassd import autograd as AG
    model, batch = _train_case(dev)
    try:
        if mode == "bf16_dense":
            AG.set_bev_precision("bf16")
        if mode == "bf16_sparse":
            model.train_cfg["sparse_precision"] = "bf16"
        if mode == "deterministic":
            model.train_cfg["deterministic"] = True
        loss, grads = _step(model, batch)
        if mode == "deterministic":                # the input layer's gradient included: two steps agree bit for bit
            loss2, grads2 = _step(model, batch)
            assert loss2 == loss and grads.keys() == grads2.keys()
            for n, g in grads.items():
                assert torch.equal(g, grads2[n]), n
    finally:
        AG.set_bev_precision("fp32")
        model.train_cfg.pop("sparse_precision", None)
        model.train_cfg.pop("deterministic", None)
