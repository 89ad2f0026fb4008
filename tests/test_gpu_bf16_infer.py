"""-m gpu: the bf16 inference mode (InferencePlan(precision="bf16"), test_cfg['precision'] = 'bf16').

Per kernel against float64 on the bf16-rounded operands; the bf16 densify bit for bit; whole frames against the bf16-rule
oracle of test_bf16_infer_cpu.py (bars sized by its measured noise floor); the captured frame in both graph forms; the
reference-style API."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sassd import kernels as K, synth, anchors as A
from sassd.config import Config
from sassd.detector import build_detector
from sassd.pipeline import InferencePlan, fold_bn
from oracle.train_ref import round_bf16
import helpers as H
import test_bf16_infer_cpu as B16

pytestmark = pytest.mark.gpu

CFG = B16.CFG
# fp32 accumulation term of the per-kernel bar: an output is a sum of K = 9 Cin (<= 2880) exact bf16 x bf16 products, formed as
# 16-wide MFMA dot products accumulated in fp32 over K / 16 <= 180 k-steps; the worst-case error of that sum is about
# (K / 16 + 16) x 2^-24 x sum |x w| = 1.2e-5 x sum |x w| (Higham's recursive-summation bound), so EPS = 1.5e-5 covers it.
EPS = 1.5e-5


def _bar(name):
    return np.maximum(1e-4, B16.BAR_FACTOR * np.asarray(B16.FLOOR[name], np.float64))


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(b.norm().item(), 1e-30))


def _check_bf16_store(got, acc, asum, scale, shift, relu, tag):
    """got: bf16 output; acc / asum: float64 accumulators sum x w and sum |x w| [B,C,H,W]; epilogue in float64"""
    v = lambda t: t.double().cpu().view(1, -1, 1, 1)      # noqa: E731
    ref = acc * v(scale) + v(shift) if scale is not None else acc + (v(shift) if shift is not None else 0.0)
    if relu:
        ref = torch.relu(ref)
    g = got.double().cpu()
    mag = torch.maximum(ref.abs(), g.abs()).clamp_min(1e-38)
    half_ulp = torch.exp2(torch.floor(torch.log2(mag)) - 8)          # bf16: 8 significant bits -> ulp = 2^(e - 7)
    tol = half_ulp + (v(scale).abs() if scale is not None else 1.0) * EPS * asum + 1e-30
    bad = (g - ref).abs() > tol
    assert not bool(bad.any()), (tag, int(bad.sum()), float(((g - ref).abs() - tol).max()))


def _ref_conv(x, w, pad):
    xd, wd = x.double().cpu(), round_bf16(w.float()).double().cpu()
    return F.conv2d(xd, wd, None, 1, pad), F.conv2d(xd.abs(), wd.abs(), None, 1, pad)


def _rand_map(b, c, h, w, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(b, c, h, w, generator=g)).to(torch.bfloat16).to(dev)


def _rand_bn(c, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(c, generator=g) * 0.5 + 0.5), torch.randn(c, generator=g) * 0.1


# ---- per kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,h,w,b", [(320, 256, 200, 176, 1), (256, 28, 200, 176, 2), (256, 256, 188, 188, 1),
                                            (256, 256, 24, 64, 8)])
def test_conv3x3_bf16_infer_random_maps(dev, cin, cout, h, w, b):
    x = _rand_map(b, cin, h, w, dev, cin + cout)
    g = torch.Generator().manual_seed(7)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)).to(dev)
    scale, shift = _rand_bn(cout, 3)
    assert K.conv2d_bf16_infer_supported(cin, cout, h, w)
    wp = K.conv2d_bf16_infer_pack_weight(wt)
    y = K.conv2d_bf16_infer_fwd(x, wp, cout, scale.to(dev), shift.to(dev), True)
    acc, asum = _ref_conv(x, wt, 1)
    _check_bf16_store(y, acc, asum, scale, shift, True, ("3x3", cin, cout, h, w, b))
    # affine-free form with an fp32 store: the bar of the bf16 training kernels (relative L2 1e-5 against float64)
    bias = shift.to(dev)
    yf = K.conv2d_bf16_infer_fwd(x, wp, cout, None, bias, False, out_bf16=False)
    assert yf.dtype == torch.float32
    assert _rel(yf, acc + shift.double().view(1, -1, 1, 1)) < 1e-5


@pytest.mark.parametrize("cin,cout,hw,b,relu,out_bf16", [(256, 256, (200, 176), 1, True, True), (256, 20, (200, 176), 2, False, False),
                                                         (256, 60, (40, 64), 8, False, False), (28, 28, (188, 188), 1, False, False)])
def test_conv1x1_bf16_infer_random_maps(dev, cin, cout, hw, b, relu, out_bf16):
    h, w = hw
    x = _rand_map(b, cin, h, w, dev, cin * 3 + cout)
    g = torch.Generator().manual_seed(5)
    wt = (torch.randn(cout, cin, 1, 1, generator=g) / np.sqrt(cin)).to(dev)
    scale, shift = _rand_bn(cout, 4)
    wp = K.conv1x1_bf16_pack_weight(wt)
    acc, asum = _ref_conv(x, wt, 0)
    if out_bf16:
        y = K.conv1x1_bf16_infer_fwd(x, wp, cout, scale.to(dev), shift.to(dev), relu)
        _check_bf16_store(y, acc, asum, scale, shift, relu, ("1x1", cin, cout, hw, b))
    else:
        y = K.conv1x1_bf16_infer_fwd(x, wp, cout, None, shift.to(dev), False, out_bf16=False)
        assert _rel(y, acc + shift.double().view(1, -1, 1, 1)) < 1e-5


def _car_frame_plans(dev, frames=("k21",), seed=0):
    model, _ = B16.car_model()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    an, bv = B16.car_anchors()
    clouds = [H.frame(f, seed + i) for i, f in enumerate(frames)]
    return sd, an, bv, clouds


def test_live_operands_and_densify(dev):
    """conv0 (Cin 320, d-major channels), conv7 (1x1), the part-sensitive pair and the heads on the operands of a K21 frame; the
    bf16 dense map equals round_bf16 of the fp32 one bit for bit."""
    sd, an, bv, clouds = _car_frame_plans(dev)
    pts = [torch.from_numpy(p).to(dev) for p in clouds]
    p32 = InferencePlan(sd, batch_size=1, anchors=an, anchors_bv=bv, device=dev)
    p16 = InferencePlan(sd, batch_size=1, anchors=an, anchors_bv=bv, device=dev, precision="bf16")
    p32.run_from_points(pts)
    p16.run_from_points(pts)
    torch.cuda.synchronize()
    assert p16.dense.dtype == torch.bfloat16
    assert torch.equal(p16.dense.view(torch.int16), round_bf16(p32.dense).to(torch.bfloat16).view(torch.int16))
    assert int((p16.dense != 0).sum()) > 0
    D3 = p16.D3
    sdd = {k: v.to(dev) for k, v in sd.items()}
    w0 = sdd["neck.fcn.conv0.weight"].float()
    w0 = w0.view(256, 64, D3, 3, 3).permute(0, 2, 1, 3, 4).reshape(256, 64 * D3, 3, 3)      # d-major, as the plan packs it
    s0, b0 = fold_bn(sdd, "neck.fcn.bn0")
    acc, asum = _ref_conv(p16.dense, w0, 1)
    y0 = K.conv2d_bf16_infer_fwd(p16.dense, p16.bev16[0][0], 256, s0, b0, True)      # (the plan's conv0 map is overwritten)
    _check_bf16_store(y0, acc, asum, s0, b0, True, "conv0 live")
    # conv7 (1x1) on conv6's live map
    w7 = sdd["neck.fcn.conv7.weight"].float()
    s7, b7 = fold_bn(sdd, "neck.fcn.bn7")
    acc, asum = _ref_conv(p16.conv6, w7, 0)
    _check_bf16_store(p16.x, acc, asum, s7, b7, True, "conv7 live")
    # part-sensitive 3x3 (256 -> 28, bf16) and 1x1 (28 -> 28, fp32), the fused head (fp32)
    wp0 = sdd["extra_head.convs.0.weight"].float()
    sp, bp = fold_bn(sdd, "extra_head.convs.1")
    acc, asum = _ref_conv(p16.conv6, wp0, 1)
    _check_bf16_store(p16.ps_t[0], acc, asum, sp, bp, True, "ps 3x3 live")
    acc, _ = _ref_conv(p16.ps_t[0], sdd["extra_head.convs.3.weight"].float(), 0)
    assert _rel(p16.ps_t[1], acc) < 1e-5
    hw = torch.cat([sdd["rpn_head.%s.weight" % n] for n in ("conv_box", "conv_cls", "conv_dir_cls")]).float()
    hb = torch.cat([sdd["rpn_head.%s.bias" % n] for n in ("conv_box", "conv_cls", "conv_dir_cls")]).float()
    acc, _ = _ref_conv(p16.x, hw, 0)
    assert _rel(p16.head_out, acc + hb.double().cpu().view(1, -1, 1, 1)) < 1e-5


# ---- whole frames against the bf16-rule oracle ---------------------------------------------------------------------------
def _same_box(a, b, box_bar):
    """0: the boxes agree within box_bar; 1: they agree up to a heading flipped by pi (the direction classifier's two logits
    are as close as the noise floor: either side may win); -1: different boxes"""
    if not np.all(np.abs(a[:6] - b[:6]) <= box_bar[:6]):
        return -1
    dr = abs(a[6] - b[6])
    if dr <= box_bar[6]:
        return 0
    return 1 if abs(dr - np.pi) <= box_bar[6] else -1


def _match(tag, got_b, got_s, want_b, want_s, thr, box_bar, score_bar):
    """two candidate lists in the same order (anchor order / rescored order): pairs whose boxes agree within box_bar (up to a
    flipped heading: `flipped`); an entry only one side has must lie within score_bar of the threshold (a candidate the noise
    floor may put on either side)"""
    i = j = 0
    pairs, loose, flipped = [], 0, []
    while i < len(got_b) or j < len(want_b):
        m = _same_box(got_b[i], want_b[j], box_bar) if i < len(got_b) and j < len(want_b) else -1
        if m >= 0:
            (flipped if m else pairs).append((i, j)); i += 1; j += 1
        elif j < len(want_b) and abs(want_s[j] - thr) <= score_bar:
            j += 1; loose += 1
        elif i < len(got_b) and abs(got_s[i] - thr) <= score_bar:
            i += 1; loose += 1
        else:
            raise AssertionError((tag, "unmatched candidate", i, j, len(got_b), len(want_b),
                                  None if i >= len(got_b) else (list(got_b[i]), float(got_s[i])),
                                  None if j >= len(want_b) else (list(want_b[j]), float(want_s[j])), thr))
    return pairs, loose, flipped


def _match_dets(tag, got_b, got_s, want_b, want_s, thr, box_bar, score_bar):
    """detections come sorted by score, and two of nearly equal score may come in either order: each oracle detection is paired
    with the plan's detection of the same box; one that only one side has must lie within score_bar of the threshold"""
    used, pairs = set(), []
    for j in range(len(want_b)):
        i = next((i for i in range(len(got_b)) if i not in used and _same_box(got_b[i], want_b[j], box_bar) == 0), None)
        if i is None:
            assert abs(want_s[j] - thr) <= score_bar, (tag, "oracle detection without a partner", list(want_b[j]), want_s[j])
            continue
        used.add(i)
        pairs.append((i, j))
    for i in range(len(got_b)):
        if i not in used:
            assert abs(got_s[i] - thr) <= score_bar, (tag, "plan detection without a partner", list(got_b[i]), got_s[i])
    return pairs, len(got_b) + len(want_b) - 2 * len(pairs)


def _check_frame(tag, p16, p32, ref, rpn, sc, stats):
    B = p16.B
    # upstream of the dense stack the bf16 plan is the fp32 plan, bit for bit
    for lvl in (0, 3):
        n = int(p32.n[lvl].item())
        assert int(p16.n[lvl].item()) == n and torch.equal(p16.idx[lvl][:n], p32.idx[lvl][:n]), (tag, lvl)
    n0, n3 = int(p32.n[0].item()), int(p32.n[3].item())
    assert torch.equal(p16.mean[:n0], p32.mean[:n0]) and torch.equal(p16.sp_out[:n3], p32.sp_out[:n3]), tag
    assert torch.equal(p16.mask, p32.mask), tag
    for name in ("conv6", "x"):
        r = ref[name]
        e = (getattr(p16, name).double().cpu() - r).abs().max().item() / max(1.0, r.abs().max().item())
        stats[name + "_rel"] = max(stats.get(name + "_rel", 0.0), e)
        assert e <= _bar("bev_rel"), (tag, name, e)
    # the part-sensitive map under the BEV bar; a PSWarp logit is a convex combination of its samples (bilinear weights, mean
    # over the 28 parts), so its error is bounded by the map's: the logit bar is the map bar in absolute terms
    r = ref["psmap"]
    pm = max(1.0, r.abs().max().item())
    e = (p16.ps_t[1].double().cpu() - r).abs().max().item() / pm
    stats["psmap_rel"] = max(stats.get("psmap_rel", 0.0), e)
    assert e <= _bar("bev_rel"), (tag, "part-sensitive map", e)
    res = p16.results()
    box_bar, sbar, mbar = _bar("box_field"), _bar("score"), _bar("masked_score")
    lbar = float(_bar("bev_rel")) * pm
    ndet = 0
    for b in range(B):
        gb, gl, gs = ref["guided"][b]
        k = int(p16.df["counts"][b].item())
        got = p16.df["guided"][b, :k].double().cpu().numpy()
        pairs, loose, flipped = _match((tag, b, "guided"), got, p16.df["scores"][b, :k].cpu().numpy(), gb.numpy(), gs.numpy(),
                                       rpn, box_bar, mbar)
        stats["guided_loose"] = stats.get("guided_loose", 0) + loose
        stats["guided_heading_flips"] = stats.get("guided_heading_flips", 0) + len(flipped)
        stats["guided_matched"] = stats.get("guided_matched", 0) + len(pairs)
        # a heading flip is a near-tie of the direction logits; it stays rare (it also moves the PSWarp sampling grid, so the
        # logits of such a candidate are not compared)
        assert len(flipped) <= 2 + 0.02 * len(pairs), (tag, b, "heading flips", len(flipped), len(pairs))
        if pairs:
            ii, jj = np.array(pairs).T
            stats["guided_field"] = np.maximum(stats.get("guided_field", 0.0), np.abs(got[ii] - gb.numpy()[jj]).max(0))
            assert np.array_equal(p16.df["labels"][b, :k].cpu().numpy()[ii], gl.numpy()[jj]), (tag, b)
            le = np.abs(p16.logits[b, :k].double().cpu().numpy()[ii] - ref["logits"][b].numpy()[jj]).max()
            stats["logit"] = max(stats.get("logit", 0.0), float(le))
            assert le <= lbar, (tag, b, "logits", le)
        d = ref["dets"][b]
        gd = res[b]
        wb, ws = (d[0], d[1]) if d is not None else (np.zeros((0, 7)), np.zeros(0))
        hb_, hs = (gd[0], gd[1]) if gd[0] is not None else (np.zeros((0, 7)), np.zeros(0))
        # (a candidate that fell on the other side of the rpn threshold, or whose heading flipped, can change what NMS keeps:
        # then only the count is held, to within those candidates)
        if loose or flipped:
            dp, dl, dflip = [], abs(len(hb_) - len(wb)), []
            assert dl <= loose + len(flipped) + int((np.abs(ws - sc) <= sbar).sum()), (tag, b, "detection count", len(hb_), len(wb))
        else:
            dp, dl = _match_dets((tag, b, "dets"), hb_, hs, wb, ws, sc, box_bar, sbar)
        if dp:
            ii, jj = np.array(dp).T
            stats["det_box_field"] = np.maximum(stats.get("det_box_field", 0.0), np.abs(hb_[ii] - wb[jj]).max(0))
            se = float(np.abs(hs[ii] - ws[jj]).max())
            stats["det_score"] = max(stats.get("det_score", 0.0), se)
            assert se <= sbar, (tag, b, "scores", se)
            assert np.array_equal(gd[2][ii], d[2][jj]), (tag, b, "labels")
        stats["det_loose"] = stats.get("det_loose", 0) + dl
        ndet += len(hb_)
    return ndet


def _print(tag, stats, ref):
    print("bf16 plan vs bf16-rule oracle (%s): %s; bars: BEV / part-sensitive map rel %.1e (logits: that x max|map|), box %s, "
          "score %.1e; threshold clearance %s"
          % (tag, {k: (["%.1e" % x for x in v] if isinstance(v, np.ndarray) else "%.2e" % v) for k, v in stats.items()},
             _bar("bev_rel"), ["%.1e" % x for x in _bar("box_field")], _bar("score"),
             ["%.1e" % x for x in ref["threshold_clearance"]]))


@pytest.mark.parametrize("frames,seed,score_thr", [(("k21",), 0, 0.3), (("small", "k17"), 1, 0.6)])
def test_car_frames_vs_bf16_oracle(dev, frames, seed, score_thr):
    sd, an, bv, clouds = _car_frame_plans(dev, frames, seed)
    ft = H.oracle_features(sd, clouds, an, bv, CFG)
    ref, rpn, sc = B16.bf16_forward_safe(sd, ft, score_thr=score_thr)
    B = len(clouds)
    pts = [torch.from_numpy(p).to(dev) for p in clouds]
    p32 = InferencePlan(sd, batch_size=B, anchors=an, anchors_bv=bv, device=dev, rpn_thr=rpn, score_thr=sc)
    p16 = InferencePlan(sd, batch_size=B, anchors=an, anchors_bv=bv, device=dev, rpn_thr=rpn, score_thr=sc, precision="bf16")
    p32.run_from_points(pts)
    p16.run_from_points(pts)
    torch.cuda.synchronize()
    assert int(p16.status.item()) == 0
    stats = {}
    ndet = _check_frame("car", p16, p32, ref, rpn, sc, stats)
    _print("+".join(frames), stats, ref)
    assert ndet >= 1


def test_multi_class_batch8_vs_bf16_oracle(dev):
    c = Config.fromfile("configs/multi_cfg.py")
    model = H.randomize_detector(build_detector(c.model, c.train_cfg, c.test_cfg).eval(), 4)
    names = c.data.val.class_names
    an, bv = B16.car_anchors(names)
    clouds = [H.frame("small", 20 + i) for i in range(8)]
    H.calibrate_cls_head(model, clouds[0], bv, CFG, target_count=300)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    ft = H.oracle_features(sd, clouds, an, bv, CFG, num_class=3)
    ref, rpn, sc = B16.bf16_forward_safe(sd, ft, num_class=3)
    pts = [torch.from_numpy(p).to(dev) for p in clouds]
    kw = dict(batch_size=8, num_class=3, anchors=an, anchors_bv=bv, device=dev, cap_k=4096, cap_d=1024, rpn_thr=rpn, score_thr=sc)
    p32 = InferencePlan(sd, **kw)
    p16 = InferencePlan(sd, precision="bf16", **kw)
    p32.run_from_points(pts)
    p16.run_from_points(pts)
    torch.cuda.synchronize()
    assert int(p16.status.item()) == 0
    stats = {}
    ndet = _check_frame("multi", p16, p32, ref, rpn, sc, stats)
    _print("multi_cfg batch 8", stats, ref)
    assert ndet >= 1


def test_waymo_scale_batch4_bf16(dev):
    """BEV 188 x 188 (a partial last 16-column tile), batch 4: status 0 and the oracle's detection count under the bf16 rule
    (up to candidates within the score bar of a threshold)."""
    W = dict(voxel_size=synth.WAYMO_VOXEL, pc_range=synth.WAYMO_RANGE, max_points=5, max_voxels=150000,
             sparse_shape=(40, 1504, 1504), grid_xyz=(1504, 1504, 40))
    c = Config.fromfile("configs/car_cfg.py")
    mcfg = dict(c.model)
    mcfg["neck"] = dict(mcfg["neck"], output_shape=[40, 1504, 1504])
    mcfg["extra_head"] = dict(mcfg["extra_head"], grid_offsets=(75.2, 75.2), featmap_stride=0.8)
    model = H.randomize_detector(build_detector(mcfg, c.train_cfg, c.test_cfg).eval(), 7, sparse_fan_div=1)
    an = A.AnchorGeneratorStride(sizes=[1.6, 3.9, 1.56], anchor_strides=[.8, .8, 1.], anchor_offsets=[-74.8, -74.8, -1.0],
                                 rotations=[0, 1.57])([1, 188, 188]).reshape(-1, 7)
    bv = A.rbbox2d_to_near_bbox(an[:, [0, 1, 3, 4, 6]]).astype(np.float32)
    clouds = [synth.waymo_synth(s)[:180000] for s in range(4)]
    H.calibrate_cls_head(model, clouds[0], bv, W, target_count=600)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    wcfg = dict(W, grid_offsets=(75.2, 75.2), featmap_stride=0.8)
    ft = H.oracle_features(sd, clouds, an, bv, wcfg)
    ref, rpn, sc = B16.bf16_forward_safe(sd, ft, span=(1e-3, 1e-3))     # (the configured thresholds, nudged)
    p16 = InferencePlan(sd, batch_size=4, anchors=an, anchors_bv=bv, device=dev, voxel_size=W["voxel_size"],
                        point_cloud_range=W["pc_range"], max_voxels=150000, sparse_shape=W["sparse_shape"],
                        grid_offsets=(75.2, 75.2), featmap_stride=0.8, cap_k=4096, cap_d=2048, rpn_thr=rpn, score_thr=sc,
                        precision="bf16")
    p16.run_from_points([torch.from_numpy(p).to(dev) for p in clouds])
    res = p16.results()
    assert int(p16.status.item()) == 0
    mbar, sbar = _bar("masked_score"), _bar("score")
    for b in range(4):
        want = 0 if ref["dets"][b] is None else len(ref["dets"][b][0])
        got = 0 if res[b][0] is None else len(res[b][0])
        kg, kw_ = int(p16.df["counts"][b].item()), len(ref["guided"][b][0])
        near_g = int((np.abs(ref["masked_scores"].numpy() - rpn) <= mbar).sum())
        lg = torch.sigmoid(ref["logits"][b]).numpy()
        near = near_g + int((np.abs(lg - sc) <= sbar).sum())
        print("waymo-scale bf16 sample %d: %d guided anchors (oracle %d), %d detections (oracle %d); %d / %d oracle candidates "
              "within a bar of the rpn / score threshold" % (b, kg, kw_, got, want, near_g, near - near_g))
        assert kw_ >= 1 and abs(kg - kw_) <= near_g, (b, kg, kw_, near_g)
        assert abs(got - want) <= near, (b, got, want, near)


# ---- the captured frame ------------------------------------------------------------------------------------------------
def _state(plan):
    k = int(plan.det["counts"][0].item())
    c = int(plan.df["counts"][0].item())
    return [t.clone() for t in (plan.det["counts"], plan.det["boxes"][0, :k], plan.det["scores"][0, :k], plan.det["labels"][0, :k],
                                plan.df["counts"], plan.df["guided"][0, :c], plan.logits[0, :c], plan.mask, plan.x, plan.conv6)]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8) if a.dtype == torch.bfloat16 else a,
                                                                      b.view(torch.uint8) if b.dtype == torch.bfloat16 else b)


@pytest.mark.parametrize("overlap", [True, False])
def test_bf16_graph_replays_equal_the_eager_frame(dev, overlap):
    """three bf16 plans captured (two-branch or one-branch graph) and replayed in flight, with the host recycling device
    memory between replays: every replay leaves exactly what the eager bf16 frame leaves"""
    sd, an, bv, _ = _car_frame_plans(dev)
    clouds = [torch.from_numpy(H.frame(f, i)).to(dev) for i, f in enumerate(("k21", "small", "k17"))]
    cap = max(int(p.shape[0]) for p in clouds) + 64
    eager = InferencePlan(sd, batch_size=1, anchors=an, anchors_bv=bv, device=dev, precision="bf16")
    want = []
    for p in clouds:
        eager.run_from_points([p])
        torch.cuda.synchronize()
        assert int(eager.status.item()) == 0
        want.append(_state(eager))
    assert sum(int(w_[0].sum().item()) for w_ in want) >= 1
    plans = [InferencePlan(sd, batch_size=1, anchors=an, anchors_bv=bv, device=dev, overlap=overlap, precision="bf16")
             for _ in range(3)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
    for pl, st in zip(plans, streams):
        with torch.cuda.stream(st):
            pl.capture(cap)
    torch.cuda.synchronize()
    for nbytes in (2 << 20, 64 << 20, 1 << 30):
        junk = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        junk.fill_(255)
        torch.cuda.synchronize()
        del junk
        for rnd in range(2):
            order = [(rnd + j) % 3 for j in range(3)]
            for pl, st, i in zip(plans, streams, order):
                with torch.cuda.stream(st):
                    pl.run_graph([clouds[i]])
            torch.cuda.synchronize()
            for pl, i in zip(plans, order):
                assert int(pl.status.item()) == 0
                for j, (got, ref) in enumerate(zip(_state(pl), want[i])):
                    assert _same(got, ref), ("replay", overlap, nbytes, rnd, i, j)


# ---- reference-style API -----------------------------------------------------------------------------------------------
def test_forward_test_precision_from_test_cfg(dev):
    from sassd.voxel_generator import VoxelGenerator
    from oracle import nets as onets
    model, c = B16.car_model()
    model = model.to(dev)
    an, bv = B16.car_anchors()
    gen = VoxelGenerator(**{k: v for k, v in c.data.val.generator.items() if k != "type"})
    clouds = [H.frame("k21", 5), H.frame("small", 6)]
    kw = dict(voxels=[], coordinates=[], num_points=[], anchors=[], anchors_mask=[])
    for p in clouds:
        v, co, n = gen.generate(p)
        m = onets.anchors_mask(co, bv, gen.voxel_size, gen.point_cloud_range, gen.grid_size, 1)
        kw["voxels"].append(torch.from_numpy(v).to(dev)); kw["coordinates"].append(torch.from_numpy(co).to(dev))
        kw["num_points"].append(torch.from_numpy(n).to(dev)); kw["anchors"].append(torch.from_numpy(an).to(dev))
        kw["anchors_mask"].append(torch.from_numpy(m).to(dev))
    metas = [dict(sample_idx=0), dict(sample_idx=1)]
    assert "precision" not in model.test_cfg
    out32 = model(None, metas, return_loss=False, **kw)
    assert model._plan.precision == "fp32"
    model.test_cfg["precision"] = "bf16"
    out16 = model(None, metas, return_loss=False, **kw)
    assert model._plan.precision == "bf16"                 # the precision is part of the plan cache key
    # the same frames through InferencePlan directly, fp32 and bf16
    sd = model.state_dict()
    tc = model.test_cfg.get("extra", model.test_cfg)
    ret = model.merge_second_batch(kw)
    with torch.no_grad():
        vx = model.backbone(ret["voxels"], ret["num_points"])
    for prec, out in (("fp32", out32), ("bf16", out16)):
        plan = InferencePlan(sd, batch_size=2, anchors=an, device=dev, score_thr=tc.get("score_thr", 0.3),
                             iou_thr=tc.get("nms", {}).get("iou_thr", 0.1), precision=prec, **model._cfg)
        plan.run_from_voxels(vx, ret["coordinates"], ret["anchors_mask"])
        res = plan.results()
        for b in range(2):
            if res[b][0] is None:
                assert out[b]["boxes_lidar"] is None, (prec, b)
                continue
            assert np.array_equal(out[b]["boxes_lidar"], res[b][0]) and np.array_equal(out[b]["scores"], res[b][1]), (prec, b)
            assert np.array_equal(out[b]["labels"], res[b][2]), (prec, b)
    assert any(o["boxes_lidar"] is not None for o in out16), "no bf16 detections through the reference-style API"
