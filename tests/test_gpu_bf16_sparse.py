"""-m gpu: the bf16 sparse backbone (InferencePlan(sparse_precision="bf16"), test_cfg['sparse_precision'] = 'bf16').

Per layer against float64 on the rounded operands; densify bit for bit; whole frames against the bf16-sparse-rule oracle of
test_bf16_sparse_infer_cpu.py (bars sized by its measured noise floor), with bf16 and with fp32 dense convs; what the mode must not
touch (voxels, rulebooks, anchor masks) bit for bit against the fp32 plan; run-to-run and captured-frame bit equality; the
reference-style API."""
import functools

import numpy as np
import pytest
import torch

from sassd import kernels as K, synth, anchors as A
from sassd.config import Config
from sassd.detector import build_detector
from sassd.pipeline import InferencePlan, VXNET
from oracle.train_ref import round_bf16
import helpers as H
import test_bf16_infer_cpu as B16
import test_bf16_sparse_infer_cpu as S16
import test_gpu_bf16_infer as G16

pytestmark = pytest.mark.gpu

CFG = B16.CFG
# fp32 accumulation term of the per-layer bar: an output is <= 27 x 64 exact bf16 x bf16 products (fp32 x fp32 products rounded
# once each by the fused multiply-add chain of the 4-channel layer), summed in fp32 over at most ~80 dependent additions
# (MFMA chains, quarter sums, slab adds, the wave-slab sum); the worst case is below 1e-5 x sum |x w|
EPS = 1.5e-5


def _bar(name):
    return np.maximum(1e-4, S16.BAR_FACTOR * np.asarray(S16.FLOOR[name], np.float64))


def _check_rows(got, acc, asum, scale, shift, relu, tag):
    """got: bf16 [n, C]; acc / asum: float64 sum x w and sum |x w| [n, C]; epilogue in float64: within half a bf16 ulp of the
    rounded result plus the fp32 accumulation bar (the _check_bf16_store form of test_gpu_bf16_infer)"""
    sc, sh = scale.double().cpu().view(1, -1), shift.double().cpu().view(1, -1)
    ref = acc * sc + sh
    if relu:
        ref = torch.relu(ref)
    g = got.double().cpu()
    mag = torch.maximum(ref.abs(), g.abs()).clamp_min(1e-38)
    half_ulp = torch.exp2(torch.floor(torch.log2(mag)) - 8)
    tol = half_ulp + sc.abs() * EPS * asum + 1e-30
    bad = (g - ref).abs() > tol
    assert not bool(bad.any()), (tag, int(bad.sum()), float(((g - ref).abs() - tol).max()))


def _rand_rulebook(n_out, n_in, kind, g, density=0.25):
    nbr = torch.where(torch.rand(n_out, 27, generator=g) < density, torch.randint(0, n_in, (n_out, 27), generator=g),
                      torch.full((n_out, 27), -1, dtype=torch.int64))
    if kind == "subm":
        nbr[:, 13] = torch.arange(n_out)                 # the centre offset pairs every row with itself
    return nbr.int()


# (capacity, rows): car batch 1 (level 0 and a deeper level), batch 2, multi_cfg batch 8, Waymo-scale batch 4 (> 64 k rows: several
# blocks per XCD), a layer filled to its capacity, an empty layer
CAPS = [(20000, 16111), (40000, 14579), (80000, 33000), (320000, 106000), (1200000, 140000), (9000, 9000), (40000, 0)]
LAYERS = sorted({(kind, cin, cout) for _, _, kind, cin, cout, _ in VXNET})


@pytest.mark.parametrize("kind,cin,cout", LAYERS)
def test_layer_vs_float64(dev, kind, cin, cout):
    g = torch.Generator().manual_seed(cin * 7 + cout)
    k = 1 if kind == "1x1" else 27
    w = torch.randn(k, cin, cout, generator=g) / np.sqrt(cin * min(k, 8))
    scale, shift = torch.rand(cout, generator=g) * 0.5 + 0.75, torch.randn(cout, generator=g) * 0.1
    wp = K.spconv_bf16_pack_weight(w.to(dev))
    wr = w.double() if cin == 4 else round_bf16(w).double()
    for cap, n in CAPS:
        n_in = max(n, 1) + (n // 3 if kind == "down" else 0)
        if cin == 4:      # voxel means in metres: the first layer's operands stay fp32
            x = (torch.rand(n_in, 4, generator=g) * torch.tensor([70.4, 80., 4., 1.]) - torch.tensor([0., 40., 3., 0.])).float()
            xd = x.to(dev)
        else:
            x = torch.relu(torch.randn(n_in, cin, generator=g)).to(torch.bfloat16)
            xd = x.to(dev)
        n_dev = torch.tensor([n], dtype=torch.int32, device=dev)
        nbr = None if kind == "1x1" else _rand_rulebook(cap, n_in, kind, g)
        y = torch.full((cap, cout), float("nan"), dtype=torch.bfloat16, device=dev)
        K.spconv_fwd_bf16(xd, None if nbr is None else nbr.to(dev), n_dev, cap, wp, k, cin, cout, scale.to(dev), shift.to(dev),
                          True, y)
        torch.cuda.synchronize()
        assert torch.isnan(y[n:].float()).all(), (kind, cin, cout, cap, n, "rows past the count were written")
        if n == 0:
            continue
        xx = x.double()
        if nbr is None:
            acc, asum = xx[:n] @ wr[0], xx[:n].abs() @ wr[0].abs()
        else:
            acc, asum = S16.sparse_conv64(xx, nbr[:n].numpy(), wr)
        _check_rows(y[:n], acc, asum, scale, shift, True, (kind, cin, cout, cap, n))


@functools.lru_cache(maxsize=None)
def _car(frames, seed):
    model, _ = B16.car_model()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    an, bv = B16.car_anchors()
    clouds = [H.frame(f, seed + i) for i, f in enumerate(frames)]
    ft = H.oracle_features(sd, clouds, an, bv, CFG)
    x3, acts = S16.bf16_sparse_trunk(sd, ft)
    return sd, an, bv, clouds, ft, x3


def _match(tag, got_b, got_s, want_b, want_s, thr, box_bar, score_bar, window=64):
    """G16._match for a noise floor of this size: two candidate lists in anchor order, pairs whose boxes agree within box_bar (up
    to a flipped heading); where the heads of the lists disagree, the side whose next partner is nearer is taken to hold extra
    candidates, and each of them must lie within score_bar of the threshold (a greedy skip can desynchronise the two lists when
    many candidates lie within the bar)"""
    i = j = 0
    pairs, loose, flipped = [], 0, []
    same = lambda a, b: G16._same_box(got_b[a], want_b[b], box_bar)        # noqa: E731
    while i < len(got_b) or j < len(want_b):
        m = same(i, j) if i < len(got_b) and j < len(want_b) else -1
        if m >= 0:
            (flipped if m else pairs).append((i, j)); i += 1; j += 1
            continue
        jj = next((t for t in range(j, min(j + window, len(want_b))) if same(i, t) >= 0), None) if i < len(got_b) else None
        ii = next((t for t in range(i, min(i + window, len(got_b))) if same(t, j) >= 0), None) if j < len(want_b) else None
        if jj is not None and (ii is None or jj - j <= ii - i):
            skip_w, skip_g = range(j, jj), range(0)
        elif ii is not None:
            skip_w, skip_g = range(0), range(i, ii)
        else:
            skip_w = range(j, j + 1) if j < len(want_b) else range(0)
            skip_g = range(i, i + 1) if i < len(got_b) else range(0)
        for t in skip_w:
            assert abs(want_s[t] - thr) <= score_bar, (tag, "oracle candidate without a partner", t, list(want_b[t]), float(want_s[t]), thr)
        for t in skip_g:
            assert abs(got_s[t] - thr) <= score_bar, (tag, "plan candidate without a partner", t, list(got_b[t]), float(got_s[t]), thr)
        loose += len(skip_w) + len(skip_g)
        i += len(skip_g)
        j += len(skip_w)
    return pairs, loose, flipped


def _match_dets(tag, got_b, got_s, want_b, want_s, thr, box_bar, score_bar, got_cand, want_cand):
    """G16._match_dets, plus NMS decisions: a detection one side keeps and the other does not, far from the score threshold, must
    be a candidate of the other side too (two overlapping candidates whose scores or overlap sit within the noise floor of a tie
    or of the IoU threshold: either may survive); such decisions stay rare"""
    used, pairs, nms = set(), [], 0
    for j in range(len(want_b)):
        i = next((i for i in range(len(got_b)) if i not in used and G16._same_box(got_b[i], want_b[j], box_bar) == 0), None)
        if i is None:
            if abs(want_s[j] - thr) > score_bar:
                assert any(G16._same_box(c, want_b[j], box_bar) >= 0 for c in got_cand), (tag, "oracle detection", list(want_b[j]))
                nms += 1
            continue
        used.add(i)
        pairs.append((i, j))
    for i in range(len(got_b)):
        if i not in used and abs(got_s[i] - thr) > score_bar:
            assert any(G16._same_box(c, got_b[i], box_bar) >= 0 for c in want_cand), (tag, "plan detection", list(got_b[i]))
            nms += 1
    return pairs, len(got_b) + len(want_b) - 2 * len(pairs), nms


def _near_ties(boxes, scores, thr, bar, dist=4.0):
    """oracle candidates above thr - bar whose rescored score lies within 2 x bar of a neighbour's (centres closer than `dist`
    metres): the candidates whose NMS fate the noise floor may decide"""
    keep = scores > thr - bar
    b, s = boxes[keep], scores[keep]
    if len(s) < 2:
        return 0
    d = np.hypot(b[:, None, 0] - b[None, :, 0], b[:, None, 1] - b[None, :, 1])
    tie = (np.abs(s[:, None] - s[None, :]) <= 2 * bar) & (d < dist)
    np.fill_diagonal(tie, False)
    return int(tie.any(1).sum())


def _check_frame(tag, p, p32, ref, rpn, sc, stats):
    """the plan under test against the oracle of its own rule (the _check_frame form of test_gpu_bf16_infer, sparse features
    included); what the mode must not touch against the fp32 plan, bit for bit"""
    B = p.B
    for lvl in range(4):
        n = int(p32.n[lvl].item())
        assert int(p.n[lvl].item()) == n and torch.equal(p.idx[lvl][:n], p32.idx[lvl][:n]), (tag, lvl)
    n0, n3 = int(p32.n[0].item()), int(p32.n[3].item())
    assert torch.equal(p.mean[:n0], p32.mean[:n0]), tag
    for key, t in p32.nbr.items():
        assert torch.equal(p.nbr[key], t), (tag, key)
    assert torch.equal(p.mask, p32.mask), tag
    assert p.sp_out.dtype == torch.bfloat16
    e = (p.sp_out[:n3].double().cpu() - ref["x3_bf16"]).abs().max().item() / max(1.0, ref["x3_bf16"].abs().max().item())
    stats["sparse_rel"] = max(stats.get("sparse_rel", 0.0), e)
    assert e <= _bar("sparse_rel"), (tag, "sparse", e)
    for name in ("conv6", "x"):
        r = ref[name]
        e = (getattr(p, name).double().cpu() - r).abs().max().item() / max(1.0, r.abs().max().item())
        stats[name + "_rel"] = max(stats.get(name + "_rel", 0.0), e)
        assert e <= _bar("bev_rel"), (tag, name, e)
    r = ref["psmap"]
    pm = max(1.0, r.abs().max().item())
    e = (p.ps_t[1].double().cpu() - r).abs().max().item() / pm
    stats["psmap_rel"] = max(stats.get("psmap_rel", 0.0), e)
    assert e <= _bar("bev_rel"), (tag, "part-sensitive map", e)
    res = p.results()
    box_bar, sbar, mbar = _bar("box_field"), _bar("score"), _bar("masked_score")
    lbar = float(_bar("bev_rel")) * pm
    ndet = 0
    for b in range(B):
        gb, gl, gs = ref["guided"][b]
        k = int(p.df["counts"][b].item())
        got = p.df["guided"][b, :k].double().cpu().numpy()
        pairs, loose, flipped = _match((tag, b, "guided"), got, p.df["scores"][b, :k].cpu().numpy(), gb.numpy(), gs.numpy(),
                                           rpn, box_bar, mbar)
        stats["guided_loose"] = stats.get("guided_loose", 0) + loose
        stats["guided_matched"] = stats.get("guided_matched", 0) + len(pairs)
        assert len(flipped) <= 2 + 0.02 * len(pairs), (tag, b, "heading flips", len(flipped), len(pairs))
        if pairs:
            ii, jj = np.array(pairs).T
            stats["guided_field"] = np.maximum(stats.get("guided_field", 0.0), np.abs(got[ii] - gb.numpy()[jj]).max(0))
            assert np.array_equal(p.df["labels"][b, :k].cpu().numpy()[ii], gl.numpy()[jj]), (tag, b)
            le = np.abs(p.logits[b, :k].double().cpu().numpy()[ii] - ref["logits"][b].numpy()[jj]).max()
            stats["logit"] = max(stats.get("logit", 0.0), float(le))
            assert le <= lbar, (tag, b, "logits", le)
        d = ref["dets"][b]
        gd = res[b]
        wb, ws = (d[0], d[1]) if d is not None else (np.zeros((0, 7)), np.zeros(0))
        hb_, hs = (gd[0], gd[1]) if gd[0] is not None else (np.zeros((0, 7)), np.zeros(0))
        ties = _near_ties(gb.numpy(), torch.sigmoid(ref["logits"][b]).numpy(), sc, sbar)
        if loose or flipped:
            dl = abs(len(hb_) - len(wb))
            assert dl <= 2 + loose + len(flipped) + ties + int((np.abs(ws - sc) <= sbar).sum()), \
                (tag, b, "detection count", len(hb_), len(wb))
        else:
            dp, dl, nms = _match_dets((tag, b, "dets"), hb_, hs, wb, ws, sc, box_bar, sbar, got, gb.numpy())
            stats["det_nms_decisions"] = stats.get("det_nms_decisions", 0) + nms
            assert nms <= 2 + ties, (tag, b, "NMS decisions", nms, "near ties", ties, len(dp))
            if dp:
                ii, jj = np.array(dp).T
                se = float(np.abs(hs[ii] - ws[jj]).max())
                stats["det_score"] = max(stats.get("det_score", 0.0), se)
                assert se <= sbar, (tag, b, "scores", se)
                assert np.array_equal(gd[2][ii], d[2][jj]), (tag, b, "labels")
        ndet += len(hb_)
    return ndet


def _print(tag, stats):
    print("bf16-sparse plan vs its oracle (%s): %s; bars: sparse rel %.1e, BEV rel %.1e, score %.1e"
          % (tag, {k: (["%.1e" % x for x in v] if isinstance(v, np.ndarray) else "%.2e" % v) for k, v in stats.items()},
             _bar("sparse_rel"), _bar("bev_rel"), _bar("score")))


@pytest.mark.parametrize("dense", ["bf16", "fp32"])
@pytest.mark.parametrize("frames,seed,score_thr", [(("k21",), 0, 0.3), (("small", "k17"), 1, 0.6)])
def test_car_frames_vs_bf16_sparse_oracle(dev, frames, seed, score_thr, dense):
    sd, an, bv, clouds, ft, x3 = _car(frames, seed)
    f = S16.with_sparse(ft, x3)
    f = B16.bf16_features(sd, f) if dense == "bf16" else S16.fp32_dense_features(sd, f)
    ref, rpn, sc = S16.select_safe(f, score_thr=score_thr)
    B = len(clouds)
    pts = [torch.from_numpy(p).to(dev) for p in clouds]
    kw = dict(batch_size=B, anchors=an, anchors_bv=bv, device=dev, rpn_thr=rpn, score_thr=sc)
    p32 = InferencePlan(sd, **kw)
    p = InferencePlan(sd, precision=dense, sparse_precision="bf16", **kw)
    assert p.feat[0].dtype == torch.bfloat16 and p.dense.dtype == (torch.bfloat16 if dense == "bf16" else torch.float32)
    p32.run_from_points(pts)
    p.run_from_points(pts)
    torch.cuda.synchronize()
    assert int(p.status.item()) == 0
    stats = {}
    ndet = _check_frame(("car", frames, dense), p, p32, ref, rpn, sc, stats)
    _print("+".join(frames) + ", %s dense" % dense, stats)
    assert ndet >= 1


@functools.lru_cache(maxsize=None)
def _multi8():
    c = Config.fromfile("configs/multi_cfg.py")
    model = H.randomize_detector(build_detector(c.model, c.train_cfg, c.test_cfg).eval(), 4)
    an, bv = B16.car_anchors(c.data.val.class_names)
    clouds = [H.frame("small", 20 + i) for i in range(8)]
    H.calibrate_cls_head(model, clouds[0], bv, CFG, target_count=300)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    ft = H.oracle_features(sd, clouds, an, bv, CFG, num_class=3)
    return sd, an, bv, clouds, ft, S16.bf16_sparse_trunk(sd, ft)[0]


@pytest.mark.parametrize("dense", ["bf16", "fp32"])
def test_multi_class_batch8_vs_bf16_sparse_oracle(dev, dense):
    sd, an, bv, clouds, ft, x3 = _multi8()
    f = S16.with_sparse(ft, x3)
    f = B16.bf16_features(sd, f, 3) if dense == "bf16" else S16.fp32_dense_features(sd, f, 3)
    ref, rpn, sc = S16.select_safe(f)
    pts = [torch.from_numpy(p).to(dev) for p in clouds]
    kw = dict(batch_size=8, num_class=3, anchors=an, anchors_bv=bv, device=dev, cap_k=4096, cap_d=1024, rpn_thr=rpn, score_thr=sc)
    p32 = InferencePlan(sd, **kw)
    p = InferencePlan(sd, precision=dense, sparse_precision="bf16", **kw)
    p32.run_from_points(pts)
    p.run_from_points(pts)
    torch.cuda.synchronize()
    assert int(p.status.item()) == 0
    stats = {}
    ndet = _check_frame(("multi", dense), p, p32, ref, rpn, sc, stats)
    _print("multi_cfg batch 8, %s dense" % dense, stats)
    assert ndet >= 1


def test_waymo_scale_batch4_bf16_sparse(dev):
    """capacity 600 k / 1.2 M rows per level (the > 64 k-row dispatch), batch 4, bf16 dense and sparse: status 0, the guided-anchor
    and detection counts of the oracle up to candidates within a bar of a threshold"""
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
    ft = H.oracle_features(sd, clouds, an, bv, dict(W, grid_offsets=(75.2, 75.2), featmap_stride=0.8))
    ref, rpn, sc = S16.select_safe(S16.features(sd, ft, "bf16"), span=(1e-3, 1e-3))
    p = InferencePlan(sd, batch_size=4, anchors=an, anchors_bv=bv, device=dev, voxel_size=W["voxel_size"],
                      point_cloud_range=W["pc_range"], max_voxels=150000, sparse_shape=W["sparse_shape"],
                      grid_offsets=(75.2, 75.2), featmap_stride=0.8, cap_k=4096, cap_d=2048, rpn_thr=rpn, score_thr=sc,
                      precision="bf16", sparse_precision="bf16")
    assert p.caps[1] > 65536
    p.run_from_points([torch.from_numpy(q).to(dev) for q in clouds])
    res = p.results()
    assert int(p.status.item()) == 0
    n3 = int(p.n[3].item())
    e = (p.sp_out[:n3].double().cpu() - ref["x3_bf16"]).abs().max().item() / max(1.0, ref["x3_bf16"].abs().max().item())
    assert e <= _bar("sparse_rel"), ("waymo sparse", e)
    mbar, sbar = _bar("masked_score"), _bar("score")
    for b in range(4):
        want = 0 if ref["dets"][b] is None else len(ref["dets"][b][0])
        got = 0 if res[b][0] is None else len(res[b][0])
        kg, kw_ = int(p.df["counts"][b].item()), len(ref["guided"][b][0])
        near_g = int((np.abs(ref["masked_scores"].numpy() - rpn) <= mbar).sum())
        lg = torch.sigmoid(ref["logits"][b]).numpy()
        near = near_g + int((np.abs(lg - sc) <= sbar).sum())
        print("waymo-scale bf16-sparse sample %d: %d guided anchors (oracle %d), %d detections (oracle %d); sparse rel %.1e"
              % (b, kg, kw_, got, want, e))
        assert kw_ >= 1 and abs(kg - kw_) <= near_g, (b, kg, kw_, near_g)
        assert abs(got - want) <= near, (b, got, want, near)


def test_densify_from_bf16_is_a_scatter(dev):
    sd, an, bv, clouds, _, _ = _car(("k21",), 0)
    p = InferencePlan(sd, batch_size=1, anchors=an, anchors_bv=bv, device=dev, sparse_precision="bf16")
    p.run_from_points([torch.from_numpy(clouds[0]).to(dev)])
    torch.cuda.synchronize()
    n3 = int(p.n[3].item())
    feats, idx = p.sp_out[:n3].clone(), p.idx[3][:n3].long()
    D, Hh, Ww = p.shapes[3]
    want = torch.zeros(1, D, 64, Hh, Ww, dtype=torch.bfloat16, device=dev)
    want[idx[:, 0], idx[:, 1], :, idx[:, 2], idx[:, 3]] = feats
    want = want.view(1, D * 64, Hh, Ww)
    for out_bf16 in (True, False):
        got = K.densify_from_bf16(p.sp_out, p.idx[3], p.n[3], p.caps[3], p.shapes[3], 1, 1, out_bf16=out_bf16)
        torch.cuda.synchronize()
        if out_bf16:
            assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        else:
            assert got.dtype == torch.float32 and torch.equal(got, want.float())
    assert torch.equal(p.dense, want.float())                 # the plan's own map (fp32 dense convs)
    assert int((want != 0).sum()) > 0


def test_bit_identity_and_run_to_run(dev):
    """two eager frames of a bf16-sparse plan are bit-equal; the coordinate work equals the fp32 plan's bit for bit"""
    sd, an, bv, clouds, _, _ = _car(("k21",), 0)
    pts = [torch.from_numpy(clouds[0]).to(dev)]
    p32 = InferencePlan(sd, batch_size=1, anchors=an, anchors_bv=bv, device=dev)
    p = InferencePlan(sd, batch_size=1, anchors=an, anchors_bv=bv, device=dev, precision="bf16", sparse_precision="bf16")
    p32.run_from_points(pts)
    p.run_from_points(pts)
    torch.cuda.synchronize()
    first = [t.clone() for t in (p.sp_out, p.dense, p.x, p.head_out, p.det["boxes"], p.det["scores"], p.det["counts"])]
    p.backbone(keep_middle=True)
    torch.cuda.synchronize()
    mid = {li: m[0].clone() for li, m in p.middle.items()}
    assert len(mid) == 14 and all(m.dtype == torch.bfloat16 for m in mid.values())
    p.run_from_points(pts)
    torch.cuda.synchronize()
    for a, b in zip(first, (p.sp_out, p.dense, p.x, p.head_out, p.det["boxes"], p.det["scores"], p.det["counts"])):
        assert G16._same(a, b)
    for lvl in range(4):
        n = int(p32.n[lvl].item())
        assert int(p.n[lvl].item()) == n and torch.equal(p.idx[lvl][:n], p32.idx[lvl][:n])
    for key, t in p32.nbr.items():
        assert torch.equal(p.nbr[key], t), key
    assert torch.equal(p.mask, p32.mask)


@pytest.mark.parametrize("overlap", [True, False])
def test_bf16_sparse_graph_replays_equal_the_eager_frame(dev, overlap):
    sd, an, bv, _, _, _ = _car(("k21",), 0)
    clouds = [torch.from_numpy(H.frame(f, i)).to(dev) for i, f in enumerate(("k21", "small"))]
    cap = max(int(q.shape[0]) for q in clouds) + 64
    for dense in ("bf16", "fp32"):
        kw = dict(batch_size=1, anchors=an, anchors_bv=bv, device=dev, precision=dense, sparse_precision="bf16")
        eager = InferencePlan(sd, **kw)
        want = []
        for q in clouds:
            eager.run_from_points([q])
            torch.cuda.synchronize()
            assert int(eager.status.item()) == 0
            want.append(G16._state(eager) + [eager.sp_out.clone()])
        assert sum(int(w_[0].sum().item()) for w_ in want) >= 1
        pl = InferencePlan(sd, overlap=overlap, **kw)
        st = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(st):
            pl.capture(cap)
        torch.cuda.synchronize()
        for rnd in range(2):
            for i in (1, 0) if rnd else (0, 1):
                with torch.cuda.stream(st):
                    pl.run_graph([clouds[i]])
                torch.cuda.synchronize()
                assert int(pl.status.item()) == 0
                for j, (got, ref) in enumerate(zip(G16._state(pl) + [pl.sp_out], want[i])):
                    assert G16._same(got, ref), ("replay", dense, overlap, rnd, i, j)


def test_forward_test_sparse_precision_from_test_cfg(dev):
    from sassd.voxel_generator import VoxelGenerator
    from oracle import nets as onets
    model, c = B16.car_model()
    model = model.to(dev)
    an, bv = B16.car_anchors()
    gen = VoxelGenerator(**{k: v for k, v in c.data.val.generator.items() if k != "type"})
    clouds = [H.frame("k21", 5), H.frame("small", 6)]
    kw = dict(voxels=[], coordinates=[], num_points=[], anchors=[], anchors_mask=[])
    for q in clouds:
        v, co, n = gen.generate(q)
        m = onets.anchors_mask(co, bv, gen.voxel_size, gen.point_cloud_range, gen.grid_size, 1)
        kw["voxels"].append(torch.from_numpy(v).to(dev)); kw["coordinates"].append(torch.from_numpy(co).to(dev))
        kw["num_points"].append(torch.from_numpy(n).to(dev)); kw["anchors"].append(torch.from_numpy(an).to(dev))
        kw["anchors_mask"].append(torch.from_numpy(m).to(dev))
    metas = [dict(sample_idx=0), dict(sample_idx=1)]
    assert "sparse_precision" not in model.test_cfg
    model(None, metas, return_loss=False, **kw)
    assert model._plan.sparse_precision == "fp32"
    model.test_cfg["sparse_precision"] = "bf16"
    out = model(None, metas, return_loss=False, **kw)
    assert model._plan.sparse_precision == "bf16" and model._plan.precision == "fp32"      # part of the plan cache key
    sd = model.state_dict()
    tc = model.test_cfg.get("extra", model.test_cfg)
    ret = model.merge_second_batch(kw)
    with torch.no_grad():
        vx = model.backbone(ret["voxels"], ret["num_points"])
    plan = InferencePlan(sd, batch_size=2, anchors=an, device=dev, score_thr=tc.get("score_thr", 0.3),
                         iou_thr=tc.get("nms", {}).get("iou_thr", 0.1), sparse_precision="bf16", **model._cfg)
    plan.run_from_voxels(vx, ret["coordinates"], ret["anchors_mask"])
    res = plan.results()
    for b in range(2):
        if res[b][0] is None:
            assert out[b]["boxes_lidar"] is None, b
            continue
        assert np.array_equal(out[b]["boxes_lidar"], res[b][0]) and np.array_equal(out[b]["scores"], res[b][1]), b
        assert np.array_equal(out[b]["labels"], res[b][2]), b
    assert any(o["boxes_lidar"] is not None for o in out), "no detections through the reference-style API"
