"""bf16 inference mode (InferencePlan(precision="bf16")) without a GPU: the new C-ABI entry points, and the bf16-rule oracle the
GPU parity test (test_gpu_bf16_infer.py) compares against, with its own rounding-flip noise floor.

The bf16 rule: every dense conv of the frame (BEV conv0-conv7, the fused SSD head, both part-sensitive convs) rounds its input
map and its RAW weights to bf16 (nearest even) and accumulates exactly (float64 here); eval BatchNorm + ReLU are applied to the
accumulator, and a map that feeds another dense conv is rounded.  Two implementations of that rule agree except where an
accumulator lands within its own rounding error of a bf16 rounding boundary: one element then differs by one bf16 ulp (2^-8
relative), and the flip propagates through the following layers.  The size of that effect is measured here by evaluating the
oracle twice with BatchNorm in two algebraically equal forms -- the plan's fp32 fold (acc * scale + shift) and the textbook
(acc - mean) / sqrt(var + eps) * gamma + beta in float64 -- whose only difference is ~1e-7 relative: exactly a source of flips.
The recorded figures (FLOOR_*) size the whole-frame bars of the GPU test."""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

import sassd  # noqa: F401
from sassd import _C, synth, anchors as A
from sassd.config import Config
from sassd.detector import build_detector
from sassd.pipeline import fold_bn, BN_EPS
from oracle import nets as onets
from oracle.train_ref import round_bf16
import helpers as H

EINVAL = -1

# The noise floor, measured on the car model of test_gpu_pipeline (seed 0) with a K21 frame (test_noise_floor_of_the_bf16_oracle
# prints it; the measured figure in brackets, recorded with ~1.5 x headroom): the largest difference between the two BatchNorm
# forms.  1.8 M of the 9 M elements of the final BEV map differ by at least one bf16 ulp -- a flip moves the accumulators of
# every pixel it touches in the next layer, so flips multiply through the eight layers.
FLOOR = dict(bev_rel=4e-3,                      # conv6 / x / part-sensitive map, relative to the map's maximum (2.8e-3)
             masked_score=2.5e-2,               # sigmoid score of a masked anchor (1.7e-2)
             box_field=np.array([1e-2, 1.2e-2, 6e-3, 4e-3, 1.1e-2, 4e-3, 3e-3]),   # decoded anchors x y z w l h r (8.2e-3 max)
             logit=2.2e-2,                      # part-sensitive logit of a guided anchor (1.5e-2)
             score=3.5e-3)                      # its rescored sigmoid (2.3e-3)
# The GPU plan differs from the oracle by the same mechanism, with a larger seed: its fp32 accumulation order perturbs the
# accumulators by ~1e-6 relative instead of the ~1e-7 of the BatchNorm forms, so more roundings flip (measured on the MI355X:
# guided-anchor fields up to ~3 x the floor).  Its bars are BAR_FACTOR x the recorded floor (at least 1e-4).
BAR_FACTOR = 4.0

CFG = dict(voxel_size=synth.KITTI_VOXEL, pc_range=synth.KITTI_RANGE, max_points=5, max_voxels=20000,
           sparse_shape=(40, 1600, 1408), grid_xyz=(1408, 1600, 40))


def R(t):
    """the bf16 operand of a dense conv, carried in float64 (round_bf16 of the fp32 value: what the kernels round)"""
    return round_bf16(t.float()).double()


def _bn_relu(acc, sd, prefix, bn_form):
    v = lambda t: t.double().view(1, -1, 1, 1)      # noqa: E731
    if bn_form == "folded":                         # the plan's fp32 fold (pipeline.fold_bn), applied in float64
        scale, shift = fold_bn(sd, prefix)
        y = acc * v(scale) + v(shift)
    else:
        g, b = sd[prefix + ".weight"], sd[prefix + ".bias"]
        m, var = sd[prefix + ".running_mean"], sd[prefix + ".running_var"]
        y = (acc - v(m)) / torch.sqrt(v(var) + BN_EPS) * v(g) + v(b)
    return torch.relu(y)


def bf16_features(sd, ft, num_class=1, bn_form="folded"):
    """The dense part of the frame under the bf16 rule, on the fp32 oracle's dense map `ft` (helpers.oracle_features).
    Returns a copy of ft with x, conv6, box, cls, dirp, masked_scores replaced and psmap (the part-sensitive map) added; all
    float64."""
    ft = dict(ft)
    x = R(ft["dense"])
    conv6 = None
    for i in range(8):
        w = sd["neck.fcn.conv%d.weight" % i]
        x = R(_bn_relu(F.conv2d(x, R(w), None, 1, 1 if w.shape[-1] == 3 else 0), sd, "neck.fcn.bn%d" % i, bn_form))
        if i == 6:
            conv6 = x
    hp = {n: dict(weight=R(sd["rpn_head.%s.weight" % n]), bias=sd["rpn_head.%s.bias" % n].double())
          for n in ("conv_box", "conv_cls", "conv_dir_cls")}
    box, cls, dirp = onets.ssd_head_forward(x, hp, num_class)
    p0 = R(_bn_relu(F.conv2d(conv6, R(sd["extra_head.convs.0.weight"]), None, 1, 1), sd, "extra_head.convs.1", bn_form))
    psmap = F.conv2d(p0, R(sd["extra_head.convs.3.weight"]))
    B = ft["B"]
    bcls = torch.sigmoid(cls.reshape(B, -1, num_class)).max(-1)[0]
    ms = torch.cat([bcls[b][torch.from_numpy(ft["masks"][b])] for b in range(B)])
    ft.update(x=x, conv6=conv6, box=box, cls=cls, dirp=dirp, psmap=psmap, masked_scores=ms)
    return ft


def _ps_logits(psmap, guided, grid_offsets, featmap_stride):
    """PSWarp sampling of oracle.nets.pswarp_forward on a given part-sensitive map (float64)"""
    scale = 1.0 / featmap_stride
    out = []
    for i, ga in enumerate(guided):
        if len(ga) == 0:
            out.append(torch.empty(0, dtype=torch.float64))
            continue
        ga = ga.double()
        n = ga.shape[0]
        xg, yg, wg, lg, rg = [ga[:, j] for j in (0, 1, 3, 4, 6)]
        ct, st = torch.cos(rg), torch.sin(rg)
        xx = torch.linspace(-.5, .5, 4, dtype=torch.float64).view(1, 4, 1) * wg.view(n, 1, 1)
        yy = torch.linspace(-.5, .5, 7, dtype=torch.float64).view(1, 1, 7) * lg.view(n, 1, 1)
        sx = xx * ct.view(n, 1, 1) + yy * st.view(n, 1, 1) + xg.view(n, 1, 1)
        sy = yy * ct.view(n, 1, 1) - xx * st.view(n, 1, 1) + yg.view(n, 1, 1)
        sx = ((sx.permute(1, 2, 0).contiguous() + grid_offsets[0]) * scale).view(28, n)
        sy = ((sy.permute(1, 2, 0).contiguous() + grid_offsets[1]) * scale).view(28, n)
        im = psmap[i].unsqueeze(1)
        h, w = im.shape[-2:]
        g = torch.stack([sx / (w - 1), sy / (h - 1)], -1).view(28, n, 1, 2) * 2 - 1
        out.append(torch.mean(F.grid_sample(im, g, align_corners=True), 0).view(-1))
    return out


def bf16_select(ft, rpn_thr, score_thr, iou_thr=0.1):
    """guided anchors, part-sensitive logits and rescored / NMS detections of a bf16_features result"""
    B, nc = ft["B"], ft["num_class"]
    an = torch.from_numpy(ft["anchors"]).double().view(1, -1, 7).expand(B, -1, -1)
    guided = onets.guided_anchors(ft["box"], ft["cls"], ft["dirp"], an, torch.from_numpy(ft["masks"]), nc, rpn_thr)
    logits = _ps_logits(ft["psmap"], [g[0] for g in guided], ft["grid_offsets"], ft["featmap_stride"])
    dets = [onets.rescore(g[0].float(), lg, g[1], score_thr, iou_thr) for g, lg in zip(guided, logits)]
    return dict(guided=guided, logits=logits, dets=dets)


def bf16_forward_safe(sd, ft, num_class=1, rpn_thr=0.1, score_thr=0.3, span=(5e-2, 1e-1)):
    """bf16-rule oracle with both thresholds in the widest gap between oracle scores near the given ones (the distances are
    returned in ["threshold_clearance"]; candidates closer to a threshold than the score bar may fall either way) ->
    (features + selection, rpn_thr, score_thr)"""
    b = bf16_features(sd, ft, num_class)
    rpn, near_rpn = H.widest_gap_threshold(rpn_thr, b["masked_scores"].numpy(), span=span[0])
    sel = bf16_select(b, rpn, 2.0)
    lg = torch.cat([l.reshape(-1) for l in sel["logits"]]) if sel["logits"] else torch.zeros(0)
    sc, near = H.widest_gap_threshold(score_thr, torch.sigmoid(lg).numpy(), span=span[1])
    sel = bf16_select(b, rpn, sc)
    b.update(sel)
    b["threshold_clearance"] = (near_rpn, near)
    return b, rpn, sc


def car_model(seed=0):
    c = Config.fromfile("configs/car_cfg.py")
    m = H.randomize_detector(build_detector(c.model, c.train_cfg, c.test_cfg).eval(), seed)
    H.calibrate_cls_head(m, H.frame("small", 11), car_anchors()[1], CFG)
    return m, c


def car_anchors(names=("Car",)):
    sizes = dict(Car=[1.6, 3.9, 1.56], Pedestrian=[0.6, 0.8, 1.73], Cyclist=[0.6, 1.76, 1.73])
    an = np.concatenate([A.AnchorGeneratorStride(sizes=sizes[n], anchor_strides=[.4, .4, 1.], anchor_offsets=[.2, -39.8, -1.78],
                                                 rotations=[0, 1.57])([1, 200, 176]).reshape(-1, 7) for n in names], 0)
    return an, A.rbbox2d_to_near_bbox(an[:, [0, 1, 3, 4, 6]]).astype(np.float32)


# ---- tests ---------------------------------------------------------------------------------------------------------------
def test_bf16_inference_abi_without_a_device():
    L = _C.lib()
    null, p16 = None, C.c_void_p(16)
    # NULL pointers
    assert L.sassd_conv2d_bf16_infer_fwd(null, null, null, null, 1, null, 1, 1, 256, 256, 200, 176, null) == EINVAL
    assert L.sassd_conv2d_bf16_infer_fwd(p16, null, null, null, 1, p16, 1, 1, 256, 256, 200, 176, null) == EINVAL
    assert L.sassd_conv2d_bf16_infer_fwd(p16, p16, null, null, 1, null, 1, 1, 256, 256, 200, 176, null) == EINVAL
    assert L.sassd_conv1x1_bf16_infer_fwd(null, p16, null, null, 0, p16, 0, 1, 256, 20, 35200, null) == EINVAL
    assert L.sassd_conv1x1_bf16_infer_fwd(p16, null, null, null, 0, p16, 0, 1, 256, 20, 35200, null) == EINVAL
    assert L.sassd_densify_bf16(null, p16, p16, 100, 64, 5, 200, 176, 1, 1, p16, null) == EINVAL
    assert L.sassd_densify_bf16(p16, p16, p16, 100, 64, 5, 200, 176, 1, 1, null, null) == EINVAL
    assert L.sassd_conv2d_bf16_infer_pack_weight(null, 28, 256, p16, null) == EINVAL
    # unsupported shapes / batch / alignment
    assert L.sassd_conv2d_bf16_infer_fwd(p16, p16, null, null, 1, p16, 1, 1, 256, 256, 200, 18, null) == EINVAL   # W % 4
    assert L.sassd_conv2d_bf16_infer_fwd(p16, p16, null, null, 1, p16, 1, 1, 256, 256, 200, 12, null) == EINVAL   # W < 16
    assert L.sassd_conv2d_bf16_infer_fwd(p16, p16, null, null, 1, p16, 1, 0, 256, 256, 200, 176, null) == EINVAL  # batch
    assert L.sassd_conv2d_bf16_infer_fwd(C.c_void_p(18), p16, null, null, 1, p16, 1, 1, 256, 256, 200, 176, null) == EINVAL
    assert L.sassd_conv2d_bf16_infer_fwd(p16, p16, null, null, 1, C.c_void_p(24), 0, 1, 256, 28, 200, 176, null) == EINVAL
    assert L.sassd_conv1x1_bf16_infer_fwd(p16, p16, null, null, 0, p16, 0, 1, 300, 20, 35200, null) == EINVAL     # Cin > 256
    assert L.sassd_conv1x1_bf16_infer_fwd(p16, p16, null, null, 0, p16, 0, 1, 256, 20, 35202, null) == EINVAL     # HW % 4
    assert L.sassd_densify_bf16(p16, p16, p16, 100, 64, 5, 3, 5, 1, 1, p16, null) == EINVAL                       # H W % 8
    assert L.sassd_densify_bf16(p16, p16, p16, 100, 64, 5, 200, 176, 1, 1, C.c_void_p(24), null) == EINVAL        # 16-byte
    # the shapes of the frame: car (200 x 176, conv0 Cin 320), multi_cfg (head 256 -> 60), Waymo scale (188 x 188)
    for h, w in ((200, 176), (188, 188)):
        assert L.sassd_densify_bf16_supported(64, 5, h, w)
        for cin, cout in ((320, 256), (256, 256), (256, 28)):
            assert L.sassd_conv2d_bf16_infer_supported(cin, cout, h, w), (cin, cout, h, w)
        for cin, cout in ((256, 256), (256, 20), (256, 60), (28, 28)):
            assert L.sassd_conv1x1_bf16_infer_supported(cin, cout, h * w), (cin, cout, h, w)
    assert L.sassd_conv2d_bf16_infer_packed_elems(256, 28) == 9 * 256 * 32          # Cout padded to 32
    assert L.sassd_conv2d_bf16_infer_packed_elems(320, 256) == 9 * 320 * 256


def noise_floor(sd, ft, num_class=1, rpn_thr=0.1):
    """the two BatchNorm forms of the bf16 oracle against each other: BEV maps (relative to the map's maximum), masked-anchor
    scores, decoded boxes of the anchors above rpn_thr / 2 (per field), part-sensitive logits and scores of the guided anchors"""
    a = bf16_features(sd, ft, num_class, bn_form="folded")
    b = bf16_features(sd, ft, num_class, bn_form="textbook")
    fl = {}
    for name in ("conv6", "x", "psmap"):
        fl[name + "_rel"] = (a[name] - b[name]).abs().max().item() / max(1.0, a[name].abs().max().item())
    fl["masked_score"] = (a["masked_scores"] - b["masked_scores"]).abs().max().item()
    B = ft["B"]
    an = torch.from_numpy(ft["anchors"]).double().view(1, -1, 7).expand(B, -1, -1)
    m = torch.from_numpy(ft["masks"]).view(B, -1)
    hot = torch.sigmoid(a["cls"].reshape(B, -1, num_class)).max(-1)[0] > rpn_thr / 2
    da = onets.box_decode(a["box"].reshape(B, -1, 7), an)[m & hot]
    db = onets.box_decode(b["box"].reshape(B, -1, 7), an)[m & hot]
    fl["box_field"] = (da - db).abs().max(0)[0].numpy() if len(da) else np.zeros(7)
    sel = bf16_select(a, rpn_thr, 0.3)
    ga = [g[0] for g in sel["guided"]]
    la = torch.cat(_ps_logits(a["psmap"], ga, ft["grid_offsets"], ft["featmap_stride"]))
    lb = torch.cat(_ps_logits(b["psmap"], ga, ft["grid_offsets"], ft["featmap_stride"]))
    fl["logit"] = (la - lb).abs().max().item() if la.numel() else 0.0
    fl["score"] = (torch.sigmoid(la) - torch.sigmoid(lb)).abs().max().item() if la.numel() else 0.0
    fl["flips_x"] = int((a["x"] != b["x"]).sum().item())
    fl["bf16_vs_fp32_x_rel"] = (a["x"] - ft["x"].double()).abs().max().item() / max(1.0, ft["x"].abs().max().item())
    return fl


def test_noise_floor_of_the_bf16_oracle():
    model, _ = car_model()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    an, bv = car_anchors()
    ft = H.oracle_features(sd, [H.frame("k21", 0)], an, bv, CFG)
    fl = noise_floor(sd, ft)
    print("bf16 oracle noise floor (K21, BatchNorm folded vs textbook):",
          {k: (["%.1e" % x for x in v] if isinstance(v, np.ndarray) else "%.2e" % v) for k, v in fl.items()})
    assert fl["flips_x"] > 0, "the two BatchNorm forms should flip some roundings"
    assert max(fl["conv6_rel"], fl["x_rel"]) <= FLOOR["bev_rel"], fl
    assert fl["psmap_rel"] <= FLOOR["bev_rel"], fl
    assert fl["masked_score"] <= FLOOR["masked_score"], fl
    assert np.all(fl["box_field"] <= FLOOR["box_field"]), fl
    assert fl["logit"] <= FLOOR["logit"] and fl["score"] <= FLOOR["score"], fl
    # the floor is small against the effect of the rounding rule itself (bf16 against the fp32 oracle)
    assert fl["bf16_vs_fp32_x_rel"] > max(fl["conv6_rel"], fl["x_rel"])
