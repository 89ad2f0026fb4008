"""bf16 sparse backbone (InferencePlan(sparse_precision="bf16"), test_cfg['sparse_precision']) without a GPU: the new C-ABI entry
points, the device assembly of the new kernels, the plan's argument and cache-key plumbing, and the bf16-sparse-rule oracle the GPU
test (test_gpu_bf16_sparse.py) compares against, with its own rounding-flip noise floor.

The bf16-sparse rule (include/sassd.h "bf16 sparse backbone"): the first layer (4 -> 16) multiplies the fp32 voxel means by the fp32
weights, every other sparse layer its bf16-stored input by its raw weights rounded to bf16; products are summed exactly (float64
here), eval BatchNorm + ReLU are applied to the sum and the result is rounded to bf16.  The dense part is then the fp32 oracle or
the bf16 rule of test_bf16_infer_cpu on the densified map.  As there, the noise floor is the oracle against itself with BatchNorm
in its two algebraically equal forms, now in the sparse layers as well."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sassd  # noqa: F401
from sassd import _C
from sassd.pipeline import fold_bn, BN_EPS, VXNET
from oracle import nets as onets
from oracle.train_ref import round_bf16
import helpers as H
import test_bf16_infer_cpu as B16

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# The noise floor of the bf16-sparse rule with bf16 dense convs, measured on the car model of test_gpu_pipeline (seed 0) with a
# K21 frame (test_noise_floor_of_the_bf16_sparse_oracle prints it; the measured figure in brackets, recorded with ~1.5 x
# headroom).  The GPU test holds both dense precisions to BAR_FACTOR x these figures.
FLOOR = dict(sparse_rel=1.1e-2,                 # level-3 sparse features, relative to their maximum (7.5e-3; 34 k flipped elements)
             bev_rel=1.6e-2,                    # conv6 / x / part-sensitive map, relative to the map's maximum (1.07e-2)
             masked_score=0.1,                  # sigmoid score of a masked anchor (6.8e-2)
             box_field=np.array([5.5e-2, 6e-2, 2.4e-2, 1.8e-2, 7.5e-2, 2e-2, 1.4e-2]),   # decoded anchors x y z w l h r (5.1e-2 max)
             logit=7.5e-2,                      # part-sensitive logit of a guided anchor (4.9e-2)
             score=5e-3)                        # its rescored sigmoid (3.3e-3)
BAR_FACTOR = 4.0
CFG = B16.CFG


def R(t):
    """bf16 value of an fp32 / float64 tensor, carried in float64"""
    return round_bf16(t.float()).double()


def sparse_conv64(x, nbr, w):
    """oracle.nets.sparse_conv in float64: y[o] = sum_k x[nbr[o,k]] @ w[k]; also sum_k |x| @ |w| (the accumulation bar)"""
    nbr_t = torch.as_tensor(np.asarray(nbr), dtype=torch.int64)
    y = torch.zeros(nbr_t.shape[0], w.shape[2], dtype=torch.float64)
    a = torch.zeros_like(y)
    for k in range(nbr_t.shape[1]):
        o = torch.nonzero(nbr_t[:, k] >= 0).view(-1)
        if o.numel() == 0:
            continue
        xs = x[nbr_t[o, k]]
        y.index_add_(0, o, xs @ w[k])
        a.index_add_(0, o, xs.abs() @ w[k].abs())
    return y, a


def bn_relu_rows(acc, sd, prefix, bn_form="folded"):
    """eval BatchNorm + ReLU of a [rows, C] float64 accumulator: the plan's fp32 fold applied in float64, or the textbook form"""
    if bn_form == "folded":
        scale, shift = fold_bn(sd, prefix)
        y = acc * scale.double().cpu() + shift.double().cpu()
    else:
        g, b = sd[prefix + ".weight"].double().cpu(), sd[prefix + ".bias"].double().cpu()
        m, v = sd[prefix + ".running_mean"].double().cpu(), sd[prefix + ".running_var"].double().cpu()
        y = (acc - m) / torch.sqrt(v + BN_EPS) * g + b
    return torch.relu(y)


def bf16_sparse_trunk(sd, ft, bn_form="folded"):
    """The 14 sparse layers under the bf16-sparse rule on the oracle's voxels and rulebooks (helpers.oracle_features) ->
    level-3 features (bf16 values in float64) and every layer's output"""
    x = torch.as_tensor(ft["feats"], dtype=torch.float32).double()          # voxel means: fp32 operands of the first layer
    acts = []
    for li, (wname, bnname, kind, cin, cout, key) in enumerate(VXNET):
        k = 1 if kind == "1x1" else 27
        w = sd["neck.backbone.%s.weight" % wname].float().cpu().reshape(k, cin, cout)
        w = w.double() if li == 0 else R(w)
        acc = x @ w[0] if key is None else sparse_conv64(x, ft["books"][key][1], w)[0]
        x = R(bn_relu_rows(acc, sd, "neck.backbone.%s" % bnname, bn_form))
        acts.append(x)
    return x, acts


def with_sparse(ft, x3):
    """ft with the dense map rebuilt from bf16-rule level-3 features"""
    B, CD, Hh, Ww = ft["dense"].shape
    dense = onets.densify(x3.float(), ft["idx3"], (CD // 64, Hh, Ww), B)
    return dict(ft, dense=dense, x3_bf16=x3)


def fp32_dense_features(sd, ft, num_class=1, bn_form="folded"):
    """the dense part of the frame in float64 without rounding (the fp32 dense path) -- the keys of B16.bf16_features"""
    ft = dict(ft)
    x = ft["dense"].double()
    conv6 = None
    for i in range(8):
        w = sd["neck.fcn.conv%d.weight" % i].double().cpu()
        x = B16._bn_relu(F.conv2d(x, w, None, 1, 1 if w.shape[-1] == 3 else 0), sd, "neck.fcn.bn%d" % i, bn_form)
        if i == 6:
            conv6 = x
    hp = {n: dict(weight=sd["rpn_head.%s.weight" % n].double().cpu(), bias=sd["rpn_head.%s.bias" % n].double().cpu())
          for n in ("conv_box", "conv_cls", "conv_dir_cls")}
    box, cls, dirp = onets.ssd_head_forward(x, hp, num_class)
    p0 = B16._bn_relu(F.conv2d(conv6, sd["extra_head.convs.0.weight"].double().cpu(), None, 1, 1), sd, "extra_head.convs.1", bn_form)
    psmap = F.conv2d(p0, sd["extra_head.convs.3.weight"].double().cpu())
    B = ft["B"]
    bcls = torch.sigmoid(cls.reshape(B, -1, num_class)).max(-1)[0]
    ms = torch.cat([bcls[b][torch.from_numpy(ft["masks"][b])] for b in range(B)])
    ft.update(x=x, conv6=conv6, box=box, cls=cls, dirp=dirp, psmap=psmap, masked_scores=ms)
    return ft


def features(sd, ft, dense_precision, num_class=1, bn_form="folded"):
    """the whole threshold-free frame under the bf16-sparse rule, dense part in `dense_precision`"""
    x3, acts = bf16_sparse_trunk(sd, ft, bn_form)
    f = with_sparse(ft, x3)
    f = B16.bf16_features(sd, f, num_class, bn_form) if dense_precision == "bf16" else fp32_dense_features(sd, f, num_class, bn_form)
    f["sparse_acts"] = acts
    return f


def select_safe(b, rpn_thr=0.1, score_thr=0.3, span=(5e-2, 1e-1)):
    """B16.bf16_forward_safe on given features: thresholds in the widest gap near the given ones -> (ref, rpn_thr, score_thr)"""
    rpn, near_rpn = H.widest_gap_threshold(rpn_thr, b["masked_scores"].numpy(), span=span[0])
    sel = B16.bf16_select(b, rpn, 2.0)
    lg = torch.cat([l.reshape(-1) for l in sel["logits"]]) if sel["logits"] else torch.zeros(0)
    sc, near = H.widest_gap_threshold(score_thr, torch.sigmoid(lg).numpy(), span=span[1])
    b = dict(b)
    b.update(B16.bf16_select(b, rpn, sc))
    b["threshold_clearance"] = (near_rpn, near)
    return b, rpn, sc


def noise_floor(sd, ft, num_class=1, rpn_thr=0.1):
    """the two BatchNorm forms of the bf16-sparse + bf16-dense oracle against each other (the metrics of B16.noise_floor, plus
    the level-3 sparse features)"""
    a = features(sd, ft, "bf16", num_class, "folded")
    b = features(sd, ft, "bf16", num_class, "textbook")
    fl = {"sparse_rel": (a["x3_bf16"] - b["x3_bf16"]).abs().max().item() / max(1.0, a["x3_bf16"].abs().max().item())}
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
    sel = B16.bf16_select(a, rpn_thr, 0.3)
    ga = [g[0] for g in sel["guided"]]
    la = torch.cat(B16._ps_logits(a["psmap"], ga, ft["grid_offsets"], ft["featmap_stride"]))
    lb = torch.cat(B16._ps_logits(b["psmap"], ga, ft["grid_offsets"], ft["featmap_stride"]))
    fl["logit"] = (la - lb).abs().max().item() if la.numel() else 0.0
    fl["score"] = (torch.sigmoid(la) - torch.sigmoid(lb)).abs().max().item() if la.numel() else 0.0
    fl["flips_sparse"] = int((a["x3_bf16"] != b["x3_bf16"]).sum().item())
    fl["bf16_vs_fp32_sparse_rel"] = (a["x3_bf16"] - ft["x3"].double()).abs().max().item() / max(1.0, ft["x3"].abs().max().item())
    return fl


# ---- tests ---------------------------------------------------------------------------------------------------------------
SHAPES = [(27, 4, 16), (27, 16, 16), (27, 16, 32), (27, 32, 32), (27, 32, 64), (27, 64, 64), (1, 64, 64)]


def test_bf16_sparse_abi_without_a_device():
    L = _C.lib()
    null, p16 = None, C.c_void_p(16)
    # every layer of the trunk, at the capacities of car batch 1, multi_cfg batch 8 and Waymo-scale batch 4
    for _, _, kind, cin, cout, key in VXNET:
        k = 1 if key is None else 27
        for cap in (20000, 40000, 160000, 320000, 600000, 1200000):
            assert L.sassd_spconv_bf16_supported(k, cin, cout, cap), (kind, cin, cout, cap)
    for k, cin, cout in ((27, 64, 32), (27, 32, 16), (27, 4, 32), (1, 4, 16), (9, 64, 64), (27, 8, 16), (27, 64, 128)):
        assert not L.sassd_spconv_bf16_supported(k, cin, cout, 20000), (k, cin, cout)
    assert not L.sassd_spconv_bf16_supported(27, 64, 64, 0) and not L.sassd_spconv_bf16_supported(27, 64, 64, 1 << 25)
    # pack sizes: bf16 images for Cin >= 16, the fp32 image for the first layer, 0 for a shape without a kernel
    for k, cin, cout in SHAPES:
        assert L.sassd_spconv_bf16_packed_bytes(k, cin, cout) == k * cin * cout * (4 if cin == 4 else 2)
    assert L.sassd_spconv_bf16_packed_bytes(27, 64, 32) == 0
    assert L.sassd_spconv_bf16_pack_weight(null, 27, 64, 64, p16, null) == EINVAL
    assert L.sassd_spconv_bf16_pack_weight(p16, 27, 64, 64, null, null) == EINVAL
    assert L.sassd_spconv_bf16_pack_weight(p16, 27, 64, 32, p16, null) == EINVAL
    assert L.sassd_spconv_bf16_pack_weight(p16, 27, 64, 64, C.c_void_p(24), null) == EINVAL
    fwd = L.sassd_spconv_fwd_bf16
    ok = (p16, 0, p16, p16, 1000, p16, 27, 64, 64, null, null, 1, p16, 0, null)

    def call(**kw):
        a = list(ok)
        names = ("x", "x_is_f32", "nbr", "n", "cap", "w", "K", "cin", "cout", "scale", "shift", "relu", "y", "cfg", "stream")
        for n_, v in kw.items():
            a[names.index(n_)] = v
        return fwd(*a)
    assert call(x=null) == EINVAL and call(n=null) == EINVAL and call(w=null) == EINVAL and call(y=null) == EINVAL
    assert call(cap=0) == EINVAL and call(cfg=1) == EINVAL                     # (cfg is reserved: 0)
    assert call(cin=64, cout=32) == EINVAL and call(K=9) == EINVAL             # no kernel for the shape
    assert call(nbr=null) == EINVAL and call(K=1) == EINVAL                    # K = 1 <-> identity rulebook
    assert call(x_is_f32=1) == EINVAL                                          # fp32 operands only for Cin = 4
    assert call(cin=4, cout=16, x_is_f32=0) == EINVAL                          # ... and there they are required
    assert call(x=C.c_void_p(24)) == EINVAL and call(y=C.c_void_p(18)) == EINVAL and call(scale=C.c_void_p(20)) == EINVAL
    dn = L.sassd_densify_from_bf16
    assert dn(null, p16, p16, 100, 64, 5, 200, 176, 1, 1, p16, 1, null) == EINVAL
    assert dn(p16, p16, p16, 100, 64, 5, 200, 176, 1, 1, null, 0, null) == EINVAL
    assert dn(p16, p16, p16, 100, 64, 5, 3, 5, 1, 1, p16, 1, null) == EINVAL           # H W % 8
    assert dn(p16, p16, p16, 100, 64, 5, 200, 176, 1, 1, C.c_void_p(24), 0, null) == EINVAL
    assert dn(p16, p16, p16, 0, 64, 5, 200, 176, 1, 1, p16, 1, null) == EINVAL
    assert dn(p16, p16, p16, 100, 64, 5, 200, 176, 0, 1, p16, 1, null) == EINVAL


def _device_asm(tmp_path):
    src = os.path.join(ROOT, "sa-ssd_amd", "csrc", "spconv.hip")
    asm = str(tmp_path / "spconv.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math",
             "-fhip-fp32-correctly-rounded-divide-sqrt", "-ffp-contract=on"]
    subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", src, "-o", asm], check=True, cwd=os.path.dirname(src),
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(asm).read()


def _functions(asm, pattern):
    out = {}
    for m in re.finditer(r"^(_Z\w*%s\w*):.*?$(.*?)^\s*\.size\s+\1," % pattern, asm, re.S | re.M):
        out[m.group(1)] = m.group(2)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_bf16_sparse_kernels_are_bf16_mfma_without_float_atomics(tmp_path):
    asm = _device_asm(tmp_path)
    convs = _functions(asm, "spconv_bf16_kernel")
    shapes = {(int(a), int(b)) for a, b in (re.search(r"ILi(\d+)ELi(\d+)E", n).groups() for n in convs)}
    assert shapes == {(16, 16), (16, 32), (32, 32), (32, 64), (64, 64)}, shapes
    new = dict(convs)
    new.update(_functions(asm, "spconv_c4_kernelILi16EtE"))
    new.update(_functions(asm, "densify_from_bf16_kernel"))
    new.update(_functions(asm, "pack_weight_bf16_kernel"))
    assert len(new) == len(convs) + 4, sorted(new)
    for name, body in new.items():
        assert not re.search(r"\b(global|flat|buffer)_atomic", body), name
        assert "scratch_" not in body, (name, "register spills")
    for name, body in convs.items():
        assert set(re.findall(r"\bv_mfma\w*", body)) == {"v_mfma_f32_4x4x4_16b_bf16"}, name    # bf16 operands only
        assert "v_cvt_pk_bf16_f32" in body, (name, "bf16 store not rounded by the conversion instruction")


def test_sparse_precision_argument_and_plan_cache_key(monkeypatch):
    from sassd import detector as D
    from sassd.config import Config
    from sassd.pipeline import InferencePlan
    with pytest.raises(ValueError, match="sparse_precision"):
        InferencePlan({}, sparse_precision="fp16")
    with pytest.raises(ValueError, match="sparse_precision"):
        InferencePlan({}, precision="bf16", sparse_precision="int8")
    built = []

    class FakePlan:
        def __init__(self, sd, **kw):
            built.append(kw)
            self.anchors = torch.as_tensor(kw["anchors"])
            self.precision, self.sparse_precision = kw["precision"], kw["sparse_precision"]
    monkeypatch.setattr(D, "InferencePlan", FakePlan)
    c = Config.fromfile("configs/car_cfg.py")
    model = D.build_detector(c.model, c.train_cfg, c.test_cfg).eval()
    an = np.zeros((10, 7), np.float32)
    p = model.plan(1, an, "cpu")
    assert p.sparse_precision == "fp32" and p.precision == "fp32" and len(built) == 1
    assert model.plan(1, an, "cpu") is p and len(built) == 1                    # cached
    model.test_cfg["sparse_precision"] = "bf16"
    p2 = model.plan(1, an, "cpu")
    assert len(built) == 2 and p2.sparse_precision == "bf16" and p2.precision == "fp32"
    model.test_cfg["precision"] = "bf16"
    p3 = model.plan(1, an, "cpu")
    assert len(built) == 3 and (p3.precision, p3.sparse_precision) == ("bf16", "bf16")
    del model.test_cfg["sparse_precision"]
    p4 = model.plan(1, an, "cpu")
    assert len(built) == 4 and (p4.precision, p4.sparse_precision) == ("bf16", "fp32")


def test_noise_floor_of_the_bf16_sparse_oracle():
    model, _ = B16.car_model()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    an, bv = B16.car_anchors()
    ft = H.oracle_features(sd, [H.frame("k21", 0)], an, bv, CFG)
    fl = noise_floor(sd, ft)
    print("bf16-sparse oracle noise floor (K21, BatchNorm folded vs textbook, bf16 dense):",
          {k: (["%.1e" % x for x in v] if isinstance(v, np.ndarray) else "%.2e" % v) for k, v in fl.items()})
    assert fl["flips_sparse"] > 0, "the two BatchNorm forms should flip some roundings"
    assert fl["sparse_rel"] <= FLOOR["sparse_rel"], fl
    assert max(fl["conv6_rel"], fl["x_rel"], fl["psmap_rel"]) <= FLOOR["bev_rel"], fl
    assert fl["masked_score"] <= FLOOR["masked_score"], fl
    assert np.all(fl["box_field"] <= FLOOR["box_field"]), fl
    assert fl["logit"] <= FLOOR["logit"] and fl["score"] <= FLOOR["score"], fl
    # the floor is small against the effect of the rounding rule itself (bf16-sparse against the fp32 oracle)
    assert fl["bf16_vs_fp32_sparse_rel"] > fl["sparse_rel"]
