"""The deterministic training mode without a GPU: the `_det` entry points exist and validate their arguments before any
device work (SASSD_EINVAL / SASSD_ENOSPC, host-arithmetic workspace queries), their kernels hold no float atomics (device
assembly), a numpy model of the summation-order contract of include/sassd.h, and the plumbing of the one switch
(train_cfg['deterministic'] or torch.use_deterministic_algorithms) down to the kernel wrappers, which are mocked here."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import _C

EINVAL, ENOSPC = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def interp_grad_model(g, idx, w, init):
    """The 3-NN interpolation-gradient contract: grad[r] = init[r], then fl(g[p] * w[p, j]) added one at a time in
    ascending (p, j) over the entries with idx[p, j] == r, in fp32 (products rounded before the add)."""
    n, c = g.shape
    m = init.shape[0]
    out = init.astype(np.float32).copy()
    rows = idx.reshape(-1).astype(np.int64)
    e = np.arange(rows.size)
    keep = (rows >= 0) & (rows < m)
    rows, e = rows[keep], e[keep]
    order = np.lexsort((e, rows))                       # by row, then ascending entry (p * 3 + j)
    rows, e = rows[order], e[order]
    prod = g[e // 3] * w.reshape(-1)[e][:, None]        # float32 x float32: rounded products
    assert prod.dtype == np.float32
    rank = np.arange(rows.size) - np.searchsorted(rows, rows, "left")
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.searchsorted(rank[by_rank], np.arange(rank.max() + 2 if rank.size else 1))
    for k in range(len(bounds) - 1):
        sel = by_rank[bounds[k]:bounds[k + 1]]          # the k-th entry of every row that has one (rows distinct)
        out[rows[sel]] = out[rows[sel]] + prod[sel]
    return out


def test_interp_grad_model_is_the_sequential_sum():
    rng = np.random.default_rng(0)
    n, m, c = 50, 7, 3
    idx = rng.integers(0, m, size=(n, 3)).astype(np.int32)
    idx[5, 1] = -1                                       # ignored
    w = rng.random((n, 3)).astype(np.float32)
    g = rng.standard_normal((n, c)).astype(np.float32)
    init = rng.standard_normal((m, c)).astype(np.float32)
    ref = init.copy()
    for p in range(n):
        for j in range(3):
            r = idx[p, j]
            if 0 <= r < m:
                for ch in range(c):
                    ref[r, ch] = np.float32(ref[r, ch] + np.float32(g[p, ch] * w[p, j]))
    assert np.array_equal(interp_grad_model(g, idx, w, init).view(np.uint32), ref.view(np.uint32))


def test_summation_order_matters_in_fp32():
    """Why the contract fixes the order: the same three terms in two orders give different fp32 sums."""
    t = np.array([1e8, 1.0, -1e8], np.float32)
    assert np.float32(np.float32(t[0] + t[1]) + t[2]) != np.float32(np.float32(t[0] + t[2]) + t[1])


def test_det_entry_points_validate_before_device_work():
    L = _C.lib()
    null, p16 = None, C.c_void_p(16)
    # workspace queries: host arithmetic, 0 for impossible shapes
    assert L.sassd_three_interpolate_grad_det_workspace_bytes(1000, 200) >= 3000 * 4 * 2 + 200 * 4 * 3
    assert L.sassd_three_interpolate_grad_det_workspace_bytes(-1, 5) == 0
    M = (C.c_int * 3)(900, 400, 150)
    base = L.sassd_aux_head_workspace_bytes(3000)
    assert L.sassd_aux_head_bwd_det_workspace_bytes(3000, M) >= base + 9 * 3000 * 4 * 2
    assert L.sassd_aux_head_bwd_det_workspace_bytes(3000, (C.c_int * 3)(900, 0, 150)) == 0
    assert L.sassd_aux_head_bwd_det_workspace_bytes(0, M) == 0
    assert L.sassd_pswarp_sample_bwd_det_workspace_bytes(2, 4096) == 0
    assert L.sassd_grad_sumsq_det_workspace_bytes(5_000_000) == 1024 * 4
    assert L.sassd_grad_sumsq_det_workspace_bytes(1) == 256
    assert L.sassd_grad_sumsq_det_workspace_bytes(-1) == 0
    # three_interpolate_grad_det
    tig = L.sassd_three_interpolate_grad_det
    assert tig(0, 10, 10, p16, p16, p16, p16, p16, 1 << 20, null) == EINVAL               # c < 1
    assert tig(8, 10, 10, null, p16, p16, p16, p16, 1 << 20, null) == EINVAL              # grad_out NULL
    assert tig(8, 10, 10, p16, null, p16, p16, p16, 1 << 20, null) == EINVAL
    assert tig(8, 10, 10, p16, p16, p16, p16, null, 1 << 20, null) == EINVAL              # workspace NULL
    assert tig(8, 10, 10, p16, p16, p16, p16, p16, 16, null) == ENOSPC
    # aux_head_bwd_det: the arguments of sassd_aux_head_bwd
    P3 = C.c_void_p * 3
    f3, i3 = P3(16, 16, 16), P3(16, 16, 16)
    need = L.sassd_aux_head_bwd_det_workspace_bytes(3000, M)
    aux = L.sassd_aux_head_bwd_det
    args = [3000, f3, M, i3, p16, p16, p16, p16, p16, p16, f3, p16, p16, p16, need, null]
    assert aux(*([0] + args[1:])) == EINVAL                                                 # N < 1
    assert aux(*(args[:2] + [null] + args[3:])) == EINVAL                                    # M NULL
    assert aux(*(args[:2] + [(C.c_int * 3)(900, -1, 150)] + args[3:])) == EINVAL           # impossible level size
    assert aux(*(args[:13] + [null] + args[14:])) == EINVAL                                  # workspace NULL
    assert aux(*(args[:14] + [need - 1, null])) == ENOSPC
    assert aux(*(args[:14] + [base, null])) == ENOSPC                 # the atomic kernel's workspace is not enough
    # pswarp_sample_bwd_det
    pw = L.sassd_pswarp_sample_bwd_det
    assert pw(null, 1, 200, 176, p16, p16, 64, 0.0, 40.0, 2.5, p16, p16, p16, null, 0, null) == EINVAL
    assert pw(p16, 0, 200, 176, p16, p16, 64, 0.0, 40.0, 2.5, p16, p16, p16, null, 0, null) == EINVAL      # batch
    assert pw(p16, 1, 200, 176, p16, p16, 0, 0.0, 40.0, 2.5, p16, p16, p16, null, 0, null) == EINVAL       # capK
    assert pw(p16, 1, 200, 176, p16, p16, 64, 0.0, 40.0, 2.5, p16, null, p16, null, 0, null) == EINVAL     # dfeat
    # grad_sumsq_det
    gs = L.sassd_grad_sumsq_det
    assert gs(null, 10, p16, p16, 4096, null) == EINVAL
    assert gs(C.c_void_p(20), 10, p16, p16, 4096, null) == EINVAL                      # grad not 16-byte aligned
    assert gs(p16, 10, p16, null, 4096, null) == EINVAL
    assert gs(p16, 5_000_000, p16, p16, 1024 * 4 - 4, null) == ENOSPC


DET_KERNELS = {
    "aux_head.hip": ["inv_zero_kernel", "inv_count_kernel", "inv_scan_kernel", "inv_fill_kernel", "inv_rank_kernel",
                     "aux_gather_det_kernel"],
    "pointops.hip": ["inv_zero_kernel", "inv_count_kernel", "inv_scan_kernel", "inv_fill_kernel", "inv_rank_kernel",
                     "three_interpolate_gather_det_kernel"],
    "heads.hip": ["pswarp_dfeat_det_kernel", "pswarp_bwd_kernelILb0E"],
    "optim.hip": ["sumsq_det_part_kernel", "sumsq_det_final_kernel"],
}
FLOAT_ATOMICS = re.compile(r"global_atomic_add_f32|global_atomic_pk_add_|flat_atomic_add_f32|buffer_atomic_add_f32")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("src", sorted(DET_KERNELS))
def test_det_kernels_have_no_float_atomics(tmp_path, src):
    path = os.path.join(ROOT, "sa-ssd_amd", "csrc", src)
    asm = str(tmp_path / (src + ".s"))
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math",
             "-fhip-fp32-correctly-rounded-divide-sqrt", "-ffp-contract=on"]
    subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", path, "-o", asm], check=True, cwd=os.path.dirname(path),
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(asm).read()
    bodies = {}
    for m in re.finditer(r"^(_Z\S+):\s*;", text, re.M):
        end = text.find(".Lfunc_end", m.end())
        bodies[m.group(1)] = text[m.end():end]
    found_atomic_kernel = False
    for name in DET_KERNELS[src]:
        hits = [s for s in bodies if name in s]
        assert hits, "kernel %s not found in %s" % (name, src)
        for s in hits:
            assert not FLOAT_ATOMICS.search(bodies[s]), "%s holds a float atomic" % s
    for s, body in bodies.items():              # the guard can see them: the atomic kernels next door do hold them
        found_atomic_kernel |= bool(FLOAT_ATOMICS.search(body))
    assert found_atomic_kernel, "the pattern no longer matches the float atomics of the default kernels"


# ---- plumbing ----------------------------------------------------------------------------------------------------------
def _car_model(deterministic=None):
    from sassd import synth
    model, cfg = synth.build_detector_for(synth.workload("car"), 0, train=True)
    if deterministic is not None:
        model.train_cfg['deterministic'] = deterministic
    return model, cfg


def test_reference_configs_have_no_deterministic_key_and_default_off():
    from sassd import train
    model, cfg = _car_model()
    assert 'deterministic' not in model.train_cfg
    assert not model.deterministic_training()
    assert train.resolve_deterministic(model) is False


def test_build_optimizer_resolves_the_switch(monkeypatch):
    from sassd import kernels as K, train
    model, cfg = _car_model(True)
    optim_cfg = dict(cfg.optimizer, pack_plan=False)
    assert train.build_optimizer(model, optim_cfg).deterministic
    assert not train.build_optimizer(model, optim_cfg, deterministic=False).deterministic
    model2, _ = _car_model()
    assert not train.build_optimizer(model2, optim_cfg).deterministic
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        assert train.build_optimizer(model2, optim_cfg).deterministic
        assert model2.deterministic_training()
    finally:
        torch.use_deterministic_algorithms(prev)
    # AdamOneCycle.step hands the flag to grad_sumsq
    seen = []
    monkeypatch.setattr(K, "grad_sumsq", lambda g, out=None, deterministic=False: seen.append(deterministic) or out)
    monkeypatch.setattr(K, "adam_step", lambda *a, **k: None)
    opt = train.build_optimizer(model, optim_cfg)
    assert opt.max_norm > 0
    opt.step()
    assert seen == [True]


def test_autograd_functions_pass_the_flag(monkeypatch):
    from sassd import autograd as AG, kernels as K
    seen = {}

    def fake_pswarp_bwd(feat, guided, counts, cap_k, off, scale, dlog, deterministic=False):
        seen["pswarp"] = deterministic
        return torch.zeros_like(feat), torch.zeros(guided.shape[0], cap_k, 7)

    def fake_aux_bwd(feats, nn_idx, w1, w2, wgt, h, gout, g, deterministic=False):
        seen["aux"] = deterministic
        return [torch.zeros_like(f) for f in feats], torch.zeros(64, 160), torch.zeros(4, 64)

    monkeypatch.setattr(K, "pswarp_sample", lambda feat, boxes, counts, cap_k, off, scale, logits=None:
                        feat.new_zeros(boxes.shape[0], cap_k))
    monkeypatch.setattr(K, "pswarp_sample_bwd", fake_pswarp_bwd)
    monkeypatch.setattr(K, "aux_head_fwd", lambda feats, nn_idx, nn_d2, w1, w2, label, target, npos:
                        (torch.zeros(2), torch.zeros(4, 9), torch.zeros(4, 64), torch.zeros(4, 4), torch.zeros(4, 4)))
    monkeypatch.setattr(K, "aux_head_bwd", fake_aux_bwd)
    monkeypatch.setattr(AG, "_n_ptr", lambda k, dev: torch.tensor([k], dtype=torch.int32))
    for det in (False, True):
        feat = torch.zeros(1, 28, 4, 4, requires_grad=True)
        boxes = torch.zeros(3, 7, requires_grad=True)
        AG.PSWarpFn.apply(feat, boxes, (0.0, 0.0), 1.0, det).sum().backward()
        assert seen.pop("pswarp") is det
        AG.PSWarpBatchFn.apply(feat, boxes.view(1, 3, 7), torch.tensor([3], dtype=torch.int32), (0.0, 0.0), 1.0,
                               det).sum().backward()
        assert seen.pop("pswarp") is det
        fs = [torch.zeros(5, c, requires_grad=True) for c in (32, 64, 64)]
        ws = [torch.zeros(64, 160, requires_grad=True), torch.zeros(1, 64, requires_grad=True),
              torch.zeros(3, 64, requires_grad=True)]
        AG.AuxHeadFn.apply(*fs, *ws, None, None, None, None, None, det).sum().backward()
        assert seen.pop("aux") is det
    # the default keeps the atomic kernels
    feat = torch.zeros(1, 28, 4, 4, requires_grad=True)
    AG.PSWarpFn.apply(feat, torch.zeros(3, 7), (0.0, 0.0), 1.0).sum().backward()
    assert seen.pop("pswarp") is False


def test_three_interpolate_backward_follows_the_torch_flag(monkeypatch):
    from sassd import kernels as K, pointnet2_utils as PU
    seen = []
    monkeypatch.setattr(K, "three_interpolate", lambda f, i, w: torch.zeros(i.shape[0], f.shape[1]))
    monkeypatch.setattr(K, "three_interpolate_grad", lambda go, i, w, m, deterministic=False:
                        seen.append(deterministic) or torch.zeros(m, go.shape[1]))
    f = torch.zeros(6, 4, requires_grad=True)
    idx, w = torch.zeros(3, 3, dtype=torch.int32), torch.ones(3, 3) / 3
    PU.three_interpolate(f, idx, w).sum().backward()
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        f.grad = None
        PU.three_interpolate(f, idx, w).sum().backward()
    finally:
        torch.use_deterministic_algorithms(prev)
    assert seen == [False, True]


def test_detector_passes_the_switch_to_the_heads(monkeypatch):
    """forward_train resolves train_cfg['deterministic'] / the torch flag once and hands it to the aux head and the
    PSWarp head (the forward itself is mocked down to the calls that carry the flag)."""
    from sassd import detector as D
    model, _ = _car_model(True)
    seen = {}
    monkeypatch.setattr(model, "merge_second_batch", lambda kw: dict(voxels=None, num_points=None, coordinates=None,
                                                                      gt_bboxes=[], gt_labels=[], gt_types=[],
                                                                      anchors=None, anchors_mask=None))
    monkeypatch.setattr(model.backbone, "forward", lambda v, n: None)
    monkeypatch.setattr(model.neck, "forward", lambda *a, **k: (torch.zeros(1), torch.zeros(1), (None, None, None)))
    monkeypatch.setattr(type(model.neck), "aux_loss", lambda self, *a, gt_bboxes=None, deterministic=False:
                        seen.setdefault("aux", deterministic) and {} or {})
    monkeypatch.setattr(model.rpn_head, "forward", lambda x: (None, None, None))
    monkeypatch.setattr(model.rpn_head, "loss", lambda *a, **k: {})
    monkeypatch.setattr(model.rpn_head, "get_guided_anchors", lambda *a, **k: ([], None))
    monkeypatch.setattr(model.extra_head, "forward", lambda x, guided, is_test=False, deterministic=False:
                        seen.setdefault("pswarp", deterministic))
    monkeypatch.setattr(model.extra_head, "loss", lambda *a, **k: {})
    model.forward_train(None, [{}])
    assert seen == dict(aux=True, pswarp=True)
    seen.clear()
    model.train_cfg['deterministic'] = False
    model.forward_train(None, [{}])
    assert seen == dict(aux=False, pswarp=False)
    seen.clear()
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        model.forward_train(None, [{}])
    finally:
        torch.use_deterministic_algorithms(prev)
    assert seen == dict(aux=True, pswarp=True)
    assert D.SingleStageDetector.deterministic_training
