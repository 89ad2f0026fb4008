"""-m gpu: box fusion through the public interface -- InferencePlan(fuse_iou=...), FrameStream(fuse_iou=...), test_cfg['fuse_iou']
-- on bench.py's car workload, batch 1, the 4 seeded car frames.

The bar is equality of bytes.  Scores, labels and counts are those of the same plan without fusion; the boxes are
sassd.fuse.fuse_host on the plan's OWN buffers -- the candidate list it handed to rescore / NMS (plan.df, or plan.pool under
tta), the device's scores of its logits, its unfused detections plan.det -- with the device's own IoU
(K.boxes_iou_bev(bev(detections), bev(candidates)): the kernel's function in the kernel's argument order).  The kernel is held
to the CPU oracle's IoU in tests/test_gpu_box_fuse_kernel.py."""
import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import fuse as F, kernels as K
from sassd.pipeline import InferencePlan
from sassd.stream import FrameStream, calib_block_of, decode_record

import box_fuse_cases as BC
import tta_cases as TC
import kitti_anno_cases as KA
import test_gpu_frame_stream as TS

pytestmark = pytest.mark.gpu

FUSE = 0.7
CAL = dict(calib=KA.calibration(), img_shape=KA.IMG_SHAPE)
_CACHE = {}


def _frames(w):
    return [np.ascontiguousarray(w["frame"](i)) for i in range(4)]


def _plan(sd, w, dev, **kw):
    return InferencePlan(sd, batch_size=1, anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev, **dict(w["plan"], **kw))


def _stream(sd, w, dev, inflight, **kw):
    return FrameStream(sd, inflight=inflight, points_cap=w["points_cap"], batch_size=1, anchors=w["anchors"],
                       anchors_bv=w["anchors_bv"], device=dev, **dict(w["plan"], **kw))


def _unfused(dev, tta, overlap=True):
    """results() of the plan without fusion on the 4 frames (computed once per configuration)."""
    key = ("unfused", None if tta is None else len(tta), overlap)
    if key not in _CACHE:
        sd, w, _ = TS._workload(dev)
        plan = _plan(sd, w, dev, overlap=overlap, **({} if tta is None else dict(tta=tta)))
        out = []
        for p in _frames(w):
            plan.run_from_points([torch.from_numpy(p).to(dev)])
            out.append(plan.results())
        _CACHE[key] = out
    return _CACHE[key]


def _statement(plan, dev):
    """fuse_host on the buffers the plan holds after a frame -> (fused boxes [1, capD, 7], members of the busiest detection)."""
    cand = plan.df if plan.tta is None else plan.pool
    logits = plan.logits if plan.tta is None else plan.pool["logits"]
    c = dict(guided=cand["guided"].cpu().numpy(), labels=cand["labels"].cpu().numpy(), counts=cand["counts"].cpu().numpy(),
             scores=K.candidate_scores(logits).cpu().numpy())
    det = {k: v.cpu().numpy() for k, v in plan.det.items()}

    def iou(a, b):
        return K.boxes_iou_bev(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)).cpu().numpy()
    mats = BC.iou_matrices(c, det, iou)
    mem = BC.members(c, det, mats, c["scores"], plan.fuse_iou)
    return F.fuse_host(c, det, plan.score_thr, plan.fuse_iou, mats), max([int(m.max()) for m in mem if m.size] or [0])


def _fused(dev, tta, overlap=True):
    """results() of the fused plan on the 4 frames, each checked against the statement (computed once per configuration)."""
    key = ("fused", None if tta is None else len(tta), overlap)
    if key not in _CACHE:
        sd, w, _ = TS._workload(dev)
        plan = _plan(sd, w, dev, fuse_iou=FUSE, overlap=overlap, **({} if tta is None else dict(tta=tta)))
        assert plan.fuse_iou == FUSE and plan.out is not plan.det and plan.out["boxes"] is plan.fused
        assert plan.out["scores"] is plan.det["scores"] and plan.out["counts"] is plan.det["counts"]
        base = _unfused(dev, tta, overlap)
        out, moved, most = [], 0, 0
        for i, p in enumerate(_frames(w)):
            ret = plan.run_from_points([torch.from_numpy(p).to(dev)])
            assert ret is plan.out
            got = plan.results()
            want, m = _statement(plan, dev)
            most = max(most, m)
            b0 = base[i][0]
            assert got[0][0] is not None and b0[0] is not None, i
            n = len(b0[0])
            assert BC.same_bits(got[0][1], b0[1]) and BC.same_bits(got[0][2], b0[2]), ("scores / labels", i)
            assert got[0][0].shape == (n, 7) and int(plan.det["counts"][0].item()) == n
            assert BC.same_bits(plan.det["boxes"][0, :n].cpu().numpy(), b0[0]), ("plan.det keeps the unfused boxes", i)
            assert BC.same_bits(got[0][0], want[0, :n]), ("fused boxes against the statement", i)
            moved += int((got[0][0] != b0[0]).any(-1).sum())
            out.append(got)
        print("fuse_iou %.2f, %s: %d of %d boxes moved over 4 frames, busiest detection has %d members"
              % (FUSE, "plain" if tta is None else "tta V%d" % len(tta), moved, sum(len(r[0][0]) for r in out), most))
        assert moved >= 1 and most >= 2, "no box moved: the comparison is empty"
        _CACHE[key] = out
    return _CACHE[key]


# ---- 1: off is off ----------------------------------------------------------------------------------------------------------
def test_fuse_iou_none_is_the_plain_plan(dev):
    sd, w, _ = TS._workload(dev)
    plan = _plan(sd, w, dev, fuse_iou=None)
    assert plan.fuse_iou is None and plan.fused is None and plan.out is plan.det
    for i, p in enumerate(_frames(w)):
        assert plan.run_from_points([torch.from_numpy(p).to(dev)]) is plan.det
        TS._same_dets(plan.results(), _unfused(dev, None)[i], ("fuse_iou=None", i))


# ---- 2: the fused plan is the statement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tta", [None, "V2"])
def test_fused_plan_equals_the_statement(dev, tta):
    _fused(dev, None if tta is None else TC.V2)


# ---- 3: the captured frame ------------------------------------------------------------------------------------------------
def test_captured_frame_replays_the_eager_result_with_one_more_kernel_node(dev):
    KERNEL = 0                                                          # hipGraphNodeTypeKernel
    sd, w, _ = TS._workload(dev)
    want = _fused(dev, TC.V2)
    plan = _plan(sd, w, dev, fuse_iou=FUSE, tta=TC.V2)
    plan.capture(w["points_cap"])
    for i in (1, 0, 3, 2, 1):                                           # out of order, one frame twice: nothing carries over
        assert plan.run_graph([torch.from_numpy(_frames(w)[i]).to(dev)]) is plan.out
        TS._same_dets(plan.results(), want[i], ("graph", i))
    base = _plan(sd, w, dev, tta=TC.V2)
    base.capture(w["points_cap"])
    torch.cuda.synchronize()
    n0, n1 = TS._node_types(base, dev), TS._node_types(plan, dev)
    print("frame graph nodes by type: tta V2", n0, "with fuse_iou", n1)
    assert set(n1) == {KERNEL} and set(n0) == {KERNEL}, (n0, n1)
    assert n1[KERNEL] == n0[KERNEL] + 1
    plan.run_graph([torch.from_numpy(_frames(w)[0]).to(dev)])           # the plan still works after the second capture
    TS._same_dets(plan.results(), want[0], "graph after recapture")


# ---- 4: the stream --------------------------------------------------------------------------------------------------------
def test_stream_with_two_frames_in_flight_equals_the_plan(dev):
    sd, w, _ = TS._workload(dev)
    frames = _frames(w)
    want = _fused(dev, None, overlap=False)                             # a stream in flight runs one-branch plans
    for i in range(4):                                                  # (the branch count does not change a bit)
        TS._same_dets(want[i], _fused(dev, None)[i], ("one-branch plan", i))
    with _stream(sd, w, dev, 2, fuse_iou=FUSE) as fs:
        assert all(p.fuse_iou == FUSE and p.tta is None for p in fs.plans)
        order = [0, 1, 2, 3, 3, 1]
        got = list(fs.map([frames[i]] for i in order))
        for (_, d), i in zip(got, order):
            TS._same_dets(d, want[i], ("stream inflight 2", i))
        assert all(int(p.status.item()) == 0 for p in fs.plans)


def test_stream_annotations_are_those_of_the_fused_boxes(dev):
    sd, w, _ = TS._workload(dev)
    frames = _frames(w)
    want = _fused(dev, None, overlap=False)
    plan = _plan(sd, w, dev, fuse_iou=FUSE, overlap=False)
    block = torch.from_numpy(calib_block_of(CAL["calib"], CAL["img_shape"])).to(dev).view(1, -1)
    with _stream(sd, w, dev, 2, fuse_iou=FUSE, annos=True) as fs:
        got = [d for _, d in fs.map(([p], None, [CAL]) for p in frames)]
    n_cam = 0
    for i, p in enumerate(frames):
        plan.run_from_points([torch.from_numpy(p).to(dev)])             # the plan's fused detections ...
        seq = torch.tensor([i + 1], dtype=torch.int32, device=dev)
        rec = K.frame_seal_kitti(plan.out, seq, plan.status, block)     # ... and the annotation path on them
        torch.cuda.synchronize()
        ref = decode_record(rec.cpu().numpy(), 1, plan.capD, i + 1, annos=True)
        assert len(got[i]) == 1 and len(got[i][0]) == 4
        TS._same_dets([got[i][0][:3]], want[i], ("annos stream against the fused plan", i))
        TS._same_dets([ref[0][:3]], want[i], ("sealed plan against the fused plan", i))
        for k in ref[0][3]:
            assert TC.same_bits(got[i][0][3][k], ref[0][3][k]), (i, k)
        n_cam += len(ref[0][3]["index"])
    assert n_cam >= 1, "no detection meets the image: the comparison is empty"


# ---- 5: the detector ------------------------------------------------------------------------------------------------------
def test_detector_plan_honours_test_cfg_fuse_iou(dev):
    sd, w, model = TS._workload(dev)
    model = model.to(dev).eval()
    an = torch.from_numpy(w["anchors"]).to(dev)
    kw = dict(cap_k=w["plan"]["cap_k"], cap_d=w["plan"]["cap_d"])
    had, old = "fuse_iou" in model.test_cfg, model.test_cfg.get("fuse_iou")
    try:
        model.test_cfg.pop("fuse_iou", None)
        plain = model.plan(1, an, dev, **kw)
        assert plain.fuse_iou is None and plain.out is plain.det
        model.test_cfg["fuse_iou"] = FUSE
        p1 = model.plan(1, an, dev, **kw)
        assert p1 is not plain and p1.fuse_iou == FUSE
        assert model.plan(1, an, dev, **kw) is p1                       # the same value: the cached plan
        model.test_cfg["fuse_iou"] = 0.55
        p2 = model.plan(1, an, dev, **kw)                               # a changed value rebuilds the plan
        assert p2 is not p1 and p2.fuse_iou == 0.55
        assert model.plan(1, an, dev, fuse_iou=None, **kw).fuse_iou is None     # an explicit fuse_iou= overrides test_cfg
        assert model.plan(1, an, dev, fuse_iou=FUSE, **kw).fuse_iou == FUSE
        with pytest.raises(ValueError, match="fuse_iou"):
            model.test_cfg["fuse_iou"] = 1.5
            model.plan(1, an, dev, **kw)
        model.test_cfg["fuse_iou"] = FUSE
        plan = model.plan(1, an, dev, **kw)
        ref = _plan(sd, w, dev, fuse_iou=FUSE, score_thr=plan.score_thr, iou_thr=plan.iou_thr, rpn_thr=plan.rpn_thr)
        pts = torch.from_numpy(_frames(w)[0]).to(dev)
        plan.run_from_points([pts])
        ref.run_from_points([pts])
        TS._same_dets(plan.results(), ref.results(), "detector plan")
        with model.frame_stream(an, inflight=1, points_cap=w["points_cap"], device=dev, **kw) as fs:
            assert fs.plans[0].fuse_iou == FUSE
        with model.frame_stream(an, inflight=1, points_cap=w["points_cap"], device=dev, fuse_iou=None, **kw) as fs:
            assert fs.plans[0].fuse_iou is None
    finally:
        model.test_cfg.pop("fuse_iou", None)
        if had:
            model.test_cfg["fuse_iou"] = old
        model._plan, model._plan_key = None, None


# ---- 6: the other precisions ----------------------------------------------------------------------------------------------
def test_bf16_plan_fuses_its_own_candidates(dev):
    """precision= and sparse_precision= change what the heads see, not the node behind NMS: the statement on the plan's own buffers."""
    sd, w, _ = TS._workload(dev)
    kw = dict(precision="bf16", sparse_precision="bf16")
    base, plan = _plan(sd, w, dev, **kw), _plan(sd, w, dev, fuse_iou=FUSE, **kw)
    n_det = 0
    for i, p in enumerate(_frames(w)[:2]):
        pts = torch.from_numpy(p).to(dev)
        base.run_from_points([pts])
        plan.run_from_points([pts])
        want, got = base.results(), plan.results()
        if want[0][0] is None:
            assert got[0][0] is None
            continue
        n = len(want[0][0])
        n_det += n
        assert BC.same_bits(got[0][1], want[0][1]) and BC.same_bits(got[0][2], want[0][2]), i
        assert BC.same_bits(plan.det["boxes"][0, :n].cpu().numpy(), want[0][0]), i
        assert BC.same_bits(got[0][0], _statement(plan, dev)[0][0, :n]), i
    assert n_det >= 1
