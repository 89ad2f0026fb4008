"""-m gpu: sassd_box_fuse alone (include/sassd.h "Box fusion") on the seeded clusters of tests/box_fuse_cases.py: candidates per
sample at the edges of the 64-lane chunk (1, 63, 64, 65, 257), detection counts at the edges of the wave / workgroup split
(1, 4, 5, capD), unequal counts in a batch of 2, a sample without candidates, a sample without detections, a count above
capK.  The detections are K.rescore_nms's on the same candidates.

Two statements, both BIT FOR BIT (no tolerance):
  (a) sassd.fuse.fuse_host fed with the device's own scores (K.candidate_scores) and the device's own IoU,
      K.boxes_iou_bev(bev(detections), bev(candidates)) -- the function and the argument order of the kernel;
  (b) the same fed with the CPU oracle's IoU.  The two IoUs agree to 1e-5 (test_gpu_kernels.py), so a membership can only differ
      where an IoU lies that close to fuse_iou: the test ASSERTS that none lies within 1e-3 (box_fuse_cases.MARGIN) on the
      CPU matrix -- the seeds were chosen for it on the CPU -- and skips no pair."""
import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import fuse as F, kernels as K
from oracle import clib

import box_fuse_cases as BC

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-777.25)
_REF = {}


def _dev(d, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}


def _gpu_iou(dev):
    def iou(a, b):
        return K.boxes_iou_bev(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)).cpu().numpy()
    return iou


def _reference(dev, name):
    """Per case, computed once and left unchanged: candidates, the device's detections and scores, both IoU matrix lists."""
    if name not in _REF:
        _, seed, cap_k, cap_d, samples, counts, want = next(c for c in BC.CASES if c[0] == name)
        cand = BC.batch(seed, cap_k, samples, counts)
        t = _dev(cand, dev)
        det_t = K.rescore_nms(t["guided"], t["logits"], t["labels"], t["counts"], BC.SCORE_THR, BC.IOU_THR, cap_d,
                              out=dict(boxes=torch.zeros(len(samples), cap_d, 7, device=dev)), status=K.new_status(dev))
        scores = K.candidate_scores(t["logits"]).cpu().numpy()
        det = {k: v.cpu().numpy() for k, v in det_t.items()}
        assert tuple(int(c) for c in det["counts"]) == want, (name, det["counts"])
        _REF[name] = dict(cand=cand, t=t, det=det, det_t=det_t, scores=scores, cap_d=cap_d,
                          gpu=BC.iou_matrices(cand, det, _gpu_iou(dev)), cpu=BC.iou_matrices(cand, det, clib.boxes_iou_bev))
    return _REF[name]


def _launch(r, fuse_iou, dev):
    B = r["cand"]["guided"].shape[0]
    out = torch.full((B, r["cap_d"], 7), float(SENTINEL), dtype=torch.float32, device=dev)
    t = r["t"]
    got = K.box_fuse(t["guided"], t["logits"], t["labels"], t["counts"], BC.SCORE_THR, fuse_iou, r["det_t"], out=out)
    assert got is out
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("fuse_iou", BC.FUSE_IOUS)
@pytest.mark.parametrize("name", [c[0] for c in BC.CASES])
def test_kernel_equals_the_statement_bit_for_bit(dev, name, fuse_iou):
    r = _reference(dev, name)
    cand, det = dict(r["cand"], scores=r["scores"]), r["det"]
    before = {k: v.copy() for k, v in det.items()}
    got = _launch(r, fuse_iou, dev)
    counts = [int(c) for c in det["counts"]]
    # (a) the device's own IoU: the kernel's function, the kernel's argument order
    want = F.fuse_host(cand, det, BC.SCORE_THR, fuse_iou, r["gpu"])
    for b, n in enumerate(counts):
        assert BC.same_bits(got[b, :n], want[b, :n]), (name, fuse_iou, b, "device IoU")
        assert (got[b, n:] == SENTINEL).all(), (name, b, "a row at or past the count was written")
    # (b) the CPU oracle's IoU, with the margin asserted on the CPU matrix
    mg = BC.margin(r["cpu"], fuse_iou)
    apart = max([float(np.abs(a.astype(np.float64) - c).max()) for a, c in zip(r["gpu"], r["cpu"]) if a.size] or [0.0])
    mem = BC.members(r["cand"], det, r["cpu"], r["scores"], fuse_iou)
    most = max([int(m.max()) for m in mem if m.size] or [0])
    moved = sum(int((got[b, :n] != det["boxes"][b, :n]).any(-1).sum()) for b, n in enumerate(counts))
    print("%s fuse_iou %.2f: detections %s, most members %d, %d boxes moved, closest IoU to the threshold %.2e (bar %.0e), "
          "device IoU - oracle IoU <= %.1e" % (name, fuse_iou, counts, most, moved, mg, BC.MARGIN, apart))
    assert mg > BC.MARGIN, (name, fuse_iou, mg)
    want_cpu = F.fuse_host(cand, det, BC.SCORE_THR, fuse_iou, r["cpu"])
    for b, n in enumerate(counts):
        assert BC.same_bits(got[b, :n], want_cpu[b, :n]), (name, fuse_iou, b, "oracle IoU")
    # not vacuous
    if sum(counts) >= 4:
        assert most >= 3 and moved >= 1, (name, most, moved)
    # det itself is untouched, and a second launch gives the same bytes
    after = {k: v.cpu().numpy() for k, v in r["det_t"].items()}
    assert all(BC.same_bits(after[k], before[k]) for k in before)
    assert BC.same_bits(_launch(r, fuse_iou, dev), got)


def test_device_scores_are_the_scores_of_the_detections(dev):
    """K.candidate_scores is the sigmoid rescore_nms reports: every detection's score is its candidate's, to the bit."""
    r = _reference(dev, "k257_empty")
    n = int(r["det"]["counts"][0])
    assert n == 28
    for t in range(n):
        j = np.flatnonzero((r["cand"]["guided"][0] == r["det"]["boxes"][0, t]).all(-1))
        assert len(j) == 1 and BC.same_bits(r["scores"][0, j[0]], r["det"]["scores"][0, t])
