"""Box fusion without a GPU (include/sassd.h "Box fusion"): the numpy statement sassd.fuse.fuse_host against a CPU loop over the
kernel's own __host__ __device__ rule (csrc/box_fuse_core.h through tests/box_fuse_harness.hip), bit for bit; the properties
the rule promises; the argument errors of every layer.  The IoU is the CPU oracle's; the scores are numpy's sigmoid, handed to
both sides (the rule takes scores and IoU as inputs)."""
import ctypes

import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import _C, fuse as F, kernels as K
from oracle import clib

import box_fuse_cases as BC

_CASES = {}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return BC.harness(tmp_path_factory.mktemp("box_fuse_harness"))


def _case(name):
    """(candidates, host detections, oracle IoU matrices, scores) of a case -- computed once, never written to."""
    if name not in _CASES:
        _, seed, cap_k, cap_d, samples, counts, want = next(c for c in BC.CASES if c[0] == name)
        cand = BC.batch(seed, cap_k, samples, counts)
        det = BC.nms_host(cand, cap_d, clib.boxes_iou_bev)
        assert tuple(int(c) for c in det["counts"]) == want, (name, det["counts"])
        _CASES[name] = (cand, det, BC.iou_matrices(cand, det, clib.boxes_iou_bev), F.sigmoid_host(cand["logits"]))
    return _CASES[name]


def _fuse(cand, det, fuse_iou, mats=None, scores=None):
    c = dict(cand) if scores is None else dict(cand, scores=scores)
    return F.fuse_host(c, det, BC.SCORE_THR, fuse_iou, clib.boxes_iou_bev if mats is None else mats)


# ---- 1: the statement is the header's loop ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse_iou", BC.FUSE_IOUS)
@pytest.mark.parametrize("name", [c[0] for c in BC.CASES])
def test_fuse_host_equals_the_harness_bit_for_bit(lib, name, fuse_iou):
    cand, det, mats, scores = _case(name)
    want = BC.harness_fuse(lib, cand, scores, det, BC.SCORE_THR, fuse_iou, mats)
    got = _fuse(cand, det, fuse_iou, mats, scores)
    assert BC.same_bits(got, want)
    assert BC.same_bits(_fuse(cand, det, fuse_iou), got)                # logits + a callable: the same statement
    mem = BC.members(cand, det, mats, scores, fuse_iou)
    if sum(int(c) for c in det["counts"]) >= 4:                         # not vacuous
        assert max(int(m.max()) for m in mem if m.size) >= 3
        assert (got != det["boxes"]).any()
    for b in range(got.shape[0]):                                       # rows at and past the count: as det has them
        assert BC.same_bits(got[b, int(det["counts"][b]):], det["boxes"][b, int(det["counts"][b]):])


def test_result_does_not_depend_on_rows_past_the_counts(lib):
    cand, det, mats, scores = _case("clamped")
    want = _fuse(cand, det, 0.55, mats, scores)
    other = {k: v.copy() for k, v in cand.items()}
    other["guided"][1, 40:] += 0.01
    other["logits"][1, 40:] = 9.0
    other["labels"][1, 40:] ^= 1
    assert BC.same_bits(_fuse(other, det, 0.55), want)
    d2 = {k: v.copy() for k, v in det.items()}
    d2["boxes"][1, 4:] = 7.0
    got = _fuse(cand, d2, 0.55)
    assert BC.same_bits(got[1, :4], want[1, :4]) and (got[1, 4:] == 7.0).all()


# ---- 2: properties ----------------------------------------------------------------------------------------------------------
BOX = np.array([12.5, -3.25, -1.1, 1.62, 3.93, 1.54, 0.7], np.float32)


def _one(boxes, logits, labels, det_box, det_label=0, fuse_iou=0.7, lib=None, count=None):
    """One sample, one detection `det_box`; returns (fuse_host, harness) results for that row."""
    g = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(1, -1, 7))
    n = g.shape[1]
    cand = dict(guided=g, logits=np.asarray(logits, np.float32).reshape(1, n), labels=np.asarray(labels, np.int32).reshape(1, n),
                counts=np.array([n if count is None else count], np.int32))
    det = dict(boxes=np.asarray(det_box, np.float32).reshape(1, 1, 7).copy(), labels=np.array([[det_label]], np.int32),
               counts=np.array([1], np.int32))
    got = _fuse(cand, det, fuse_iou)
    if lib is not None:
        mats = BC.iou_matrices(cand, det, clib.boxes_iou_bev)
        h = BC.harness_fuse(lib, cand, F.sigmoid_host(cand["logits"]), det, BC.SCORE_THR, fuse_iou, mats)
        assert BC.same_bits(got, h)
    return got[0, 0]


def test_a_lone_detection_is_unchanged_bit_for_bit(lib):
    rng = np.random.default_rng(0)
    for i in range(200):                # by arithmetic, not by a special case: (s * f) / s == f, delta == 0
        box = (BOX + rng.standard_normal(7) * [20, 20, 1, 0.2, 0.4, 0.2, 3]).astype(np.float32)
        box[3:6] = np.abs(box[3:6]) + np.float32(0.1)
        if i == 0:
            box[2] = np.float32(-0.0)   # a -0.0 field stays -0.0 (the sum of one term is the term)
        logit = np.float32(rng.uniform(-0.8, 6.0))
        got = _one([box], [logit], [1], box, det_label=1, lib=lib if i < 20 else None)
        assert BC.same_bits(got, box), (i, got, box)


@pytest.mark.parametrize("turn", [np.pi, -np.pi, 2 * np.pi, -4 * np.pi, 6 * np.pi, 3 * np.pi])
def test_a_turned_copy_does_not_drag_the_heading(lib, turn):
    other = BOX.copy()
    other[6] = np.float32(np.float64(BOX[6]) + turn)
    got = _one([BOX, other], [2.0, 1.0], [0, 0], BOX, lib=lib)
    assert BC.same_bits(got[:6], BOX[:6])
    # float32(yaw + turn) is not yaw + turn: the offset that remains is that rounding (half a float32 spacing of the turned
    # yaw), weighted by s_2 / W < 1/2
    assert abs(float(got[6]) - float(BOX[6])) <= 0.5 * np.spacing(np.float32(abs(other[6])))
    # and a heading that does differ pulls, from either side of the half turn
    for d in (0.04, -0.04):
        o2 = other.copy()
        o2[6] = np.float32(np.float64(other[6]) + d)
        pulled = float(_one([BOX, o2], [2.0, 1.0], [0, 0], BOX, lib=lib)[6]) - float(BOX[6])
        assert 0.2 * abs(d) < pulled * np.sign(d) < 0.5 * abs(d), (d, pulled)


def test_another_label_or_a_low_score_is_never_a_member(lib):
    near = BOX.copy()
    near[:2] += np.float32(0.05)
    thr_logit = float(np.log(BC.SCORE_THR / (1 - BC.SCORE_THR)))
    assert BC.same_bits(_one([BOX, near], [2.0, 3.0], [0, 1], BOX, lib=lib), BOX)              # another label
    assert BC.same_bits(_one([BOX, near], [2.0, thr_logit - 0.01], [0, 0], BOX, lib=lib), BOX)  # a score below the threshold
    s = F.sigmoid_host(np.float32(1.0))                                                         # a score EQUAL to it: '>' fails
    got = F.fuse_host(dict(guided=np.stack([BOX, near])[None], scores=np.array([[0.9, s]], np.float32),
                           labels=np.zeros((1, 2), np.int32), counts=[2]),
                      dict(boxes=BOX.reshape(1, 1, 7), labels=np.zeros((1, 1), np.int32), counts=[1]), float(s), 0.7,
                      clib.boxes_iou_bev)
    assert BC.same_bits(got[0, 0], BOX)
    moved = _one([BOX, near], [2.0, 3.0], [0, 0], BOX, lib=lib)                                 # the control: it does move
    assert BOX[0] < moved[0] < near[0] and BOX[1] < moved[1] < near[1]


def test_a_nan_candidate_is_ignored(lib):
    for field in (0, 1, 3, 4, 6):
        bad = BOX.copy()
        bad[field] = np.nan
        assert BC.same_bits(_one([BOX, bad], [2.0, 3.0], [0, 0], BOX, lib=lib), BOX), field
    assert BC.same_bits(_one([BOX, BOX], [2.0, np.nan], [0, 0], BOX, lib=lib), BOX)             # a NaN score
    nan_iou = np.array([[1.0, np.nan]], np.float32)                                             # a NaN IoU, whatever made it
    got = F.fuse_host(dict(guided=np.stack([BOX, BOX + np.float32(0.01)])[None], logits=np.array([[2.0, 3.0]], np.float32),
                           labels=np.zeros((1, 2), np.int32), counts=[2]),
                      dict(boxes=BOX.reshape(1, 1, 7), labels=np.zeros((1, 1), np.int32), counts=[1]), BC.SCORE_THR, 0.7, [nan_iou])
    assert BC.same_bits(got[0, 0], BOX)


def test_a_zero_size_detection_is_returned_as_it_is(lib):
    flat = BOX.copy()
    flat[3:5] = 0
    near = BOX.copy()
    assert BC.same_bits(_one([flat, near], [2.0, 3.0], [0, 0], flat, lib=lib), flat)
    # no member at all (the detection is not among the candidates), and W not positive (scores of zero pass a negative threshold)
    assert BC.same_bits(_one([near], [2.0], [1], BOX, det_label=0, lib=lib), BOX)
    got = F.fuse_host(dict(guided=np.stack([BOX, near])[None], scores=np.zeros((1, 2), np.float32), labels=np.zeros((1, 2), np.int32),
                           counts=[2]),
                      dict(boxes=BOX.reshape(1, 1, 7), labels=np.zeros((1, 1), np.int32), counts=[1]), -1.0, 0.7, clib.boxes_iou_bev)
    assert BC.same_bits(got[0, 0], BOX)


# ---- 3: errors --------------------------------------------------------------------------------------------------------------
def test_check_fuse_iou():
    assert F.check_fuse_iou(None) is None
    assert F.check_fuse_iou(0.7) == 0.7 and F.check_fuse_iou(np.float32(0.5)) == 0.5 and isinstance(F.check_fuse_iou(np.float32(0.5)), float)
    for bad in (0, 1, 0.0, 1.0, -0.1, 1.5, float("nan"), float("inf"), True, "0.7", [0.7], 1.0 - 1e-12, 1e-60):
        with pytest.raises(ValueError, match="fuse_iou"):
            F.check_fuse_iou(bad)
    from sassd.pipeline import InferencePlan
    from sassd.stream import FrameStream
    with pytest.raises(ValueError, match="fuse_iou"):                   # before anything is looked at or allocated
        InferencePlan({}, fuse_iou=1.0)
    with pytest.raises(ValueError, match="fuse_iou"):
        FrameStream({}, fuse_iou=0.0)


def _args(b=1, cap_k=4, cap_d=2):
    det = dict(boxes=torch.zeros(b, cap_d, 7), scores=torch.zeros(b, cap_d), labels=torch.zeros(b, cap_d, dtype=torch.int32),
               counts=torch.zeros(b, dtype=torch.int32))
    return [torch.zeros(b, cap_k, 7), torch.zeros(b, cap_k), torch.zeros(b, cap_k, dtype=torch.int32),
            torch.zeros(b, dtype=torch.int32), 0.3, 0.7, det]


def test_kernels_box_fuse_argument_errors():
    def bad(i, v, match, **kw):
        a = _args()
        if isinstance(i, str):
            a[6][i] = v
        else:
            a[i] = v
        with pytest.raises(ValueError, match=match):
            K.box_fuse(*a, **kw)
    bad(5, None, "fuse_iou")
    bad(5, 1.0, "fuse_iou")
    bad(5, float("nan"), "fuse_iou")
    bad(0, torch.zeros(1, 4, 6), "guided")
    bad(0, torch.zeros(1, 4097, 7), "capK")
    bad(0, torch.zeros(1, 4, 7, dtype=torch.float64), "guided")
    bad(1, torch.zeros(1, 5), "logits")
    bad(2, torch.zeros(1, 4, dtype=torch.int64), "labels")
    bad(3, torch.zeros(2, dtype=torch.int32), "counts")
    bad("boxes", torch.zeros(2, 2, 7), "boxes")
    bad("labels", torch.zeros(1, 2), "labels")
    bad("counts", torch.zeros(1, dtype=torch.int64), "counts")
    bad(0, torch.zeros(1, 4, 7), "out", out=torch.zeros(1, 3, 7))
    a = _args()
    with pytest.raises(ValueError, match="in place"):
        K.box_fuse(*a, out=a[6]["boxes"])


def test_c_abi_refuses_bad_arguments_before_any_hip_call():
    L = _C.lib()
    EINVAL = -1                                                         # SASSD_EINVAL
    n = ctypes.c_void_p(None)
    assert L.sassd_box_fuse(n, n, n, n, 1, 4, 0.3, 0.7, n, n, n, 2, n, n) == EINVAL
    bufs = [np.zeros(64, np.float32) for _ in range(8)]
    g, lo, la, c, db, dl, dc, out = (b.ctypes.data for b in bufs)       # host memory: every call below must return before a launch

    def call(guided=g, logits=lo, labels=la, counts=c, batch=1, cap_k=4, thr=0.3, fuse=0.7, boxes=db, dlabels=dl, dcounts=dc,
             cap_d=2, fused=out):
        return L.sassd_box_fuse(guided, logits, labels, counts, batch, cap_k, thr, fuse, boxes, dlabels, dcounts, cap_d, fused, n)
    assert call(guided=None) == call(fused=None) == call(dcounts=None) == call(logits=None) == EINVAL
    assert call(guided=g + 2) == EINVAL and call(fused=out + 1) == EINVAL
    assert call(batch=0) == EINVAL and call(cap_k=0) == EINVAL and call(cap_d=0) == EINVAL and call(cap_k=4097) == EINVAL
    for f in (0.0, 1.0, -0.5, 2.0, float("nan"), float("inf")):
        assert call(fuse=f) == EINVAL, f
    assert call(fused=db) == EINVAL and call(fused=db + 28) == EINVAL   # fused is, or overlaps, det_boxes
    assert L.sassd_candidate_scores(n, 4, n, n) == EINVAL


# ---- 4: the switch on the public entries ----------------------------------------------------------------------------------
def test_detector_frame_stream_reads_test_cfg_and_an_explicit_keyword_overrides_it(monkeypatch):
    from sassd import stream as S, synth
    model, _ = synth.build_detector_for(synth.workload("car"), 0)
    seen = {}
    monkeypatch.setattr(S, "FrameStream", lambda sd, **kw: (seen.clear(), seen.update(kw)) and "fs")
    an = synth.workload("car")["anchors"]
    model.test_cfg.pop("fuse_iou", None)
    model.frame_stream(an, points_cap=1000)
    assert "fuse_iou" not in seen                                       # off: the call made before
    model.frame_stream(an, points_cap=1000, fuse_iou=0.6)
    assert seen["fuse_iou"] == 0.6
    model.test_cfg["fuse_iou"] = 0.7
    model.frame_stream(an, points_cap=1000)
    assert seen["fuse_iou"] == 0.7
    model.frame_stream(an, points_cap=1000, fuse_iou=None)              # an explicit None is off
    assert "fuse_iou" not in seen
    model.frame_stream(an, points_cap=1000, fuse_iou=0.55)
    assert seen["fuse_iou"] == 0.55


def test_single_test_needs_a_stream_for_fuse_iou():
    import test_runner_cpu as TR
    from sassd import runner as R
    with pytest.raises(ValueError, match="fuse_iou needs inflight"):
        R.single_test(TR._Model(), TR._DS(2), rank=0, world=1, fuse_iou=0.7)
