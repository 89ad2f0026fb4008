"""Box fusion: the switch, and the numpy statement of the rule (include/sassd.h "Box fusion"; csrc/box_fuse_core.h).

InferencePlan(fuse_iou=t) / FrameStream(fuse_iou=t) / test_cfg['fuse_iou'] launch sassd_box_fuse behind rescore / NMS: every
detection becomes the score-weighted mean of the candidates of its label whose rotated BEV IoU with it is at least `t` -- its
own box and the overlapping ones NMS dropped; under test-time augmentation, the boxes of all views.  Scores, labels, counts
and the order of the detections stay; only boxes move.  `fuse_host` states what the kernel computes, float64 operation by
float64 operation in ascending candidate row; the tests hold the kernel to it bit for bit.  The two device functions the rule
rests on are inputs of the statement: the IoU matrix, and (optionally) the candidates' scores."""
import numpy as np

MAX_CANDIDATES = 4096               # the most candidates per sample sassd_rescore_nms and sassd_box_fuse take


def check_fuse_iou(fuse_iou):
    """The switch as a float strictly inside (0, 1) -- what float32 makes of it included -- or None (off).  ValueError for
    anything else: a bool, a string, a NaN, 0, 1."""
    if fuse_iou is None:
        return None
    if isinstance(fuse_iou, (bool, np.bool_, str, bytes)):
        raise ValueError("fuse_iou must be a number inside (0, 1) or None, got %r" % (fuse_iou,))
    try:
        t = float(fuse_iou)
    except (TypeError, ValueError):
        raise ValueError("fuse_iou must be a number inside (0, 1) or None, got %r" % (fuse_iou,)) from None
    if not (np.isfinite(t) and 0.0 < float(np.float32(t)) < 1.0):
        raise ValueError("fuse_iou must lie strictly inside (0, 1), got %r" % (fuse_iou,))
    return t


def bev(boxes):
    """(x - w/2, y - l/2, x + w/2, y + l/2, yaw) of boxes [n, 7] f32, float32 operation by operation: the BEV boxes
    sassd_rescore_nms and sassd_box_fuse hand to the rotated IoU."""
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 7)
    with np.errstate(invalid="ignore", over="ignore"):
        hx, hy = b[:, 3] / np.float32(2), b[:, 4] / np.float32(2)
        return np.ascontiguousarray(np.stack([b[:, 0] - hx, b[:, 1] - hy, b[:, 0] + hx, b[:, 1] + hy, b[:, 6]], 1), np.float32)


def sigmoid_host(logits):
    """1 / (1 + exp(-x)) in float32.  The device's expf is not numpy's to the last bit: a caller that compares bits hands
    fuse_host the device's scores (kernels.candidate_scores) instead."""
    x = np.asarray(logits, np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)


def fuse_host(cand, det, score_thr, fuse_iou, iou):
    """The fused boxes [B, capD, 7] f32 of sassd_box_fuse.

    cand: dict(guided [B, capK, 7] f32, labels [B, capK] i32, counts [B], and scores [B, capK] f32 -- or logits [B, capK] f32,
    whose scores are sigmoid_host's) -- the candidate list handed to rescore / NMS.  det: dict(boxes [B, capD, 7] f32, labels
    [B, capD] i32, counts [B]) -- what it left behind.  iou: per sample b a [D_b, K_b] float32 matrix of the rotated BEV IoU of
    detection row t < D_b = clamp(det counts) and candidate row j < K_b = clamp(counts) (a list of B matrices, or one [B, >= D,
    >= K] array), or a callable (bev(detections) [D, 5], bev(candidates) [K, 5]) -> that matrix.  Rows at and past the
    detection count are returned as `det` has them (the kernel does not write them)."""
    fuse_iou = np.float32(check_fuse_iou(fuse_iou))
    score_thr = np.float32(score_thr)
    guided = np.ascontiguousarray(cand["guided"], dtype=np.float32)
    labels = np.asarray(cand["labels"])
    boxes = np.ascontiguousarray(det["boxes"], dtype=np.float32)
    dlabels = np.asarray(det["labels"])
    if guided.ndim != 3 or guided.shape[2] != 7 or boxes.ndim != 3 or boxes.shape[2] != 7 or boxes.shape[0] != guided.shape[0]:
        raise ValueError("guided must be [B, capK, 7] and boxes [B, capD, 7], got %s and %s" % (guided.shape, boxes.shape))
    B, capK, capD = guided.shape[0], guided.shape[1], boxes.shape[1]
    scores = cand.get("scores")
    scores = sigmoid_host(cand["logits"]) if scores is None else np.asarray(scores, np.float32)
    counts = np.asarray(cand["counts"], np.int64).reshape(B)
    dcounts = np.asarray(det["counts"], np.int64).reshape(B)
    fused = boxes.copy()
    pi = np.float64(np.pi)
    for b in range(B):
        K, D = int(min(max(counts[b], 0), capK)), int(min(max(dcounts[b], 0), capD))
        if D == 0:
            continue
        if callable(iou):
            m = iou(bev(boxes[b, :D]), bev(guided[b, :K])) if K else np.zeros((D, 0), np.float32)
        else:
            m = iou[b]
        m = np.asarray(m, np.float32)[:D, :K]
        if m.shape != (D, K):
            raise ValueError("sample %d: the IoU matrix must cover %d detections x %d candidates, got %s" % (b, D, K, m.shape))
        s = scores[b, :K]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for t in range(D):
                member = (s > score_thr) & (labels[b, :K] == dlabels[b, t]) & (m[t] >= fuse_iou)      # NaN compares false
                yaw_d = np.float64(boxes[b, t, 6])
                sums = None                             # W, F_x .. F_h, D: float64, ascending j, the sum of one term is the term
                for j in np.flatnonzero(member):
                    sj = np.float64(s[j])
                    d = np.float64(guided[b, j, 6]) - yaw_d
                    delta = d - pi * np.floor(d / pi + np.float64(0.5))
                    terms = [sj] + [sj * np.float64(guided[b, j, q]) for q in range(6)] + [sj * delta]
                    sums = terms if sums is None else [a + x for a, x in zip(sums, terms)]
                if sums is None or not (sums[0] > 0 and np.isfinite(sums[0])):
                    continue                            # the detection as it is, bit for bit
                for q in range(6):
                    fused[b, t, q] = np.float32(sums[1 + q] / sums[0])
                fused[b, t, 6] = np.float32(yaw_d + sums[7] / sums[0])
    return fused
