"""Cases shared by the box fusion tests (tests/test_box_fuse_cpu.py, tests/test_gpu_box_fuse_kernel.py): seeded clusters of
jittered candidates around well-separated objects, the CPU harness over csrc/box_fuse_core.h (tests/box_fuse_harness.hip),
and a host NMS that produces detections without a GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from sassd import fuse as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

SCORE_THR, IOU_THR = 0.3, 0.1
FUSE_IOUS = (0.55, 0.7)
MARGIN = 1e-3               # no (detection, candidate) IoU may lie this close to fuse_iou: 100 x the 1e-5 bar GPU IoU / oracle
JITTER = ((0.04, 0.01, 0.01), (0.08, 0.025, 0.02), (0.16, 0.05, 0.03))       # (centre m, yaw rad, relative size): three levels


def cluster_sample(rng, K, n_obj, cap_k, low=False):
    """One sample's candidate buffers, every one of the cap_k rows filled: rows < K are candidates of n_obj objects (row i
    belongs to object perm[i] % n_obj, so an object's members are spread over the 64-row chunks), the rows behind are copies
    of leading rows with a high logit, so that a row read from beyond the count would show.  Objects stand 9 m apart; an
    object has a label 0 / 1, one candidate in seven carries the other label, one in five is turned by pi, one in five by a
    multiple of 2 pi.  Logits are distinct and stay away from the score threshold, so that the device's and numpy's sigmoid
    order and threshold them alike.  `low`: every logit below the threshold (a sample without detections)."""
    g = np.zeros((cap_k, 7), np.float32)
    lo = np.zeros(cap_k, np.float32)
    la = np.zeros(cap_k, np.int32)
    if K:
        centres = np.array([[9.0 * (o % 6) + 5.0, 9.0 * (o // 6) - 20.0] for o in range(n_obj)])
        yaw0 = rng.uniform(-np.pi, np.pi, n_obj)
        lab0 = rng.integers(0, 2, n_obj)
        obj = rng.permutation(K) % n_obj
        for i in range(K):
            o = obj[i]
            jc, jy, js = JITTER[int(rng.integers(0, 3))]
            size = np.array([1.6, 3.9, 1.56]) * (1.0 + js * rng.standard_normal(3))
            yaw = yaw0[o] + jy * rng.standard_normal()
            u = rng.random()
            if u < 0.2:
                yaw += np.pi
            elif u < 0.4:
                yaw += 2.0 * np.pi * int(rng.integers(-2, 3))
            g[i] = [centres[o, 0] + jc * rng.standard_normal(), centres[o, 1] + jc * rng.standard_normal(),
                    -1.0 + 0.05 * rng.standard_normal(), size[0], size[1], size[2], yaw]
            la[i] = lab0[o] ^ int(rng.random() < 1.0 / 7.0)
        grid = np.linspace(-3.0, -1.2, K) if low else np.linspace(-1.6, 3.0, K) if K > 1 else np.array([1.0])
        thr_logit = np.log(SCORE_THR / (1.0 - SCORE_THR))
        grid = np.where(np.abs(grid - thr_logit) < 0.01, thr_logit + 0.02, grid)
        lo[:K] = rng.permutation(grid).astype(np.float32)
    for i in range(K, cap_k):           # what must not be read
        src = (i - K) % max(K, 1)
        g[i], la[i], lo[i] = (g[src], la[src], 4.0) if K else ([5.0, -20.0, -1.0, 1.6, 3.9, 1.56, 0.3], 0, 4.0)
    return g, lo, la


def batch(seed, cap_k, samples, counts=None):
    """dict(guided [B, cap_k, 7], logits, labels, counts [B]) of samples [(K, n_obj) or (K, n_obj, low)]; `counts` replaces the
    counts handed to the kernels (above cap_k: clamped)."""
    rng = np.random.default_rng(seed)
    rows = [cluster_sample(rng, s[0], s[1], cap_k, low=len(s) > 2 and s[2]) for s in samples]
    return dict(guided=np.ascontiguousarray(np.stack([r[0] for r in rows])), logits=np.ascontiguousarray(np.stack([r[1] for r in rows])),
                labels=np.ascontiguousarray(np.stack([r[2] for r in rows])),
                counts=np.asarray([s[0] for s in samples] if counts is None else counts, np.int32))


# (name, seed, cap_k, cap_d, samples, counts handed over, detection counts expected).  The seeds were chosen on the CPU
# (oracle IoU, nms_host) so that both FUSE_IOUS clear MARGIN; test_gpu_box_fuse_kernel.py asserts that on the CPU matrix.
CASES = (
    ("k1_k63", 3, 64, 8, ((1, 1), (63, 4)), None, (1, 4)),                         # K = 1 and 63, D = 1 and 4
    ("k64_k65", 6, 65, 8, ((64, 5), (65, 7)), None, (5, 7)),                       # K = 64 and 65, D = 5 (a second workgroup)
    ("k257_empty", 7, 257, 28, ((257, 28), (0, 0)), None, (28, 0)),                # five chunks, D = capD; no candidate at all
    ("nodet_capd", 5, 64, 4, ((20, 3, True), (63, 4)), None, (0, 4)),              # candidates but no detection; D = capD
    ("clamped", 0, 64, 8, ((64, 5), (40, 4)), (100, 40), (5, 4)),                  # a count above capK is clamped
)


def nms_host(cand, cap_d, iou_bev, scores=None):
    """rescore / NMS on the host: scores (numpy's sigmoid unless given) > SCORE_THR, stable descending sort, greedy rotated
    NMS at IOU_THR over all labels -> dict(boxes [B, cap_d, 7], scores, labels, counts).  `iou_bev(a [n, 5], b [m, 5])`."""
    g, la = cand["guided"], cand["labels"]
    B, cap_k = g.shape[:2]
    sc = F.sigmoid_host(cand["logits"]) if scores is None else scores
    det = dict(boxes=np.zeros((B, cap_d, 7), np.float32), scores=np.zeros((B, cap_d), np.float32),
               labels=np.zeros((B, cap_d), np.int32), counts=np.zeros(B, np.int32))
    for b in range(B):
        K = int(min(max(int(cand["counts"][b]), 0), cap_k))
        sel = np.flatnonzero(sc[b, :K] > np.float32(SCORE_THR))
        order = sel[np.argsort(-sc[b, sel], kind="stable")]
        keep = []
        if len(order):
            m = iou_bev(F.bev(g[b, order]), F.bev(g[b, order]))
            dead = np.zeros(len(order), bool)
            for i in range(len(order)):
                if not dead[i]:
                    keep.append(order[i])
                    dead |= (m[i] > np.float32(IOU_THR)) & (np.arange(len(order)) > i)
        keep = np.asarray(keep[:cap_d], np.int64)
        n = len(keep)
        det["boxes"][b, :n], det["scores"][b, :n], det["labels"][b, :n], det["counts"][b] = g[b, keep], sc[b, keep], la[b, keep], n
    return det


def iou_matrices(cand, det, iou_bev):
    """Per sample the [D, K] matrix iou_bev(bev(detections), bev(candidates)) -- the detection first."""
    out = []
    for b in range(cand["guided"].shape[0]):
        K = int(min(max(int(cand["counts"][b]), 0), cand["guided"].shape[1]))
        D = int(det["counts"][b])
        out.append(iou_bev(F.bev(det["boxes"][b, :D]), F.bev(cand["guided"][b, :K])) if D and K else np.zeros((D, K), np.float32))
    return out


def margin(mats, fuse_iou):
    """The smallest |IoU - fuse_iou| over all (detection, candidate) pairs."""
    return min([float(np.abs(m.astype(np.float64) - fuse_iou).min()) for m in mats if m.size] or [1.0])


def members(cand, det, mats, scores, fuse_iou):
    """Member counts per detection, per sample (is_member of csrc/box_fuse_core.h)."""
    out = []
    for b, m in enumerate(mats):
        D, K = m.shape
        ok = (scores[b, :K] > np.float32(SCORE_THR))[None] & (cand["labels"][b, :K][None] == det["labels"][b, :D][:, None])
        out.append((ok & (m >= np.float32(fuse_iou))).sum(1))
    return out


_harness = None


def harness(tmp_dir):
    """The CPU harness over box_fuse_core.h, compiled once per process into `tmp_dir` (hipcc --cuda-host-only)."""
    global _harness
    if _harness is None:
        dst = os.path.join(str(tmp_dir), "libbox_fuse_harness.so")
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-fno-fast-math", "-ffp-contract=on", "-shared",
                               "-fPIC", "-o", dst, os.path.join(ROOT, "tests", "box_fuse_harness.hip")])
        _harness = C.CDLL(dst)
        _harness.hst_box_fuse.restype = None
        _harness.hst_box_fuse.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return _harness


def harness_fuse(lib, cand, scores, det, score_thr, fuse_iou, mats):
    """fuse_host through the harness: the header's functions, one detection after the other."""
    out = det["boxes"].copy()
    for b, m in enumerate(mats):
        D, K = m.shape
        if D == 0:
            continue
        g, s, la = (np.ascontiguousarray(x[b, :K]) for x in (cand["guided"], scores, cand["labels"]))
        db, dl = np.ascontiguousarray(det["boxes"][b, :D]), np.ascontiguousarray(det["labels"][b, :D])
        m = np.ascontiguousarray(m, np.float32)
        fused = np.zeros((D, 7), np.float32)
        lib.hst_box_fuse(g.ctypes.data, s.ctypes.data, la.ctypes.data, K, score_thr, fuse_iou, db.ctypes.data, dl.ctypes.data, D,
                         m.ctypes.data, fused.ctypes.data)
        out[b, :D] = fused
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
