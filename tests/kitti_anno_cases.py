"""Inputs, screening and bars shared by test_kitti_anno_cpu.py and test_gpu_kitti_anno.py: seeded lidar boxes, the host
quantities of kitti_common.kitti_bbox2results, the candidates whose decisions sit on a threshold, and the comparison of
one sample's device annotation (decode_record's `cam`) with kitti_bbox2results on the same boxes.

Bars (a device annotation against the host function on the same boxes):
  index, dimensions, score   equal
  location                   within one float32 spacing (float64 sums in another order, rounded once)
  rotation_y, alpha          1e-5 rad: a few float32 ulps of atan2f and of the wrap at |yaw| <= 9.5
  bbox                       5e-3 px: a 4-ulp float32 difference in a corner coordinate at depth >= 2 m moves a projected
                             pixel by < 2e-3 px; the only sources are float32 sin / cos and rounding order
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import augment_synth as AS
from sassd import kitti_common as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
IMG_SHAPE = (375, 1242)
N_CAND = 300
ANGLE_BAR, BBOX_BAR = 1e-5, 5e-3
CLASS_NAMES = ["Car", "Pedestrian", "Cyclist"]


def calibration():
    return kc.Calibration(matrices=AS.calib_matrices())


def calib_block(img_shape=IMG_SHAPE):
    from sassd.stream import calib_block_of
    return calib_block_of(calibration(), img_shape)


def meta(sample_idx=0, img_shape=IMG_SHAPE):
    return dict(calib=calibration(), sample_idx=sample_idx, img_shape=img_shape)


def candidates(seed, n=N_CAND):
    """[n,7] float32 lidar boxes (x, y, z, w, l, h, yaw), drawn in this order from default_rng(seed)."""
    r = np.random.default_rng(seed)
    cols = [r.uniform(lo, hi, n) for lo, hi in ((4, 70), (-40, 40), (-2.5, -0.5), (0.5, 2.2), (0.6, 5.0), (1.2, 2.0),
                                                (-9.5, 9.5))]
    return np.stack(cols, 1).astype(np.float32)


def host_quantities(boxes):
    """What kitti_bbox2results computes on the way, with kitti_common's own functions: the wrapped yaw, the unclipped 2-D
    boxes [n,4] float64, the smallest corner depth [n], and keep [n]."""
    calib = calibration()
    img_h, img_w = IMG_SHAPE
    b = boxes.copy()
    b[:, -1] = kc.limit_period(b[:, -1], offset=0.5, period=np.pi * 2)
    cam = np.zeros_like(b)
    cam[:, :3] = kc.project_velo_to_rect(b[:, :3], calib)
    cam[:, 3:] = b[:, [4, 5, 3, 6]]
    corners = kc._camera_box_corners(cam)
    uv = kc.project_rect_to_image(corners, calib)
    box2d = np.concatenate([uv.min(axis=1), uv.max(axis=1)], axis=1)
    keep = ~((box2d[:, 0] > img_w) | (box2d[:, 1] > img_h) | (box2d[:, 2] < 0) | (box2d[:, 3] < 0))
    return dict(yaw=b[:, -1], box2d=box2d, depth=corners[..., 2].min(axis=1), keep=keep)


def screened(seed):
    """-> dict(boxes [m,7] f32 (the candidates that stay), left_out, kept, clipped, dropped -- boolean masks over `boxes`).
    A candidate is left out where a decision sits on a threshold: the smallest corner depth is < 2 m, a keep or clip
    comparand is within 1 px of its threshold, or yaw is within 1e-2 rad of an odd multiple of pi."""
    boxes = candidates(seed)
    q = host_quantities(boxes)
    img_h, img_w = IMG_SHAPE
    bd = q["box2d"]
    near = np.zeros(len(boxes), bool)
    for col, lim in ((0, img_w), (1, img_h), (2, img_w), (3, img_h)):
        near |= (np.abs(bd[:, col] - lim) <= 1.0) | (np.abs(bd[:, col]) <= 1.0)
    yaw = boxes[:, 6].astype(np.float64)
    near_wrap = np.abs(np.mod(yaw, 2 * np.pi) - np.pi) <= 1e-2    # each period [2k pi, 2(k+1) pi) holds one odd multiple
    out = (q["depth"] < 2.0) | near | near_wrap
    ok = ~out
    bd, keep = bd[ok], q["keep"][ok]
    clipped = keep & ((bd[:, 0] < 0) | (bd[:, 1] < 0) | (bd[:, 2] > img_w) | (bd[:, 3] > img_h))
    return dict(boxes=boxes[ok], left_out=int(out.sum()), kept=keep, clipped=clipped, dropped=~keep)


_harness = None


def harness(tmp_dir):
    """The CPU harness over kitti_anno_core.h, compiled once per process into `tmp_dir` (hipcc --cuda-host-only)."""
    global _harness
    if _harness is None:
        dst = os.path.join(str(tmp_dir), "libkitti_anno_harness.so")
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-fno-fast-math", "-ffp-contract=on", "-shared",
                               "-fPIC", "-o", dst, os.path.join(ROOT, "tests", "kitti_anno_harness.hip")])
        _harness = C.CDLL(dst)
        _harness.hst_box_annos.restype = None
        _harness.hst_box_annos.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
    return _harness


def harness_cam(lib, boxes, block):
    """The harness on `boxes` -> the `cam` dict decode_record(annos=True) returns for them."""
    n = len(boxes)
    boxes = np.ascontiguousarray(boxes, np.float32)
    block = np.ascontiguousarray(block, np.float64)
    cam, alpha = np.zeros((n, 7), np.float32), np.zeros(n, np.float32)
    bbox, keep = np.zeros((n, 4), np.float64), np.zeros(n, np.uint8)
    lib.hst_box_annos(boxes.ctypes.data, n, block.ctypes.data, cam.ctypes.data, alpha.ctypes.data, bbox.ctypes.data,
                      keep.ctypes.data)
    idx = np.flatnonzero(keep).astype(np.int64)
    return dict(index=idx, location=cam[idx, :3], dimensions=cam[idx, 3:6], rotation_y=cam[idx, 6], alpha=alpha[idx],
                bbox=bbox[idx])


def compare_annos(got, want, maxima=None):
    """Assert the bars between two result annotations of one frame (`want`: kitti_bbox2results).  `maxima` (a dict)
    collects the largest differences seen.  -> the number of annotation rows."""
    k = len(want["name"])
    assert len(got["name"]) == k, "kept %d rows, the host keeps %d" % (len(got["name"]), k)
    assert set(got) == set(want)
    if k == 0:
        return 0
    assert np.array_equal(got["score"], want["score"]) and np.array_equal(got["name"], want["name"])
    assert np.array_equal(got["dimensions"], want["dimensions"])
    assert np.array_equal(got["image_idx"], want["image_idx"])
    d_loc = np.abs(got["location"].astype(np.float64) - want["location"]) / np.spacing(np.abs(want["location"]))
    d_ry = np.abs(got["rotation_y"].astype(np.float64) - want["rotation_y"])
    d_al = np.abs(got["alpha"].astype(np.float64) - want["alpha"])
    d_bb = np.abs(got["bbox"] - want["bbox"])
    if maxima is not None:
        for key, v in (("location_ulp", d_loc), ("rotation_y", d_ry), ("alpha", d_al), ("bbox_px", d_bb)):
            maxima[key] = max(maxima.get(key, 0.0), float(v.max()))
    assert d_loc.max() <= 1.0, "location differs by %.2f float32 spacings" % d_loc.max()
    assert d_ry.max() <= ANGLE_BAR and d_al.max() <= ANGLE_BAR, (d_ry.max(), d_al.max())
    assert d_bb.max() <= BBOX_BAR, "bbox differs by %.3g px" % d_bb.max()
    for key in want:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
    return k


def compare(cam, boxes, scores, labels, img_shape=IMG_SHAPE, calib=None, maxima=None):
    """Assert the bars for one sample: `cam` (decode_record's, or the harness's) against kitti_bbox2results on copies of
    the same boxes / scores / labels, and that `index` names the rows the host keeps, in order.  -> the number of rows."""
    m = dict(calib=calib if calib is not None else calibration(), sample_idx=7, img_shape=img_shape)
    want = kc.kitti_bbox2results(boxes.copy(), scores.copy(), labels.copy(), m, class_names=CLASS_NAMES)
    got = kc.result_anno_from_cam(cam, scores, labels, 7, CLASS_NAMES)
    k = compare_annos(got, want, maxima)
    assert len(cam["index"]) == k
    if k:
        assert np.all(np.diff(cam["index"]) > 0), "annotation rows are not in detection order"
        # the host's own dimensions and score are those of the rows `index` names
        assert np.array_equal(np.asarray(scores)[cam["index"]], want["score"])
        assert np.array_equal(boxes[cam["index"]][:, [4, 5, 3]], want["dimensions"])
    return k
