"""Cases shared by the test-time augmentation tests (tests/test_tta_cpu.py, tests/test_gpu_tta_kernels.py, tests/test_gpu_tta.py):
view specs, clouds with the bit patterns that arithmetic would destroy, candidate buffers with the counts the issue names,
and the CPU harness over the shared __host__ __device__ headers (tests/tta_harness.hip)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from sassd import tta as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

ID = (0, 0.0, 1.0)
V1 = [ID]
V2 = [ID, (1, 0.0, 1.0)]                                            # identity + flip
V3 = [ID, (1, 0.0, 1.0), (1, -0.3, 1.05)]                           # ... + flip, rotate and scale in one view
V4 = [ID, (1, 0.0, 1.0), (0, np.pi / 8, 1.0), (0, -np.pi / 8, 1.0)]  # identity + flip + rotations of +-pi/8
V4_MIXED = [ID, (1, 0.0, 1.0), (0, np.pi / 8, 1.0), (1, -0.37, 0.95)]   # the last view flips, rotates and scales

NAN_PAYLOAD, NEG_ZERO, INF = 0x7FC00123, 0x80000000, 0x7F800000


def cloud(n, ndim, seed):
    """[n, ndim] f32 with -0.0 in x, y, z, Inf in z and in a feature, a NaN payload in a feature (ndim > 3).  No Inf or NaN in
    x / y: Inf * 0 would make a NaN whose sign and payload the host and the device are free to choose."""
    r = np.random.default_rng(seed)
    p = np.ascontiguousarray(r.standard_normal((n, ndim)) * ([20.0, 15.0, 1.0] + [1.0] * (ndim - 3)), np.float32)
    u = p.view(np.uint32)
    if n >= 1:
        u[0, :3] = NEG_ZERO
    if n >= 2:
        u[1, 2] = INF
    if n >= 3 and ndim > 3:
        u[2, 3] = NAN_PAYLOAD
        u[n - 1, ndim - 1] = INF | 0x80000000
    return p


def candidates(b, V, capK, counts, seed):
    """The inner-batch candidate buffers of a frame: guided [b V, capK, 7], logits, labels, and the given counts [b V] (which
    may exceed capK: the kernel clamps).  Every row is filled, so that a row copied from beyond a count shows."""
    r = np.random.default_rng(seed)
    g = (r.standard_normal((b * V, capK, 7)) * [20, 15, 1, 0.3, 0.6, 0.2, 1.5] + [35, 0, -1, 1.6, 3.9, 1.56, 0]).astype(np.float32)
    g.view(np.uint32)[0, 0, 2] = NAN_PAYLOAD                         # the identity view's boxes are copied as bits
    g.view(np.uint32)[0, 1, 1] = NEG_ZERO
    lo = r.standard_normal((b * V, capK)).astype(np.float32)
    la = r.integers(0, 3, (b * V, capK)).astype(np.int32)
    cnt = np.asarray(counts, np.int32).reshape(b * V)
    return np.ascontiguousarray(g), lo, la, cnt


_harness = None


def harness(tmp_dir):
    """The CPU harness over augment_core.h / tta_core.h, compiled once per process into `tmp_dir` (hipcc --cuda-host-only)."""
    global _harness
    if _harness is None:
        dst = os.path.join(str(tmp_dir), "libtta_harness.so")
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-fno-fast-math", "-ffp-contract=on", "-shared",
                               "-fPIC", "-o", dst, os.path.join(ROOT, "tests", "tta_harness.hip")])
        _harness = C.CDLL(dst)
        _harness.hst_tta_view.restype = None
        _harness.hst_tta_view.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p]
        _harness.hst_tta_unview.restype = None
        _harness.hst_tta_unview.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float]
    return _harness


def harness_views(lib, points, views):
    """views_host through the harness: the identity view is the rows, every other view the header's loop."""
    p = T.view_params(views)
    points = np.ascontiguousarray(points, np.float32)
    out = [points.copy()]
    for v in range(1, len(views)):
        dst = np.zeros_like(points)
        lib.hst_tta_view(points.ctypes.data, points.shape[0], points.shape[1], int(p["flip"][v]), float(p["sin"][v]),
                         float(p["cos"][v]), float(p["scale"][v]), dst.ctypes.data)
        out.append(dst)
    return out


def harness_unview(lib, boxes, views, v):
    p = T.view_params(views)
    b = np.ascontiguousarray(boxes, np.float32).copy().reshape(-1, 7)
    lib.hst_tta_unview(b.ctypes.data, len(b), int(p["flip"][v]), float(p["sin"][v]), float(p["cos"][v]), float(p["scale"][v]),
                       float(p["angle"][v]))
    return b


def harness_pool(lib, guided, logits, labels, counts, views, cap):
    """pool_host with the header's loop on the boxes: the kernel's row walk, one pooled row per iteration."""
    V = len(views)
    b, capK = guided.shape[0] // V, guided.shape[1]
    out = dict(guided=np.zeros((b, cap, 7), np.float32), logits=np.zeros((b, cap), np.float32),
               labels=np.zeros((b, cap), np.int32), counts=np.zeros(b, np.int32), overflow=False)
    for s in range(b):
        j = 0
        for v in range(V):
            k = int(min(max(int(counts[s * V + v]), 0), capK))
            boxes = guided[s * V + v, :k] if v == 0 else harness_unview(lib, guided[s * V + v, :k], views, v)
            for i in range(k):
                if j < cap:
                    out["guided"][s, j], out["logits"][s, j], out["labels"][s, j] = boxes[i], logits[s * V + v, i], labels[s * V + v, i]
                j += 1
        out["counts"][s] = min(j, cap)
        out["overflow"] |= j > cap
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
