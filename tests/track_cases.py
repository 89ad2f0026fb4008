"""Cases shared by the tracking tests (tests/test_track_cpu.py, tests/test_gpu_track_kernel.py): seeded sequences of 12 frames,
B = 2, capD = 8, in which objects of two labels move at constant world velocity while the ego of sample 0 turns and translates
(sample 1 stands and gives no pose), the CPU harness over csrc/track_core.h (tests/track_harness.hip), and the statement's
trace of every case, computed once.

What the script of a sequence makes happen (test_track_cpu.py asserts that it does, on the statement's trace):
  frame 0   the ego has not moved since the frame before and the initial state holds two label-1 tracks at rest exactly
            symmetric about a detection: the costs tie and the lowest slot must win.  Which slots they are depends on the
            capacity (TIE_SLOTS): two lanes of a wave, two waves, two passes of one thread.
  frame 1   an object appears with a score below birth_score (no track), and is born in frame 2
  frame 2   object A is missed for one frame and re-found in frame 3; sample 1 has D = 0
  frame 3   the count handed over is capD + 5: clamped to capD, the filler rows become detections
  3 .. 6    object B is missed for max_age + 1 frames: its track coasts, dies, and B gets a new id in frame 7
  frame 4   an object appears; around frames 4 / 5 object E (label 0) passes within max_dist of object C (label 1)
  frame 5   one detection has a NaN x
  frame 6   dt = 0 (the time stamp of frame 5)
  frame 7   D = capD
  frame 8   a reset in mid-sequence; its births take the lowest slots, two of them at (10, -1) and (10, 1)
  frame 9   the ego stands, one detection at (10, 0): the second tie
  frame 10  the status word is not zero
  frame 11  sample 0 has D = 0
Rows past the count hold shifted copies of the leading rows with a score of 0.99, so that a read beyond the count would show.
The initial state parks far-away tracks (which never die: their miss count starts far below zero) in every slot but a seeded
dozen -- the last slot among them unless the tie pair holds it -- so that births and matches reach the high slots of every
capacity until the reset."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from sassd import track as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

N_FRAMES, B, CAP_D, DT = 12, 2, 8, 0.1
SPEC = dict(max_dist=(2.0, 1.5), max_age=3, alpha=0.5, birth_score=0.3)
CAPS = (1, 4, 64, 65, 257)
TIE_SLOTS = {4: (1, 3), 64: (31, 63), 65: (63, 64), 257: (0, 256)}        # cap 1 has no pair
STATUS_FRAME, RESET_FRAME, DT0_FRAME, NAN_FRAME, OVER_FRAME, FULL_FRAME = 10, 8, 6, 5, 3, 7
EMPTY_FRAME = (11, 2)                                                       # per sample: the frame with D = 0
SIZE = {0: (1.6, 3.9, 1.56), 1: (0.6, 0.8, 1.73)}


def params(cap):
    return T.check_track(dict(SPEC, cap=cap))


def _ego_pose(s):
    """sensor-to-world pose after s steps of a left turn"""
    yaw = 0.03 * s
    c, sn = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -sn, 0, 1.2 * s], [sn, c, 0, 0.05 * s * s], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)


def _script(b):
    """objects of sample b: (label, p0 world xy, v world m/s, yaw, frames seen, score override per frame)"""
    off, k = (np.array([0.0, 0.0]), 1.0) if b == 0 else (np.array([3.0, -2.0]), 0.8)
    early = range(0, RESET_FRAME)
    objs = [
        (0, np.array([15.0, 3.0]) + off, k * np.array([8.0, 0.5]), 0.1, [t for t in early if t != 2], {}),                  # A
        (0, np.array([25.0, -6.0]) + off, k * np.array([-3.0, 1.0]), 3.0, [t for t in early if not 3 <= t <= 6], {}),       # B
        (1, np.array([20.0, 5.0]) + off, np.array([0.5, 0.0]), 1.5, list(early), {}),                                       # C
        (0, np.array([20.2, 8.3]) + off, np.array([0.0, -6.0]), -1.6, [t for t in early if t >= 1], {1: 0.2}),              # E
        (0, np.array([40.0, -10.0]) + off, k * np.array([-5.0, 0.0]), 3.1, [t for t in early if t >= 4], {}),               # late
    ]
    for j in range(3):                                                                                                       # frame 7
        objs.append((j % 2, np.array([50.0 + 4 * j, 12.0 - 9 * j]) + off, np.zeros(2), 0.3 * j, [FULL_FRAME], {}))
    return objs


def _scripted_tail(t, b):
    """sensor-frame detections (label, x, y) of the frames from the reset on"""
    if t == RESET_FRAME:
        return [(0, 10.0, -1.0), (1, 30.0, 4.0), (0, 10.0, 1.0)]
    if t == RESET_FRAME + 1:
        return [(1, 30.0, 4.2), (0, 10.0, 0.0)]
    if t == STATUS_FRAME:
        return [(0, 10.4, 0.1), (1, 30.1, 4.3)]
    return [(0, 10.8, 0.2), (1, 30.2, 4.5), (0, 22.0, -3.0)]


def sequence(seed):
    """-> dict(frames=[dict(det=, desc=, status=, items=)] * N_FRAMES).  The descriptors are
    TrackBook's, from the poses and times; the book has seen the frame before frame 0, so frame 0 carries no reset flag."""
    rng = np.random.default_rng(seed)
    steps = [0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 9, 10]                            # ego steps of frames -1, 0 .. 11
    times = [-DT, 0.0]                                                          # frames -1, 0 .. 11
    for t in range(1, N_FRAMES):
        times.append(times[-1] + (0.0 if t == DT0_FRAME else DT))
    book = T.TrackBook(B)
    book.commit(book.plan([dict(time=times[0], pose=_ego_pose(steps[0])), dict(time=times[0])]))
    frames = []
    for t in range(N_FRAMES):
        now = times[t + 1]
        boxes = np.zeros((B, CAP_D, 7), np.float32)
        scores = np.zeros((B, CAP_D), np.float32)
        labels = np.zeros((B, CAP_D), np.int32)
        counts = np.zeros(B, np.int32)
        items = []
        for b in range(B):
            pose = _ego_pose(steps[t + 1]) if b == 0 else None
            items.append(dict(time=now, pose=pose, first=t == RESET_FRAME))
            rows = []
            if t < RESET_FRAME:
                R, origin, ego_yaw = (pose[:2, :2], pose[:2, 3], 0.03 * steps[t + 1]) if b == 0 else (np.eye(2), np.zeros(2), 0.0)
                for label, p0, v, yaw, seen, low in _script(b):
                    if t not in seen:
                        continue
                    p = R.T @ (p0 + v * now - origin) + rng.normal(0, 0.04, 2)
                    rows.append((label, p[0], p[1], yaw - ego_yaw + rng.normal(0, 0.01), low.get(t)))
                if t == 0:
                    rows.append((1, 30.0, 0.0, 0.0, None))                      # the detection of the first tie
                if t == NAN_FRAME:
                    rows.append((0, np.nan, 3.0, 0.2, None))
            else:
                rows = [(label, x, y, 0.1, None) for label, x, y in _scripted_tail(t, b)]
            if t == EMPTY_FRAME[b]:
                rows = []
            if t not in (0, RESET_FRAME, RESET_FRAME + 1):
                rows = [rows[i] for i in rng.permutation(len(rows))]
            assert len(rows) <= CAP_D, (t, b, len(rows))
            n = len(rows)
            for d, (label, x, y, yaw, score) in enumerate(rows):
                w, l, h = SIZE[label]
                boxes[b, d] = [x, y, -1.0 + 0.02 * d, w, l, h, yaw]
                labels[b, d] = label
                scores[b, d] = rng.uniform(0.35, 0.95) if score is None else score
            for d in range(n, CAP_D):                                           # what must not be read
                src = (d - n) % max(n, 1)
                boxes[b, d] = boxes[b, src] + np.float32([0.3, -0.2, 0, 0, 0, 0, 0]) if n else [12.0, 1.0, -1.0, 1.6, 3.9, 1.56, 0.0]
                labels[b, d], scores[b, d] = (labels[b, src] if n else 0), 0.99
            counts[b] = n
        if t == OVER_FRAME:
            counts[:] = CAP_D + 5
        if t == FULL_FRAME:
            assert (counts == CAP_D).all(), counts
        d = book.plan(items)
        book.commit(d)
        desc = {k: d[k] for k in ("T", "dyaw", "dt", "flags")}
        frames.append(dict(det=dict(boxes=boxes, scores=scores, labels=labels, counts=counts), desc=desc,
                           status=4 if t == STATUS_FRAME else 0, items=items))
    return dict(frames=frames)


def initial_state(seed, cap):
    """Parked tracks in every slot but a seeded dozen, and for cap >= 4 the tie pair of frame 0:
    two label-1 tracks at rest at (30, -1) and (30, 1) in the slots TIE_SLOTS[cap]."""
    rng = np.random.default_rng(seed + 1000 * cap)
    st = T.empty_state(B, cap)
    pair = TIE_SLOTS.get(cap, ())
    pool = [i for i in range(cap) if i not in pair and i != cap - 1]
    n_free = min(len(pool), 11)
    for b in range(B):
        f = T.slot_fields(st["slots"][b])
        free = {0} if cap == 1 else set(rng.choice(pool, n_free, replace=False).tolist()) | ({cap - 1} - set(pair))
        nid = 0
        for i in range(cap):
            if i in free:
                continue
            if i in pair:
                y = -1.0 if i == pair[1] else 1.0           # the HIGHER slot sits at -1: no order of y decides the winner
                f["label"][i], f["box"][i] = 1, [30.0, y, -1.0, 0.6, 0.8, 1.73, 0.0]
                f["misses"][i], f["hits"][i] = 0, 3
            else:
                f["label"][i], f["box"][i] = int(rng.integers(0, 2)), [500.0 + i, 500.0 + 3 * b, -1.0, 1.6, 3.9, 1.56, 0.0]
                f["misses"][i], f["hits"][i] = -(1 << 20), 5
            f["id"][i], f["score"][i] = nid, 0.5
            nid += 1
        st["next_id"][b] = nid
    return st


_TRACE = {}


def trace(seed, cap):
    """The statement over the whole sequence, computed once and left unchanged: dict(seq=, state0=, steps=[(state, out)] per
    frame)."""
    key = (seed, cap)
    if key not in _TRACE:
        seq, st = sequence(seed), initial_state(seed, cap)
        steps, cur = [], st
        for fr in seq["frames"]:
            cur, out = T.track_host(cur, fr["det"], fr["desc"], params(cap), fr["status"])
            steps.append((cur, out))
        _TRACE[key] = dict(seq=seq, state0=st, steps=steps)
    return _TRACE[key]


SEEDS = (0, 1)
CASES = [(seed, cap) for seed in SEEDS for cap in CAPS]

# ---- the crowd: more detections than one chunk of 256, more slots than one pass ----------------------------------------------
CROWD_CAP_D, CROWD_N, CROWD_CAPS, CROWD_FRAMES = 300, (290, 130), (257, 1024), 3


def crowd(seed):
    """3 frames, B = 2, capD = 300, D = 290 and 130 (less the tenth that is missed in frame 1): objects on a jittered 3 m grid,
    each with a velocity of its own, in a new order every frame; no ego motion.  Frame 0 resets.  With cap = 257 the births
    of frame 0 overflow the table (dropped > 0); with cap = 1024 every pass of the 256 threads holds live slots."""
    rng = np.random.default_rng(100 + seed)
    n_max = max(CROWD_N)
    p0 = np.stack([5.0 + 3.0 * (np.arange(n_max) % 20), -40.0 + 3.0 * (np.arange(n_max) // 20)], 1) + rng.uniform(-0.3, 0.3, (n_max, 2))
    v = rng.uniform(-5.0, 5.0, (n_max, 2))
    lab = rng.integers(0, 2, n_max)
    frames = []
    for t in range(CROWD_FRAMES):
        boxes = np.zeros((B, CROWD_CAP_D, 7), np.float32)
        boxes[:, :, :] = [12.0, 1.0, -1.0, 1.6, 3.9, 1.56, 0.0]
        scores = np.full((B, CROWD_CAP_D), 0.99, np.float32)
        labels = np.zeros((B, CROWD_CAP_D), np.int32)
        counts = np.zeros(B, np.int32)
        for b in range(B):
            seen = np.flatnonzero(rng.random(CROWD_N[b]) >= (0.1 if t == 1 else 0.0))
            seen = seen[rng.permutation(len(seen))]
            n = len(seen)
            boxes[b, :n, :2] = p0[seen] + v[seen] * (t * DT) + 0.5 * b
            boxes[b, :n, 6] = 0.01 * seen
            labels[b, :n] = lab[seen]
            scores[b, :n] = rng.uniform(0.2, 0.95, n)
            counts[b] = n
        desc = T.identity_desc(B, reset=t == 0)
        desc["dt"][:] = 0.0 if t == 0 else DT
        frames.append(dict(det=dict(boxes=boxes, scores=scores, labels=labels, counts=counts), desc=desc, status=0))
    return dict(frames=frames)


def crowd_trace(seed, cap):
    key = ("crowd", seed, cap)
    if key not in _TRACE:
        seq, st = crowd(seed), T.empty_state(B, cap)
        steps, cur = [], st
        for fr in seq["frames"]:
            cur, out = T.track_host(cur, fr["det"], fr["desc"], params(cap), fr["status"])
            steps.append((cur, out))
        _TRACE[key] = dict(seq=seq, state0=st, steps=steps)
    return _TRACE[key]

_harness = None


def harness(tmp_dir):
    """The CPU harness over track_core.h, compiled once per process into `tmp_dir` (hipcc --cuda-host-only)."""
    global _harness
    if _harness is None:
        dst = os.path.join(str(tmp_dir), "libtrack_harness.so")
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-fno-fast-math", "-ffp-contract=on", "-shared",
                               "-fPIC", "-o", dst, os.path.join(ROOT, "tests", "track_harness.hip")])
        _harness = C.CDLL(dst)
        _harness.hst_track_step.restype = None
        _harness.hst_track_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_float, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]
    return _harness


def harness_step(lib, state, det, desc, p, status):
    """track_host through the harness: the header's functions, one sample after the other -> (state, outputs)."""
    slots = np.array(state["slots"], np.int32, order="C", copy=True)
    next_id = np.array(state["next_id"], np.int32, copy=True)
    nb, cap_d = det["boxes"].shape[:2]
    out = dict(det_id=np.zeros((nb, cap_d), np.int32), det_hits=np.zeros((nb, cap_d), np.int32),
               det_vel=np.zeros((nb, cap_d, 2), np.float32), dropped=np.zeros(nb, np.int32), count=np.zeros(nb, np.int32))
    packed = T.pack_desc(desc).reshape(nb, T.DESC_BYTES)
    md = np.asarray(p["max_dist"], np.float32)
    for b in range(nb):
        bx, sc, la = (np.ascontiguousarray(det[k][b]) for k in ("boxes", "scores", "labels"))
        de = np.ascontiguousarray(packed[b]).view(np.float64)                   # 8-byte aligned
        out2 = np.zeros(2, np.int32)
        lib.hst_track_step(bx.ctypes.data, sc.ctypes.data, la.ctypes.data, int(det["counts"][b]), cap_d, int(status),
                           de.ctypes.data, slots[b].ctypes.data, next_id[b:b + 1].ctypes.data, slots.shape[1], md.ctypes.data,
                           len(md), p["max_age"], p["alpha"], p["birth_score"], out["det_id"][b].ctypes.data,
                           out["det_hits"][b].ctypes.data, out["det_vel"][b].ctypes.data, out2.ctypes.data)
        out["count"][b], out["dropped"][b] = out2
    return dict(slots=slots, next_id=next_id), out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_step(got, want):
    """(state, outputs) pairs equal bit for bit -> the name of the first field that differs, or None"""
    for part, g, w in (("state", got[0], want[0]), ("out", got[1], want[1])):
        for k in w:
            if not same_bits(np.asarray(g[k]), np.asarray(w[k])):
                return "%s[%s]" % (part, k)
    return None
