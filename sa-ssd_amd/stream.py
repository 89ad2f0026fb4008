"""FrameStream: frames in flight, detections on the host, in order, the pipeline status checked per frame.

The rate README publishes for car_cfg batch 1 comes from three one-branch frame graphs (InferencePlan(overlap=False)) replayed
round-robin on three HIP streams.  This module is that recipe behind a public call, with what a user
needs added: the result leaves the GPU.  Per frame and slot:

  submit   pinned clouds + staging block -> one H2D copy per cloud + one for the block of `stage_layout` (no fill launches)
           graph.launch()            the captured frame; its last node, sassd_frame_seal, writes the frame record
           one D2H copy              the record -> a pinned host buffer; an event behind it
  collect  event.synchronize()       then decode the record: magic, seq == ticket, status, counts, boxes / scores / labels

The record layout is the contract of include/sassd.h ("Frame record"); `record_layout` is its only Python statement and the
decoder reads nothing else.  `stage_layout` is the same for the frame's small inputs: InferencePlan.capture() cuts the
device block by it, the slot its pinned twin.  Ring order, back-pressure and the error rules live in `FrameRing`, which
drives any "slot" with stage / launch / ready / wait / record -- the CPU tests hand it a fake one.

    fs = FrameStream(state_dict, inflight=3, points_cap=21504, batch_size=1, anchors=an, device=dev)
    for ticket, dets in fs.map(batches):     # dets: what plan.results() returns for that batch
        ...
    fs.close()

Raw sweeps: FrameStream(..., raw_cap=122880) puts the camera-frustum reduction (velodyne -> velodyne_reduced) into the
captured frame -- sassd_crop_polytope_dev, two kernels per sample in front of the voxelizer.  submit(clouds, frustums) then
takes clouds of up to raw_cap points and one frustum per cloud ([6,4] float64 planes of geometry.frustum_planes, or
dict(calib=..., img_shape=...)); the planes ride in the staging block of the counts (`stage_layout`).

KITTI annotations: FrameStream(..., annos=True) ends the frame with sassd_frame_seal_kitti -- the record is layout version
2, the version 1 record plus the annotation block (camera-frame boxes, alpha, clipped 2-D boxes of the detections whose
projection meets the image).  submit(clouds, frustums, calibs) then takes one dict(calib=..., img_shape=...) per cloud; the
[B,36] float64 calibration block rides in the same staging block, behind the planes.  collect() returns per sample
(boxes, scores, labels, cam); kitti_common.result_anno_from_cam turns `cam` into the result annotation by indexing alone.

Multi-sweep clouds: FrameStream(..., sweeps=S, sweep_cap=N) keeps the sweeps of every sample's sequence in a device ring and
starts the frame with sassd_merge_sweeps_dev -- one kernel per sample that merges the current sweep and the S-1 before it,
moved into the current sensor frame by the ego pose, the time lag as the last feature.  submit(clouds, sweeps=[dict(pose=,
time=), ...]) uploads the new sweep alone; the descriptors (ring slots, counts, transforms, lags) ride in the staging block.
`SweepBook` is the host bookkeeping, `sweep_transform` the pose arithmetic, `merge_sweeps_host` the numpy statement of the
kernel's contract.
"""
from collections import deque

import numpy as np

FRAME_MAGIC = 0x53460001            # SASSD_FRAME_MAGIC: 'S' 'F', layout version 1
FRAME_MAGIC_KITTI = 0x53460002      # SASSD_FRAME_MAGIC_KITTI: layout version 2, the annotation block behind the v1 record
CALIB_DOUBLES = 36                  # per sample: Tr_velo_to_cam 12 | R0_rect 9 | P2 12 | img_w | img_h | pad
MAX_SWEEPS = 16                     # descriptor entries of one merged frame (sassd_merge_sweeps_dev)
MAX_INFLIGHT = 4                    # one HIP stream per frame in flight; the runtime multiplexes a process onto 4 hardware queues
_SEQ_MASK = 0x7FFFFFFF


def record_layout(B, capD, annos=False):
    """Byte offsets of the frame record for `B` samples x `capD` detection rows (include/sassd.h "Frame record"):
    dict(magic, seq, status, B, capD, counts, boxes, scores, labels, total) -- every field 4-byte aligned, in this order.
    annos=True: layout version 2 -- the same offsets, then the annotation block ("KITTI annotations") at the next 8-byte
    boundary: annos (its start), kept, index, cam, alpha, bbox (8-byte aligned), and the new total."""
    B, capD = int(B), int(capD)
    if B < 1 or capD < 1 or B * capD > (1 << 24):
        raise ValueError("no frame record for batch %d x capD %d" % (B, capD))
    hdr = (5 + B + 3) // 4 * 4                  # SASSD_FRAME_HEADER_WORDS
    n = B * capD
    boxes = 4 * hdr
    scores = boxes + 4 * 7 * n
    labels = scores + 4 * n
    L = dict(magic=0, seq=4, status=8, B=12, capD=16, counts=20, boxes=boxes, scores=scores, labels=labels,
             total=labels + 4 * n)
    if annos:
        at = (L["total"] + 7) // 8 * 8
        index = at + 4 * ((B + 1) // 2 * 2)         # kept[B], one zero word when B is odd
        alpha = index + 4 * n + 28 * n
        bbox = alpha + 4 * n + 4 * (n & 1)          # one zero word when n is odd
        L.update(annos=at, kept=at, index=index, cam=index + 4 * n, alpha=alpha, bbox=bbox, total=bbox + 32 * n)
    return L


def stage_layout(B, raw=False, annos=False, seal=False, sweeps=0):
    """Byte offsets of the frame's staging block -- its small per-frame inputs, one H2D copy -- for `B` samples:
    dict(planes, calib, words, seq, counts, total), in this order: the crop planes [B,6,4] f64 (`raw`: a frame that crops raw
    sweeps), the calibration block [B,CALIB_DOUBLES] f64 (`annos`), then the int32 words: [seq] when `seal`, counts[B] (the
    points per cloud).  A part that is absent has length 0; `seq` is None when not sealed.  The float64 parts come first, so
    they are 8-byte aligned.
    sweeps=S (1..MAX_SWEEPS; a frame that merges sweeps, include/sassd.h "Multi-sweep merge") adds the keys sweep_T -- the
    transforms [B,S,3,4] f64, the last of the float64 parts, in front of `words` -- and, behind counts, sweep_slot,
    sweep_count, sweep_xform ([B,S] i32 each) and sweep_dt ([B,S] f32); `total` covers them.  With sweeps=0 the dict is the
    one above, key for key."""
    B, S = int(B), int(sweeps)
    if B < 1:
        raise ValueError("no staging block for batch %d" % B)
    if not 0 <= S <= MAX_SWEEPS:
        raise ValueError("sweeps must be 0..%d, got %d" % (MAX_SWEEPS, S))
    calib = 8 * 6 * 4 * B if raw else 0
    sweep_T = calib + (8 * CALIB_DOUBLES * B if annos else 0)
    words = sweep_T + 8 * 12 * S * B
    counts = words + (4 if seal else 0)
    L = dict(planes=0, calib=calib, words=words, seq=words if seal else None, counts=counts, total=counts + 4 * B)
    if S:
        at, n = L["total"], 4 * B * S
        L.update(sweep_T=sweep_T, sweep_slot=at, sweep_count=at + n, sweep_xform=at + 2 * n, sweep_dt=at + 3 * n,
                 total=at + 4 * n)
    return L


def stage_views(buf, B, L):
    """numpy views into `buf` (uint8, at least L['total'] bytes) of the parts of L = stage_layout(B, ...):
    dict(planes [B,6,4] f64 | None, calib [B,CALIB_DOUBLES] f64 | None, seq [1] i32 | None, counts [B] i32), and for a
    layout with sweeps=S also sweep_T [B,S,3,4] f64, sweep_slot / sweep_count / sweep_xform [B,S] i32, sweep_dt [B,S] f32."""
    def f64(lo, hi, *shape):
        return buf[lo:hi].view(np.float64).reshape(B, *shape) if hi > lo else None
    V = dict(planes=f64(L["planes"], L["calib"], 6, 4), calib=f64(L["calib"], L.get("sweep_T", L["words"]), CALIB_DOUBLES),
             seq=None if L["seq"] is None else buf[L["seq"]:L["counts"]].view(np.int32),
             counts=buf[L["counts"]:L["counts"] + 4 * B].view(np.int32))
    if "sweep_T" in L:
        S = (L["sweep_count"] - L["sweep_slot"]) // (4 * B)
        V["sweep_T"] = f64(L["sweep_T"], L["words"], S, 3, 4)
        for key, end, dt in (("sweep_slot", "sweep_count", np.int32), ("sweep_count", "sweep_xform", np.int32),
                             ("sweep_xform", "sweep_dt", np.int32), ("sweep_dt", "total", np.float32)):
            V[key] = buf[L[key]:L[end]].view(dt).reshape(B, S)
    return V


def sweep_transform(pose_now, pose_then):
    """The [3,4] float64 matrix that moves a point of the sensor frame at `pose_then` into the sensor frame at `pose_now`:
    the upper rows of inv(pose_now) @ pose_then.  Poses are sensor-to-world 4x4 float64 RIGID transforms [R | t]; the inverse
    is formed explicitly as [R^T | -R^T t] (exact for a rotation, no linalg.inv).  Equal poses -- a vehicle that stands --
    give exactly [I | 0], not the rounded R^T R."""
    a, b = np.asarray(pose_now, dtype=np.float64), np.asarray(pose_then, dtype=np.float64)
    if a.shape != (4, 4) or b.shape != (4, 4):
        raise ValueError("poses must be 4x4, got %s and %s" % (a.shape, b.shape))
    out = np.zeros((3, 4))
    if np.array_equal(a, b):
        out[:, :3] = np.eye(3)
        return out
    rt = a[:3, :3].T
    out[:, :3] = rt @ b[:3, :3]
    out[:, 3] = rt @ b[:3, 3] + -(rt @ a[:3, 3])
    return out


def merge_sweeps_host(entries, time_feature):
    """The numpy statement of sassd_merge_sweeps_dev's contract (include/sassd.h "Multi-sweep merge") for entries that are all
    present: `entries` is a list of (points [n, ndim_in] f32, T [3,4] f64 or None, dt) in entry order -- T None is xform = 0,
    the rows copied as they are -- -> the merged cloud [sum n, ndim_in + (1 if time_feature else 0)] f32.  What a caller
    without FrameStream(sweeps=...) does per frame on the host."""
    out = []
    for pts, T, dt in entries:
        pts = np.asarray(pts, dtype=np.float32)
        rows = np.empty((len(pts), pts.shape[1] + (1 if time_feature else 0)), np.float32)
        rows[:, :pts.shape[1]] = pts
        if T is not None:
            T = np.asarray(T, dtype=np.float64)
            x, y, z = (pts[:, i].astype(np.float64) for i in range(3))
            for i in range(3):                      # every product and sum rounded on its own, in the kernel's order
                rows[:, i] = (((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3]).astype(np.float32)
        if time_feature:
            rows[:, -1] = np.float32(dt)
        out.append(rows)
    return np.ascontiguousarray(np.concatenate(out, 0))


class SweepBook:
    """The host bookkeeping of a stream that merges sweeps: which ring slot every sweep of a sample's sequence lives in, and
    the poses and times the descriptors of the next frame are made of.  `plan` checks one frame's inputs and returns its
    descriptors WITHOUT changing the book; `commit` makes them the book's state -- a refused submit leaves no trace.

    Every submit writes one sweep per sample, so the samples share the running sweep number k (0, 1, ...) and sweep k lives
    in ring slot k % R.  The frame of sweep k reads sweeps k-S+1 .. k; R >= S + inflight - 1 keeps the slot that sweep k
    overwrites (that of sweep k-R) out of the reach of the inflight-1 frames that may still run (FrameStream, "Ordering")."""

    def __init__(self, B, S, R, sweep_cap, ndim, inflight=1):
        B, S, R = int(B), int(S), int(R)
        if not 1 <= S <= MAX_SWEEPS:
            raise ValueError("sweeps must be 1..%d, got %d" % (MAX_SWEEPS, S))
        if int(sweep_cap) < 1:
            raise ValueError("sweep_cap (the largest sweep the stream accepts) must be >= 1")
        assert R >= S + int(inflight) - 1, "a ring of %d slots is overwritten under frames in flight" % R
        self.B, self.S, self.R, self.sweep_cap, self.ndim = B, S, R, int(sweep_cap), int(ndim)
        self.k = 0                                      # sweeps written so far
        self.hist = [[] for _ in range(B)]              # per sample, newest first: (k, pose, time, points) of its sweeps

    def plan(self, clouds, sweeps):
        B, S = self.B, self.S
        if sweeps is None:
            raise ValueError("a stream with sweeps needs submit(clouds, sweeps=[dict(pose=, time=), ...]), one per cloud")
        if len(clouds) != B:
            raise ValueError("a batch of %d clouds for a stream of batch_size %d" % (len(clouds), B))
        if len(sweeps) != B:
            raise ValueError("%d sweep descriptions for a stream of batch_size %d" % (len(sweeps), B))
        d = dict(k=self.k, write=self.k % self.R, slot=np.full((B, S), -1, np.int32), count=np.zeros((B, S), np.int32),
                 xform=np.zeros((B, S), np.int32), T=np.zeros((B, S, 3, 4)), dt=np.zeros((B, S), np.float32), hist=[])
        d["T"][:, :, :, :3] = np.eye(3)
        for b, (pts, sw) in enumerate(zip(clouds, sweeps)):
            if pts.ndim != 2 or pts.shape[1] != self.ndim:
                raise ValueError("cloud %d has shape %s, expected [N, %d]" % (b, tuple(pts.shape), self.ndim))
            if pts.shape[0] > self.sweep_cap:           # never detect on a silently truncated sweep
                raise ValueError("cloud %d has %d points, the stream was sized for %d (sweep_cap)"
                                 % (b, pts.shape[0], self.sweep_cap))
            if not isinstance(sw, dict) or sw.get("pose") is None or sw.get("time") is None:
                raise ValueError("sweep %d: a dict with `pose` and `time` is needed" % b)
            pose = np.array(sw["pose"], dtype=np.float64)
            if pose.shape != (4, 4) or not np.isfinite(pose).all():
                raise ValueError("sweep %d: pose must be a finite 4x4 matrix" % b)
            time = float(sw["time"])
            if not np.isfinite(time):
                raise ValueError("sweep %d: time must be finite" % b)
            past = [] if sw.get("first", False) else self.hist[b][:S - 1]
            d["slot"][b, 0], d["count"][b, 0] = d["write"], int(pts.shape[0])
            for s, (k, pose_j, time_j, n_j) in enumerate(past, 1):
                d["slot"][b, s], d["count"][b, s], d["xform"][b, s] = k % self.R, n_j, 1
                d["T"][b, s] = sweep_transform(pose, pose_j)
                d["dt"][b, s] = np.float32(time - time_j)
            d["hist"].append([(self.k, pose, time, int(pts.shape[0]))] + past)
        d["reads"] = sorted({int(v) for v in d["slot"][:, 1:].ravel() if v >= 0})
        return d

    def commit(self, d):
        assert d["k"] == self.k
        self.k += 1
        self.hist = [h[:max(self.S - 1, 0)] for h in d["hist"]]


class FrameStatusError(RuntimeError):
    """A frame whose status word was not zero: the RuntimeError of InferencePlan.results(), with the word in `.status`."""

    def __init__(self, st):
        super().__init__("sassd pipeline status flags 0x%x (capacity overflow / hash full)" % st)
        self.status = int(st)


def status_error(st):
    """The error InferencePlan.results() raises for a non-zero status word."""
    return FrameStatusError(st)


def _extend4(m):
    """3x3 / 3x4 / 4x4 calibration matrix -> 4x4 float64, padded as kitti_common.get_kitti_image_info(extend_matrix=True)."""
    m = np.asarray(m, dtype=np.float64)
    if m.shape == (4, 4):
        return m
    out = np.zeros((4, 4))
    out[3, 3] = 1.
    out[:m.shape[0], :m.shape[1]] = m
    return out


def _calib_matrices(calib):
    """(P2, R0_rect, Tr_velo_to_cam) as float64 matrices from a kitti_common.Calibration or a dict of them (the forms of
    frustum_of): flat rows of a KITTI calib file are reshaped, 3x3 / 3x4 / 4x4 are taken as they are."""
    if isinstance(calib, dict):
        get = lambda *ks: next(calib[k] for k in ks if k in calib)      # noqa: E731
        p2, r0, v2c = get("P2", "calib/P2"), get("R0_rect", "calib/R0_rect"), get("Tr_velo_to_cam", "calib/Tr_velo_to_cam")
    else:
        p2, r0, v2c = calib.P2, calib.R0, calib.V2C
    p2, r0, v2c = (np.asarray(m, dtype=np.float64) for m in (p2, r0, v2c))
    if p2.ndim == 1:
        p2 = p2.reshape(3, 4)
    if r0.ndim == 1:
        r0 = r0.reshape(3, 3)
    if v2c.ndim == 1:
        v2c = v2c.reshape(3, 4)
    return p2, r0, v2c


def calib_block_of(calib, img_shape):
    """One sample's calibration block for the annotation kernel (include/sassd.h "KITTI annotations"): [36] float64 --
    Tr_velo_to_cam [3,4], R0_rect [3,3], P2 [3,4], img_w, img_h, 0 -- from the forms frustum_of accepts.  ValueError for a
    matrix that is not finite or an image size that is not positive."""
    p2, r0, v2c = _calib_matrices(calib)
    h, w = int(img_shape[0]), int(img_shape[1])
    if h < 1 or w < 1:
        raise ValueError("img_shape must be positive, got %s" % (tuple(img_shape),))
    out = np.zeros(CALIB_DOUBLES)
    out[:12], out[12:21], out[21:33] = v2c[:3, :4].ravel(), r0[:3, :3].ravel(), p2[:3, :4].ravel()
    out[33], out[34] = w, h
    if not np.isfinite(out).all():
        raise ValueError("calibration matrices must be finite")
    return out


def frustum_of(calib, img_shape):
    """The [6,4] float64 planes of a frame's camera-2 viewing frustum (geometry.frustum_planes) from its calibration -- a
    kitti_common.Calibration (P2, R0, V2C) or a dict with P2, R0_rect, Tr_velo_to_cam (3x3 / 3x4 / 4x4, or the flat rows
    of a KITTI calib file) -- and its image shape (h, w).  Host arithmetic only."""
    from .geometry import frustum_planes
    p2, r0, v2c = _calib_matrices(calib)
    planes, f32 = frustum_planes(_extend4(r0), _extend4(v2c), _extend4(p2), (int(img_shape[0]), int(img_shape[1])))
    assert not f32                                  # float64 calibration gives float64 planes: the stream's crop is float64
    return planes


def _check_calibs(calibs, frustums, B, annos):
    """The calibration side of check_frame_inputs -> [B,36] float64, or None on a stream without annos."""
    if not annos:
        if calibs is not None:
            raise ValueError("calibs given to a stream without annos (its record holds lidar-frame detections only)")
        return None
    if calibs is None and frustums is not None and len(frustums) == B and all(isinstance(f, dict) for f in frustums):
        calibs = frustums                       # a raw stream fed with dict(calib=, img_shape=): the same dicts serve both
    if calibs is None:
        raise ValueError("a stream with annos projects every detection: submit(..., calibs=) needs one "
                         "dict(calib=, img_shape=) per cloud")
    if len(calibs) != B:
        raise ValueError("%d calibs for a stream of batch_size %d" % (len(calibs), B))
    out = np.empty((B, CALIB_DOUBLES), dtype=np.float64)
    for b, c in enumerate(calibs):
        if not isinstance(c, dict) or c.get("calib") is None or c.get("img_shape") is None:
            raise ValueError("calib %d: a dict with `calib` and `img_shape` is needed" % b)
        try:
            out[b] = calib_block_of(c["calib"], c["img_shape"])
        except ValueError as e:
            raise ValueError("calib %d: %s" % (b, e)) from None
    return out


def check_frame_inputs(clouds, frustums, B, ndim, points_cap, raw_cap=None, calibs=None, annos=False):
    """The checks a slot makes on one frame's inputs before it queues anything (host only).  ValueError for: the wrong
    number of clouds, a cloud that is not [N, ndim], a cloud above the stream's capacity (raw_cap on a raw stream, else
    points_cap), frustums missing on a raw stream or given to a stream without raw_cap, the wrong number of frustums,
    planes that are not [6,4] or not finite.  -> the planes as one [B,6,4] float64 array, or None without raw_cap.
    With annos=True (a stream that writes KITTI annotations) also: calibs missing (unless the frustums are
    dict(calib=, img_shape=), which then serve as calibs too) or miscounted, a non-finite calibration matrix, a non-positive
    image size -> (planes, the [B,36] float64 calibration block).  calibs given with annos=False is a ValueError too."""
    planes = _check_clouds_and_frustums(clouds, frustums, B, ndim, points_cap, raw_cap)
    block = _check_calibs(calibs, frustums, B, annos)
    return (planes, block) if annos else planes


def _check_clouds_and_frustums(clouds, frustums, B, ndim, points_cap, raw_cap):
    if len(clouds) != B:
        raise ValueError("a batch of %d clouds for a stream of batch_size %d" % (len(clouds), B))
    cap, what = (points_cap, "points_cap") if raw_cap is None else (raw_cap, "raw_cap")
    for b, pts in enumerate(clouds):        # never detect on a silently truncated cloud
        if pts.ndim != 2 or pts.shape[1] != ndim:
            raise ValueError("cloud %d has shape %s, expected [N, %d]" % (b, tuple(pts.shape), ndim))
        if pts.shape[0] > cap:
            raise ValueError("cloud %d has %d points, the stream was sized for %d (%s)" % (b, pts.shape[0], cap, what))
    if raw_cap is None:
        if frustums is not None:
            raise ValueError("frustums given to a stream without raw_cap (its clouds are taken as they are)")
        return None
    if frustums is None:
        raise ValueError("a stream with raw_cap crops every cloud: submit(clouds, frustums) needs one frustum per cloud")
    if len(frustums) != B:
        raise ValueError("%d frustums for a stream of batch_size %d" % (len(frustums), B))
    out = np.empty((B, 6, 4), dtype=np.float64)
    for b, f in enumerate(frustums):
        if isinstance(f, dict):
            if "calib" not in f or "img_shape" not in f:
                raise ValueError("frustum %d: a dict needs `calib` and `img_shape`" % b)
            f = frustum_of(f["calib"], f["img_shape"])
        f = np.asarray(f)
        if f.shape != (6, 4) or f.dtype != np.float64:
            raise ValueError("frustum %d: planes must be a [6, 4] float64 array, got %s %s" % (b, f.shape, f.dtype))
        if not np.isfinite(f).all():
            raise ValueError("frustum %d: planes must be finite" % b)
        out[b] = f
    return out


def decode_record(buf, B, capD, seq, annos=False):
    """One frame record (bytes-like / uint8 array of record_layout(B, capD)['total'] bytes) -> what plan.results() returns:
    per sample (boxes [k,7] f32, scores [k] f32, labels [k] i64), or (None, None, None) for a sample without detections.
    The arrays are copies.  RuntimeError("stale frame record") unless the record carries the magic word, this B / capD and
    `seq`; the status error of plan.results() when its status word is not zero.
    annos=True: a record of layout version 2 (its magic word is checked instead) -> per sample (boxes, scores, labels, cam),
    cam = dict(index i64[k'], location f32[k',3], dimensions f32[k',3], rotation_y f32[k'], alpha f32[k'], bbox f64[k',4])
    of the k' detections whose projection meets the image (`index`: their rows in boxes), all copies; (None,) * 4 for a
    sample without detections, zero-length arrays when every detection missed the image."""
    L = record_layout(B, capD, annos)
    if memoryview(buf).nbytes < L["total"]:
        raise RuntimeError("stale frame record")
    raw = np.frombuffer(buf, dtype=np.uint8, count=L["total"])
    words = raw.view(np.int32)
    n = B * capD
    if (int(words[0]) != (FRAME_MAGIC_KITTI if annos else FRAME_MAGIC) or int(words[3]) != B or int(words[4]) != capD
            or int(words[1]) != (int(seq) & _SEQ_MASK)):
        raise RuntimeError("stale frame record")
    st = int(words[2])
    if st:
        raise status_error(st)
    counts = words[L["counts"] // 4:L["counts"] // 4 + B]
    boxes = raw[L["boxes"]:L["scores"]].view(np.float32).reshape(B, capD, 7)
    scores = raw[L["scores"]:L["labels"]].view(np.float32).reshape(B, capD)
    labels = words[L["labels"] // 4:L["labels"] // 4 + n].reshape(B, capD)
    if annos:
        kept = words[L["kept"] // 4:L["kept"] // 4 + B]
        index = words[L["index"] // 4:L["index"] // 4 + n].reshape(B, capD)
        cam = raw[L["cam"]:L["alpha"]].view(np.float32).reshape(B, capD, 7)
        alpha = raw[L["alpha"]:L["alpha"] + 4 * n].view(np.float32).reshape(B, capD)
        bbox = raw[L["bbox"]:L["total"]].view(np.float64).reshape(B, capD, 4)
    out = []
    for b in range(B):
        k = min(max(int(counts[b]), 0), capD)
        if k == 0:
            out.append((None,) * (4 if annos else 3))
            continue
        det = (boxes[b, :k].copy(), scores[b, :k].copy(), labels[b, :k].astype(np.int64))
        if annos:
            m = min(max(int(kept[b]), 0), k)
            det += (dict(index=index[b, :m].astype(np.int64), location=cam[b, :m, :3].copy(),
                         dimensions=cam[b, :m, 3:6].copy(), rotation_y=cam[b, :m, 6].copy(), alpha=alpha[b, :m].copy(),
                         bbox=bbox[b, :m].copy()),)
        out.append(det)
    return out


class FrameRing:
    """Tickets over a ring of slots.  Ticket t (1, 2, ...) runs on slot (t - 1) % len(slots); a slot is

        stage(seq, clouds)   check and queue the inputs of one frame (ValueError for inputs it cannot take: nothing queued);
                             called as stage(seq, clouds, frustums) when submit() was given frustums, and only then;
                             with calibs=<calibs> as a keyword when submit() was given calibs, and only then;
                             with sweeps=<sweeps> as a keyword when submit() was given sweeps, and only then;
                             with track=<track> as a keyword when submit() was given track, and only then
        launch()             queue the frame and the copy of its record
        ready() / wait()     has the record arrived / block until it has
        record()             the arrived record, valid until the next stage()
        recover()            (optional) called after a record that carried a status flag (FrameStatusError), before the slot
                             is used again

    `decode(record, seq)` turns a record into a result or raises.  A busy slot is harvested -- waited for, decoded, its
    result (or its error) parked under its ticket -- before it is staged again, so a result is neither overwritten nor
    skipped; an error belongs to its ticket alone and is raised by that ticket's collect()."""

    def __init__(self, slots, decode):
        if not 1 <= len(slots) <= MAX_INFLIGHT:
            raise ValueError("inflight must be 1..%d, got %d" % (MAX_INFLIGHT, len(slots)))
        self.slots, self.decode = list(slots), decode
        self.busy = [None] * len(self.slots)        # ticket in flight on each slot
        self.done = {}                              # ticket -> (result, None) | (None, exception)
        self.next_ticket = 1
        self.closed = False

    def in_flight(self):
        return sum(t is not None for t in self.busy)

    def _harvest(self, i):
        slot, t = self.slots[i], self.busy[i]
        slot.wait()
        try:
            self.done[t] = (self.decode(slot.record(), t), None)
        except RuntimeError as e:
            self.done[t] = (None, e)
            recover = getattr(slot, "recover", None)
            if isinstance(e, FrameStatusError) and recover is not None:     # a stale record says nothing about the status word
                recover()
        self.busy[i] = None

    def submit(self, clouds, frustums=None, calibs=None, sweeps=None, track=None):
        if self.closed:
            raise RuntimeError("FrameStream is closed")
        t = self.next_ticket
        i = (t - 1) % len(self.slots)
        if self.busy[i] is not None:
            self._harvest(i)
        args = (clouds,) if frustums is None else (clouds, frustums)
        kw = {} if calibs is None else dict(calibs=calibs)
        if sweeps is not None:
            kw["sweeps"] = sweeps
        if track is not None:
            kw["track"] = track
        self.slots[i].stage(t & _SEQ_MASK, *args, **kw)    # a ValueError leaves the ticket unused and the slot free
        self.slots[i].launch()
        self.busy[i] = t
        self.next_ticket = t + 1
        return t

    def poll(self):
        """Harvest every frame whose record has arrived -> the tickets that collect() now returns without waiting."""
        for i in sorted(range(len(self.slots)), key=lambda j: self.busy[j] or 0):
            if self.busy[i] is not None and self.slots[i].ready():
                self._harvest(i)
        return sorted(self.done)

    def collect(self, ticket):
        if ticket not in self.done:
            if ticket not in self.busy:
                raise KeyError("ticket %r is unknown or was collected already" % (ticket,))
            self._harvest(self.busy.index(ticket))
        result, err = self.done.pop(ticket)
        if err is not None:
            raise err
        return result

    def drain(self):
        """Wait for everything in flight (oldest first); the results stay collectable."""
        for i in sorted(range(len(self.slots)), key=lambda j: self.busy[j] or 0):
            if self.busy[i] is not None:
                self._harvest(i)

    def map(self, batches):
        """(ticket, result) per batch of `batches`, in order, with at most len(slots) frames submitted and not yet yielded.
        A batch is a list of clouds, or the tuple (clouds, frustums) for a stream with raw_cap, or the tuple
        (clouds, frustums-or-None, calibs) for a stream with annos, or the tuple
        (clouds, frustums-or-None, calibs-or-None, sweeps) for a stream with sweeps, or the tuple
        (clouds, frustums-or-None, calibs-or-None, None, track) for a tracking stream without sweeps."""
        pending = deque()
        try:
            batches = iter(batches)
            while True:
                if len(pending) == len(self.slots):
                    t = pending.popleft()
                    yield t, self.collect(t)
                try:
                    clouds = next(batches)
                except StopIteration:
                    break
                if isinstance(clouds, tuple):           # (clouds, frustums[, calibs[, sweeps[, track]]])
                    pending.append(self.submit(*clouds))
                else:
                    pending.append(self.submit(clouds))
            while pending:
                t = pending.popleft()
                yield t, self.collect(t)
        finally:
            for t in pending:                           # left early (an error, a break): nothing stays in flight or parked
                try:
                    self.collect(t)
                except RuntimeError:
                    pass

    def close(self):
        if not self.closed:
            self.drain()
            self.closed = True
            for s in self.slots:
                fin = getattr(s, "close", None)
                if fin is not None:
                    fin()


class _PlanSlot:
    """One frame in flight: an InferencePlan captured with the seal as its last node, its HIP stream, the pinned host side
    of the plan's staging block (`stage_layout`: planes with raw_cap, calibration with annos, seq, counts), pinned clouds
    [B x points_cap x ndim f32], a pinned record buffer and the event behind the record's copy.
    With raw_cap the frame crops: the pinned clouds are [B x raw_cap x ndim f32], they go to plan.raw_in and the plan's
    first nodes cut them down to points_cap rows of plan.pts_in.  With annos the record is layout version 2.
    With `sweeps` -- dict(book=<SweepBook>, ring=<[B,R,sweep_cap,ndim] f32 device>, events=<one per ring slot>,
    time_feature=), shared by the stream's slots -- `ndim` is the width of a submitted sweep, the pinned clouds are
    [B x sweep_cap x ndim f32] and go into the ring slot the book names; the plan's first node merges the ring slots of
    the frame's descriptors into plan.pts_in (ndim + time_feature columns).
    With `track` -- dict(tracker=<sassd.track.Tracker>, book=<TrackBook>, events=<one per slot>, last=<the slot index of the
    previous ticket or None>), shared by the stream's slots -- the slot owns a pinned descriptor block, a device and a pinned
    track record, and launch() queues the tracker behind the frame (FrameStream, "Tracking")."""

    def __init__(self, plan, points_cap, ndim, raw_cap=None, annos=False, sweeps=None, track=None, index=0):
        import torch
        self.torch, self.plan = torch, plan
        dev, B = plan.dev, plan.b_user               # the clouds of a frame (a plan with tta runs more samples inside)
        self.stream = torch.cuda.Stream(device=dev)
        self.sw = sweeps
        kw = dict(annos=True) if annos else {}
        S, ndim_plan = 0, ndim
        if sweeps is not None:
            S, tf = sweeps["book"].S, bool(sweeps["time_feature"])
            kw["sweeps"] = dict(ring=sweeps["ring"], S=S, sweep_cap=sweeps["book"].sweep_cap, time_feature=tf)
            ndim_plan = int(ndim) + (1 if tf else 0)
        with torch.cuda.stream(self.stream):
            plan.capture(points_cap, ndim=ndim_plan, seal=True, raw_cap=raw_cap, **kw)
        self.stream.synchronize()
        self.cap, self.ndim = int(points_cap), int(ndim)
        self.raw_cap = None if raw_cap is None else int(raw_cap)
        self.annos = bool(annos)
        L = stage_layout(B, self.raw_cap is not None, self.annos, seal=True, **(dict(sweeps=S) if S else {}))
        self.pin_block = torch.zeros(L["total"], dtype=torch.uint8).pin_memory()     # the host side of plan._stage_block
        self.np_stage = stage_views(self.pin_block.numpy(), B, L)
        self.dev_pts, rows = (plan.pts_in, self.cap) if self.raw_cap is None else (plan.raw_in, self.raw_cap)
        if S:
            self.dev_pts, rows = None, sweeps["book"].sweep_cap      # the ring slot of the frame's sweep, chosen per frame
        self.pin_pts = torch.zeros(B, rows, self.ndim, dtype=torch.float32).pin_memory()
        self.pin_rec = torch.zeros(plan.record.numel(), dtype=torch.uint8).pin_memory()
        self.np_pts, self.np_rec = self.pin_pts.numpy(), self.pin_rec.numpy()
        self.event = torch.cuda.Event()
        self.feed = torch.cuda.Event()          # orders device-tensor clouds (produced on the caller's stream) before their copy
        self.trk, self.index = track, int(index)
        if track is not None:
            from .track import DESC_BYTES
            tracker = track["tracker"]
            self.pin_desc = torch.zeros(B * DESC_BYTES, dtype=torch.uint8).pin_memory()
            self.np_desc = self.pin_desc.numpy()
            self.dev_trk = tracker.new_record()     # the slot's own: the next ticket's step may run while this one is copied
            self.pin_trk = torch.zeros(tracker.record_bytes, dtype=torch.uint8).pin_memory()
            self.np_trk = self.pin_trk.numpy()

    def stage(self, seq, clouds, frustums=None, calibs=None, sweeps=None, track=None):
        torch, plan = self.torch, self.plan
        view = self.np_stage
        tplan = None
        if self.trk is not None or track is not None:
            from .track import track_items
            titems = track_items(self.trk is not None, self.sw is not None, sweeps, track)
        if self.sw is None:
            if sweeps is not None:
                raise ValueError("sweeps given to a stream built without sweeps= (its clouds are taken as they are)")
            checked = check_frame_inputs(clouds, frustums, plan.b_user, self.ndim, self.cap, self.raw_cap, calibs,
                                         self.annos)                                         # nothing is queued before this
            planes, calib = checked if self.annos else (checked, None)
            if self.trk is not None:
                tplan = self.trk["book"].plan(titems)                                        # the book is unchanged
            dev_pts = self.dev_pts
        else:
            if frustums is not None:
                raise ValueError("frustums given to a stream with sweeps (merged clouds are not cropped)")
            book = self.sw["book"]
            d = book.plan(clouds, sweeps)                                                    # nothing is queued before this,
            planes, calib = None, _check_calibs(calibs, None, plan.b_user, self.annos)            # and the book is unchanged
            if self.trk is not None:
                tplan = self.trk["book"].plan(titems)
            assert (d["k"] + 1) & _SEQ_MASK == seq      # ticket t carries sweep t - 1: frame t - inflight, the last reader of
            book.commit(d)                              # the ring slot written now, ran on this slot's stream
            for key in ("slot", "count", "xform", "T", "dt"):
                view["sweep_" + key][...] = d[key]
            dev_pts = [self.sw["ring"][b, d["write"]] for b in range(plan.b_user)]
        if tplan is not None:                           # every check has passed: the submit is accepted
            from .track import pack_desc
            self.trk["book"].commit(tplan)
            self.np_desc[...] = pack_desc(tplan)
        if planes is not None:
            view["planes"][...] = planes
        if calib is not None:
            view["calib"][...] = calib
        on_dev = [torch.is_tensor(p) and p.is_cuda for p in clouds]
        if any(on_dev):
            self.feed.record(torch.cuda.current_stream(plan.dev))
            self.stream.wait_event(self.feed)
        view["seq"][0] = seq
        with torch.cuda.stream(self.stream):
            for b, pts in enumerate(clouds):
                n = int(pts.shape[0])
                view["counts"][b] = n
                if n == 0:
                    continue
                if on_dev[b]:
                    dev_pts[b][:n].copy_(pts, non_blocking=True)
                    pts.record_stream(self.stream)      # the caller may drop the cloud now: its memory is not handed out
                                                        # again before this copy has run
                else:
                    self.np_pts[b, :n] = pts.numpy() if torch.is_tensor(pts) else pts
                    dev_pts[b][:n].copy_(self.pin_pts[b, :n], non_blocking=True)
            plan._stage_block.copy_(self.pin_block, non_blocking=True)
        if self.sw is not None:
            events = self.sw["events"]
            events[d["write"]].record(self.stream)      # the sweep is in the ring for the frames that read it later ...
            for r in d["reads"]:                        # ... and this frame reads sweeps other slots' streams uploaded
                self.stream.wait_event(events[r])

    def launch(self):
        torch = self.torch
        with torch.cuda.stream(self.stream):
            self.plan.graph.launch()
            self.pin_rec.copy_(self.plan.record, non_blocking=True)
            if self.trk is not None:
                self._launch_tracker()
            self.event.record(self.stream)              # last: it covers both records

    def _launch_tracker(self):
        """Behind the frame, on the slot's stream (the caller has made it current): wait for the previous ticket's step --
        it ran on another slot's stream when inflight > 1 --, copy the descriptors, step the stream's tracker on this plan's
        detections and status word, record the slot's track event, copy the record out."""
        trk, plan = self.trk, self.plan
        if trk["last"] is not None and trk["last"] != self.index:
            self.stream.wait_event(trk["events"][trk["last"]])
        trk["tracker"].step(plan.out, plan.status, self.pin_desc, seq=plan._seq, record=self.dev_trk)
        trk["events"][self.index].record(self.stream)
        trk["last"] = self.index
        self.pin_trk.copy_(self.dev_trk, non_blocking=True)

    def ready(self):
        return self.event.query()

    def wait(self):
        self.event.synchronize()

    def record(self):
        return self.np_rec if self.trk is None else (self.np_rec, self.np_trk)

    def recover(self):
        """InferencePlan's status word is sticky and the plan, its kernels and the seal leave it so.  The STREAM clears it, and
        only here: after a frame whose record carried a flag (that frame's collect() raises it), on the slot's stream, in
        front of the slot's next frame -- so that the flag is reported once, by its ticket, and later tickets start clean."""
        with self.torch.cuda.stream(self.stream):
            self.plan.status.fill_(0)

    def close(self):
        self.stream.synchronize()


class FrameStream:
    """`inflight` frames in flight over `inflight` InferencePlans, each captured once with the frame seal as its last node,
    each on its own HIP stream (and no other stream: with inflight > 1 the plans are one-branch, overlap=False; inflight == 1
    keeps the default two-branch plan, which is the faster form for a frame that runs alone -- INTEGRATION section 6).

    submit(clouds) -> ticket; collect(ticket) -> per sample (boxes, scores, labels) exactly as plan.results() returns them;
    map(batches) yields (ticket, detections) in order and keeps `inflight` frames queued; poll() harvests what has arrived;
    drain() waits for everything in flight; close() drains and ends the stream.  `clouds` is a list of batch_size point clouds
    [N, ndim] f32: numpy arrays / CPU tensors (copied through the pinned staging block) or device tensors (copied on the
    slot's stream, after the work queued on the caller's current stream).  Lifetime: a host cloud has been copied out when
    submit() returns; a device cloud is read by a copy that may still be pending then -- the caller may DROP it at once (it is
    recorded on the slot's stream, so the allocator keeps its memory until the copy has run) but must not WRITE into it before
    the ticket has been collected.  A cloud of more than points_cap points raises
    ValueError at submit, before anything is queued.  With `raw_cap` the stream takes raw sweeps of up to raw_cap points:
    every submit needs `frustums`, one per cloud -- a [6,4] float64 plane array (geometry.frustum_planes) or
    dict(calib=..., img_shape=...) (frustum_of) -- the frame crops each cloud to its frustum on the GPU, in order, and
    detects on the kept points exactly as if they had been submitted to a stream without raw_cap; a frame that keeps more
    than points_cap points raises FrameStatusError with SASSD_ST_POINT_OVERFLOW (16) from its collect().  A cloud above
    raw_cap, missing / miscounted frustums, planes that are not [6,4] float64 or not finite, and frustums given to a stream
    without raw_cap raise ValueError at submit, before anything is queued.  With `annos=True` the frame
    also writes the KITTI result annotation of its detections (include/sassd.h "KITTI annotations"):
    submit(clouds, frustums, calibs) takes one dict(calib=<kitti_common.Calibration or dict of P2 / R0_rect /
    Tr_velo_to_cam>, img_shape=(h, w[, c])) per cloud -- on a raw stream whose frustums are such dicts, calibs defaults to
    them -- and collect() returns per sample (boxes, scores, labels, cam), cam as decode_record(annos=True) documents it
    (kitti_common.result_anno_from_cam builds the annotation from it).  Missing / miscounted calibs, a non-finite matrix, a
    non-positive image size, and calibs given to a stream without annos raise ValueError at submit, before anything is
    queued.  A frame whose status word is not zero raises plan.results()'s
    RuntimeError from ITS collect(); a record that is not the ticket's own raises RuntimeError("stale frame record").
    `plans` are the InferencePlans (for tools); plan_kwargs go to InferencePlan (precision, sparse_precision, ...).

    Multi-sweep clouds: FrameStream(..., sweeps=S, sweep_cap=N, time_feature=True) detects on the current sweep plus the up
    to S-1 sweeps before it, each moved into the current sensor frame by the ego pose (include/sassd.h "Multi-sweep merge",
    one kernel per sample in front of the voxelizer).  `ndim` is then the width of a SUBMITTED sweep; the detector reads
    ndim + 1 columns with time_feature (the last one the time lag in seconds, 0 for the current sweep).  Each sample index
    is its own sensor sequence.  submit(clouds, sweeps=[dict(pose=<4x4 f64 sensor-to-world>, time=<seconds>,
    first=<bool, default False>), ...]) takes the NEW sweep of every sample only, [n <= sweep_cap, ndim]: it crosses the bus
    once, into the stream's device ring [B, R, sweep_cap, ndim], R = S + inflight - 1, at slot k % R for the k-th submit, and
    stays there while later frames read it.  The frame's descriptors list the current sweep first (copied bit for bit),
    then the earlier sweeps of the sequence, newest first, with T = sweep_transform(pose_now, pose_then) and
    dt = float32(time_now - time_then); first=True starts a new sequence for that sample.  points_cap bounds the MERGED
    cloud: a frame above it raises FrameStatusError with SASSD_ST_POINT_OVERFLOW (16) from its collect(), and its sweep
    stays in the ring for the frames after it.  Missing / miscounted sweeps, a pose that is not a finite 4x4 matrix, a
    non-finite time, a cloud above sweep_cap or of another width, frustums given to such a stream, and sweeps= given to a
    stream built without it raise ValueError at submit, before anything is queued and with the sequence unchanged.
    sweeps excludes raw_cap; annos composes with it unchanged.
    Ordering: a sweep is uploaded on the stream of the slot whose frame brings it, and an event per ring slot is recorded
    behind the upload.  (1) read after write: before its graph is launched, a frame's stream waits on the events of the
    earlier sweeps it reads -- other slots' streams uploaded them.  (2) write after read: sweep k overwrites the ring slot
    of sweep k - R; the last frame that read that one is the frame of sweep k - R + S - 1 = k - inflight, ticket
    t - inflight, which ran on this same slot and stream, so stream order covers it; the frames that may still run on the
    other streams, tickets t - inflight + 1 .. t - 1, read no sweep older than k - R + 1.  This holds because every ticket
    writes exactly one sweep (a refused submit uses neither) -- the slot asserts it.

    Test-time augmentation: FrameStream(..., tta=[(0, 0.0, 1.0), (1, 0.0, 1.0), ...]) -- 1..8 views (flip, angle, scale), the
    first the identity (sassd.tta) -- detects on every view of every cloud inside the captured frame and suppresses the
    candidates of a cloud's views together (InferencePlan(tta=...); include/sassd.h "Test-time augmentation").  submit and
    collect are unchanged: batch_size clouds in, batch_size result sets out; the views are fixed for the life of the
    stream.  Composes with raw_cap, annos, sweeps, precision and sparse_precision: the views are made from the cropped /
    merged cloud.  A malformed spec raises ValueError here, before anything is allocated.

    Box fusion: FrameStream(..., fuse_iou=0.7) ends every frame's rescore / NMS with sassd_box_fuse (InferencePlan(fuse_iou=...);
    include/sassd.h "Box fusion"; sassd.fuse): the boxes of the record and of the annotations are the score-weighted means of
    the candidates each detection stands for -- of all views under tta -- while scores, labels, counts and order are those of
    the stream without it.  None (default) leaves the frame as it was.  Composes with tta, raw_cap, annos, sweeps, precision
    and sparse_precision.  A value outside (0, 1) raises ValueError here, before anything is allocated.

    Tracking: FrameStream(..., track=dict(max_dist=2.0 | one per label, max_age=3, alpha=0.5, cap=256, birth_score=0.0)) keeps
    the tracks of every sample in device memory for the life of the stream and steps them behind every frame with ONE kernel,
    sassd_track_step (include/sassd.h "Tracking"; sassd.track.track_host states it): greedy centre-distance association in the
    detector's order, a velocity per track, tracks that coast for up to max_age frames.  The kernel is launched OUTSIDE the
    captured graph, on the slot's stream behind graph.launch(), because its state is shared between the plans; it reads that
    plan's `out` and `status`.  Order per ticket: wait on the track event of the previous ticket (another slot's stream when
    inflight > 1), copy the descriptors, step, record the slot's track event, copy the track record to a pinned buffer; the
    slot's completion event comes last and covers both records.  Pose and time: on a stream with sweeps= those of the sweep
    dicts, `first` included -- nothing new is passed; on any other stream submit(clouds, ..., track=[dict(time=<seconds>,
    pose=<4x4 f64 sensor-to-world or None>, first=<bool>), ...]), one per cloud.  The host keeps the previous pose and time per
    sample (sassd.track.TrackBook) and commits them only when the submit is accepted; a sample's first frame and a frame with
    first=True reset its tracks (ids are never reused).  collect() appends one element per sample, trk = dict(ids, vel, hits,
    dropped, coast=dict(ids, labels, boxes, vel, misses, scores)): ids / vel / hits per detection, `coast` the tracks alive but
    not seen in this frame, at their predicted places; everything before it is byte for byte what the stream without track=
    returns.  A frame whose status word is not zero raises from its collect() as ever; its step only carried the tracks into
    its sensor frame.  A missing or miscounted track=, a non-finite time, a pose that is not a finite 4x4 matrix, track= next
    to sweeps=, and track= given to a stream built without it raise ValueError at submit, before anything is queued and with
    the book unchanged.  Composes with raw_cap, annos, sweeps, tta, fuse_iou and the precisions: the tracker reads whatever
    plan.out is.  A malformed spec raises ValueError here, before anything is allocated."""

    def __init__(self, state_dict, inflight=3, points_cap=None, batch_size=1, anchors=None, device=None, ndim=4,
                 raw_cap=None, annos=False, sweeps=None, sweep_cap=None, time_feature=True, tta=None, fuse_iou=None,
                 track=None, **plan_kwargs):
        from .pipeline import InferencePlan, input_features_of
        if track is not None:
            from .track import check_track
            track = check_track(track)
        if fuse_iou is not None:
            from .fuse import check_fuse_iou
            fuse_iou = check_fuse_iou(fuse_iou)
        cin = input_features_of(state_dict)
        if tta is not None:
            from .tta import check_views
            tta = check_views(tta)
        if sweeps is not None:
            if not 1 <= int(sweeps) <= MAX_SWEEPS:
                raise ValueError("sweeps must be 1..%d, got %d" % (MAX_SWEEPS, int(sweeps)))
            if raw_cap is not None:
                raise ValueError("sweeps and raw_cap exclude each other: merged clouds are not cropped")
            if sweep_cap is None or int(sweep_cap) < 1:
                raise ValueError("sweep_cap (the largest sweep the stream accepts) is required with sweeps")
            if int(ndim) < 3:
                raise ValueError("a sweep has at least x, y, z: FrameStream(ndim=%d)" % int(ndim))
        ndim_plan = int(ndim) + (1 if sweeps is not None and time_feature else 0)
        if ndim_plan < cin:
            raise ValueError("the detector reads %d features per point: FrameStream(ndim=%d) is too narrow" % (cin, ndim_plan))
        inflight = int(inflight)
        if not 1 <= inflight <= MAX_INFLIGHT:
            raise ValueError("inflight must be 1..%d, got %d" % (MAX_INFLIGHT, inflight))
        if points_cap is None or int(points_cap) < 1:
            raise ValueError("points_cap (the largest cloud the stream accepts) is required")
        if "overlap" in plan_kwargs:
            raise ValueError("FrameStream chooses `overlap` itself: one-branch plans in flight, the two-branch plan alone")
        if raw_cap is not None and int(raw_cap) < 1:
            raise ValueError("raw_cap (the largest raw sweep the stream accepts) must be >= 1")
        self.inflight, self.points_cap, self.batch_size = inflight, int(points_cap), int(batch_size)
        self.raw_cap = None if raw_cap is None else int(raw_cap)
        self.annos = bool(annos)
        self.plans = [InferencePlan(state_dict, batch_size=batch_size, anchors=anchors, device=device,
                                    overlap=inflight == 1, **({} if tta is None else dict(tta=tta)),
                                    **({} if fuse_iou is None else dict(fuse_iou=fuse_iou)), **plan_kwargs)
                      for _ in range(inflight)]
        B, capD = self.plans[0].b_user, self.plans[0].capD
        self.sweeps = None if sweeps is None else int(sweeps)
        extra = {}
        if self.sweeps is not None:
            import torch
            R = self.sweeps + inflight - 1              # class docstring, "Ordering"
            self.sweep_cap, self.time_feature = int(sweep_cap), bool(time_feature)
            self.sweep_ring = torch.zeros(B, R, self.sweep_cap, int(ndim), dtype=torch.float32, device=self.plans[0].dev)
            self._book = SweepBook(B, self.sweeps, R, self.sweep_cap, ndim, inflight)
            extra["sweeps"] = dict(book=self._book, ring=self.sweep_ring, time_feature=self.time_feature,
                                   events=[torch.cuda.Event() for _ in range(R)])
        self.track = track
        if track is None:
            self._slots = [_PlanSlot(p, self.points_cap, ndim, self.raw_cap, self.annos, **extra) for p in self.plans]
            self._ring = FrameRing(self._slots, lambda rec, seq: decode_record(rec, B, capD, seq, self.annos))
            return
        import torch
        from .track import Tracker, TrackBook, decode_track_record, results_of
        self.tracker = Tracker(B, capD, self.plans[0].dev, **track)
        self._track_book = TrackBook(B)
        extra["track"] = dict(tracker=self.tracker, book=self._track_book, last=None,
                              events=[torch.cuda.Event() for _ in range(inflight)])
        self._slots = [_PlanSlot(p, self.points_cap, ndim, self.raw_cap, self.annos, index=i, **extra)
                       for i, p in enumerate(self.plans)]
        cap = self.tracker.cap

        def decode(rec, seq):
            dets = decode_record(rec[0], B, capD, seq, self.annos)      # raises the frame's status error
            trk = decode_track_record(rec[1], B, capD, cap, seq)
            return [tuple(d) + (results_of(trk, b),) for b, d in enumerate(dets)]
        self._ring = FrameRing(self._slots, decode)

    def submit(self, clouds, frustums=None, calibs=None, sweeps=None, track=None):
        kw = {} if sweeps is None else dict(sweeps=sweeps)
        if track is not None:
            kw["track"] = track
        return self._ring.submit(clouds, frustums, calibs, **kw)

    def collect(self, ticket):
        return self._ring.collect(ticket)

    def map(self, batches):
        return self._ring.map(batches)

    def poll(self):
        return self._ring.poll()

    def drain(self):
        self._ring.drain()

    def close(self):
        self._ring.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
