"""Tracking: the switch, the per-frame descriptor, the device record, and the numpy statement of the rule (include/sassd.h
"Tracking"; csrc/track_core.h).

FrameStream(track=dict(max_dist=2.0, max_age=3, alpha=0.5, cap=256, birth_score=0.0)) launches sassd_track_step behind every
frame: a greedy centre-distance tracker of the CenterPoint kind, one kernel per frame, the tracks of every sample in device
memory for the life of the stream.  Every detection gets a track id, a velocity (m/s, sensor frame) and a hit count; the
tracks that were not seen in a frame coast at their predicted places.  `track_host` states what the kernel computes, float64
operation by float64 operation; the tests hold the kernel to it bit for bit.  The host's part of a frame is the descriptor
(`TrackBook`): the transform of the previous sensor frame into the current one, its yaw, the time step and the reset flag --
the kernel needs no trigonometry.

A tracker state is dict(slots [B, cap, SLOT_WORDS] int32, next_id [B] int32): slot words id | label | box[7] f32 | vel[2] f32 |
hits | misses | score f32 (`slot_fields` gives typed views), id -1 for a free slot."""
import numpy as np

SLOT_WORDS = 14                     # SASSD_TRACK_SLOT_WORDS
ID, LABEL, BOX, VEL, HITS, MISSES, SCORE = 0, 1, 2, 9, 11, 12, 13
MAX_CAP, MAX_LABELS, MAX_CAP_D, MAX_HITS = 1024, 8, 16384, 1 << 30
TRACK_MAGIC = 0x53540001            # SASSD_TRACK_MAGIC: 'S' 'T', layout version 1
HEADER_WORDS = 8                    # SASSD_TRACK_HEADER_WORDS
DESC_DTYPE = np.dtype([("T", "<f8", (12,)), ("dyaw", "<f8"), ("dt", "<f8"), ("flags", "<i4"), ("pad", "<i4")])
DESC_BYTES = 120                    # SASSD_TRACK_DESC_BYTES
assert DESC_DTYPE.itemsize == DESC_BYTES
_SEQ_MASK = 0x7FFFFFFF
_DEFAULTS = dict(max_dist=2.0, max_age=3, alpha=0.5, cap=256, birth_score=0.0)


def _number(name, v):
    if isinstance(v, (bool, np.bool_, str, bytes)) or v is None:
        raise ValueError("track: %s must be a number, got %r" % (name, v))
    try:
        return float(v)
    except (TypeError, ValueError):
        raise ValueError("track: %s must be a number, got %r" % (name, v)) from None


def _integer(name, v):
    f = _number(name, v)
    if not np.isfinite(f) or f != int(f):
        raise ValueError("track: %s must be an integer, got %r" % (name, v))
    return int(f)


def check_track(spec):
    """The switch, normalised: None (off), or dict(max_dist=, max_age=, alpha=, cap=, birth_score=) with every key optional ->
    dict(max_dist=<tuple of 1..8 floats, one per label, as float32 holds them; a scalar stands for all 8 labels>, max_age=<int
    >= 0>, alpha=<float in (0, 1]>, cap=<int 1..1024>, birth_score=<float, as float32 holds it>).  ValueError for anything else:
    not a dict, an unknown key, a bool / string / NaN where a number belongs, a negative or infinite max_dist, more than 8 of
    them or none, a negative or fractional max_age, alpha outside (0, 1], cap outside 1..1024, a NaN birth_score."""
    if spec is None:
        return None
    if not isinstance(spec, dict):
        raise ValueError("track must be a dict(max_dist=, max_age=, alpha=, cap=, birth_score=) or None, got %r" % (spec,))
    unknown = sorted(set(spec) - set(_DEFAULTS))
    if unknown:
        raise ValueError("track: unknown key(s) %s (known: %s)" % (unknown, sorted(_DEFAULTS)))
    s = dict(_DEFAULTS, **spec)
    md = s["max_dist"]
    if isinstance(md, (list, tuple, np.ndarray)):
        md = [_number("max_dist", v) for v in (md.tolist() if isinstance(md, np.ndarray) else md)]
        if not 1 <= len(md) <= MAX_LABELS:
            raise ValueError("track: max_dist takes 1..%d values, one per label, got %d" % (MAX_LABELS, len(md)))
    else:
        md = [_number("max_dist", md)] * MAX_LABELS
    with np.errstate(over="ignore"):
        md = tuple(float(np.float32(v)) for v in md)
    if not all(np.isfinite(v) and v >= 0.0 for v in md):
        raise ValueError("track: max_dist must be finite and >= 0, got %r" % (s["max_dist"],))
    max_age = _integer("max_age", s["max_age"])
    if not 0 <= max_age < (1 << 30):
        raise ValueError("track: max_age must be >= 0, got %r" % (s["max_age"],))
    alpha = _number("alpha", s["alpha"])
    if not 0.0 < alpha <= 1.0:
        raise ValueError("track: alpha must lie in (0, 1], got %r" % (s["alpha"],))
    cap = _integer("cap", s["cap"])
    if not 1 <= cap <= MAX_CAP:
        raise ValueError("track: cap must be 1..%d slots per sample, got %r" % (MAX_CAP, s["cap"]))
    birth = _number("birth_score", s["birth_score"])
    if np.isnan(birth):
        raise ValueError("track: birth_score must not be NaN")
    with np.errstate(over="ignore"):
        birth = float(np.float32(birth))
    return dict(max_dist=md, max_age=max_age, alpha=alpha, cap=cap, birth_score=birth)


# ---- the state ----------------------------------------------------------------------------------------------------------------
def empty_state(B, cap):
    """A tracker state without tracks: every slot free, next_id 0."""
    slots = np.zeros((int(B), int(cap), SLOT_WORDS), np.int32)
    slots[:, :, ID] = -1
    return dict(slots=slots, next_id=np.zeros(int(B), np.int32))


def slot_fields(slots):
    """Typed VIEWS into slots [..., SLOT_WORDS] int32: dict(id, label, box [..., 7] f32, vel [..., 2] f32, hits, misses, score)."""
    f = slots.view(np.float32)
    return dict(id=slots[..., ID], label=slots[..., LABEL], box=f[..., BOX:BOX + 7], vel=f[..., VEL:VEL + 2],
                hits=slots[..., HITS], misses=slots[..., MISSES], score=f[..., SCORE])


# ---- the descriptor -----------------------------------------------------------------------------------------------------------
def identity_desc(B, reset=False):
    """The descriptors of a frame without ego motion and without time: T = [I|0], dyaw = 0, dt = 0; `reset` sets flag bit 0."""
    T = np.zeros((int(B), 3, 4))
    T[:, :, :3] = np.eye(3)
    return dict(T=T, dyaw=np.zeros(int(B)), dt=np.zeros(int(B)), flags=np.full(int(B), 1 if reset else 0, np.int32))


def pack_desc(desc):
    """dict(T [B,3,4] f64, dyaw [B] f64, dt [B] f64, flags [B] i32) -> the B descriptors of sassd_track_step as one uint8 array
    of B * DESC_BYTES bytes."""
    T = np.asarray(desc["T"], np.float64)
    B = T.shape[0]
    if T.shape != (B, 3, 4):
        raise ValueError("track descriptor: T must be [B, 3, 4], got %s" % (T.shape,))
    out = np.zeros(B, DESC_DTYPE)
    out["T"] = T.reshape(B, 12)
    out["dyaw"], out["dt"] = np.asarray(desc["dyaw"], np.float64).reshape(B), np.asarray(desc["dt"], np.float64).reshape(B)
    out["flags"] = np.asarray(desc["flags"], np.int32).reshape(B)
    return out.view(np.uint8).reshape(-1)


def track_items(tracking, has_sweeps, sweeps, track):
    """Which per-cloud dicts carry a frame's pose and time for the tracker.  On a stream with sweeps= they are the sweep
    dicts (nothing new is passed); on any other tracking stream submit(..., track=[dict(time=, pose=None, first=False), ...]).
    ValueError: track= given to a stream built without it, track= given next to sweeps=, a missing track=."""
    if not tracking:
        if track is not None:
            raise ValueError("track= given to a stream built without track= (its frames carry no identities)")
        return None
    if has_sweeps:
        if track is not None:
            raise ValueError("a stream with sweeps tracks by the pose and time of its sweep dicts: track= must not be given")
        return sweeps
    if track is None:
        raise ValueError("a stream with track= needs submit(clouds, ..., track=[dict(time=, pose=None, first=False), ...]), "
                         "one per cloud")
    return track


class TrackBook:
    """The host bookkeeping of a tracking stream: the pose and time of every sample's previous frame.  `plan` checks one
    frame's items and returns its descriptors WITHOUT changing the book; `commit` makes them the book's state -- a refused
    submit leaves no trace (as SweepBook).  A sample's first frame, and a frame with first=True, carries the reset flag."""

    def __init__(self, B):
        self.B = int(B)
        self.prev = [None] * self.B                     # per sample (pose or None, time) of the frame before

    def plan(self, items):
        from .stream import sweep_transform
        B = self.B
        if items is None or isinstance(items, dict) or not hasattr(items, "__len__"):
            raise ValueError("tracking needs one dict(time=, pose=None, first=False) per cloud")
        if len(items) != B:
            raise ValueError("%d track descriptions for a stream of batch_size %d" % (len(items), B))
        d = identity_desc(B)
        d["prev"] = []
        for b, it in enumerate(items):
            if not isinstance(it, dict) or it.get("time") is None:
                raise ValueError("track %d: a dict with `time` is needed" % b)
            try:
                time = float(it["time"])
            except (TypeError, ValueError):
                raise ValueError("track %d: time must be a finite number" % b) from None
            if not np.isfinite(time):
                raise ValueError("track %d: time must be finite" % b)
            pose = it.get("pose")
            if pose is not None:
                try:
                    pose = np.array(pose, dtype=np.float64)
                except (TypeError, ValueError):
                    raise ValueError("track %d: pose must be a finite 4x4 matrix" % b) from None
                if pose.shape != (4, 4) or not np.isfinite(pose).all():
                    raise ValueError("track %d: pose must be a finite 4x4 matrix" % b)
            before = self.prev[b]
            if before is None or bool(it.get("first", False)):
                d["flags"][b] = 1
            else:
                if pose is not None and before[0] is not None:
                    d["T"][b] = sweep_transform(pose, before[0])
                d["dyaw"][b] = np.arctan2(d["T"][b, 1, 0], d["T"][b, 0, 0])
                d["dt"][b] = time - before[1]
            d["prev"].append((pose, time))
        return d

    def commit(self, d):
        self.prev = list(d["prev"])


# ---- the record ---------------------------------------------------------------------------------------------------------------
def track_record_layout(B, capD, cap):
    """Byte offsets of the track record for `B` samples x `capD` detection rows x `cap` slots (include/sassd.h "Tracking"):
    dict(magic, seq, status, B, capD, cap, count, dropped, next_id, det_id, det_hits, det_vel, slots, total), in this order,
    every field 4-byte aligned: eight header words, count / dropped / next_id [B] i32, det_id / det_hits [B, capD] i32,
    det_vel [B, capD, 2] f32, slots [B, cap, SLOT_WORDS]."""
    B, capD, cap = int(B), int(capD), int(cap)
    if not (1 <= B <= 65535 and 1 <= capD <= MAX_CAP_D and 1 <= cap <= MAX_CAP):
        raise ValueError("no track record for batch %d x capD %d x cap %d" % (B, capD, cap))
    n = B * capD
    count = 4 * HEADER_WORDS
    L = dict(magic=0, seq=4, status=8, B=12, capD=16, cap=20, count=count, dropped=count + 4 * B, next_id=count + 8 * B)
    L["det_id"] = count + 12 * B
    L["det_hits"] = L["det_id"] + 4 * n
    L["det_vel"] = L["det_hits"] + 4 * n
    L["slots"] = L["det_vel"] + 8 * n
    L["total"] = L["slots"] + 4 * B * cap * SLOT_WORDS
    return L


def decode_track_record(buf, B, capD, cap, seq=None):
    """One track record (bytes-like / uint8 array) -> dict(status, count [B], dropped [B], next_id [B], det_id [B, capD] i32,
    det_hits [B, capD] i32, det_vel [B, capD, 2] f32, slots [B, cap, SLOT_WORDS] i32), all copies.  RuntimeError("stale track
    record") unless it carries the magic word, this B / capD / cap and -- when `seq` is given -- that seq word."""
    L = track_record_layout(B, capD, cap)
    if memoryview(buf).nbytes < L["total"]:
        raise RuntimeError("stale track record")
    raw = np.frombuffer(buf, dtype=np.uint8, count=L["total"])
    w = raw.view(np.int32)
    if (int(w[0]) != TRACK_MAGIC or int(w[3]) != B or int(w[4]) != capD or int(w[5]) != cap
            or (seq is not None and int(w[1]) != (int(seq) & _SEQ_MASK))):
        raise RuntimeError("stale track record")
    n = B * capD

    def words(key, count, *shape):
        return w[L[key] // 4:L[key] // 4 + count].reshape(*shape).copy()
    return dict(status=int(w[2]), seq=int(w[1]), count=words("count", B, B), dropped=words("dropped", B, B),
                next_id=words("next_id", B, B), det_id=words("det_id", n, B, capD), det_hits=words("det_hits", n, B, capD),
                det_vel=words("det_vel", 2 * n, B, capD, 2).view(np.float32), slots=words("slots", B * cap * SLOT_WORDS, B, cap, SLOT_WORDS))


def encode_track_record(state, out, B, capD, cap, seq=0, status=0):
    """The record sassd_track_step writes for the state and the outputs of track_host: the bytes of track_record_layout."""
    L = track_record_layout(B, capD, cap)
    rec = np.zeros(L["total"], np.uint8)
    w = rec.view(np.int32)
    w[:HEADER_WORDS] = [TRACK_MAGIC, int(seq) & _SEQ_MASK, int(status), B, capD, cap, 0, 0]
    for key, src in (("count", out["count"]), ("dropped", out["dropped"]), ("next_id", state["next_id"]),
                     ("det_id", out["det_id"]), ("det_hits", out["det_hits"]),
                     ("det_vel", np.ascontiguousarray(out["det_vel"], np.float32).view(np.int32)), ("slots", state["slots"])):
        flat = np.ascontiguousarray(src, dtype=np.int32).reshape(-1)
        w[L[key] // 4:L[key] // 4 + flat.size] = flat
    return rec


def results_of(rec, b):
    """Sample b of a decoded record -> the `trk` element FrameStream.collect() appends: dict(ids i32 [k], vel f32 [k, 2], hits
    i32 [k], dropped int, coast=dict(ids, labels, boxes [m, 7], vel [m, 2], misses, scores)) -- k the frame's detection count,
    coast the m tracks that are alive but were not seen in this frame (id >= 0, misses > 0), at their predicted places."""
    k = int(rec["count"][b])
    f = slot_fields(rec["slots"][b])
    c = np.flatnonzero((f["id"] >= 0) & (f["misses"] > 0))
    return dict(ids=rec["det_id"][b, :k].copy(), vel=rec["det_vel"][b, :k].copy(), hits=rec["det_hits"][b, :k].copy(),
                dropped=int(rec["dropped"][b]),
                coast=dict(ids=f["id"][c].copy(), labels=f["label"][c].copy(), boxes=f["box"][c].copy(), vel=f["vel"][c].copy(),
                           misses=f["misses"][c].copy(), scores=f["score"][c].copy()))


# ---- the statement ------------------------------------------------------------------------------------------------------------
def track_host(state, det, desc, params, status=0):
    """One step of sassd_track_step in numpy -> (state, outputs).

    state: dict(slots [B, cap, SLOT_WORDS] i32, next_id [B] i32) -- not modified.  det: dict(boxes [B, capD, 7] f32, scores
    [B, capD] f32, labels [B, capD] i32, counts [B]).  desc: dict(T [B, 3, 4] f64, dyaw [B], dt [B], flags [B]) (TrackBook.plan /
    identity_desc).  params: a track spec (check_track).  status: the pipeline status word the step sees.
    outputs: dict(det_id [B, capD] i32, det_hits [B, capD] i32, det_vel [B, capD, 2] f32, dropped [B] i32, count [B] i32)."""
    p = check_track(dict(params))
    slots = np.array(state["slots"], dtype=np.int32, order="C", copy=True)
    next_id = np.array(state["next_id"], dtype=np.int32, copy=True)
    boxes = np.ascontiguousarray(det["boxes"], dtype=np.float32)
    scores = np.ascontiguousarray(det["scores"], dtype=np.float32)
    labels = np.asarray(det["labels"])
    B, cap = slots.shape[:2]
    capD = boxes.shape[1]
    if slots.shape != (B, cap, SLOT_WORDS) or boxes.shape != (B, capD, 7) or cap != p["cap"]:
        raise ValueError("slots must be [B, cap = %d, %d] and boxes [B, capD, 7], got %s and %s"
                         % (p["cap"], SLOT_WORDS, slots.shape, boxes.shape))
    counts = np.asarray(det["counts"], np.int64).reshape(B)
    out = dict(det_id=np.full((B, capD), -1, np.int32), det_hits=np.zeros((B, capD), np.int32),
               det_vel=np.zeros((B, capD, 2), np.float32), dropped=np.zeros(B, np.int32), count=np.zeros(B, np.int32))
    f64 = np.float64
    gates = [f64(np.float32(m)) * f64(np.float32(m)) for m in p["max_dist"]]
    alpha, birth = f64(p["alpha"]), np.float32(p["birth_score"])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for b in range(B):
            s = slot_fields(slots[b])
            T, dyaw, dt = np.asarray(desc["T"][b], f64), f64(desc["dyaw"][b]), f64(desc["dt"][b])
            if int(desc["flags"][b]) & 1:                                   # 1 reset
                s["id"][:] = -1
            live = np.flatnonzero(s["id"] >= 0)
            if len(live):                                                   # 2 predict
                x, y, z = (s["box"][live, q].astype(f64) for q in range(3))
                vx, vy = s["vel"][live, 0].astype(f64), s["vel"][live, 1].astype(f64)
                px, py, pz = x + vx * dt, y + vy * dt, z
                for q in range(3):
                    s["box"][live, q] = (((T[q, 0] * px + T[q, 1] * py) + T[q, 2] * pz) + T[q, 3]).astype(np.float32)
                s["box"][live, 6] = (s["box"][live, 6].astype(f64) + dyaw).astype(np.float32)
                s["vel"][live, 0] = (T[0, 0] * vx + T[0, 1] * vy).astype(np.float32)
                s["vel"][live, 1] = (T[1, 0] * vx + T[1, 1] * vy).astype(np.float32)
            if int(status) != 0:
                continue
            D = int(min(max(counts[b], 0), capD))
            out["count"][b] = D
            matched = np.zeros(cap, bool)
            slot_of = np.full(D, -1, np.int64)
            for d in range(D):                                              # 3 associate
                label = int(labels[b, d])
                if not 0 <= label < len(gates):
                    continue
                dx = f64(boxes[b, d, 0]) - s["box"][:, 0].astype(f64)
                dy = f64(boxes[b, d, 1]) - s["box"][:, 1].astype(f64)
                c = dx * dx + dy * dy
                ok = (s["id"] >= 0) & ~matched & (s["label"] == label) & (c <= gates[label])
                if not ok.any():
                    continue
                i = int(np.argmin(np.where(ok, c, np.inf)))                 # the first of the least: the lowest slot
                g = f64(1.0) if int(s["hits"][i]) == 1 else alpha           # 4 update
                if np.isfinite(dt) and dt > 0:
                    for q in range(2):
                        r = (f64(boxes[b, d, q]) - f64(s["box"][i, q])) / dt
                        s["vel"][i, q] = np.float32(f64(s["vel"][i, q]) + g * r)
                s["box"][i] = boxes[b, d]
                s["score"][i] = scores[b, d]
                s["hits"][i] = min(int(s["hits"][i]) + 1, MAX_HITS)
                s["misses"][i] = 0
                matched[i], slot_of[d] = True, i
            for i in np.flatnonzero((s["id"] >= 0) & ~matched):             # 5 age
                s["misses"][i] += 1
                if s["misses"][i] > p["max_age"]:
                    s["id"][i] = -1
            for d in range(D):                                              # 6 births
                if slot_of[d] >= 0 or not scores[b, d] >= birth:
                    continue
                free = np.flatnonzero(s["id"] < 0)
                if not len(free):
                    out["dropped"][b] += 1
                    continue
                i = int(free[0])
                s["id"][i], s["label"][i] = next_id[b], labels[b, d]
                next_id[b] = (int(next_id[b]) + 1 + (1 << 31)) % (1 << 32) - (1 << 31)      # the kernel's 32-bit add
                s["box"][i], s["vel"][i], s["score"][i] = boxes[b, d], 0.0, scores[b, d]
                s["hits"][i], s["misses"][i] = 1, 0
                slot_of[d] = i
            for d in np.flatnonzero(slot_of >= 0):
                i = slot_of[d]
                out["det_id"][b, d], out["det_hits"][b, d], out["det_vel"][b, d] = s["id"][i], s["hits"][i], s["vel"][i]
    return dict(slots=slots, next_id=next_id), out


# ---- the device side ----------------------------------------------------------------------------------------------------------
class Tracker:
    """The device state of one tracker -- slots [B, cap, SLOT_WORDS] i32 and next_id [B] i32 -- its descriptor block and its
    record buffer.  step() copies one frame's descriptors and launches sassd_track_step on the detection buffers `det`
    (dict(boxes, scores, labels, counts), e.g. InferencePlan.out) and the status word `status`; the record is `self.record`
    (decode_track_record reads it) unless another buffer is named.  reset() frees every slot; ids are not reused."""

    def __init__(self, B, capD, device, **spec):
        import torch
        self.params = check_track(spec)
        self.B, self.capD, self.cap, self.dev = int(B), int(capD), self.params["cap"], device
        L = track_record_layout(self.B, self.capD, self.cap)           # ValueError for shapes the kernel refuses
        self.record_bytes = L["total"]
        self.slots = torch.zeros(self.B, self.cap, SLOT_WORDS, dtype=torch.int32, device=device)
        self.slots[:, :, ID] = -1
        self.next_id = torch.zeros(self.B, dtype=torch.int32, device=device)
        self.desc = torch.zeros(self.B * DESC_BYTES, dtype=torch.uint8, device=device)
        self.seq = torch.zeros(1, dtype=torch.int32, device=device)
        self.record = self.new_record()

    def new_record(self):
        import torch
        return torch.zeros(self.record_bytes, dtype=torch.uint8, device=self.dev)

    def step(self, det, status, desc, stream=None, seq=None, record=None):
        """desc: the frame's descriptors as a dict (TrackBook.plan / identity_desc) or as a uint8 tensor of B * DESC_BYTES bytes
        (pack_desc; a pinned one is copied asynchronously).  stream: the torch stream to queue on (default: the current one).
        seq: a device int32 word for the record's header (default: a zero word).  -> the record buffer written."""
        import contextlib
        import torch
        from . import kernels as K
        if isinstance(desc, dict):
            desc = torch.from_numpy(pack_desc(desc))
        record = self.record if record is None else record
        with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            self.desc.copy_(desc, non_blocking=bool(desc.is_pinned()))
            K.track_step(det, self.seq if seq is None else seq, status, self.desc, self.slots, self.next_id, self.params, record)
        return record

    def reset(self):
        self.slots[:, :, ID] = -1

    def state(self):
        """The device state as numpy (a synchronising copy): what track_host takes."""
        return dict(slots=self.slots.cpu().numpy(), next_id=self.next_id.cpu().numpy())

    def load_state(self, state):
        import torch
        self.slots.copy_(torch.from_numpy(np.ascontiguousarray(state["slots"], dtype=np.int32)))
        self.next_id.copy_(torch.from_numpy(np.ascontiguousarray(state["next_id"], dtype=np.int32)))
