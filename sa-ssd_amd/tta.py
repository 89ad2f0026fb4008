"""Test-time augmentation: the view spec, and the numpy statement of both directions (include/sassd.h "Test-time
augmentation").

A view is (flip, angle, scale): flip 0 / 1 means y -> -y, angle is in radians, scale > 0.  A spec is a list of 1..8 views whose
first is the identity (0, 0.0, 1.0).  InferencePlan(tta=spec) / FrameStream(tta=spec) run the detector on every view of a
cloud inside the captured frame -- sassd_tta_views_dev makes the clouds, sassd_tta_pool brings the candidates back into the
sensor frame as one list -- and suppress the candidates of all views together.  `views_host` and `pool_host` state what the
two kernels compute, in numpy, float32 operation by float32 operation; they are what a caller without tta= does per frame on
the host, and what the tests hold the kernels to, bit for bit."""
import numpy as np

MAX_VIEWS = 8                       # sassd_tta::kMaxViews
MAX_POOL = 4096                     # the most candidates per sample sassd_rescore_nms takes
IDENTITY = (0, 0.0, 1.0)


def check_views(views):
    """The spec as a tuple of (flip int, angle float, scale float).  ValueError for: no list of 1..8 views, a view that is not
    (flip, angle, scale), a flip that is not 0 / 1, an angle that is not finite, a scale that is not positive and finite, a
    first view that is not the identity."""
    if isinstance(views, (str, bytes)) or not hasattr(views, "__len__"):
        raise ValueError("tta must be a list of (flip, angle, scale) views, got %r" % (views,))
    if not 1 <= len(views) <= MAX_VIEWS:
        raise ValueError("tta takes 1..%d views, got %d" % (MAX_VIEWS, len(views)))
    out = []
    for i, v in enumerate(views):
        try:
            flip, angle, scale = v
            angle, scale = float(angle), float(scale)
            if isinstance(flip, (bool, np.bool_)):
                flip = int(flip)
            if flip != 0 and flip != 1:
                raise ValueError
            flip = int(flip)
        except (TypeError, ValueError):
            raise ValueError("tta view %d must be (flip 0 / 1, angle, scale), got %r" % (i, v)) from None
        if not np.isfinite(angle) or not np.isfinite(np.float32(angle)):
            raise ValueError("tta view %d: the angle must be finite, got %r" % (i, angle))
        if not np.isfinite(scale) or not np.isfinite(np.float32(scale)) or not np.float32(scale) > 0:
            raise ValueError("tta view %d: the scale must be positive and finite, got %r" % (i, scale))
        out.append((flip, angle, scale))
    if out[0] != IDENTITY:
        raise ValueError("the first tta view must be the identity (0, 0.0, 1.0), got %r" % (out[0],))
    return tuple(out)


def view_params(views):
    """What the host hands the kernels, rounded as PointAugmentor._global rounds: dict(flip [V] i32, sin [V] = float32(sin(angle)),
    cos [V] = float32(cos(angle)), scale [V] = float32(scale), angle [V] = float32(angle))."""
    views = check_views(views)
    return dict(flip=np.array([v[0] for v in views], np.int32),
                sin=np.array([np.float32(np.sin(v[1])) for v in views], np.float32),
                cos=np.array([np.float32(np.cos(v[1])) for v in views], np.float32),
                scale=np.array([np.float32(v[2]) for v in views], np.float32),
                angle=np.array([np.float32(v[1]) for v in views], np.float32))


def views_host(points, views):
    """The V clouds of `points` [n, ndim >= 3] f32: the identity view is the rows themselves, bit for bit; every other view
    applies global_point of csrc/augment_core.h to x, y, z -- flip, then rotate, then scale, every float32 product and sum
    rounded on its own -- and copies the other columns."""
    p = view_params(views)
    points = np.ascontiguousarray(points, dtype=np.float32)
    if points.ndim != 2 or points.shape[1] < 3:
        raise ValueError("points must be [n, ndim >= 3], got %s" % (points.shape,))
    out = [points.copy()]
    with np.errstate(invalid="ignore", over="ignore"):
        for v in range(1, len(p["flip"])):
            s, c, sc = p["sin"][v], p["cos"][v], p["scale"][v]
            q = points.copy()
            x = points[:, 0]
            y = -points[:, 1] if p["flip"][v] else points[:, 1]
            q[:, 0] = (x * c + y * s) * sc
            q[:, 1] = (x * (-s) + y * c) * sc
            q[:, 2] = points[:, 2] * sc
            out.append(q)
    return out


def unview_boxes(boxes, flip, s, c, scale, angle):
    """unview_box of csrc/tta_core.h on boxes [k, 7] f32 (x, y, z, w, l, h, yaw) of one view -> the boxes in the sensor frame:
    the first six fields divided by scale; x = x' c - y' s, y = x' s + y' c, yaw -= angle; with flip y = -y, yaw = -yaw + pi."""
    s, c, scale, angle = np.float32(s), np.float32(c), np.float32(scale), np.float32(angle)
    b = np.array(boxes, dtype=np.float32).reshape(-1, 7)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        b[:, :6] = b[:, :6] / scale
        x, y = b[:, 0].copy(), b[:, 1].copy()
        b[:, 0] = x * c - y * s
        b[:, 1] = x * s + y * c
        b[:, 6] = b[:, 6] - angle
        if flip:
            b[:, 1] = -b[:, 1]
            b[:, 6] = -b[:, 6] + np.float32(np.pi)
    return b


def pool_host(guided, logits, labels, counts, views, cap):
    """The pooled candidates of sassd_tta_pool: guided [b * V, capK, 7] f32, logits [b * V, capK] f32, labels [b * V, capK] i32,
    counts [b * V] i32 of the inner batch (inner sample s * V + v is view v of user sample s) ->
    dict(guided [b, cap, 7], logits [b, cap], labels [b, cap], counts [b], overflow bool).  View-major per sample: view v
    contributes its first min(counts, capK) rows in their order, boxes through unview_boxes (the identity view's bit for
    bit), logits and labels copied; rows past `cap` are dropped (overflow: SASSD_ST_BOX_OVERFLOW); rows past counts are 0."""
    p = view_params(views)
    V = len(p["flip"])
    guided = np.ascontiguousarray(guided, dtype=np.float32)
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if guided.ndim != 3 or guided.shape[2] != 7 or guided.shape[0] % V or counts.shape[0] != guided.shape[0]:
        raise ValueError("guided must be [b * %d, capK, 7] with one count per inner sample, got %s and %d counts"
                         % (V, guided.shape, counts.shape[0]))
    cap = int(cap)
    if not 1 <= cap <= MAX_POOL:
        raise ValueError("the pool takes 1..%d rows, got %d" % (MAX_POOL, cap))
    b, capK = guided.shape[0] // V, guided.shape[1]
    out = dict(guided=np.zeros((b, cap, 7), np.float32), logits=np.zeros((b, cap), np.float32),
               labels=np.zeros((b, cap), np.int32), counts=np.zeros(b, np.int32), overflow=False)
    for s in range(b):
        g, lo, la = [], [], []
        for v in range(V):
            i, k = s * V + v, int(min(max(counts[s * V + v], 0), capK))
            g.append(guided[i, :k].copy() if v == 0 else
                     unview_boxes(guided[i, :k], p["flip"][v], p["sin"][v], p["cos"][v], p["scale"][v], p["angle"][v]))
            lo.append(logits[i, :k])
            la.append(labels[i, :k])
        g, lo, la = np.concatenate(g, 0), np.concatenate(lo, 0), np.concatenate(la, 0)
        n = min(len(g), cap)
        out["overflow"] |= len(g) > cap
        out["guided"][s, :n], out["logits"][s, :n], out["labels"][s, :n], out["counts"][s] = g[:n], lo[:n], la[:n], n
    return out
