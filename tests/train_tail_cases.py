"""References and seeded inputs of the training-tail kernel tests (test_train_tail_cases_cpu.py, test_gpu_aux_kernels.py,
test_gpu_rescore_loss_kernels.py): numpy / torch-CPU only, no GPU import.

The references restate sassd_aux_prepare, sassd_aux_head_fwd / _bwd, sassd_focal_loss, sassd_boxes_iou3d_batch and the
overlap branch of sassd_assign_targets (include/sassd.h) in float64 from the fp32 inputs.  The builders keep every DISCRETE
outcome away from the point where fp32 and float64 could decide differently, so labels and counts compare exactly:

  point in box   every point is PT_MARGIN away from every face (rotated frame), from the z slab and from the 10 m gate of
                 every box of its own sample
  smooth-L1      every |out - target| of a positive point is SL1_MARGIN away from beta = 1/9 and from 0 (branch and sign)
  assignment     no best overlap lies within head_cases.IOU_BAND of a threshold, and the two best rows of every ground
                 truth are IOU_BAND apart (composed test only: with a given matrix the assignment is exact arithmetic)

Floating results are compared with `figure`: the largest |x - ref| / scale, where the scale of an elementwise tensor is
max |ref| and the scale of a summed one is, per element, the float64 sum of the absolute values of its terms (a sum of sums
carries the inner scales, so cancellation is paid for).  Every reference comes with an fp32 twin (dt=np.float32): the same
formula in numpy float32 -- the 4 / 64 / 160-term dot products accumulated left to right (no BLAS: its blocking is
unspecified), the reductions over points by numpy's own float32 sum along the contiguous axis (pairwise), the scatter by
np.add.at.  The kernels get four times the twin's figure, and never less than FLOOR = 4 x 2^-24."""
import functools

import numpy as np

import head_cases as HC

PT_MARGIN = 1e-3
SL1_MARGIN = 1e-3
BETA = 1.0 / 9.0
FLOOR = 4.0 * 2.0 ** -24
VOXEL_SIZE = (0.05, 0.05, 0.1)
OFFSET = (0.0, -40.0, -3.0)
AUX_C = (32, 64, 64)
AUX_KOFF = (0, 32, 96)


def figure(x, ref, scale):
    """largest |x - ref| / scale (scale: a scalar or an array like ref); where the scale is 0 the value must be exactly 0"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    scale = np.broadcast_to(np.asarray(scale, np.float64), ref.shape)
    live = scale > 0
    assert np.all(x[~live] == 0) and np.all(ref[~live] == 0), "a value with no terms is not exactly 0"
    if not live.any():
        return 0.0
    return float((np.abs(x - ref)[live] / scale[live]).max())


def bar(fp32_figure):
    return max(4.0 * fp32_figure, FLOOR)


def _seq_matmul(a, bt, dt):
    """a [n, k] @ bt [k, m]: float64 as it comes, float32 accumulated over k left to right"""
    if dt == np.float64:
        return a @ bt
    acc = np.zeros((a.shape[0], bt.shape[1]), np.float32)
    for k in range(a.shape[1]):
        acc = acc + a[:, k, None] * bt[k][None]
    return acc


def _sum_points(t, dt):
    """sum of a 1-D array in dt (numpy's pairwise sum)"""
    return np.ascontiguousarray(t).sum(dtype=dt)


# ---- aux_prepare ----------------------------------------------------------------------------------------------------------
def box_terms(p, box):
    """p [n, 3] and ONE box [7], float64: the five signed distances to the decisions of aux_pt_in_box3d [n, 5] (inside when
    all are >= 0): the 10 m gates in x and y, the z slab about box[2] + box[5] / 2, and the two faces in the rotated frame"""
    p, b = np.asarray(p, np.float64), np.asarray(box, np.float64)
    dx, dy = p[:, 0] - b[0], p[:, 1] - b[1]
    cz = b[2] + b[5] / 2.0
    c, s = np.cos(b[6]), np.sin(b[6])
    xr, yr = dx * c - dy * s, dx * s + dy * c
    return np.stack([10.0 - np.abs(dx), 10.0 - np.abs(dy), b[5] / 2.0 - np.abs(p[:, 2] - cz), b[3] / 2.0 - np.abs(xr),
                     b[4] / 2.0 - np.abs(yr)], 1)


def _car(g, cx, cy):
    return [cx, cy, g.uniform(-1.9, -1.5), g.uniform(1.4, 1.9), g.uniform(3.2, 4.6), g.uniform(1.4, 1.7), g.uniform(-3.3, 3.3)]


def prepare_boxes(seed):
    """B = 3, the middle sample without boxes.  Sample 0: five cars and one long box (w 2, l 26) whose ends lie past the
    10 m gate.  Sample 2: four cars, the second a copy of the first moved by 0.3 m (they overlap: the LAST one wins).
    -> (gt [T, 7] fp32, counts)"""
    g = np.random.default_rng(1000 + seed)
    s0 = [_car(g, g.uniform(8, 60), g.uniform(-30, 30)) for _ in range(5)]
    s0.append([35.0, 0.0, -1.8, 2.0, 26.0, 2.0, 0.05])
    s2 = [_car(g, g.uniform(8, 60), g.uniform(-30, 30)) for _ in range(4)]
    s2[1] = list(s2[0])
    s2[1][0] += 0.3; s2[1][1] += 0.3; s2[1][2] += 0.1
    return np.asarray(s0 + s2, np.float32), (6, 0, 4)


def _inside(g, box, frac=1.0, z_in=True):
    """a point in the rotated frame of `box`: |u| < frac * w/2 - 0.02 etc. for frac <= 1, just outside a face for frac > 1"""
    b = np.asarray(box, np.float64)
    if frac <= 1:
        u = g.uniform(-1, 1) * (frac * b[3] / 2 - 0.02)
        v = g.uniform(-1, 1) * (frac * b[4] / 2 - 0.02)
    else:
        u = np.sign(g.uniform(-1, 1)) * (b[3] / 2 + g.uniform(0.01, 0.4))
        v = g.uniform(-1, 1) * b[4] / 2
    z = b[2] + b[5] / 2 + (g.uniform(-1, 1) * (b[5] / 2 - 0.02) if z_in else (b[5] / 2 + g.uniform(0.01, 0.5)))
    c, s = np.cos(b[6]), np.sin(b[6])
    return [b[0] + u * c + v * s, b[1] - u * s + v * c, z]


def prepare_case(seed, n, m, vstride, with_boxes=True):
    """A seeded aux_prepare input: dict(vfeat [n, vstride], coors [n, 4] (b, z, y, x), indices 3 x [M_s, 4], gt [T, 7] or
    None, counts, B, planted=dict(overlap, foreign, gate: point indices)).  The first points are the planted ones: inside
    both overlapping boxes of sample 2; a point of sample 0 at the centre of a box of sample 2 and a point of the box-less
    sample 1 inside a box of sample 0 (both stay negative); a point of sample 0 inside the long box past the 10 m gate."""
    g = np.random.default_rng(seed)
    gt, counts = prepare_boxes(seed)
    off = np.concatenate([[0], np.cumsum(counts)])
    own = [gt[off[b]:off[b + 1]] for b in range(3)]
    pts, smp, kinds = [], [], []

    def add(p, b, kind):
        p32 = np.asarray(p, np.float32)
        if len(own[b]):
            t = np.concatenate([box_terms(p32[None], bx) for bx in own[b]])
            if np.abs(t).min() < 2 * PT_MARGIN:
                return False
        pts.append(p32); smp.append(b); kinds.append(kind)
        return True

    b0, b1 = own[2][0].astype(np.float64), own[2][1].astype(np.float64)
    mid = [(b0[0] + b1[0]) / 2, (b0[1] + b1[1]) / 2, (b0[2] + b1[2]) / 2 + 0.7]
    assert add(mid, 2, "overlap")
    assert add([own[2][2][0], own[2][2][1], own[2][2][2] + 0.6], 0, "foreign")
    lb = own[0][5].astype(np.float64)
    c, s = np.cos(lb[6]), np.sin(lb[6])
    assert add([lb[0] + 11.5 * s, lb[1] + 11.5 * c, lb[2] + 1.0], 0, "gate")
    assert add(_inside(g, own[0][1], 0.5), 1, "foreign")
    assert add([mid[0] + 0.05, mid[1] - 0.05, mid[2]], 2, "overlap")
    while len(pts) < n:
        b = int(g.integers(0, 3))
        kind = g.uniform(0, 1)
        if len(own[b]) and kind < 0.4:
            add(_inside(g, own[b][g.integers(0, len(own[b]))]), b, "in")
        elif len(own[b]) and kind < 0.55:
            add(_inside(g, own[b][g.integers(0, len(own[b]))], 2.0), b, "near")
        elif len(own[b]) and kind < 0.65:
            add(_inside(g, own[b][g.integers(0, len(own[b]))], 1.0, z_in=False), b, "above")
        else:
            add([g.uniform(0, 70.4), g.uniform(-40, 40), g.uniform(-3, 1)], b, "free")
    pts, smp, kinds = np.stack(pts[:n]), np.asarray(smp[:n], np.int32), kinds[:n]
    vfeat = g.uniform(0, 1, (n, vstride)).astype(np.float32)
    vfeat[:, :3] = pts
    coors = np.zeros((n, 4), np.int32)
    coors[:, 0] = smp
    coors[:, 3] = np.clip(pts[:, 0] / 0.05, 0, 1407)
    coors[:, 2] = np.clip((pts[:, 1] + 40) / 0.05, 0, 1599)
    coors[:, 1] = np.clip((pts[:, 2] + 3) / 0.1, 0, 39)
    indices = []
    for k, ms in enumerate(m):
        i = np.zeros((ms, 4), np.int32)
        i[:, 0] = g.integers(0, 3, ms)
        i[:, 1] = g.integers(0, 41 >> (k + 1), ms)
        i[:, 2] = g.integers(0, 1600 >> (k + 1), ms)
        i[:, 3] = g.integers(0, 1408 >> (k + 1), ms)
        indices.append(i)
    planted = {k: [i for i, kk in enumerate(kinds) if kk == k] for k in ("overlap", "foreign", "gate")}
    return dict(vfeat=vfeat, coors=coors, indices=indices, gt=gt if with_boxes else None,
                counts=counts if with_boxes else (0, 0, 0), B=3, planted=planted, kinds=kinds)


def prepare_margin(case):
    """the closest any point comes to a decision of a box of its own sample"""
    if case["gt"] is None:
        return np.inf
    off = np.concatenate([[0], np.cumsum(case["counts"])])
    best = np.inf
    for b in range(case["B"]):
        p = case["vfeat"][case["coors"][:, 0] == b, :3]
        for bx in case["gt"][off[b]:off[b + 1]]:
            if len(p):
                best = min(best, float(np.abs(box_terms(p, bx)).min()))
    return best


def aux_prepare_ref(case, voxel_size=VOXEL_SIZE, offset=OFFSET):
    """-> dict(points [n, 4], known 3 x [M_s, 4], label [n] u8, target [n, 3] fp32, npos)"""
    vf, co = case["vfeat"], case["coors"]
    n = len(vf)
    points = np.concatenate([co[:, :1].astype(np.float32), vf[:, :3]], 1)
    known = []
    for k, idx in enumerate(case["indices"]):
        vs = np.asarray(voxel_size, np.float32) * np.float32(2 << k)
        half = np.float32(0.5) * vs
        kn = np.zeros((len(idx), 4), np.float32)
        kn[:, 0] = idx[:, 0]
        kn[:, 1:] = (idx[:, [3, 2, 1]].astype(np.float32) * vs + np.asarray(offset, np.float32)) + half
        known.append(kn)
    label = np.zeros(n, np.uint8)
    target = np.zeros((n, 3), np.float32)
    if case["gt"] is not None:
        off = np.concatenate([[0], np.cumsum(case["counts"])])
        p64 = vf[:, :3].astype(np.float64)
        for b in range(case["B"]):
            rows = np.flatnonzero(co[:, 0] == b)
            for bx in case["gt"][off[b]:off[b + 1]]:                          # in order: the last containing box wins
                inside = rows[(box_terms(p64[rows], bx) >= 0).all(1)]
                b64 = bx.astype(np.float64)
                label[inside] = 1
                target[inside, 0] = (p64[inside, 0] - b64[0]).astype(np.float32)
                target[inside, 1] = (p64[inside, 1] - b64[1]).astype(np.float32)
                target[inside, 2] = (p64[inside, 2] - (b64[2] + b64[3] / 2.0)).astype(np.float32)   # index 3: the reference's
    return dict(points=points, known=known, label=label, target=target, npos=int(label.sum()))


# ---- focal loss -----------------------------------------------------------------------------------------------------------
def focal_terms(x, t, cw, dt=np.float64):
    """sassd_focal_loss / the aux head's focal term per element: x logits, t in {0, 1}, cw the weight -> (loss, d loss / d x)"""
    x, t, cw = np.asarray(x).astype(dt), np.asarray(t).astype(dt), np.asarray(cw).astype(dt)
    one = dt(1)
    with np.errstate(over="ignore"):
        p = one / (one + np.exp(-x))
        pt = (one - p) * t + p * (one - t)
        aw = (dt(0.25) * t + dt(0.75) * (one - t)) * cw
        w = aw * (pt * pt)
        bce = np.maximum(x, dt(0)) - x * t + np.log1p(np.exp(-np.abs(x)))
        dpt = p * (one - p) * (one - dt(2) * t)
        return bce * w, (p - t) * w + bce * aw * dt(2) * pt * dpt


def focal_ref(logits, labels, num_pos, dt=np.float64):
    """labels -1 / 0 / > 0, weight (label >= 0) / max(sum num_pos, 1) -> (loss sum, grad [n], the terms of the sum)"""
    labels = np.asarray(labels)
    norm = dt(max(float(np.sum(num_pos)), 1.0))
    cw = (labels >= 0).astype(dt) / norm
    l, g = focal_terms(logits, labels > 0, cw, dt)
    return _sum_points(l, dt), g, l


def focal_case(seed, n, all_ignored=False):
    """logits N(0, 2) with planted +-100, +-20 and +-0.0, labels drawn from {-1, 0, 1, 2} (or all -1)"""
    g = np.random.default_rng(seed)
    x = g.normal(0, 2, n).astype(np.float32)
    plant = np.array([100, -100, 20, -20, 0.0, -0.0], np.float32)
    lab = np.full(n, -1, np.int64) if all_ignored else g.integers(-1, 3, n).astype(np.int64)
    if n >= 64:
        at = g.choice(n, 24, replace=False)
        x[at] = np.tile(plant, 4)
        if not all_ignored:
            lab[at] = np.repeat(np.array([-1, 0, 1, 2]), 6)
    return x, lab


# ---- aux head forward / backward ------------------------------------------------------------------------------------------
def aux_sizes(n, kind):
    return (3, 3, 3) if kind == "tiny" else (n, n // 2 + 3, n // 4 + 3)


@functools.lru_cache(maxsize=None)
def aux_case(seed, n, kind, positives=True):
    """A seeded aux-head input of n points over the M of aux_sizes: dict(feats, nn_idx, nn_d2 (3 each), w1, w2, label, target,
    npos, zero (the point with d2 = 0 at every scale), same (the point whose three neighbours are one row per scale)).
    positives=False: no positive point, npos = 0."""
    g = np.random.default_rng(seed)
    m = aux_sizes(n, kind)
    c = dict(n=n, m=m, zero=0, same=n // 2)
    c["feats"] = [g.normal(0, 1, (m[s], AUX_C[s])).astype(np.float32) for s in range(3)]
    c["nn_idx"] = [g.integers(0, m[s], (n, 3)).astype(np.int32) for s in range(3)]
    if m[0] > 3:
        c["nn_idx"][0][c["nn_idx"][0] == m[0] - 1] = 0           # the last row of level 0: nobody's neighbour
    c["nn_d2"] = [(g.uniform(0.02, 2.0, (n, 3)) ** 2).astype(np.float32) for s in range(3)]
    for s in range(3):
        c["nn_d2"][s][c["zero"], 0] = 0.0
        c["nn_idx"][s][c["same"], :] = c["nn_idx"][s][c["same"], 0]
    c["w1"] = g.normal(0, 0.08, (64, 160)).astype(np.float32)
    c["w2"] = g.normal(0, 0.12, (4, 64)).astype(np.float32)
    label = (g.uniform(0, 1, n) < 0.3).astype(np.uint8)
    if positives:
        label[n - 1] = 1
    else:
        label[:] = 0
    c["label"] = label
    c["npos"] = int(label.sum())
    target = g.normal(0, 0.3, (n, 3)).astype(np.float32)
    # small offsets on a third of the points: the quadratic branch of smooth-L1 needs |out - target| < 1/9
    out = aux_fwd_ref(dict(c, target=target))["out"][:, 1:]
    near = g.uniform(0, 1, (n, 3)) < 0.35
    target = np.where(near, out + g.uniform(-0.1, 0.1, (n, 3)), target).astype(np.float32)
    for _ in range(4):                                   # clear of beta and of 0, by moving the target away from the output
        diff = out - target.astype(np.float64)
        d = np.abs(diff)
        bad = (np.abs(d - BETA) < 2 * SL1_MARGIN) | (d < 2 * SL1_MARGIN)
        if not bad.any():
            break
        target = np.where(bad, out - (diff + np.where(diff >= 0, 1.0, -1.0) * 5 * SL1_MARGIN), target).astype(np.float32)
    c["target"] = target
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    for lst in (c["feats"], c["nn_idx"], c["nn_d2"]):
        for v in lst:
            v.setflags(write=False)
    return c


def sl1_margin(case):
    """closest |out - target| of a positive point to beta and to 0 (inf without positives)"""
    out = aux_fwd_ref(case)["out"][:, 1:]
    d = np.abs(out - case["target"].astype(np.float64))[case["label"] > 0]
    return float(min(np.abs(d - BETA).min(), d.min())) if d.size else np.inf


def aux_weights(case, dt=np.float64):
    """[n, 9] inverse-distance weights, w = r_j / ((r0 + r1) + r2), r = 1 / (sqrt(d2) + 1e-8)"""
    out = []
    for s in range(3):
        r = dt(1) / (np.sqrt(case["nn_d2"][s].astype(dt)) + dt(1e-8))
        nrm = (r[:, 0] + r[:, 1]) + r[:, 2]
        out.append(r / nrm[:, None])
    return np.concatenate(out, 1)


def aux_interp(case, wgt, dt=np.float64, absolute=False):
    """f [n, 160] = sum_j wgt[p, s, j] * feats[s][nn_idx[s][p, j]] (absolute: of |w| |feat|)"""
    cols = []
    for s in range(3):
        ft = case["feats"][s].astype(dt)
        w = np.asarray(wgt)[:, s * 3:s * 3 + 3].astype(dt)
        if absolute:
            ft, w = np.abs(ft), np.abs(w)
        idx = case["nn_idx"][s]
        cols.append((w[:, 0, None] * ft[idx[:, 0]] + w[:, 1, None] * ft[idx[:, 1]]) + w[:, 2, None] * ft[idx[:, 2]])
    return np.concatenate(cols, 1)


def aux_fwd_ref(case, dt=np.float64):
    """sassd_aux_head_fwd -> dict(wgt [n, 9], h [n, 64], out [n, 4], gout [n, 4], sums [2]) in dt; for float64 also
    scale = dict(...) per tensor (see the module header)"""
    n = case["n"]
    w1, w2 = case["w1"].astype(dt), case["w2"].astype(dt)
    wgt = aux_weights(case, dt)
    f = aux_interp(case, wgt, dt)
    h = _seq_matmul(f, w1.T, dt)
    out = _seq_matmul(h, w2.T, dt)
    norm = dt(max(case.get("npos", 0), 1))
    t = (case["label"] > 0).astype(dt)
    l_cls, g_cls = focal_terms(out[:, 0], t, np.full(n, dt(1) / norm, dt), dt)
    diff = out[:, 1:] - case["target"].astype(dt)
    d = np.abs(diff)
    beta = dt(1) / dt(9)
    reg_w = (t / norm)[:, None]
    l_reg = np.where(d < beta, dt(0.5) * d * d / beta, d - dt(0.5) * beta) * reg_w
    g_reg = np.where(d < beta, d / beta, dt(1)) * np.sign(diff) * reg_w
    r = dict(wgt=wgt, h=h, out=out, gout=np.concatenate([g_cls[:, None], g_reg], 1).astype(dt),
             sums=np.stack([_sum_points(l_cls, dt), _sum_points(l_reg.reshape(-1), dt)]))
    if dt == np.float64:
        sh = aux_interp(case, wgt, absolute=True) @ np.abs(w1).T
        r["scale"] = dict(wgt=np.abs(wgt).max(), h=sh, out=sh @ np.abs(w2).T, gout=np.abs(r["gout"]).max(),
                          sums=np.stack([np.abs(l_cls).sum(), np.abs(l_reg).sum()]))
    return r


def aux_bwd_ref(case, wgt, h, gout, grad_sums, dt=np.float64):
    """sassd_aux_head_bwd from the forward's wgt / h / gout AS GIVEN (the kernel's inputs) -> dict(gf 3 x [M_s, C_s],
    dw1 [64, 160], dw2 [4, 64]) in dt; for float64 also scale = dict(...)"""
    w1, w2 = case["w1"].astype(dt), case["w2"].astype(dt)
    gs = np.asarray(grad_sums, np.float32).astype(dt)
    d = np.asarray(gout).astype(dt) * np.array([gs[0], gs[1], gs[1], gs[1]], dt)[None]
    wgt, h = np.asarray(wgt).astype(dt), np.asarray(h).astype(dt)
    dh = (d[:, 0, None] * w2[0] + d[:, 1, None] * w2[1]) + (d[:, 2, None] * w2[2] + d[:, 3, None] * w2[3])
    df = _seq_matmul(dh, w1, dt)
    f = aux_interp(case, wgt, dt)

    def scatter(src, wv):
        out = []
        for s in range(3):
            acc = np.zeros((case["m"][s], AUX_C[s]), dt)
            for j in range(3):
                np.add.at(acc, case["nn_idx"][s][:, j], src[:, AUX_KOFF[s]:AUX_KOFF[s] + AUX_C[s]] * wv[:, s * 3 + j, None])
            out.append(acc)
        return out

    def over_points(a, b):
        if dt == np.float64:
            return a.T @ b
        bt = np.ascontiguousarray(b.T)                                     # [k, n]: the sum over points runs along the contiguous axis
        return np.stack([(bt * a[:, o][None]).sum(1, dtype=np.float32) for o in range(a.shape[1])])

    r = dict(gf=scatter(df, wgt), dw1=over_points(dh, f), dw2=over_points(d, h))
    if dt == np.float64:
        sdh = np.abs(d) @ np.abs(w2)
        sdf = sdh @ np.abs(w1)
        r["scale"] = dict(gf=scatter(sdf, np.abs(wgt)), dw1=sdh.T @ aux_interp(case, wgt, absolute=True),
                          dw2=np.abs(d).T @ np.abs(h))
    return r


# ---- rotated 3-D IoU ------------------------------------------------------------------------------------------------------
def _rect(b):
    """corners of the BEV rectangle of one box [7] (float64): centre + (c dx + s dy, -s dx + c dy), counter-clockwise"""
    c, s = np.cos(b[6]), np.sin(b[6])
    pts = []
    for dx, dy in ((-b[3] / 2, -b[4] / 2), (b[3] / 2, -b[4] / 2), (b[3] / 2, b[4] / 2), (-b[3] / 2, b[4] / 2)):
        pts.append((b[0] + c * dx + s * dy, b[1] - s * dx + c * dy))
    area = sum(pts[i][0] * pts[(i + 1) % 4][1] - pts[(i + 1) % 4][0] * pts[i][1] for i in range(4))
    return pts if area > 0 else pts[::-1]


def _clip_area(pa, pb):
    """area of convex polygon pa clipped by convex counter-clockwise polygon pb (Sutherland-Hodgman), float64"""
    poly = pa
    for i in range(len(pb)):
        (x0, y0), (x1, y1) = pb[i], pb[(i + 1) % len(pb)]
        ex, ey = x1 - x0, y1 - y0
        nxt = []
        for k in range(len(poly)):
            p, q = poly[k], poly[(k + 1) % len(poly)]
            sp = ex * (p[1] - y0) - ey * (p[0] - x0)
            sq = ex * (q[1] - y0) - ey * (q[0] - x0)
            if sp >= 0:
                nxt.append(p)
            if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
                u = sp / (sp - sq)
                nxt.append((p[0] + u * (q[0] - p[0]), p[1] + u * (q[1] - p[1])))
        poly = nxt
        if len(poly) < 3:
            return 0.0
    return 0.5 * abs(sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[(i + 1) % len(poly)][0] * poly[i][1]
                         for i in range(len(poly))))


def iou3d_pairs(a, b):
    """[len(a), len(b)] float64 rotated 3-D IoU of fp32 boxes a against b"""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    out = np.zeros((len(a), len(b)))
    if not len(a) or not len(b):
        return out
    ra, rb = 0.5 * np.hypot(a[:, 3], a[:, 4]), 0.5 * np.hypot(b[:, 3], b[:, 4])
    dist = np.hypot(a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1])
    rect_a, rect_b = [_rect(x) for x in a], [_rect(x) for x in b]
    for i, j in zip(*np.nonzero(dist <= ra[:, None] + rb[None] + 1e-6)):
        oh = max(min(a[i, 2] + a[i, 5], b[j, 2] + b[j, 5]) - max(a[i, 2], b[j, 2]), 0.0)
        if oh <= 0:
            continue
        o3 = _clip_area(rect_a[i], rect_b[j]) * oh
        va, vb = a[i, 3] * a[i, 4] * a[i, 5], b[j, 3] * b[j, 4] * b[j, 5]
        out[i, j] = o3 / max(va + vb - o3, 1e-7)
    return out


def iou3d_ref(boxes, counts, gt, gt_counts):
    """sassd_boxes_iou3d_batch: boxes [B, rows, 7], counts [B], gt [T, 7], gt_counts [B] -> (flat float64 [ov_off[B]] of the
    samples' [rows, G_b] matrices, rows past counts[b] 0; ov_off [B + 1] int64)"""
    bsz, rows, _ = boxes.shape
    goff = np.concatenate([[0], np.cumsum(gt_counts)]).astype(np.int64)
    ov_off = np.concatenate([[0], np.cumsum(rows * np.asarray(gt_counts, np.int64))]).astype(np.int64)
    out = np.zeros(int(ov_off[-1]))
    for b in range(bsz):
        gb = gt[goff[b]:goff[b + 1]]
        m = np.zeros((rows, len(gb)))
        k = min(int(counts[b]), rows)
        m[:k] = iou3d_pairs(boxes[b, :k], gb)
        out[ov_off[b]:ov_off[b + 1]] = m.reshape(-1)
    return out, ov_off


RS_ROWS, RS_G = 300, (12, 0, 129)
RS_THRESHOLDS = (0.7, 0.6, 0.45)
RS_FIELD = 5.0             # cluster centres within +-RS_FIELD metres of the origin (see rescore_batch)
FAR = np.array([40.0, 40.0, -1.0, 1.6, 3.9, 1.5, 0.0], np.float32)


@functools.lru_cache(maxsize=None)
def rescore_batch(seed=0):
    """B = 3, rows = 300, G = (12, 0, 129), car-sized boxes in clusters.  Every sample's first rows are its ground truth
    (what sassd_guided_decode_fwd writes), then five planted rows about ground truth 0 and 1: the same centre turned by
    pi / 2, a box contained in it, a copy with no height overlap, a box touching ground truth 1 (r = 0) along an edge, and
    a copy of ground truth 0 moved by a few centimetres; the rest are jittered copies of ground truths.  A row whose best
    overlap lies within IOU_BAND of one of RS_THRESHOLDS, or which comes within IOU_BAND of a ground truth's best row, is
    moved far away (IoU 0).  The clusters lie within RS_FIELD of the origin: the corners of a rotated rectangle are formed
    in fp32 about its centre, so the fp32 oracle itself drifts from float64 with the centre's magnitude (9e-6 at 60 m, which
    would leave a kernel no room under the 1e-5 bar; 8.3e-7 here).  -> dict(boxes [3, 300, 7], gt [141, 7], gt_counts, planted=dict(name: row), full: the
    float64 IoU with every row valid (flat) and its ov_off)"""
    g = np.random.default_rng(seed)
    gts = []
    for G in RS_G:
        ncl = max(2, G // 6)
        cen = np.stack([g.uniform(-RS_FIELD, RS_FIELD, ncl), g.uniform(-RS_FIELD, RS_FIELD, ncl)], 1)
        pick = g.integers(0, ncl, G)
        gb = np.zeros((G, 7))
        gb[:, 0] = cen[pick, 0] + g.normal(0, 1.0, G)
        gb[:, 1] = cen[pick, 1] + g.normal(0, 1.0, G)
        gb[:, 2] = g.uniform(-1.9, -1.5, G)
        gb[:, 3], gb[:, 4], gb[:, 5] = g.uniform(1.4, 1.9, G), g.uniform(3.2, 4.6, G), g.uniform(1.4, 1.7, G)
        gb[:, 6] = g.uniform(-3.3, 3.3, G)
        if G > 1:
            gb[1] = [gb[1, 0], gb[1, 1], -1.75, 1.5, 4.0, 1.5, 0.0]
        gts.append(gb.astype(np.float32))
    boxes = np.zeros((3, RS_ROWS, 7), np.float32)
    planted = {}
    for b, gb in enumerate(gts):
        G = len(gb)
        boxes[b, :G] = gb
        r = G
        if G:
            g0, g1 = gb[0].astype(np.float64), gb[1].astype(np.float64)
            turned = g0.copy(); turned[6] += np.pi / 2
            inner = g0.copy(); inner[3:5] *= 0.5; inner[5] *= 0.5; inner[2] += 0.2
            above = g0.copy(); above[2] += g0[5] + 0.5
            touch = g1.copy(); touch[0] += g1[3]
            close = g0.copy(); close[0] += 0.04; close[1] -= 0.03; close[6] += 0.01
            for name, bx in (("turned", turned), ("inner", inner), ("above", above), ("touch", touch), ("close", close)):
                boxes[b, r] = bx
                if b == 0:
                    planted[name] = r
                r += 1
        for q in range(r, RS_ROWS):
            if G and g.uniform(0, 1) < 0.9:
                src = gb[g.integers(0, G)].astype(np.float64)
                bx = [src[0] + g.normal(0, 0.7), src[1] + g.normal(0, 0.7), src[2] + g.normal(0, 0.15), g.uniform(1.4, 1.9),
                      g.uniform(3.2, 4.6), g.uniform(1.4, 1.7), src[6] + g.normal(0, 0.3)]
            else:
                bx = _car(g, g.uniform(-RS_FIELD, RS_FIELD), g.uniform(-RS_FIELD, RS_FIELD))
            boxes[b, q] = bx
    gt = np.concatenate(gts)
    full = (RS_ROWS,) * 3
    moved = 0
    ov, ov_off = iou3d_ref(boxes, full, gt, RS_G)
    for b, G in enumerate(RS_G):
        if not G:
            continue
        m = ov[ov_off[b]:ov_off[b + 1]].reshape(RS_ROWS, G)                # a view: a row moved far away overlaps nothing
        for _ in range(8):
            best = m.max(1)
            bad = np.zeros(RS_ROWS, bool)
            for thr in RS_THRESHOLDS:
                bad |= np.abs(best - thr) < 2 * HC.IOU_BAND
            top = np.sort(m, 0)[-2:]                                       # [2, G]: runner-up and best of every ground truth
            for col in np.flatnonzero(top[1] - top[0] < 2 * HC.IOU_BAND):
                bad[np.argsort(m[:, col])[-2]] = True
            bad[:G + 5] = False
            if not bad.any():
                break
            boxes[b, bad] = FAR
            m[bad] = 0
            moved += int(bad.sum())
    boxes.setflags(write=False); gt.setflags(write=False); ov.setflags(write=False)
    return dict(boxes=boxes, gt=gt, gt_counts=RS_G, planted=planted, full=ov, ov_off=ov_off, moved=moved)


def rescore_margins(batch):
    """(closest best overlap of a row to one of RS_THRESHOLDS, closest runner-up to a ground truth's best row, smallest
    best overlap of a ground truth) over the samples with ground truth, every row valid"""
    thr_m, gap_m, col_m = np.inf, np.inf, np.inf
    for b, G in enumerate(batch["gt_counts"]):
        if not G:
            continue
        m = batch["full"][batch["ov_off"][b]:batch["ov_off"][b + 1]].reshape(RS_ROWS, G)
        best = m.max(1)
        thr_m = min(thr_m, min(float(np.abs(best - t).min()) for t in RS_THRESHOLDS))
        top = np.sort(m, 0)[-2:]
        gap_m = min(gap_m, float((top[1] - top[0]).min()))
        col_m = min(col_m, float(top[1].min()))
    return thr_m, gap_m, col_m


def masked_rows(ov_flat, ov_off, counts, gt_counts, rows=RS_ROWS):
    """the flat matrix with rows at or past counts[b] set to 0 (what the kernel writes there)"""
    out = np.array(ov_flat)
    for b, G in enumerate(gt_counts):
        m = out[ov_off[b]:ov_off[b + 1]].reshape(rows, G)
        m[min(int(counts[b]), rows):] = 0
    return out


# ---- assignment from a given overlap matrix -------------------------------------------------------------------------------
def assign_from_overlaps_ref(ov, mask, gt_cls, matched, unmatched):
    """the rule of oracle/train_ref.py::assign with the similarity replaced by the fp32 matrix ov [A, G]: mask [A] bool,
    gt_cls [G] int64 or None (all 1), thresholds compared as fp32 -> (labels [A] int64, best [A] fp32 (-1 where the mask is
    off), number of positives).  Exact: only comparisons of the given numbers."""
    ov = np.asarray(ov, np.float32)
    a, G = ov.shape
    mask = np.asarray(mask, bool)
    labels = np.full(a, -1, np.int64)
    best = np.full(a, -1, np.float32)
    sel = np.flatnonzero(mask)
    if G == 0:
        labels[sel], best[sel] = 0, 0
        return labels, best, 0
    cls = np.ones(G, np.int64) if gt_cls is None else np.asarray(gt_cls, np.int64)
    if len(sel):
        m = ov[sel]
        arg = m.argmax(1)                                                  # the first maximum
        bs = m[np.arange(len(sel)), arg]
        gmax = m.max(0)
        gmax = np.where(gmax == 0, np.float32(-1), gmax)
        forced = (m == gmax[None]).any(1)
        lab = np.full(len(sel), -1, np.int64)
        lab[bs >= np.float32(matched)] = cls[arg[bs >= np.float32(matched)]]
        lab[bs < np.float32(unmatched)] = 0
        lab[forced] = cls[arg[forced]]
        labels[sel], best[sel] = lab, bs
    return labels, best, int((labels > 0).sum())
