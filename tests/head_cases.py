"""References and seeded inputs of the detection-head kernel tests (test_head_cases_cpu.py, test_gpu_head_kernels.py,
test_gpu_guided_kernels.py): numpy / torch-CPU only, no GPU import.

The references restate the contracts of sassd_decode_filter, sassd_pswarp_sample, sassd_rescore_nms and of the training
twins sassd_guided_select / sassd_guided_decode_fwd / _bwd (include/sassd.h), evaluated in float64 from the fp32 inputs.
The builders keep every DISCRETE outcome (selected or not, class, direction flip, score order, suppressed or not) away
from the point where fp32 and float64 could decide differently, so counts, order, labels and kept sets compare exactly:

  cls logits   |sigmoid - thr| >= CLS_MARGIN for every logit; the two best classes of an anchor are either bit-equal or
               CLS_GAP apart (the kernel compares fp32 sigmoids; d sigmoid / d logit >= 0.017 on [-4, 4])
  rotation     |rt + ra| >= ROT_MARGIN, so `rg > 0` is the same in both precisions
  rescore      logits on a LOGIT_STEP lattice in [-4, 4] (distinct ones >= 1e-3 apart), |sigmoid - score_thr| >= 1e-3
  NMS          no pair of boxes has an oracle IoU within IOU_BAND of iou_thr (ten times the 1e-5 agreement of the IoU kernels)

The exact cases (a logit of 0 under thr 0.5, equal class logits, equal direction logits, a rotation of exactly 0, equal
scores) are decided by exact fp32 arithmetic on both sides and are the only exceptions."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import clib

ST_BOX_OVERFLOW = 4
CLS_MARGIN = 1e-3          # logits drawn closer than 1e-4 (in sigmoid) to thr are moved out to this distance
CLS_NEAR = 1e-4
CLS_GAP = 2e-3             # logit gap between the best and the second class, unless they are bit-equal
ROT_MARGIN = 1e-3
LOGIT_STEP = 1.125e-3      # rescore logits are multiples of this: neighbours stay > 1e-3 apart after fp32 rounding
IOU_BAND = 1e-4


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def logit64(p):
    return float(np.log(p / (1.0 - p)))


# ---- references -------------------------------------------------------------------------------------------------------
def box_decode(enc, anchors, dtype=np.float64):
    """second_box_decode: enc [..., 7], anchors [..., 7] -> [..., 7], every operation in `dtype`."""
    e, a = np.asarray(enc).astype(dtype), np.asarray(anchors).astype(dtype)
    xa, ya, za, wa, la, ha, ra = [a[..., j] for j in range(7)]
    xt, yt, zt, wt, lt, ht, rt = [e[..., j] for j in range(7)]
    two = dtype(2)
    za = za + ha / two
    diag = np.sqrt(la * la + wa * wa)
    xg = xt * diag + xa
    yg = yt * diag + ya
    zg = zt * ha + za
    lg = np.exp(lt) * la
    wg = np.exp(wt) * wa
    hg = np.exp(ht) * ha
    rg = rt + ra
    zg = zg - hg / two
    return np.stack([xg, yg, zg, wg, lg, hg, rg], -1)


def dir_flip(boxes, dirp, dtype=np.float64):
    """the direction flip: pi is added to the rotation where (rotation > 0) differs from argmax(dir) (first maximum wins)"""
    out = np.array(boxes, dtype)
    dl = np.asarray(dirp)[..., 1] > np.asarray(dirp)[..., 0]
    opp = (out[..., 6] > 0) != dl
    out[..., 6] = np.where(opp, out[..., 6] + dtype(np.pi), out[..., 6])
    return out


def class_scores(cls, dtype=np.float64):
    """cls [..., NC] logits -> (max-class sigmoid, argmax class; the first maximum wins)"""
    s = dtype(1) / (dtype(1) + np.exp(-np.asarray(cls).astype(dtype)))
    lab = np.argmax(s, -1)
    return np.take_along_axis(s, lab[..., None], -1)[..., 0], lab


def compact(flags, cap):
    """ordered compaction with a capacity: (ascending indices of the set flags cut at cap, the uncut count)"""
    idx = np.flatnonzero(flags)
    return idx[:cap], len(idx)


def decode_filter_ref(case, thr, cap, dtype=np.float64, masked=True):
    """the reference of sassd_decode_filter (and of guided_select + guided_decode_fwd's decoded rows) on a head case:
    per sample dict(idx [n] ascending anchor indices, total (uncut), boxes [n, 7], labels [n], scores [n])"""
    out = []
    for b in range(case["box"].shape[0]):
        s, lab = class_scores(case["cls"][b], dtype)
        flags = s > dtype(thr)
        if masked:
            flags = flags & (case["mask"][b] != 0)
        idx, total = compact(flags, cap)
        an = case["anchors"] if case["anchors"].ndim == 2 else case["anchors"][b]
        boxes = dir_flip(box_decode(case["box"][b][idx], an[idx], dtype), case["dir"][b][idx], dtype)
        out.append(dict(idx=idx, total=total, boxes=boxes, labels=lab[idx], scores=s[idx]))
    return out


def pswarp_grid(boxes, h, w, offsets, scale):
    """the sampling grid of PSWarp, formed in fp32 the way the reference module forms it: [28, n, 1, 2]"""
    br = torch.as_tensor(np.asarray(boxes, np.float32))
    n = br.shape[0]
    ct, st = torch.cos(br[:, 6]).view(n, 1, 1), torch.sin(br[:, 6]).view(n, 1, 1)
    xx = torch.linspace(-.5, .5, 4).view(1, 4, 1) * br[:, 3].view(n, 1, 1)
    yy = torch.linspace(-.5, .5, 7).view(1, 1, 7) * br[:, 4].view(n, 1, 1)
    sx = (xx * ct + yy * st + br[:, 0].view(n, 1, 1) + offsets[0]) * scale
    sy = (yy * ct - xx * st + br[:, 1].view(n, 1, 1) + offsets[1]) * scale
    return torch.stack([sx.reshape(n, 28).t() / (w - 1), sy.reshape(n, 28).t() / (h - 1)], -1).view(28, n, 1, 2) * 2 - 1


def pswarp_ref(feat, boxes, offsets, scale):
    """feat [28, H, W] fp32, boxes [n, 7] fp32 -> logits [n] float64: the fp32 grid sampled by grid_sample in float64"""
    feat = torch.as_tensor(np.asarray(feat, np.float32))
    if len(boxes) == 0:
        return np.zeros(0)
    grid = pswarp_grid(boxes, feat.shape[1], feat.shape[2], offsets, scale)
    o = F.grid_sample(feat.double().unsqueeze(1), grid.double(), align_corners=True)
    return o.mean(0).view(-1).numpy()


def to_bev(b, dtype=np.float32):
    b = np.asarray(b).astype(dtype)
    h = dtype(2)
    return np.stack([b[:, 0] - b[:, 3] / h, b[:, 1] - b[:, 4] / h, b[:, 0] + b[:, 3] / h, b[:, 1] + b[:, 4] / h, b[:, 6]], 1)


def rescore_ref(guided, logits, labels, count, cap_k, score_thr, iou_thr, cap_d, dtype=np.float64):
    """the reference of sassd_rescore_nms for one sample: sigmoid, strict threshold, stable descending sort, greedy rotated
    NMS (clib.nms_rotated on the fp32 BEV boxes), gather, capacity -> dict(rows (indices into guided), scores, kept (uncut))"""
    k = min(int(count), cap_k)
    s = dtype(1) / (dtype(1) + np.exp(-np.asarray(logits[:k]).astype(dtype)))
    cand = np.flatnonzero(s > dtype(score_thr))
    if len(cand) == 0:
        return dict(rows=np.zeros(0, np.int64), scores=np.zeros(0, dtype), kept=0, m=0)
    order = np.argsort(-s[cand], kind="stable")
    keep = clib.nms_rotated(to_bev(np.asarray(guided)[cand[order]]), iou_thr)
    rows = cand[order[keep]]
    return dict(rows=rows[:cap_d], scores=s[rows[:cap_d]], kept=len(rows), m=len(cand))


# ---- head tensors -------------------------------------------------------------------------------------------------------
def head_channels(nc, a):
    return nc * a * 7, nc * a * nc, nc * a * 2


def to_head(box, cls, dirp, nc, a, h, w):
    """anchor-major [B, Atot, 7 | NC | 2] (anchor r = ci*(H*W*A) + pix*A + a) -> the head tensor [B, head_c, H, W] of box,
    cls and dir channel blocks, channel (ci*A + a)*width + j of a block"""
    bsz = box.shape[0]
    parts = []
    for t in (box, cls, dirp):
        k = t.shape[-1]
        parts.append(t.reshape(bsz, nc, h * w, a, k).transpose(0, 1, 3, 4, 2).reshape(bsz, nc * a * k, h, w))
    return np.ascontiguousarray(np.concatenate(parts, 1))


def make_anchors(g, atot, nc, a, hw):
    """[Atot, 7] fp32: centres spread over a 70 m x 80 m field, class sizes, rotations 0 and 1.57 by anchor slot"""
    sizes = np.array([[1.6, 3.9, 1.56], [0.6, 0.8, 1.73], [0.6, 1.76, 1.73]], np.float32)
    r = np.arange(atot)
    an = np.zeros((atot, 7), np.float32)
    an[:, 0] = g.uniform(0, 70.4, atot)
    an[:, 1] = g.uniform(-40, 40, atot)
    an[:, 2] = g.uniform(-1.9, -0.5, atot)
    an[:, 3:6] = sizes[(r // (hw * a)) % 3]
    an[:, 6] = np.where(r % a == 0, 0.0, 1.57)
    return an


def clear_of_threshold(cls, thr):
    """move every logit whose sigmoid lies within CLS_NEAR of thr out to CLS_MARGIN, on the side it is on"""
    s = sigmoid64(cls)
    near = np.abs(s - thr) < CLS_NEAR
    side = np.where(s > thr, 1.0, -1.0)
    moved = np.log((thr + side * CLS_MARGIN) / (1 - thr - side * CLS_MARGIN))
    return np.where(near, moved, cls).astype(np.float32)


def split_best_two(cls):
    """the best class of every anchor leads the second by CLS_GAP at least (lifted where it did not)"""
    if cls.shape[-1] < 2:
        return cls
    srt = np.sort(cls.astype(np.float64), -1)
    close = (srt[..., -1] - srt[..., -2]) < CLS_GAP
    top = np.argmax(cls, -1)
    lift = np.zeros(cls.shape, np.float32)
    np.put_along_axis(lift, top[..., None], np.where(close, 2 * CLS_GAP, 0.0).astype(np.float32)[..., None], -1)
    return (cls + lift).astype(np.float32)


def head_case(seed, bsz, nc, a, h, w, thr, want=None, per_sample_anchors=False):
    """A seeded head: dict(box [B,Atot,7], cls [B,Atot,NC], dir [B,Atot,2], anchors [Atot,7] or [B,Atot,7], mask [B,Atot] u8,
    head [B,head_c,H,W], and the shape).  want: per sample None (whatever the draw selects) or the exact set of anchor
    indices to select -- every other anchor that the draw would select is switched off, by its mask byte (even index) or
    by lowering its logits below the threshold (odd index), so both ways of not selecting run next to the selected."""
    g = np.random.default_rng(seed)
    hw = h * w
    atot = nc * hw * a
    box = g.uniform(-1, 1, (bsz, atot, 7)).astype(np.float32)
    box[..., 6] = g.uniform(-2, 2, (bsz, atot))
    cls = g.uniform(-4, 4, (bsz, atot, nc)).astype(np.float32)
    dirp = g.normal(0, 1, (bsz, atot, 2)).astype(np.float32)
    if per_sample_anchors:
        anchors = np.stack([make_anchors(g, atot, nc, a, hw) for _ in range(bsz)])
    else:
        anchors = make_anchors(g, atot, nc, a, hw)
    mask = (g.uniform(0, 1, (bsz, atot)) < 0.8).astype(np.uint8)
    lo = logit64(thr - 0.05) if thr > 0.06 else logit64(thr / 2)
    for b in range(bsz):
        if want is None or want[b] is None:
            continue
        keep = np.zeros(atot, bool)
        keep[np.asarray(want[b], np.int64)] = True
        best = cls[b].max(-1)
        would = sigmoid64(best) > thr
        # wanted: mask on, and the best class lifted above the threshold where the draw left it below
        mask[b][keep] = 1
        lift = keep & ~would
        top = np.argmax(cls[b], -1)
        cls[b][lift, top[lift]] = g.uniform(logit64(thr) + 0.05, 4, int(lift.sum())).astype(np.float32)
        # unwanted: mask off (even index), or every logit pushed below the threshold (odd index)
        off = ~keep & would
        idx = np.arange(atot)
        mask[b][off & (idx % 2 == 0)] = 0
        low = off & (idx % 2 == 1)
        cls[b][low] = g.uniform(-4, lo, (int(low.sum()), nc)).astype(np.float32)
        mask[b][low] = 1
    for _ in range(8):                      # either rule can undo the other by a few 1e-3: repeat until both hold
        nxt = clear_of_threshold(split_best_two(cls), thr)
        if np.array_equal(nxt, cls):
            break
        cls = nxt
    # the decoded rotation stays ROT_MARGIN away from 0
    an_r = anchors[..., 6] if anchors.ndim == 3 else anchors[None, :, 6]
    rg = box[..., 6].astype(np.float64) + an_r
    small = np.abs(rg) < ROT_MARGIN
    box[..., 6] = np.where(small, (np.where(rg >= 0, 4 * ROT_MARGIN, -4 * ROT_MARGIN) - an_r), box[..., 6]).astype(np.float32)
    case = dict(box=box, cls=cls, dir=dirp, anchors=anchors, mask=mask, nc=nc, a=a, h=h, w=w, atot=atot, thr=thr)
    return finish(case)


def finish(case):
    """(re)build the head tensor after the anchor-major arrays were edited by a test"""
    case["head"] = to_head(case["box"], case["cls"], case["dir"], case["nc"], case["a"], case["h"], case["w"])
    return case


def head_margins(case, exempt=()):
    """the margins head_case promises, measured: dict(thr (closest |sigmoid - thr|), gap (closest unequal best-two logit gap;
    inf for one class), rot (closest |rt + ra| to 0)), leaving out the (sample, anchor) pairs of `exempt` (the exact cases)"""
    ok = np.ones(case["cls"].shape[:2], bool)
    for b, r in exempt:
        ok[b, r] = False
    s = sigmoid64(case["cls"])
    m_thr = float(np.abs(s - case["thr"])[ok].min())
    gap = np.inf
    if case["nc"] > 1:
        srt = np.sort(case["cls"].astype(np.float64), -1)
        d = (srt[..., -1] - srt[..., -2])[ok]
        d = d[d > 0]
        gap = float(d.min()) if d.size else np.inf
    an_r = case["anchors"][..., 6] if case["anchors"].ndim == 3 else case["anchors"][None, :, 6]
    rot = float(np.abs(case["box"][..., 6].astype(np.float64) + an_r)[ok].min())
    return dict(thr=m_thr, gap=gap, rot=rot)


def fp32_error(case, thr):
    """The largest error of a plain numpy fp32 evaluation of decode + flip (per box column, [7]) and of the max-class sigmoid
    against the float64 reference, over EVERY anchor of the case: a property of the reference alone.  The kernels get four
    times this (FMA contraction, a device expf that is not correctly rounded)."""
    eb, es = np.zeros(7), 0.0
    for b in range(case["box"].shape[0]):
        an = case["anchors"] if case["anchors"].ndim == 2 else case["anchors"][b]
        hi = dir_flip(box_decode(case["box"][b], an), case["dir"][b])
        lo = dir_flip(box_decode(case["box"][b], an, np.float32), case["dir"][b], np.float32)
        eb = np.maximum(eb, np.abs(lo.astype(np.float64) - hi).max(0))
        es = max(es, float(np.abs(class_scores(case["cls"][b], np.float32)[0].astype(np.float64) -
                                  class_scores(case["cls"][b])[0]).max()))
    return eb, es


# ---- box layouts for NMS ------------------------------------------------------------------------------------------------
def _sites(g, n, pitch, kmax, jitter):
    """n boxes [n, 7] fp32 in sites on a `pitch` grid centred on the origin, 1..kmax boxes per site; -> (boxes, site [n])"""
    per = []
    while sum(per) < n:
        per.append(int(g.integers(1, kmax + 1)))
    per[-1] -= sum(per) - n
    ns = len(per)
    side = int(np.ceil(np.sqrt(ns)))
    site = np.repeat(np.arange(ns), per)
    cx = ((site % side) - (side - 1) / 2.0) * pitch
    cy = ((site // side) - (side - 1) / 2.0) * pitch
    b = np.zeros((n, 7), np.float32)
    b[:, 0] = cx + g.uniform(-jitter, jitter, n)
    b[:, 1] = cy + g.uniform(-jitter, jitter, n)
    b[:, 2] = -1.0
    b[:, 3] = 1.6 * g.uniform(0.8, 1.2, n)
    b[:, 4] = 3.9 * g.uniform(0.8, 1.2, n)
    b[:, 5] = 1.5
    b[:, 6] = g.uniform(-np.pi, np.pi, n)
    centre = np.stack([cx, cy], 1)
    return b, site, centre


def sites_disjoint(boxes, site, centre, pitch):
    """every box's circumscribed circle lies inside its site's cell: boxes of two sites have IoU exactly 0"""
    rad = 0.5 * np.sqrt(boxes[:, 3].astype(np.float64) ** 2 + boxes[:, 4].astype(np.float64) ** 2)
    reach = np.abs(boxes[:, :2].astype(np.float64) - centre).max(1) + rad
    return bool((reach < pitch / 2 - 1e-2).all())


def site_pairs(boxes, site):
    """oracle IoU of every pair of boxes that share a site: (i [P], j [P] with i < j, iou [P] fp32)"""
    bev = to_bev(boxes)
    order = np.argsort(site, kind="stable")
    bounds = np.flatnonzero(np.diff(site[order])) + 1
    ii, jj, vv = [], [], []
    for grp in np.split(order, bounds):
        if len(grp) < 2:
            continue
        grp = np.sort(grp)
        m = clib.boxes_iou_bev(bev[grp], bev[grp])
        a, b = np.triu_indices(len(grp), 1)
        ii.append(grp[a]); jj.append(grp[b]); vv.append(m[a, b])
    if not ii:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    return np.concatenate(ii), np.concatenate(jj), np.concatenate(vv)


def tight(n, seed):
    """Sites on a 12 m pitch, 1-6 boxes each, centres within 0.4 m: every two boxes of a site overlap well above 0.1, boxes
    of two sites not at all -- NMS keeps the top scorer of each site and nothing else.  -> (boxes [n,7], site [n], centre)"""
    return _sites(np.random.default_rng(seed), n, 12.0, 6, 0.4)


def loose(n, seed, iou_thr=0.1, exact=False):
    """Sites on a 16 m pitch, 1-9 boxes each, centres within 2.5 m, rows shuffled: in-site IoUs from 0 upward, chains of
    suppression.  The later box of every pair whose oracle IoU lies within IOU_BAND of iou_thr is dropped.
    -> (boxes, site, centre, dropped); exact: exactly n rows (drawn from a larger layout, cut after the trim)."""
    g = np.random.default_rng(seed)
    m = n + max(8, n // 16) if exact else n
    b, site, centre = _sites(g, m, 16.0, 9, 2.5)
    p = g.permutation(m)
    b, site, centre = b[p], site[p], centre[p]
    i, j, v = site_pairs(b, site)
    bad = np.unique(j[np.abs(v.astype(np.float64) - iou_thr) < IOU_BAND])
    ok = np.ones(m, bool)
    ok[bad] = False
    b, site, centre = b[ok], site[ok], centre[ok]
    if exact:
        assert len(b) >= n
        b, site, centre = b[:n], site[:n], centre[:n]
    return np.ascontiguousarray(b), site, centre, len(bad)


def chain(n):
    """w 2, l 4, r 0.05, centres 1.5 m apart along x, to be scored in descending order along the line: each box overlaps its
    two neighbours only (oracle IoU 0.140), so greedy NMS keeps 0, 2, 4, ..."""
    b = np.zeros((n, 7), np.float32)
    b[:, 0] = 1.5 * np.arange(n)
    b[:, 2] = -1.0
    b[:, 3], b[:, 4], b[:, 5], b[:, 6] = 2.0, 4.0, 1.5, 0.05
    return b


def site_winners(site, rank):
    """the rows NMS keeps of a `tight` layout: of every site the row of the lowest rank, in rank order"""
    order = np.argsort(rank, kind="stable")
    _, first = np.unique(site[order], return_index=True)
    return order[np.sort(first)]


def greedy(n, i, j, hit):
    """greedy NMS over rows 0..n-1 in row order from a pair list (i < j, hit): kept rows"""
    sup = [[] for _ in range(n)]
    for a, b in zip(i[hit], j[hit]):
        sup[a].append(b)
    dead = np.zeros(n, bool)
    keep = []
    for r in range(n):
        if not dead[r]:
            keep.append(r)
            dead[sup[r]] = True
    return np.array(keep, np.int64)


# ---- logits for rescore -------------------------------------------------------------------------------------------------
def logit_lattice(score_thr):
    """the admissible rescore logits (fp32 multiples of LOGIT_STEP in [-4, 4] whose sigmoid is 1e-3 away from score_thr),
    split into (those above the threshold, those below)"""
    k = np.arange(-int(4 / LOGIT_STEP), int(4 / LOGIT_STEP) + 1)
    v = (k * LOGIT_STEP).astype(np.float32)
    s = sigmoid64(v)
    v = v[np.abs(s - score_thr) >= 1e-3]
    s = sigmoid64(v)
    return v[s > score_thr], v[s < score_thr]


def rescore_logits(passing, seed, score_thr):
    """passing [n] bool -> [n] fp32 logits, all distinct, above score_thr exactly where `passing` is set"""
    g = np.random.default_rng(seed)
    above, below = logit_lattice(score_thr)
    passing = np.asarray(passing, bool)
    out = np.zeros(len(passing), np.float32)
    out[passing] = g.choice(above, int(passing.sum()), replace=False)
    out[~passing] = g.choice(below, int((~passing).sum()), replace=False)
    return out


def descending_logits(n, score_thr):
    """[n] fp32 distinct logits above score_thr, descending with the row index"""
    above, _ = logit_lattice(score_thr)
    assert n <= len(above)
    return np.ascontiguousarray(np.sort(above)[::-1][:n])


def logit_margins(logits, score_thr):
    """(closest gap between two unequal logits, closest |sigmoid - score_thr|)"""
    u = np.unique(np.asarray(logits, np.float64))
    gap = float(np.diff(u).min()) if len(u) > 1 else np.inf
    return gap, float(np.abs(sigmoid64(logits) - score_thr).min())


def decode_bwd_ref(box, dirp, anchors, idx, d):
    """float64 autograd of decode + flip at the anchors `idx` of one sample, the output gradient d [len(idx), 7]:
    -> (decoded [len(idx), 7], d box [len(idx), 7])"""
    t = torch.tensor(np.asarray(box)[idx], dtype=torch.float64, requires_grad=True)
    a = torch.tensor(np.asarray(anchors)[idx], dtype=torch.float64)
    za = a[:, 2] + a[:, 5] / 2
    diag = torch.sqrt(a[:, 4] ** 2 + a[:, 3] ** 2)
    hg = torch.exp(t[:, 5]) * a[:, 5]
    rg = t[:, 6] + a[:, 6]
    if dirp is not None:
        dl = torch.as_tensor(np.asarray(dirp)[idx, 1] > np.asarray(dirp)[idx, 0])
        rg = rg + ((rg.detach() > 0) != dl).double() * np.pi
    out = torch.stack([t[:, 0] * diag + a[:, 0], t[:, 1] * diag + a[:, 1], t[:, 2] * a[:, 5] + za - hg / 2,
                       torch.exp(t[:, 3]) * a[:, 3], torch.exp(t[:, 4]) * a[:, 4], hg, rg], 1)
    out.backward(torch.tensor(np.asarray(d), dtype=torch.float64))
    return out.detach().numpy(), t.grad.numpy()
