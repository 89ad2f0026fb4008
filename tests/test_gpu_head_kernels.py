"""-m gpu: the detection-head entry points alone, at their edges, against the float64 references of tests/head_cases.py:
sassd_decode_filter, sassd_pswarp_sample, sassd_rescore_nms and the first run of sassd_nms_gpu past 4096 boxes.

Discrete results (counts, order, labels, kept sets, status bits) are exact: head_cases builds the inputs so that the reference
alone decides them (test_head_cases_cpu.py checks that without a GPU).  Decoded boxes and sigmoid scores are held to four
times the error of a plain numpy fp32 evaluation of the same formulas against float64 on the same inputs (fp32_error):


  column (largest over the cases)     x        y        z        w        l        h        r        score
  numpy fp32 against float64          4.1e-6   2.2e-6   6.4e-7   8.0e-7   1.6e-6   7.6e-7   4.5e-7   8.9e-8
  bound (four times, per case)        1.6e-5   8.7e-6   2.6e-6   3.2e-6   6.5e-6   3.1e-6   1.8e-6   3.6e-7
  sassd_decode_filter, measured       3.9e-6   2.0e-6   4.5e-7   4.3e-7   1.0e-6   4.5e-7   4.5e-7   8.3e-8
  sassd_guided_decode_fwd, measured   3.0e-6   1.9e-6   2.3e-7   2.2e-7   5.8e-7   2.1e-7   3.3e-7
  sassd_rescore_nms, measured                                                                        8.4e-8

(every case measures its own fp32 figure on its own inputs and prints it with the kernel's error before it asserts: run with -s)

Every output buffer is preset to a sentinel that rows at or past the written count must keep, and `status` starts with an
unrelated bit that must survive while the overflow bit appears exactly when the reference overflows."""
import numpy as np
import pytest
import torch

import sassd
from sassd import kernels as K
import head_cases as HC

pytestmark = pytest.mark.gpu

SENT = -777.0
BIT = 2                    # an unrelated status bit (SASSD_ST_HASH_FULL) set before every call


# ---- decode_filter --------------------------------------------------------------------------------------------------------
def run_decode_filter(dev, c, thr, cap_k):
    bsz, nc, a, h, w = c["box"].shape[0], c["nc"], c["a"], c["h"], c["w"]
    assert c["anchors"].ndim == 2
    head = torch.from_numpy(c["head"]).to(dev)
    nb, ncl, _ = HC.head_channels(nc, a)
    base = head.view(-1)
    out = dict(guided=torch.full((bsz, cap_k, 7), SENT, device=dev), labels=torch.full((bsz, cap_k), int(SENT), dtype=torch.int32, device=dev),
               scores=torch.full((bsz, cap_k), SENT, device=dev), counts=torch.full((bsz,), int(SENT), dtype=torch.int32, device=dev))
    status = torch.tensor([BIT], dtype=torch.int32, device=dev)
    K.decode_filter(base, base[nb * h * w:], base[(nb + ncl) * h * w:], head.shape[1] * h * w, bsz, nc, a, h, w,
                    torch.from_numpy(c["anchors"]).to(dev), torch.from_numpy(c["mask"]).to(dev), thr, cap_k, out, status)
    return {k: v.cpu().numpy() for k, v in out.items()}, int(status.item())


def check_decode_filter(dev, c, thr, cap_k, what):
    got, status = run_decode_filter(dev, c, thr, cap_k)
    ref = HC.decode_filter_ref(c, thr, cap_k)
    eb, es = HC.fp32_error(c, thr)
    kb, ks, over = np.zeros(7), 0.0, False
    for b, r in enumerate(ref):
        n = min(r["total"], cap_k)
        over |= r["total"] > cap_k
        assert got["counts"][b] == n, (what, b, got["counts"][b], n)
        assert np.array_equal(got["labels"][b, :n], r["labels"]), (what, b)
        if n:
            kb = np.maximum(kb, np.abs(got["guided"][b, :n].astype(np.float64) - r["boxes"]).max(0))
            ks = max(ks, float(np.abs(got["scores"][b, :n].astype(np.float64) - r["scores"]).max()))
        assert (got["guided"][b, n:] == SENT).all() and (got["scores"][b, n:] == SENT).all(), (what, b)
        assert (got["labels"][b, n:] == int(SENT)).all(), (what, b)
    print("decode_filter[%s]: fp32 box error %s, bound x4, kernel %s; fp32 score error %.3g, kernel %.3g"
          % (what, np.array2string(eb, precision=3), np.array2string(kb, precision=3), es, ks))
    assert (kb <= 4 * eb).all(), (what, kb, 4 * eb)
    assert ks <= 4 * es, (what, ks, 4 * es)
    assert status == (BIT | (HC.ST_BOX_OVERFLOW if over else 0)), (what, status, over)
    return got, ref


@pytest.mark.parametrize("nc,h,w", [(1, 5, 7), (3, 5, 7), (1, 23, 57), (3, 19, 23)])
def test_decode_filter_free_draw(dev, nc, h, w):
    """whatever a free draw selects: below one block (Atot 70 and 210) and over three ragged blocks (Atot 2622, both ways)"""
    c = HC.head_case(20 + nc, 2, nc, 2, h, w, 0.3)
    got, ref = check_decode_filter(dev, c, 0.3, c["atot"], "free nc%d %dx%d" % (nc, h, w))
    assert all(0 < r["total"] < c["atot"] for r in ref)


@pytest.mark.parametrize("nc", [1, 3])
def test_decode_filter_selections(dev, nc):
    h, w = (23, 57) if nc == 1 else (19, 23)                                     # Atot = 2622: blocks of 1024, 1024 and 574
    atot = nc * 2 * h * w
    g = np.random.default_rng(nc)
    # nothing selected beside a sample whose mask is all zero
    c = HC.head_case(30, 2, nc, 2, h, w, 0.3, want=[[], None])
    c["mask"][1] = 0
    check_decode_filter(dev, c, 0.3, 64, "none")
    # the four anchors of one thread; a run across the first block boundary and one up to the last anchor
    c = HC.head_case(31, 2, nc, 2, h, w, 0.3, want=[[400, 401, 402, 403], list(range(1019, 1030)) + list(range(atot - 5, atot))])
    check_decode_filter(dev, c, 0.3, 64, "thread and boundary")
    # exactly cap_k beside cap_k + 1, then exactly cap_k alone: the overflow bit comes with the first only
    full, more = np.sort(g.choice(atot, 64, replace=False)), np.sort(g.choice(atot, 65, replace=False))
    c = HC.head_case(32, 2, nc, 2, h, w, 0.3, want=[full, more])
    got, ref = check_decode_filter(dev, c, 0.3, 64, "cap_k and cap_k + 1")
    assert ref[0]["total"] == 64 and ref[1]["total"] == 65 and np.array_equal(ref[1]["idx"], more[:64])
    c = HC.head_case(33, 2, nc, 2, h, w, 0.3, want=[full, full[:10]])
    check_decode_filter(dev, c, 0.3, 64, "cap_k")


def test_decode_filter_258_blocks(dev):
    """363 x 363 x 2 anchors = 263538: 258 blocks, so the sum over the blocks in front takes a second trip (j += 256) from block
    257 on.  The selected anchors sit in block 0, on both sides of the ends of blocks 254 to 256, and in the ragged last block."""
    atot = 2 * 363 * 363
    assert atot == 263538 and -(-atot // 1024) == 258
    e = 1024
    want0 = [0, 5, 1023, 255 * e - 1, 255 * e, 256 * e - 1, 256 * e, 257 * e - 1, 257 * e, 257 * e + 100, atot - 1]
    want1 = [100 * e + 3, 256 * e + 7, atot - 2]
    c = HC.head_case(40, 2, 1, 2, 363, 363, 0.3, want=[want0, want1])
    got, ref = check_decode_filter(dev, c, 0.3, 16, "258 blocks")
    assert np.array_equal(ref[0]["idx"], want0) and np.array_equal(ref[1]["idx"], want1)


def test_decode_filter_exact_cases(dev):
    """thr 0.5, three classes: a best logit of exactly 0 is not selected (strict >), equal class logits go to the lower class,
    equal direction logits mean direction 0, and rt = -ra gives a rotation of exactly 0 (kept with direction 0, pi with 1)"""
    sel = [1, 2, 3, 4, 5, 7]
    c = HC.head_case(50, 1, 3, 2, 5, 7, 0.5, want=[sel])
    cls, dirp, box, an = c["cls"][0], c["dir"][0], c["box"][0], c["anchors"]
    c["mask"][0, 0] = 1
    cls[0] = [0.0, -1.0, 0.0]
    cls[1] = [1.0, 1.0, -2.0]
    cls[2] = [-1.0, 2.0, 2.0]
    dirp[3] = [0.25, 0.25]
    box[3, 6] = 0.5 - an[3, 6]                       # rotation > 0, direction 0: flipped
    dirp[4] = [-1.5, -1.5]
    box[4, 6] = -0.5 - an[4, 6]                      # rotation < 0, direction 0: kept
    box[5, 6], box[7, 6] = -an[5, 6], -an[7, 6]
    assert an[5, 6] == np.float32(1.57) and an[7, 6] == np.float32(1.57)
    dirp[5] = [1.0, 0.0]
    dirp[7] = [0.0, 1.0]
    HC.finish(c)
    got, ref = check_decode_filter(dev, c, 0.5, 16, "exact")
    assert np.array_equal(ref[0]["idx"], sel)
    assert got["labels"][0, :6].tolist()[:2] == [0, 1]
    rot = got["guided"][0, :6, 6]
    assert abs(rot[2] - (0.5 + np.pi)) < 1e-6 and abs(rot[3] + 0.5) < 1e-6
    assert rot[4] == 0.0 and rot[5] == np.float32(np.pi)


# ---- pswarp_sample --------------------------------------------------------------------------------------------------------
PS_H, PS_W, PS_OFF, PS_SCALE = 9, 13, (1.0, 2.0), 2.0          # the map covers x in [-1, 5], y in [-2, 2]
PS_POOL = np.array([
    [2.0, 0.0, 0, 1.0, 1.6, 1, 0.3],                 # inside
    [4.0, 1.0, 0, 2.0, 2.0, 1, 0.0],                 # grid corners on integer pixels, the last column and the last row
    [-1.0, 0.2, 0, 1.0, 1.6, 1, -0.4],               # across the left border
    [20.0, 20.0, 0, 1.0, 1.6, 1, 0.5],               # wholly outside: exactly 0
    [5.0, -0.3, 0, 1.0, 1.6, 1, 2.5],                # across the right border
    [1.5, -0.5, 0, 0.8, 1.5, 1, 2.0],                # inside
    [2.2, -2.0, 0, 1.0, 1.6, 1, 0.9],                # across the top border
    [0.0, -1.0, 0, 2.0, 2.0, 1, 0.0],                # integer pixels, the first column and the first row
    [3.1, 2.0, 0, 1.0, 1.6, 1, -1.2],                # across the bottom border
    [-10.0, 0.0, 0, 1.0, 1.6, 1, 0.0],               # wholly outside: exactly 0
    [2.0, 0.0, 0, 2.0, 2.0, 1, 0.0],                 # integer pixels inside
    [5.0, 2.0, 0, 1.5, 3.0, 1, 0.7],                 # across a corner
    [2.0, 0.0, 0, 8.0, 10.0, 1, 0.4],                # larger than the map
], np.float32)


@pytest.mark.parametrize("cap_k", [5, 8, 13])
def test_pswarp_sample(dev, cap_k):
    g = torch.Generator().manual_seed(cap_k)
    feat = torch.randn(2, 28, PS_H, PS_W, generator=g)
    fd = feat.to(dev)
    worst = 0.0
    for counts in [(0, cap_k), (3, cap_k + 4), (cap_k, 1)]:
        boxes = np.stack([np.roll(PS_POOL, -4 * b - counts[0], 0)[:cap_k] for b in range(2)])
        logits = torch.full((2, cap_k), SENT, device=dev)
        K.pswarp_sample(fd, torch.from_numpy(boxes).to(dev), torch.tensor(counts, dtype=torch.int32, device=dev), cap_k, PS_OFF,
                        PS_SCALE, logits)
        got = logits.cpu().numpy()
        for b in range(2):
            n = min(counts[b], cap_k)
            ref = HC.pswarp_ref(feat[b].numpy(), boxes[b, :n], PS_OFF, PS_SCALE)
            if n:
                worst = max(worst, float(np.abs(got[b, :n] - ref).max()))
            assert (got[b, n:] == SENT).all(), (counts, b)
            outside = np.abs(boxes[b, :n, 0]) >= 10
            assert (got[b, :n][outside] == 0.0).all() and (ref[outside] == 0.0).all()
            assert (np.abs(ref[~outside]) > 0).all()
    print("pswarp_sample[cap_k %d]: max |kernel - float64 grid_sample| = %.3g (bar 1e-5)" % (cap_k, worst))
    assert worst < 1e-5


def test_pswarp_sample_channel_to_grid_point(dev):
    """channel k is read at grid point (k // 7, k % 7) and nowhere else: a box whose 4 x 7 grid points fall on the pixels
    (3 + ix, 1 + iy), one-hot maps with channel k lit at its own pixel, then their complements"""
    box = np.zeros((1, 2, 7), np.float32)
    box[0, :] = [1.25, 0.0, 0, 1.5, 3.0, 1, 0.0]
    onehot = np.zeros((1, 28, PS_H, PS_W), np.float32)
    for k in range(28):
        onehot[0, k, 1 + k % 7, 3 + k // 7] = 1.0
    cnt = torch.tensor([2], dtype=torch.int32, device=dev)
    for feat, want in ((onehot, 1.0), (1.0 - onehot, 0.0)):
        got = K.pswarp_sample(torch.from_numpy(feat).to(dev), torch.from_numpy(box).to(dev), cnt, 2, PS_OFF, PS_SCALE).cpu().numpy()
        ref = HC.pswarp_ref(feat[0], box[0], PS_OFF, PS_SCALE)
        assert np.abs(ref - want).max() < 1e-6
        assert np.abs(got[0] - ref).max() < 1e-5, (want, got)


# ---- rescore_nms ----------------------------------------------------------------------------------------------------------
SCORE_THR, IOU_THR = 0.3, 0.1


def rn_sample(passing_boxes, cap_k, seed, n_fail=0, logits_pass=None):
    """One sample of rescore inputs: the passing boxes with logits above SCORE_THR, n_fail rows below it mixed in (copies of
    passing boxes: they would suppress their originals if they were let through), then rows past the count that would win
    everything if the count were ignored.  -> (guided [cap_k,7], logits [cap_k], labels [cap_k], count)"""
    g = np.random.default_rng(seed)
    m = len(passing_boxes)
    n = m + n_fail
    assert n <= cap_k
    passing = np.zeros(n, bool)
    passing[np.sort(g.permutation(n)[:m])] = True
    guided = np.zeros((cap_k, 7), np.float32)
    guided[:n][passing] = passing_boxes
    if n_fail:
        guided[:n][~passing] = passing_boxes[g.integers(0, m, n_fail)] if m else HC.chain(n_fail)
    guided[n:] = passing_boxes[0] if m else 0.0
    logits = np.full(cap_k, 4.0, np.float32)
    logits[:n] = HC.rescore_logits(passing, seed, SCORE_THR)
    if logits_pass is not None:
        logits[:n][passing] = logits_pass
    labels = g.integers(0, 3, cap_k).astype(np.int32)
    return guided, logits, labels, n


def run_rescore(dev, samples, cap_d, counts=None):
    """samples: rn_sample tuples of one cap_k -> (outputs as numpy, status)"""
    guided = torch.from_numpy(np.stack([s[0] for s in samples])).to(dev)
    logits = torch.from_numpy(np.stack([s[1] for s in samples])).to(dev)
    labels = torch.from_numpy(np.stack([s[2] for s in samples])).to(dev)
    cnt = torch.tensor([s[3] for s in samples] if counts is None else counts, dtype=torch.int32, device=dev)
    bsz = len(samples)
    out = dict(boxes=torch.full((bsz, cap_d, 7), SENT, device=dev), scores=torch.full((bsz, cap_d), SENT, device=dev),
               labels=torch.full((bsz, cap_d), int(SENT), dtype=torch.int32, device=dev),
               counts=torch.full((bsz,), int(SENT), dtype=torch.int32, device=dev))
    status = torch.tensor([BIT], dtype=torch.int32, device=dev)
    K.rescore_nms(guided, logits, labels, cnt, SCORE_THR, IOU_THR, cap_d, out, status)
    return {k: v.cpu().numpy() for k, v in out.items()}, int(status.item())


def sigmoid_fp32_error(logits):
    lg = np.asarray(logits, np.float32)
    s32 = np.float32(1) / (np.float32(1) + np.exp(-lg))
    return float(np.abs(s32.astype(np.float64) - HC.sigmoid64(lg)).max())


def check_rescore(dev, samples, cap_d, what, counts=None, expect_rows=None):
    """against rescore_ref, or against expect_rows (per sample: the kept rows in order, uncut) where the layout names them"""
    got, status = run_rescore(dev, samples, cap_d, counts)
    cap_k = samples[0][0].shape[0]
    over, ks = False, 0.0
    es = max(sigmoid_fp32_error(s[1]) for s in samples)
    for b, (guided, logits, labels, n) in enumerate(samples):
        n = n if counts is None else counts[b]
        if expect_rows is not None:
            rows = np.asarray(expect_rows[b], np.int64)
            kept, rows = len(rows), rows[:cap_d]
            scores = HC.sigmoid64(logits[rows])
        else:
            r = HC.rescore_ref(guided, logits, labels, n, cap_k, SCORE_THR, IOU_THR, cap_d)
            rows, scores, kept = r["rows"], r["scores"], r["kept"]
        over |= kept > cap_d
        k = len(rows)
        assert got["counts"][b] == k, (what, b, got["counts"][b], k)
        assert np.array_equal(got["boxes"][b, :k].view(np.uint32), guided[rows].view(np.uint32)), (what, b)
        assert np.array_equal(got["labels"][b, :k], labels[rows]), (what, b)
        if k:
            ks = max(ks, float(np.abs(got["scores"][b, :k].astype(np.float64) - scores).max()))
        assert (got["boxes"][b, k:] == SENT).all() and (got["scores"][b, k:] == SENT).all(), (what, b)
        assert (got["labels"][b, k:] == int(SENT)).all(), (what, b)
    print("rescore_nms[%s]: fp32 sigmoid error %.3g, bound x4, kernel %.3g" % (what, es, ks))
    assert ks <= 4 * es, (what, ks, 4 * es)
    assert status == (BIT | (HC.ST_BOX_OVERFLOW if over else 0)), (what, status, over)
    return got


@pytest.mark.parametrize("m", [1, 63, 64, 65, 129])
def test_rescore_loose(dev, m):
    b = HC.loose(m, 10 + m, exact=True)[0]
    s = rn_sample(b, 256, m, n_fail=min(40, 256 - m))
    r = HC.rescore_ref(s[0], s[1], s[2], s[3], 256, SCORE_THR, IOU_THR, 256)
    assert r["m"] == m and (m < 63 or r["kept"] < m)
    check_rescore(dev, [s], 256, "loose %d" % m)


def test_rescore_loose_1100(dev):
    """1400 candidates, 1100 of them above the threshold: the second trip of the scan loop, 18 column blocks"""
    b = HC.loose(1100, 4, exact=True)[0]
    s = rn_sample(b, 2048, 4, n_fail=300)
    r = HC.rescore_ref(s[0], s[1], s[2], s[3], 2048, SCORE_THR, IOU_THR, 2048)
    assert r["m"] == 1100 and 300 < r["kept"] < 1000
    check_rescore(dev, [s], 1024, "loose 1100")


def test_rescore_tight_4096(dev):
    """a full cap_k = 4096 above the threshold (64 column blocks): the top scorer of each site in score order; then cap_d = 300
    below the kept count: the first 300 of them and the overflow bit"""
    b, site, _ = HC.tight(4096, 0)
    s = rn_sample(b, 4096, 6)
    assert s[3] == 4096
    rank = np.argsort(np.argsort(-s[1].astype(np.float64), kind="stable"), kind="stable")
    rows = HC.site_winners(site, rank)
    assert 700 < len(rows) < 2048
    check_rescore(dev, [s], 2048, "tight 4096", expect_rows=[rows])
    check_rescore(dev, [s], 300, "tight 4096, cap_d 300", expect_rows=[rows])


def test_rescore_chain(dev):
    """every decision at 63 -> 64 and 127 -> 128 depends on what the block before kept"""
    b = HC.chain(200)
    s = rn_sample(b, 256, 7, logits_pass=HC.descending_logits(200, SCORE_THR))
    check_rescore(dev, [s], 256, "chain", expect_rows=[np.arange(0, 200, 2)])
    check_rescore(dev, [s], 256, "chain against the reference")
    # one box far away in front: the chain's kept rows are now 1, 3, ..., so 63 suppresses 64 and 127 suppresses 128 -- the
    # only suppressions of the layout that reach from one block of 64 into the next
    far = HC.chain(1)
    far[0, 0] = -100.0
    s = rn_sample(np.concatenate([far, HC.chain(199)]), 256, 7, logits_pass=HC.descending_logits(200, SCORE_THR))
    check_rescore(dev, [s], 256, "chain behind one box", expect_rows=[np.concatenate([[0], np.arange(1, 200, 2)])])


def test_rescore_batch_and_workspace_reuse(dev):
    """B = 3 with counts (0, cap_k, all below the threshold); then a small sample after a large one in the same workspace,
    bit-equal to the small sample run in a workspace of its own"""
    full = rn_sample(HC.loose(200, 8, exact=True)[0], 256, 8, n_fail=56)
    assert full[3] == 256
    empty = (full[0], full[1], full[2], 0)
    below = rn_sample(np.zeros((0, 7), np.float32), 256, 9, n_fail=100)
    got = check_rescore(dev, [empty, full, below], 256, "batch")
    assert got["counts"][0] == 0 and got["counts"][2] == 0 and got["counts"][1] > 0
    small = rn_sample(HC.loose(70, 9, exact=True)[0], 2048, 9, n_fail=10)
    large = rn_sample(HC.loose(1100, 4, exact=True)[0], 2048, 4, n_fail=300)
    for key in [k for k in K._ws_cache if k[0] == "rescore_nms"]:
        del K._ws_cache[key]
    alone = check_rescore(dev, [small], 128, "small alone")
    check_rescore(dev, [large], 1024, "large")
    again = check_rescore(dev, [small], 128, "small after large")
    for k in alone:
        assert np.array_equal(alone[k].view(np.uint32), again[k].view(np.uint32)), k


def test_rescore_ties(dev):
    b = HC.loose(129, 12, exact=True)[0]
    # all logits equal: the output is in input order
    s = rn_sample(b, 256, 12, logits_pass=np.full(129, 0.5, np.float32))
    got = check_rescore(dev, [s], 256, "all equal")
    rows = HC.rescore_ref(s[0], s[1], s[2], s[3], 256, SCORE_THR, IOU_THR, 256)["rows"]
    assert (np.diff(rows) > 0).all()
    # ten rows share one score, and the group lies across rank 64
    s = rn_sample(b, 256, 13)
    passing = np.flatnonzero(HC.sigmoid64(s[1][:s[3]]) > SCORE_THR)
    by_rank = passing[np.argsort(-s[1][passing].astype(np.float64), kind="stable")]
    s[1][by_rank[60:70]] = s[1][by_rank[60]]
    check_rescore(dev, [s], 256, "ties across rank 64")


def test_rescore_count_above_cap_k_is_clamped(dev):
    b = HC.loose(200, 14, exact=True)[0]
    s = rn_sample(b, 256, 14, n_fail=56)
    check_rescore(dev, [s], 256, "counts > cap_k", counts=[256 + 50])


# ---- nms_gpu --------------------------------------------------------------------------------------------------------------
def test_nms_gpu_4160_boxes(dev):
    """65 column blocks: the first run of the path for more than 4096 boxes, against the per-site rule of the tight layout"""
    b, site, _ = HC.tight(4160, 1)
    order = np.random.default_rng(2).permutation(4160)                   # the score order
    bev = np.ascontiguousarray(HC.to_bev(b[order]))
    keep, num = K.nms_gpu(torch.from_numpy(bev).to(dev), IOU_THR)
    want = HC.site_winners(site[order], np.arange(4160))
    k = int(num.item())
    assert k == len(want) and np.array_equal(keep[:k].cpu().numpy(), want)
