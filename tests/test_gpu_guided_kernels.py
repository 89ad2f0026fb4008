"""-m gpu: the training twins of the detection head alone -- sassd_guided_select, sassd_guided_decode_fwd and
sassd_guided_decode_bwd -- on the anchor-major view of the very head tensors test_gpu_head_kernels.py feeds sassd_decode_filter
(tests/head_cases.py), against the same float64 references and against sassd_decode_filter's own rows.

Selected sets, counts, padding and the overflow flag are exact.  Decoded rows are held to four times the error of a plain numpy
fp32 evaluation against float64 on the same inputs (head_cases.fp32_error; figures in test_gpu_head_kernels.py's docstring),
gradients to 1e-5 x max(1, max |reference|) against float64 autograd."""
import numpy as np
import pytest
import torch

import sassd
from sassd import kernels as K
import head_cases as HC
from test_gpu_head_kernels import run_decode_filter

pytestmark = pytest.mark.gpu


def dev_case(dev, c):
    return {k: torch.from_numpy(c[k]).to(dev) for k in ("box", "cls", "dir", "anchors", "mask")}


def check_select(dev, c, thr, cap, flag, masked=True):
    """guided_select against the reference: ascending selected anchors cut at cap, padding sel[b][p] = p, counts; `flag`
    (the persistent overflow word) is set by an overflowing sample and never cleared.  -> (sel, counts) on the device"""
    d = dev_case(dev, c)
    before = int(flag.item())
    sel, cnt = K.guided_select(d["cls"], d["mask"] if masked else None, thr, cap, flag)
    ref = HC.decode_filter_ref(c, thr, cap, masked=masked)
    s, n = sel.cpu().numpy(), cnt.cpu().numpy()
    for b, r in enumerate(ref):
        k = min(r["total"], cap)
        assert n[b] == k, (b, n[b], k)
        assert np.array_equal(s[b, :k], r["idx"]), b
        assert np.array_equal(s[b, k:], np.arange(k, cap)), b
    over = any(r["total"] > cap for r in ref)
    assert int(flag.item()) == (1 if over or before else 0)
    return sel, cnt, ref


@pytest.mark.parametrize("nc,h,w", [(1, 5, 7), (3, 5, 7), (3, 19, 23)])
def test_guided_select_free_draw(dev, nc, h, w):
    c = HC.head_case(20 + nc, 2, nc, 2, h, w, 0.3)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _, _, ref = check_select(dev, c, 0.3, c["atot"], flag)
    _, _, unmasked = check_select(dev, c, 0.3, c["atot"], flag, masked=False)
    assert all(u["total"] > r["total"] > 0 for u, r in zip(unmasked, ref))
    # the same set as sassd_decode_filter selects from the head tensor of these numbers
    got, _ = run_decode_filter(dev, c, 0.3, c["atot"])
    assert [int(v) for v in got["counts"]] == [r["total"] for r in ref]


def test_guided_select_capacity_and_flag(dev):
    nc, h, w = 3, 19, 23
    atot = nc * 2 * h * w
    g = np.random.default_rng(3)
    full, more = np.sort(g.choice(atot, 64, replace=False)), np.sort(g.choice(atot, 65, replace=False))
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    c = HC.head_case(33, 2, nc, 2, h, w, 0.3, want=[full, full[:10]])
    check_select(dev, c, 0.3, 64, flag)                                    # exactly cap: no overflow
    assert int(flag.item()) == 0
    c2 = HC.head_case(32, 2, nc, 2, h, w, 0.3, want=[full, more])
    _, cnt, ref = check_select(dev, c2, 0.3, 64, flag)                     # cap + 1: the first cap, the flag
    assert int(flag.item()) == 1 and ref[1]["total"] == 65 and cnt.cpu().tolist() == [64, 64]
    check_select(dev, c, 0.3, 64, flag)                                    # the flag is persistent
    assert int(flag.item()) == 1
    # nothing selected beside a sample whose mask is all zero
    c = HC.head_case(30, 2, nc, 2, h, w, 0.3, want=[[], None])
    c["mask"][1] = 0
    _, cnt, _ = check_select(dev, c, 0.3, 64, torch.zeros(1, dtype=torch.int32, device=dev))
    assert cnt.cpu().tolist() == [0, 0]


def test_guided_select_1030_blocks(dev):
    """263538 anchors: 1030 blocks of 256, so the sum over the blocks in front takes up to five trips (i += 256)"""
    atot = 2 * 363 * 363
    e = 1024
    want0 = [0, 5, 1023, 255 * e - 1, 255 * e, 256 * e - 1, 256 * e, 257 * e - 1, 257 * e, 257 * e + 100, atot - 1]
    want1 = [100 * e + 3, 256 * e + 7, atot - 2]
    c = HC.head_case(40, 2, 1, 2, 363, 363, 0.3, want=[want0, want1])
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _, _, ref = check_select(dev, c, 0.3, 16, flag)
    assert np.array_equal(ref[0]["idx"], want0) and np.array_equal(ref[1]["idx"], want1)
    # without the mask every anchor above the threshold counts: far more than cap, the first cap in anchor order
    _, cnt, _ = check_select(dev, c, 0.3, 16, flag, masked=False)
    assert int(flag.item()) == 1 and cnt.cpu().tolist() == [16, 16]


# ---- guided_decode_fwd / _bwd -------------------------------------------------------------------------------------------
def gt_boxes(seed, n):
    g = np.random.default_rng(seed)
    b = np.zeros((n, 7), np.float32)
    b[:, 0] = g.uniform(0, 70, n); b[:, 1] = g.uniform(-40, 40, n); b[:, 2] = g.uniform(-1.9, -1.5, n)
    b[:, 3] = g.uniform(1.5, 1.8, n); b[:, 4] = g.uniform(3.5, 4.4, n); b[:, 5] = g.uniform(1.4, 1.7, n)
    b[:, 6] = g.uniform(-3.1, 3.1, n)
    return b


def padded_sel(ref, cap):
    sel = np.tile(np.arange(cap, dtype=np.int64), (len(ref), 1))
    for b, r in enumerate(ref):
        sel[b, :len(r["idx"])] = r["idx"]
    return sel


def check_decode_fwd(dev, c, thr, cap, g_per_sample, gmax, with_dir=True, sel_count=None, what=""):
    """guided_decode_fwd on the reference's own selection (sel, counts built on the host) against the float64 reference:
    ground truth first bit for bit, decoded rows within four times the fp32 figure, zero rows behind, counts"""
    d = dev_case(dev, c)
    ref = HC.decode_filter_ref(c, thr, cap)
    sel = padded_sel(ref, cap)
    cnt = [len(r["idx"]) for r in ref] if sel_count is None else sel_count
    gt = gt_boxes(5, sum(g_per_sample))
    off = np.concatenate([[0], np.cumsum(g_per_sample)]).astype(np.int32)
    guided, counts = K.guided_decode_fwd(d["box"], d["dir"] if with_dir else None, d["anchors"], torch.from_numpy(sel).to(dev),
                                         torch.tensor(cnt, dtype=torch.int32, device=dev),
                                         torch.from_numpy(gt).to(dev) if gmax else None, torch.from_numpy(off).to(dev), gmax)
    got, n = guided.cpu().numpy(), counts.cpu().numpy()
    assert got.shape == (len(ref), gmax + cap, 7)
    eb, _ = HC.fp32_error(c, thr)
    kb = np.zeros(7)
    for b, r in enumerate(ref):
        gb, k = g_per_sample[b], min(cnt[b], cap)
        assert n[b] == gb + k, (what, b)
        assert np.array_equal(got[b, :gb].view(np.uint32), gt[off[b]:off[b + 1]].view(np.uint32)), (what, b)
        an = c["anchors"] if c["anchors"].ndim == 2 else c["anchors"][b]
        rows = sel[b, :k]
        want = HC.box_decode(c["box"][b][rows], an[rows])
        if with_dir:
            want = HC.dir_flip(want, c["dir"][b][rows])
        if k:
            kb = np.maximum(kb, np.abs(got[b, gb:gb + k].astype(np.float64) - want).max(0))
        assert (got[b, gb + k:] == 0).all(), (what, b)
    print("guided_decode_fwd[%s]: fp32 box error %s, bound x4, kernel %s"
          % (what, np.array2string(eb, precision=3), np.array2string(kb, precision=3)))
    assert (kb <= 4 * eb).all(), (what, kb, 4 * eb)
    return got, ref


@pytest.mark.parametrize("per_sample", [False, True])
def test_guided_decode_fwd(dev, per_sample):
    nc, h, w = 3, 19, 23
    c = HC.head_case(60, 2, nc, 2, h, w, 0.3, want=[list(range(1019, 1030)) + [7, 2600], [3, 4, 900]], per_sample_anchors=per_sample)
    check_decode_fwd(dev, c, 0.3, 32, [0, 0], 0, what="gmax 0")
    check_decode_fwd(dev, c, 0.3, 32, [0, 6], 6, what="G = 0 beside G = gmax")
    check_decode_fwd(dev, c, 0.3, 32, [2, 5], 6, with_dir=False, what="no direction head")
    # a sample that selected nothing beside one that selected exactly cap; then its count above cap, cut to cap
    c0 = HC.head_case(61, 2, nc, 2, h, w, 0.3, want=[[], list(range(40, 80))], per_sample_anchors=per_sample)
    check_decode_fwd(dev, c0, 0.3, 40, [3, 1], 4, what="cnt 0")
    check_decode_fwd(dev, c0, 0.3, 40, [3, 1], 4, sel_count=[0, 47], what="cnt > cap")


def test_guided_decode_matches_decode_filter(dev):
    """select -> decode on the anchor-major tensors gives the rows decode_filter gives on the head tensor of the same numbers"""
    for nc, h, w, seed in [(1, 5, 7, 21), (3, 19, 23, 23)]:
        c = HC.head_case(seed, 2, nc, 2, h, w, 0.3)
        cap = c["atot"]
        d = dev_case(dev, c)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        sel, cnt = K.guided_select(d["cls"], d["mask"], 0.3, cap, flag)
        off = torch.zeros(3, dtype=torch.int32, device=dev)
        guided, counts = K.guided_decode_fwd(d["box"], d["dir"], d["anchors"], sel, cnt, None, off, 0)
        df, _ = run_decode_filter(dev, c, 0.3, cap)
        eb, _ = HC.fp32_error(c, 0.3)
        got = guided.cpu().numpy()
        assert np.array_equal(counts.cpu().numpy(), df["counts"])
        for b in range(2):
            k = int(df["counts"][b])
            assert k > 0 and (np.abs(got[b, :k].astype(np.float64) - df["guided"][b, :k]).max(0) <= 4 * eb).all()


@pytest.mark.parametrize("per_sample", [False, True])
def test_guided_decode_bwd(dev, per_sample):
    """d box against float64 autograd of decode + flip: exactly 0 at unselected anchors, nothing from the gradient aimed at
    ground-truth rows and at the rows behind the count, nothing from the flip"""
    nc, h, w, cap, gmax = 3, 19, 23, 13, 6                     # sample 0 selects exactly cap anchors
    c = HC.head_case(62, 2, nc, 2, h, w, 0.3, want=[list(range(1019, 1030)) + [7, 2600], [3, 4, 900]], per_sample_anchors=per_sample)
    d = dev_case(dev, c)
    ref = HC.decode_filter_ref(c, 0.3, cap)
    sel = padded_sel(ref, cap)
    g_per_sample = [6, 2]
    off = np.array([0, 6, 8], np.int32)
    dg = np.random.default_rng(1).normal(0, 1, (2, gmax + cap, 7)).astype(np.float32)
    assert [len(r["idx"]) for r in ref] == [13, 3]
    for cnt in ([13, 3], [cap + 9, 0]):                         # a count above cap is cut to cap
        dbox = K.guided_decode_bwd(d["box"], d["anchors"], torch.from_numpy(sel).to(dev), torch.tensor(cnt, dtype=torch.int32, device=dev),
                                   torch.from_numpy(off).to(dev), gmax, torch.from_numpy(dg).to(dev)).cpu().numpy()
        worst = 0.0
        for b in range(2):
            k, gb = min(cnt[b], cap), g_per_sample[b]
            rows = sel[b, :k]
            an = c["anchors"] if c["anchors"].ndim == 2 else c["anchors"][b]
            want = np.zeros((c["atot"], 7))
            if k:
                want[rows] = HC.decode_bwd_ref(c["box"][b], c["dir"][b], an, rows, dg[b, gb:gb + k])[1]
            rest = np.ones(c["atot"], bool)
            rest[rows] = False
            assert (dbox[b][rest] == 0).all(), b
            bar = 1e-5 * max(1.0, float(np.abs(want).max()))
            err = float(np.abs(dbox[b] - want).max())
            worst = max(worst, err / bar)
            assert err <= bar, (b, err, bar)
        print("guided_decode_bwd[counts %s]: largest error %.3g of its bar" % (cnt, worst))
