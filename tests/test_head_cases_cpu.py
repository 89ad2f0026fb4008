"""The conditions the detection-head kernel tests rest on, checked without a GPU: the layouts of tests/head_cases.py decide
every NMS outcome away from the IoU threshold, its references agree with the committed oracle (oracle/nets.py) on the same
fp32 inputs, and every margin its builders promise holds."""
import numpy as np
import pytest
import torch

from oracle import clib
from oracle import nets as onets
import head_cases as HC


# ---- layouts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 129, 1100, 2048])
@pytest.mark.parametrize("seed", [0, 1])
def test_loose_layout(n, seed):
    b, site, centre, dropped = HC.loose(n, seed)
    assert dropped <= 0.02 * n and len(b) == n - dropped
    assert HC.sites_disjoint(b, site, centre, 16.0)
    i, j, v = HC.site_pairs(b, site)
    assert not np.any(np.abs(v.astype(np.float64) - 0.1) < HC.IOU_BAND)
    assert np.any((v > 0) & (v < 0.1)) and np.any(v > 0.1)
    # chains: a box that an earlier, itself suppressed, box overlaps is kept by the greedy pass and dropped by the naive rule
    hit = v > 0.1
    kept = HC.greedy(len(b), i, j, hit)
    naive = np.setdiff1d(np.arange(len(b)), j[hit])
    assert len(kept) > len(naive) and set(naive) < set(kept)
    # the pair list is the whole story: the oracle's NMS over all pairs keeps the same rows
    assert np.array_equal(clib.nms_rotated(HC.to_bev(b), 0.1), kept)
    if n >= 1100:
        assert np.sum((v > 0) & (v < 0.1)) > 400 and len(kept) > 1.03 * len(naive)


def test_loose_exact_counts():
    for m in (1, 63, 64, 65, 129, 1100):
        b, site, centre, _ = HC.loose(m, 3, exact=True)
        assert len(b) == m
        i, j, v = HC.site_pairs(b, site)
        assert not np.any(np.abs(v.astype(np.float64) - 0.1) < HC.IOU_BAND)


@pytest.mark.parametrize("n", [4096, 4160])
def test_tight_layout(n):
    b, site, centre = HC.tight(n, 0)
    assert len(b) == n and HC.sites_disjoint(b, site, centre, 12.0)
    i, j, v = HC.site_pairs(b, site)
    assert len(v) > n and v.min() >= 0.11
    counts = np.bincount(site)
    assert counts.min() >= 1 and counts.max() <= 6 and len(counts) > n // 6
    # the per-site rule is what the oracle's NMS does: checked on the first sites (the whole layout costs n^2 / 2 IoUs)
    m = int(np.searchsorted(np.cumsum(counts), 300))
    sub = site < m
    rank = np.random.default_rng(1).permutation(int(sub.sum()))
    order = np.argsort(rank)
    keep = clib.nms_rotated(HC.to_bev(b[sub][order]), 0.1)
    assert np.array_equal(order[keep], HC.site_winners(site[sub], rank))


def test_chain_layout():
    b = HC.chain(200)
    bev = HC.to_bev(b)
    m = clib.boxes_iou_bev(bev[:6], bev[:6])
    assert abs(m[0, 1] - 0.140) < 1e-3 and m[0, 1] > 0.11 and m[2, 3] > 0.11
    assert m[0, 2] == 0.0 and m[1, 3] == 0.0 and m[0, 3] == 0.0
    far = clib.boxes_iou_bev(bev[100:101], bev[102:200])
    assert (far == 0).all()
    assert np.array_equal(clib.nms_rotated(bev, 0.1), np.arange(0, 200, 2))


# ---- references against the committed oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("nc,thr", [(1, 0.3), (3, 0.3), (3, 0.5)])
def test_decode_filter_reference_agrees_with_oracle(nc, thr):
    c = HC.head_case(7 + nc, 2, nc, 2, 5, 7, thr)
    ref = HC.decode_filter_ref(c, thr, c["atot"], np.float32)
    hi = HC.decode_filter_ref(c, thr, c["atot"])
    an = torch.from_numpy(c["anchors"]).unsqueeze(0).expand(2, -1, -1)
    args = (torch.from_numpy(c["cls"]), torch.from_numpy(c["dir"]), an, torch.from_numpy(c["mask"]).bool())
    got = onets.guided_anchors(torch.from_numpy(c["box"]), *args, num_class=nc, thr=thr)
    # the oracle returns no indices: a second call whose boxes decode to x = anchor index names them
    tag = np.zeros_like(c["box"])
    ian = np.zeros((2, c["atot"], 7), np.float32)
    ian[:, :, 0] = np.arange(c["atot"])
    ian[:, :, 3:6] = 1.0
    ian[:, :, 6] = 1.0
    names = onets.guided_anchors(torch.from_numpy(tag), args[0], args[1], torch.from_numpy(ian), args[3], num_class=nc, thr=thr)
    for b in range(2):
        idx = names[b][0][:, 0].numpy().astype(np.int64)
        assert 0 < len(idx) < c["atot"]
        assert np.array_equal(idx, ref[b]["idx"]) and np.array_equal(idx, hi[b]["idx"])
        assert np.array_equal(got[b][1].numpy(), ref[b]["labels"]) and np.array_equal(ref[b]["labels"], hi[b]["labels"])
        assert np.abs(got[b][0].numpy() - ref[b]["boxes"]).max() <= 1e-6
        assert np.abs(got[b][2].numpy() - ref[b]["scores"]).max() <= 1e-6
        assert np.any(ref[b]["boxes"][:, 6] > 3.0) and np.any(ref[b]["boxes"][:, 6] < 0)     # flipped and unflipped rows


def test_decode_filter_reference_capacity():
    c = HC.head_case(3, 1, 1, 2, 5, 7, 0.3)
    full = HC.decode_filter_ref(c, 0.3, c["atot"])[0]
    cut = HC.decode_filter_ref(c, 0.3, 5)[0]
    assert full["total"] == cut["total"] > 5 and np.array_equal(cut["idx"], full["idx"][:5])
    assert np.array_equal(cut["boxes"], full["boxes"][:5])


@pytest.mark.parametrize("m,ties", [(129, False), (129, True), (300, False)])
def test_rescore_reference_agrees_with_oracle(m, ties):
    b, site, centre, _ = HC.loose(m, 5, exact=True)
    g = np.random.default_rng(m)
    passing = g.uniform(0, 1, m) < 0.7
    logits = HC.rescore_logits(passing, 1, 0.3)
    if ties:
        logits[g.permutation(m)[:40]] = logits[np.flatnonzero(passing)[0]]
    labels = g.integers(0, 3, m).astype(np.int64)
    ref = HC.rescore_ref(b, logits, labels, m, m, 0.3, 0.1, m, np.float32)
    hi = HC.rescore_ref(b, logits, labels, m, m, 0.3, 0.1, m)
    gb, gs, gl = onets.rescore(torch.from_numpy(b), torch.from_numpy(logits), torch.from_numpy(labels), 0.3, 0.1)
    assert np.array_equal(ref["rows"], hi["rows"]) and 0 < len(ref["rows"]) < ref["m"] < m
    assert np.array_equal(gb, b[ref["rows"]]) and np.array_equal(gl, labels[ref["rows"]])
    assert np.abs(gs - ref["scores"]).max() <= 1e-6
    cut = HC.rescore_ref(b, logits, labels, m, m, 0.3, 0.1, 7)
    assert np.array_equal(cut["rows"], hi["rows"][:7]) and cut["kept"] == hi["kept"]
    assert HC.rescore_ref(b, logits, labels, 0, m, 0.3, 0.1, 7)["kept"] == 0


def test_pswarp_reference_agrees_with_oracle_module():
    """pswarp_ref is oracle/nets.py's sampling (the fp32 grid, grid_sample, the mean over the 28 parts) run in float64"""
    g = torch.Generator().manual_seed(2)
    feat = torch.randn(28, 9, 13, generator=g)
    boxes = torch.zeros(40, 7)
    boxes[:, 0] = torch.rand(40, generator=g) * 8 - 2
    boxes[:, 1] = torch.rand(40, generator=g) * 6 - 3
    boxes[:, 3] = 0.5 + torch.rand(40, generator=g)
    boxes[:, 4] = 1 + torch.rand(40, generator=g)
    boxes[:, 6] = (torch.rand(40, generator=g) - 0.5) * 6.3
    params = {"conv0": dict(weight=torch.zeros(28, 28, 3, 3), bn=dict(weight=torch.ones(28), bias=torch.zeros(28),
                                                                      running_mean=torch.zeros(28), running_var=torch.ones(28))),
              "conv1": dict(weight=torch.eye(28).view(28, 28, 1, 1))}
    params["conv0"]["weight"][torch.arange(28), torch.arange(28), 1, 1] = 1.0
    pos = feat.abs()                               # the module's ReLU is the identity on a non-negative map
    scores, x = onets.pswarp_forward(pos.unsqueeze(0), params, [boxes], grid_offsets=(1.0, 2.0), featmap_stride=0.5)
    ref = HC.pswarp_ref(x[0].numpy(), boxes.numpy(), (1.0, 2.0), 2.0)
    assert np.abs(scores[0].numpy() - ref).max() < 1e-6 and np.abs(ref).max() > 0.1


# ---- margins ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2, 5, 7), (3, 2, 5, 7), (3, 2, 19, 23), (1, 2, 363, 363)])
@pytest.mark.parametrize("thr", [0.3, 0.5])
def test_head_case_margins(shape, thr):
    nc, a, h, w = shape
    atot = nc * a * h * w
    g = np.random.default_rng(1)
    want = [np.sort(g.choice(atot, 9, replace=False)), None]
    c = HC.head_case(11, 2, nc, a, h, w, thr, want=want)
    m = HC.head_margins(c)
    assert m["thr"] >= HC.CLS_NEAR and m["gap"] >= HC.CLS_GAP * 0.999 and m["rot"] >= HC.ROT_MARGIN
    assert np.abs(c["box"][..., :6]).max() <= 1 and np.abs(c["cls"]).max() <= 4.01
    ref = HC.decode_filter_ref(c, thr, atot)
    assert np.array_equal(ref[0]["idx"], want[0])
    assert 0 < ref[1]["total"] < atot
    # an fp32 evaluation selects, labels and flips as the float64 one does
    lo = HC.decode_filter_ref(c, thr, atot, np.float32)
    for b in range(2):
        assert np.array_equal(lo[b]["idx"], ref[b]["idx"]) and np.array_equal(lo[b]["labels"], ref[b]["labels"])
        assert np.abs(lo[b]["boxes"][:, 6] - ref[b]["boxes"][:, 6]).max() < 1e-5
    # both ways of not selecting an anchor are present next to the wanted ones
    s, _ = HC.class_scores(c["cls"][0])
    assert np.any((s > thr) & (c["mask"][0] == 0)) and np.any((s < thr) & (c["mask"][0] == 1))
    # the head tensor is the anchor-major data in the layout the inference kernel slices
    nb, ncl, nd = HC.head_channels(nc, a)
    assert c["head"].shape == (2, nb + ncl + nd, h, w)
    r = int(want[0][3])
    ci, rem = divmod(r, h * w * a)
    pix, ai = divmod(rem, a)
    flat = c["head"].reshape(2, -1, h * w)
    assert np.array_equal(flat[0, (ci * a + ai) * 7:(ci * a + ai) * 7 + 7, pix], c["box"][0, r])
    assert np.array_equal(flat[0, nb + (ci * a + ai) * nc:nb + (ci * a + ai) * nc + nc, pix], c["cls"][0, r])
    assert np.array_equal(flat[0, nb + ncl + (ci * a + ai) * 2:nb + ncl + (ci * a + ai) * 2 + 2, pix], c["dir"][0, r])


@pytest.mark.parametrize("score_thr", [0.3, 0.05])
def test_rescore_logit_margins(score_thr):
    above, below = HC.logit_lattice(score_thr)
    assert len(above) >= 4096 and len(below) >= 256
    g = np.random.default_rng(0)
    passing = g.uniform(0, 1, 4096) < 0.9
    lg = HC.rescore_logits(passing, 0, score_thr)
    gap, thr_m = HC.logit_margins(lg, score_thr)
    assert gap >= 1e-3 and thr_m >= 1e-3 and np.abs(lg).max() <= 4
    assert np.array_equal(HC.sigmoid64(lg) > score_thr, passing)
    # the fp32 sigmoid orders distinct logits as the logits do
    s32 = (np.float32(1) / (np.float32(1) + np.exp(-lg))).astype(np.float32)
    o = np.argsort(lg)
    assert (np.diff(s32[o]) > 0).all()
    d = HC.descending_logits(4096, score_thr)
    assert (np.diff(d) < 0).all() and HC.logit_margins(d, score_thr)[0] >= 1e-3
