"""The conditions the training-tail kernel tests rest on, checked without a GPU: every reference of tests/train_tail_cases.py
agrees with an independent formulation (the oracle's closed-form losses under torch autograd in float64, an index /
interpolate / Linear restatement of the aux head, the oracle's rotated IoU and point-in-box), and every margin its builders
promise holds for the builders and seeds that test_gpu_aux_kernels.py and test_gpu_rescore_loss_kernels.py use."""
import numpy as np
import pytest
import torch

from oracle import clib
from oracle import train_ref as TR
import head_cases as HC
import train_tail_cases as TC

PREP_CASES = [(n, m, vs) for n in (1, 255, 257) for m, vs in (((300, 70, 1), 4), ((0, 5, 3), 5))]
AUX_N = (1, 63, 64, 65, 257, 1025, 16449)


# ---- aux_prepare ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,vstride", PREP_CASES)
def test_prepare_case_margins_and_oracle_labels(n, m, vstride):
    c = TC.prepare_case(n, n, m, vstride)
    assert TC.prepare_margin(c) >= TC.PT_MARGIN
    r = TC.aux_prepare_ref(c)
    assert c["vfeat"].shape == (n, vstride) and [len(i) for i in c["indices"]] == list(m)
    # the planted points: inside two boxes (the last wins), inside another sample's box, inside the long box past the gate
    gt, off = c["gt"], np.concatenate([[0], np.cumsum(c["counts"])])
    for i in c["planted"]["overlap"]:
        p = c["vfeat"][i:i + 1, :3]
        assert (TC.box_terms(p, gt[off[2]]) >= 0).all() and (TC.box_terms(p, gt[off[2] + 1]) >= 0).all()
        assert r["label"][i] == 1 and r["target"][i, 0] == np.float32(p[0, 0]) - gt[off[2] + 1, 0]
    for i in c["planted"]["foreign"] + c["planted"]["gate"]:
        assert r["label"][i] == 0 and (r["target"][i] == 0).all()
    for i in c["planted"]["gate"]:
        t = TC.box_terms(c["vfeat"][i:i + 1, :3], gt[5])[0]
        assert t[1] < 0 and (t[2:] > 0).all()                                  # only the gate keeps it out
    for i in c["planted"]["foreign"]:
        other = [bx for b in range(3) if b != c["coors"][i, 0] for bx in gt[off[b]:off[b + 1]]]
        assert any((TC.box_terms(c["vfeat"][i:i + 1, :3], bx) >= 0).all() for bx in other)
    if n > 1:
        assert 0 < r["npos"] < n and len(c["planted"]["gate"]) == 1 and len(c["planted"]["foreign"]) == 2
        assert set(c["kinds"]) >= {"in", "near", "above", "free"} or n < 200
    # the oracle's point-in-box (fp32, the reference's arithmetic) labels and offsets the same, sample by sample
    for b in range(3):
        rows = np.flatnonzero(c["coors"][:, 0] == b)
        boxes = gt[off[b]:off[b + 1]]
        if len(rows) and len(boxes):
            flag, reg = clib.pts_in_boxes3d(c["vfeat"][rows, :3], boxes)
            assert np.array_equal(flag.max(0), r["label"][rows])
            assert np.array_equal(reg.view(np.uint32), r["target"][rows].view(np.uint32))
        else:
            assert (r["label"][rows] == 0).all()
    # voxel centres: the torch expression of the reference, fp32
    for k, idx in enumerate(c["indices"]):
        vs = torch.tensor(TC.VOXEL_SIZE) * (2 << k)
        ref = torch.from_numpy(idx[:, [3, 2, 1]]).float() * vs + torch.tensor(TC.OFFSET) + .5 * vs
        assert np.array_equal(r["known"][k][:, 1:].view(np.uint32), ref.numpy().view(np.uint32))
        assert np.array_equal(r["known"][k][:, 0], idx[:, 0].astype(np.float32))
    none = TC.aux_prepare_ref(TC.prepare_case(n, n, m, vstride, with_boxes=False))
    assert none["npos"] == 0 and not none["label"].any() and not none["target"].any()


# ---- focal / smooth-L1 against the oracle's closed forms ------------------------------------------------------------------
@pytest.mark.parametrize("n,nb", [(1, 1), (257, 3), (70001, 3)])
def test_focal_ref_against_oracle_autograd(n, nb):
    x, lab = TC.focal_case(n, n)
    for num_pos in (np.zeros(nb, np.int32), np.arange(1, nb + 1, dtype=np.int32) * 7):
        s, g, terms = TC.focal_ref(x, lab, num_pos)
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        w = torch.tensor((lab >= 0) / max(float(num_pos.sum()), 1.0))
        ref = TR.focal_sum(xt, torch.tensor((lab > 0).astype(np.float64)), w)
        ref.backward()
        assert abs(float(ref.detach()) - s) <= 1e-12 * max(abs(s), 1e-30)
        # (at a logit of exactly 0 autograd differentiates clamp and abs at their kinks: there the central difference decides)
        kink = x == 0
        assert np.abs(xt.grad.numpy() - g)[~kink].max(initial=0) <= 1e-12 * max(np.abs(g).max(), 1e-30)
        for i in np.flatnonzero(kink):
            cw = float(lab[i] >= 0) / max(float(num_pos.sum()), 1.0)
            up, dn = (TC.focal_terms(np.array([e]), lab[i:i + 1] > 0, np.array([cw]))[0][0] for e in (1e-6, -1e-6))
            assert abs((up - dn) / 2e-6 - g[i]) <= 1e-9
        assert np.isfinite(g).all() and (g[lab < 0] == 0).all() and (terms >= 0).all()
        lo = TC.focal_ref(x, lab, num_pos, np.float32)
        assert np.isfinite(lo[1]).all() and lo[0].dtype == np.float32
    if n >= 64:
        assert {100.0, -100.0, 20.0, -20.0} <= set(x.tolist()) and np.any(np.signbit(x) & (x == 0))
    x, lab = TC.focal_case(n, n, all_ignored=True)
    s, g, _ = TC.focal_ref(x, lab, np.ones(nb, np.int32))
    assert s == 0 and not g.any()


def _aux_torch(c, grad_sums):
    """index / interpolate / Linear restatement of the aux head in torch float64 with the oracle's losses -> the leaves, the
    forward tensors and the two sums"""
    d = torch.float64
    feats = [torch.tensor(f, dtype=d, requires_grad=True) for f in c["feats"]]
    w1 = torch.tensor(c["w1"], dtype=d, requires_grad=True)
    w2 = torch.tensor(c["w2"], dtype=d, requires_grad=True)
    cols, wgts = [], []
    for s in range(3):
        rec = 1.0 / (torch.sqrt(torch.tensor(c["nn_d2"][s], dtype=d)) + 1e-8)
        wgt = rec / rec.sum(1, keepdim=True)
        cols.append((feats[s][torch.from_numpy(c["nn_idx"][s].astype(np.int64))] * wgt[..., None]).sum(1))
        wgts.append(wgt)
    h = torch.nn.functional.linear(torch.cat(cols, 1), w1)
    out = torch.nn.functional.linear(h, w2)
    out.retain_grad()
    lab = torch.tensor(c["label"].astype(np.float64))
    norm = max(c["npos"], 1)
    cls = TR.focal_sum(out[:, 0], lab, torch.ones_like(lab) / norm)
    reg = TR.smooth_l1_sum(out[:, 1:], torch.tensor(c["target"], dtype=d), (lab / norm)[:, None], 1 / 9.)
    return feats, w1, w2, torch.cat(wgts, 1), h, out, cls, reg


@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("kind", ["tiny", "wide"])
@pytest.mark.parametrize("positives", [True, False])
def test_aux_refs_against_torch_autograd(n, kind, positives):
    c = TC.aux_case(n, n, kind, positives)
    r = TC.aux_fwd_ref(c)
    feats, w1, w2, wgt, h, out, cls, reg = _aux_torch(c, None)
    for got, want in ((r["wgt"], wgt), (r["h"], h), (r["out"], out)):
        assert np.abs(got - want.detach().numpy()).max() <= 1e-12 * max(1.0, np.abs(got).max())
    fc, fr = float(cls.detach()), float(reg.detach())
    assert abs(r["sums"][0] - fc) <= 1e-12 * fc and abs(r["sums"][1] - fr) <= 1e-12 * max(fr, 1e-30)
    assert (r["sums"][1] > 0) == positives and r["sums"][0] > 0
    # gout: the gradients of the two sums with respect to out, one at a time
    gc = torch.autograd.grad(cls, out, retain_graph=True)[0].numpy()
    assert np.abs(gc[:, 0] - r["gout"][:, 0]).max() <= 1e-12 and not gc[:, 1:].any()
    if positives:
        gr = torch.autograd.grad(reg, out, retain_graph=True)[0].numpy()
        assert np.abs(gr[:, 1:] - r["gout"][:, 1:]).max() <= 1e-12 and not gr[:, 0].any()
    else:
        assert not r["gout"][:, 1:].any()
    for gs in ((1.0, 1.0), (0.37, -2.5)):
        b = TC.aux_bwd_ref(c, r["wgt"], r["h"], r["gout"], gs)
        leaves = feats + [w1, w2]
        total = np.float64(np.float32(gs[0])) * cls + np.float64(np.float32(gs[1])) * reg
        grads = torch.autograd.grad(total, leaves, retain_graph=True)
        for got, want, sc in zip(b["gf"] + [b["dw1"], b["dw2"]], grads, b["scale"]["gf"] + [b["scale"]["dw1"], b["scale"]["dw2"]]):
            assert TC.figure(got, want.numpy(), np.where(sc > 0, sc, 0)) <= 1e-12
            assert (np.abs(got) <= sc * (1 + 1e-12)).all()                         # a scale bounds what it scales
    # scales bound their tensors, and rows nobody references have none
    assert (np.abs(r["h"]) <= r["scale"]["h"]).all() and (np.abs(r["out"]) <= r["scale"]["out"]).all()
    b = TC.aux_bwd_ref(c, r["wgt"], r["h"], r["gout"], (1.0, 1.0))
    for s in range(3):
        used = np.zeros(c["m"][s], bool)
        used[c["nn_idx"][s].reshape(-1)] = True
        assert not b["scale"]["gf"][s][~used].any() and not b["gf"][s][~used].any()
        assert (b["scale"]["gf"][s][used] > 0).all()
        if kind == "wide" and n > 3 and s == 0:
            assert not used[-1]


@pytest.mark.parametrize("n", AUX_N)
@pytest.mark.parametrize("kind", ["tiny", "wide"])
def test_aux_case_margins_and_fp32_twin(n, kind):
    """the builders and seeds of test_gpu_aux_kernels.py: the smooth-L1 margin holds, the planted points are there, and the
    fp32 twin takes every branch as float64 does"""
    for positives in (True, False):
        c = TC.aux_case(n, n, kind, positives)
        assert c["m"] == TC.aux_sizes(n, kind) and c["npos"] == int(c["label"].sum()) and (c["npos"] > 0) == positives
        assert TC.sl1_margin(c) >= TC.SL1_MARGIN
        assert all(c["nn_d2"][s][c["zero"], 0] == 0 for s in range(3))
        assert all((c["nn_idx"][s][c["same"]] == c["nn_idx"][s][c["same"], 0]).all() for s in range(3))
        if n >= 65 and positives:
            d = np.abs(TC.aux_fwd_ref(c)["out"][:, 1:] - c["target"])[c["label"] > 0]
            assert (d < TC.BETA).any() and (d > TC.BETA).any()                     # both smooth-L1 branches
    if n <= 1025:
        c = TC.aux_case(n, n, kind, True)
        hi, lo = TC.aux_fwd_ref(c), TC.aux_fwd_ref(c, np.float32)
        assert all(lo[k].dtype == np.float32 for k in ("wgt", "h", "out", "gout", "sums"))
        pos = c["label"] > 0
        assert np.array_equal(np.sign(lo["gout"][pos, 1:]), np.sign(hi["gout"][pos, 1:]))
        for k in ("wgt", "h", "out", "gout", "sums"):
            assert TC.figure(lo[k], hi[k], hi["scale"][k]) <= 1e-5
        assert abs(hi["wgt"][c["zero"], 0] - 1) < 1e-6 and np.abs(hi["wgt"].reshape(n, 3, 3).sum(2) - 1).max() < 1e-12


def test_aux_wgrad_shapes():
    """the sizes of AUX_N cover what the weight-gradient kernels branch on: chunks of 64 points, at most 256 workgroups, a
    reduction in two chains of every 8th workgroup (a third trip from 17 workgroups on)"""
    def wgs(n):
        chunks = -(-n // 64)
        nwg = max(min(chunks, 256), 1)
        cpw = -(-chunks // nwg)
        return chunks, cpw, -(-chunks // cpw)
    assert wgs(16449) == (258, 2, 129) and 16449 % 64 == 1
    assert wgs(1025) == (17, 1, 17) and wgs(257) == (5, 1, 5) and wgs(63)[0] == 1 and wgs(65)[0] == 2


# ---- rotated IoU and the assignment ----------------------------------------------------------------------------------------
def test_iou3d_ref_against_oracle():
    bt = TC.rescore_batch()
    assert bt["moved"] < 30
    worst, pairs = 0.0, 0
    for b, G in enumerate(bt["gt_counts"]):
        if not G:
            continue
        gb = bt["gt"][sum(bt["gt_counts"][:b]):sum(bt["gt_counts"][:b]) + G]
        ref = bt["full"][bt["ov_off"][b]:bt["ov_off"][b + 1]].reshape(TC.RS_ROWS, G)
        orc = TR.rotated_iou3d(np.array(bt["boxes"][b]), np.array(gb))
        worst = max(worst, float(np.abs(orc - ref).max()))
        pairs += int((ref > 0).sum())
        assert np.array_equal(ref > 1e-4, orc > 1e-4) or np.abs(orc - ref).max() < 1e-6
    print("iou3d_ref against oracle.train_ref.rotated_iou3d: max difference %.3g over %d overlapping pairs" % (worst, pairs))
    assert worst <= 1e-6 and pairs > 300
    p, G = bt["planted"], 12
    m = bt["full"][:TC.RS_ROWS * G].reshape(TC.RS_ROWS, G)
    g0 = bt["gt"][0].astype(np.float64)
    assert np.abs(np.diag(m[:G]) - 1).max() < 1e-12                              # the ground truth itself: IoU 1
    w, l = sorted(g0[3:5])
    assert abs(m[p["turned"], 0] - (w * w) / (2 * w * l - w * w)) < 1e-9         # a w x w square out of two w x l rectangles
    assert abs(m[p["inner"], 0] - 0.125) < 1e-6                                  # 1/8 of the volume, wholly inside
    assert m[p["above"], 0] == 0 and m[p["touch"], 1] < 1e-9 and 0.8 < m[p["close"], 0] < 0.999
    # rows past the count are 0, and the layout is the samples' [rows, G_b] matrices back to back
    cut, off = TC.iou3d_ref(bt["boxes"], (300, 17, 0), bt["gt"], bt["gt_counts"])
    assert np.array_equal(off, bt["ov_off"]) and off.tolist() == [0, 3600, 3600, 3600 + 300 * 129]
    assert np.array_equal(cut, TC.masked_rows(bt["full"], off, (300, 17, 0), bt["gt_counts"])) and not cut[3600:].any()


def test_rescore_batch_margins():
    bt = TC.rescore_batch()
    thr_m, gap_m, col_m = TC.rescore_margins(bt)
    assert thr_m >= HC.IOU_BAND and gap_m >= HC.IOU_BAND and col_m > 0.99
    # labels of all three kinds under both threshold pairs, in the sample that crosses the 128-box chunk too
    for b in (0, 2):
        G = bt["gt_counts"][b]
        m = bt["full"][bt["ov_off"][b]:bt["ov_off"][b + 1]].reshape(TC.RS_ROWS, G).astype(np.float32)
        for hi, lo in ((0.7, 0.7), (0.6, 0.45)):
            lab, best, npos = TC.assign_from_overlaps_ref(m, np.ones(TC.RS_ROWS, bool), None, hi, lo)
            assert npos >= G and (lab == 0).sum() > 20 and ((lab == -1).sum() > 5) == (hi != lo)
    assert np.any(bt["full"][bt["ov_off"][2]:].reshape(TC.RS_ROWS, 129)[:, 128] > 0.5)


def test_assign_from_overlaps_ref_is_the_oracle_rule():
    """TR.assign with a similarity that returns the given matrix: the same labels; then the planted cases by hand"""
    bt = TC.rescore_batch()
    g = np.random.default_rng(0)
    for b in (0, 2):
        G = bt["gt_counts"][b]
        m = bt["full"][bt["ov_off"][b]:bt["ov_off"][b + 1]].reshape(TC.RS_ROWS, G).astype(np.float32)
        mask = g.uniform(0, 1, TC.RS_ROWS) < 0.8
        cls = g.integers(1, 4, G)
        gb = bt["gt"][sum(bt["gt_counts"][:b]):sum(bt["gt_counts"][:b]) + G]
        for hi, lo in ((0.7, 0.7), (0.6, 0.45)):
            want, _, wbest = TR.assign(bt["boxes"][b], mask, gb, cls, np.float32(hi), np.float32(lo), lambda a_, g_: m[mask])
            lab, best, npos = TC.assign_from_overlaps_ref(m, mask, cls, hi, lo)
            assert np.array_equal(lab, want) and np.array_equal(best[mask], wbest) and (best[~mask] == -1).all()
            assert npos == int((want > 0).sum())
    m = np.array([[0.5, 0.0, 0.2], [0.5, 0.0, 0.1], [0.3, 0.0, 0.9], [0.1, 0.0, 0.65], [0.0, 0.0, 0.0]], np.float32)
    lab, best, npos = TC.assign_from_overlaps_ref(m, np.ones(5, bool), np.array([1, 2, 3]), 0.7, 0.6)
    # rows 0 and 1 tie the best of ground truth 0 (forced), the all-zero column forces nothing, 0.65 is ignored
    assert lab.tolist() == [1, 1, 3, -1, 0] and npos == 3 and best.tolist() == m.max(1).tolist()
    lab, best, npos = TC.assign_from_overlaps_ref(m, np.array([0, 1, 1, 1, 1], bool), None, 0.7, 0.6)
    assert lab.tolist() == [-1, 1, 1, -1, 0] and best[0] == -1
    lab, best, npos = TC.assign_from_overlaps_ref(np.zeros((3, 0), np.float32), np.array([1, 0, 1], bool), None, 0.7, 0.6)
    assert lab.tolist() == [0, -1, 0] and best.tolist() == [0, -1, 0] and npos == 0
