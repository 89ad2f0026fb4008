"""-m gpu: the rescoring-loss kernels alone, against the float64 references of tests/train_tail_cases.py:
sassd_boxes_iou3d_batch, the precomputed-overlap branch of sassd_assign_targets (its 128-box chunk loop included), the two
composed as loss_padded composes them, and sassd_focal_loss.

IoU: 1e-5 absolute against the float64 polygon clipper (the agreement the project states for its IoU kernels; the clipper
itself sits 8.3e-7 from the fp32 oracle on this batch, test_train_tail_cases_cpu.py).  Measured: 8.3e-7 -- the kernel
and the oracle are the same fp32 arithmetic; the planted pairs give 1.00000024, 0.27359357, 0.12500007, 0 and 0.
The assignment from a given matrix is exact arithmetic: labels, positives and best overlaps compare bit for bit.
focal_loss: four times a numpy fp32 evaluation's figure, never below 4 x 2^-24 (gradient over max |ref|, the sum over the sum
of its terms' magnitudes).  Largest figures: gradient fp32 6.4e-7 / kernel 6.4e-7; sum fp32 1.4e-7 / kernel 1.3e-7."""
import numpy as np
import pytest
import torch

from oracle import train_ref as TR
import sassd  # noqa: F401
from sassd import _C
from sassd import kernels as K
import train_tail_cases as TC

pytestmark = pytest.mark.gpu

ROWS = TC.RS_ROWS
COUNTS = [(300, 17, 0), (211, 300, 300)]              # the second: rows of the 129-box sample are valid


def run_iou(dev, bt, counts, gmax=None, pad=64):
    """-> the whole output buffer (NaN-filled before the call, `pad` elements longer than ov_off[B]) and ov_off"""
    ov_off = np.concatenate([[0], np.cumsum(ROWS * np.asarray(bt["gt_counts"], np.int64))]).astype(np.int64)
    out = torch.full((int(ov_off[-1]) + pad,), float("nan"), device=dev)
    boxes = torch.from_numpy(np.array(bt["boxes"])).to(dev)
    gt = torch.from_numpy(np.array(bt["gt"])).to(dev)
    gmax = max(bt["gt_counts"]) if gmax is None else gmax
    cnt, goff = torch.tensor(counts, dtype=torch.int32, device=dev), K.gt_offsets(bt["gt_counts"], dev)
    ooff = torch.from_numpy(ov_off).to(dev)                                   # (named: every argument outlives the launch)
    _C.check(_C.lib().sassd_boxes_iou3d_batch(_C.ptr(boxes), _C.ptr(cnt), 3, ROWS, _C.ptr(gt), _C.ptr(goff), int(gmax),
                                              _C.ptr(ooff), _C.ptr(out), _C.stream()), "sassd_boxes_iou3d_batch")
    torch.cuda.synchronize()
    return out, ov_off


@pytest.mark.parametrize("counts", COUNTS)
def test_boxes_iou3d_batch(dev, counts):
    """B = 3, rows = 300, G = (12, 0, 129): rows x gmax = 38700 is no multiple of 256, and the three matrices have three strides"""
    bt = TC.rescore_batch()
    out, ov_off = run_iou(dev, bt, counts)
    got = out.cpu().numpy()
    tot = int(ov_off[-1])
    assert np.isnan(got[tot:]).all() and np.isfinite(got[:tot]).all()
    ref = TC.masked_rows(bt["full"], ov_off, counts, bt["gt_counts"])
    err = np.abs(got[:tot] - ref)
    print("boxes_iou3d_batch[counts %s]: max |kernel - float64| = %.3g over %d overlapping pairs (bar 1e-5)"
          % (counts, err.max(), int((ref > 0).sum())))
    assert err.max() <= 1e-5, (int(err.argmax()), err.max())
    for b, G in enumerate(bt["gt_counts"]):                                     # rows past the count: exactly 0
        m = got[ov_off[b]:ov_off[b + 1]].reshape(ROWS, G)
        assert not m[min(counts[b], ROWS):].any()
    if counts[0] == ROWS:
        m, p = got[:ROWS * 12].reshape(ROWS, 12), bt["planted"]
        print("  planted: self %.8f turned %.8f inner %.8f above %g touch %.3g close %.6f"
              % (m[0, 0], m[p["turned"], 0], m[p["inner"], 0], m[p["above"], 0], m[p["touch"], 1], m[p["close"], 0]))
        assert np.abs(np.diag(m[:12]) - 1).max() <= 1e-5 and m[p["above"], 0] == 0 and m[p["touch"], 1] <= 1e-5
        assert abs(m[p["inner"], 0] - 0.125) <= 1e-5


def test_boxes_iou3d_batch_gmax_zero(dev):
    out, ov_off = run_iou(dev, TC.rescore_batch(), (300, 17, 0), gmax=0)
    assert torch.isnan(out).all().item()


def run_assign(dev, bt, ov, ov_off, mask, cls, matched, unmatched, stride=None):
    """sassd_assign_targets with `overlaps`: -> (labels [3, stride], best [3, stride], num_pos [3]); sentinels past A"""
    stride = ROWS if stride is None else stride
    labels = torch.full((3, stride), -7, dtype=torch.int64, device=dev)
    targets = torch.full((3, stride, 7), -7.0, device=dev)
    best = torch.full((3, stride), -7.0, device=dev)
    num_pos = torch.full((3,), 99, dtype=torch.int32, device=dev)
    K.assign_targets(torch.from_numpy(np.array(bt["boxes"])).to(dev), torch.from_numpy(mask.astype(np.uint8)).to(dev),
                     torch.from_numpy(np.array(bt["gt"])).to(dev), None if cls is None else torch.from_numpy(cls).to(dev), None,
                     K.gt_offsets(bt["gt_counts"], dev), matched, unmatched, labels, targets, num_pos, out_stride=stride, best=best,
                     overlaps=ov if torch.is_tensor(ov) else torch.from_numpy(ov).to(dev),
                     overlap_offsets=torch.from_numpy(ov_off).to(dev))
    return labels.cpu().numpy(), best.cpu().numpy(), num_pos.cpu().numpy(), targets.cpu().numpy()


def check_assign(bt, ov32, ov_off, mask, cls, matched, unmatched, got, what):
    labels, best, num_pos, targets = got
    goff = np.concatenate([[0], np.cumsum(bt["gt_counts"])])
    for b, G in enumerate(bt["gt_counts"]):
        m = ov32[ov_off[b]:ov_off[b + 1]].reshape(ROWS, G)
        lab, bs, npos = TC.assign_from_overlaps_ref(m, mask[b], None if cls is None else cls[goff[b]:goff[b + 1]], matched, unmatched)
        assert np.array_equal(labels[b, :ROWS], lab), (what, b, np.flatnonzero(labels[b, :ROWS] != lab)[:8])
        assert num_pos[b] == npos, (what, b)
        assert np.array_equal(best[b, :ROWS].view(np.uint32), bs.view(np.uint32)), (what, b)
        assert (labels[b, ROWS:] == -7).all() and (best[b, ROWS:] == -7).all() and (targets[b, ROWS:] == -7).all(), (what, b)
        assert not targets[b, :ROWS][lab <= 0].any()
        if (lab > 0).any():                                                  # the targets encode the first best ground truth
            arg = m[lab > 0].argmax(1)
            enc = TR.box_encode(bt["gt"][goff[b]:goff[b + 1]][arg], bt["boxes"][b][lab > 0])
            assert np.abs(targets[b, :ROWS][lab > 0] - enc).max() <= 1e-5, (what, b)


def planted_matrix(bt, counts):
    """the host-built fp32 matrix: iou3d_ref rounded, rows past the counts 0, and per sample with ground truth a tie (two
    valid rows share, bit for bit, the best overlap of one ground truth -- below both thresholds pairs' `matched`, so only
    the forced rule makes them positive) and an all-zero column.  In the 129-box sample both sit in the second LDS chunk."""
    ov_off = bt["ov_off"]
    ov = TC.masked_rows(bt["full"], ov_off, counts, bt["gt_counts"]).astype(np.float32)
    plan = {}
    for b, G in enumerate(bt["gt_counts"]):
        if not G or counts[b] < 8:
            continue
        m = ov[ov_off[b]:ov_off[b + 1]].reshape(ROWS, G)
        tie, zero = G - 1, G - 2
        m[:, zero] = 0
        m[:, tie] = np.minimum(m[:, tie], np.float32(0.3))
        valid = min(counts[b], ROWS)
        r1, r2 = np.argsort(m[:valid].max(1), kind="stable")[:2]             # the two valid rows that overlap least
        m[r1, tie] = m[r2, tie] = np.float32(0.40625)
        plan[b] = (tie, zero, r1, r2)
    return ov, plan


@pytest.mark.parametrize("counts", COUNTS)
@pytest.mark.parametrize("matched,unmatched", [(0.7, 0.7), (0.6, 0.45)])
def test_assign_targets_from_overlaps(dev, counts, matched, unmatched):
    bt = TC.rescore_batch()
    ov, plan = planted_matrix(bt, counts)
    mask = np.arange(ROWS)[None, :] < np.asarray(counts)[:, None]
    cls = np.random.default_rng(5).integers(1, 4, sum(bt["gt_counts"])).astype(np.int64)
    for stride in (ROWS, ROWS + 37):
        got = run_assign(dev, bt, ov, bt["ov_off"], mask, cls, matched, unmatched, stride)
        check_assign(bt, ov, bt["ov_off"], mask, cls, matched, unmatched, got, (counts, matched, stride))
    goff = np.concatenate([[0], np.cumsum(bt["gt_counts"])])
    assert 2 in plan or counts[2] == 0
    for b, (tie, zero, r1, r2) in plan.items():
        lab, m = got[0][b], ov[bt["ov_off"][b]:bt["ov_off"][b + 1]].reshape(ROWS, bt["gt_counts"][b])
        for r in (r1, r2):
            assert m[r].max() == np.float32(0.40625) and lab[r] == cls[goff[b] + tie] > 0     # positive by the forced rule alone
        assert not m[:, zero].any() and m[r1, tie] == m[r2, tie] == m[:, tie].max()
    assert (got[0][:, :ROWS][~mask] == -1).all() and (got[1][:, :ROWS][~mask] == -1).all()


@pytest.mark.parametrize("counts", COUNTS)
def test_iou_then_assign_composed(dev, counts):
    """kernel IoU -> kernel assignment, as loss_padded does: the labels of the float64 IoU, exactly -- no best overlap of the
    batch lies within IOU_BAND of a threshold and no ground truth has two rows within IOU_BAND of its best"""
    bt = TC.rescore_batch()
    out, ov_off = run_iou(dev, bt, counts)
    tot = int(ov_off[-1])
    mask = np.arange(ROWS)[None, :] < np.asarray(counts)[:, None]
    ref32 = TC.masked_rows(bt["full"], ov_off, counts, bt["gt_counts"]).astype(np.float32)
    kern = out[:tot].cpu().numpy()
    for matched, unmatched in ((0.7, 0.7), (0.6, 0.45)):
        labels, best, num_pos, _ = run_assign(dev, bt, out, ov_off, mask, None, matched, unmatched)
        for b, G in enumerate(bt["gt_counts"]):
            lab, _, npos = TC.assign_from_overlaps_ref(ref32[ov_off[b]:ov_off[b + 1]].reshape(ROWS, G), mask[b], None, matched, unmatched)
            assert np.array_equal(labels[b], lab) and num_pos[b] == npos, (b, matched)
            # and `best` is the kernel matrix's own row maximum, bit for bit
            _, bs, _ = TC.assign_from_overlaps_ref(kern[ov_off[b]:ov_off[b + 1]].reshape(ROWS, G), mask[b], None, matched, unmatched)
            assert np.array_equal(best[b].view(np.uint32), bs.view(np.uint32)), (b, matched)
        assert num_pos[0] >= 12                                                     # every ground truth's own row at least


# ---- focal_loss -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
@pytest.mark.parametrize("nb", [1, 3])
def test_focal_loss(dev, n, nb):
    x, lab = TC.focal_case(n, n)
    for num_pos in (np.zeros(nb, np.int32), (np.arange(1, nb + 1) * 7).astype(np.int32)):
        s, g = K.focal_loss(torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(num_pos).to(dev))
        s, g = float(s.item()), g.cpu().numpy()
        rs, rg, terms = TC.focal_ref(x, lab, num_pos)
        ls, lg, _ = TC.focal_ref(x, lab, num_pos, np.float32)
        assert np.isfinite(g).all() and np.isfinite(s) and not g[lab < 0].any()
        scale_g, scale_s = np.abs(rg).max(), np.abs(terms).sum()
        f32 = (TC.figure(lg, rg, scale_g), TC.figure(ls, rs, scale_s))
        fk = (TC.figure(g, rg, scale_g), TC.figure(s, rs, scale_s))
        print("focal_loss[n %d, num_pos %s]: gradient fp32 %.2e / kernel %.2e; sum fp32 %.2e / kernel %.2e"
              % (n, num_pos.tolist(), f32[0], fk[0], f32[1], fk[1]))
        assert fk[0] <= TC.bar(f32[0]) and fk[1] <= TC.bar(f32[1]), (n, nb, fk, f32)
        assert (lab >= 0).any() == (s > 0)


@pytest.mark.parametrize("n", [257, 70001])
def test_focal_loss_all_ignored(dev, n):
    x, lab = TC.focal_case(n, n, all_ignored=True)
    s, g = K.focal_loss(torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), torch.tensor([3, 4], dtype=torch.int32, device=dev))
    assert float(s.item()) == 0 and not g.cpu().numpy().any()
