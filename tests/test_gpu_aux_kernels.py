"""-m gpu: the fused auxiliary head's entry points alone, at their edges, against the float64 references of
tests/train_tail_cases.py: sassd_aux_prepare, sassd_aux_head_fwd, sassd_aux_head_bwd and one cross-check of _bwd_det.

aux_prepare is bit-equal throughout (points, the three voxel-centre tensors, labels, centre offsets) and its positive count
exact: train_tail_cases keeps every point PT_MARGIN from every decision (test_train_tail_cases_cpu.py checks that).

Every floating tensor of the head is held to four times the figure of a numpy fp32 evaluation of the same formulas on the
same inputs (train_tail_cases, dt=np.float32), never below 4 x 2^-24; a figure is the largest error over the tensor's scale -- max |ref|
for wgt and gout, the float64 sum of the absolute values of its terms, per element, for everything summed
(train_tail_cases.figure).  The backward is fed the forward's reference tensors rounded to fp32, so it is judged alone.
Largest figures over the cases (each case prints its own before it asserts: run with -s):

                   wgt      h        out      gout     cls sum  reg sum  grad_feats  dw1      dw2
  numpy fp32       1.2e-7   2.5e-7   3.0e-8   1.1e-5   3.6e-7   4.2e-7   6.5e-7      2.4e-7   1.2e-7
  kernel           1.2e-7   2.4e-7   2.7e-8   9.6e-6   2.9e-7   8.2e-7   6.8e-7      3.1e-7   2.4e-7

(gout is large on its scale because the quadratic branch of smooth-L1 multiplies the error of `out` by 9; the case closest to
its own bar is dw1 at N = 64, M = (3, 3, 3), at 0.83 of the 4 x 2^-24 floor)
"""
import functools

import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import kernels as K
import train_tail_cases as TC

pytestmark = pytest.mark.gpu

AUX_N = (1, 63, 64, 65, 257, 1025, 16449)   # 1025: 17 workgroups, a third trip of the reduction; 16449: 258 chunks, two per workgroup


# ---- aux_prepare ----------------------------------------------------------------------------------------------------------
def run_prepare(dev, c):
    gt = torch.from_numpy(c["gt"]).to(dev) if c["gt"] is not None else None
    points, known, label, target, npos = K.aux_prepare(
        torch.from_numpy(c["vfeat"]).to(dev), torch.from_numpy(c["coors"]).to(dev),
        [torch.from_numpy(i).to(dev) for i in c["indices"]], TC.VOXEL_SIZE, TC.OFFSET, gt, K.gt_offsets(c["counts"], dev), c["B"])
    return dict(points=points.cpu().numpy(), known=[k.cpu().numpy() for k in known], label=label.cpu().numpy(),
                target=target.cpu().numpy(), npos=int(npos.item()))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("m,vstride", [((300, 70, 1), 4), ((0, 5, 3), 5)])
@pytest.mark.parametrize("with_boxes", [True, False])
def test_aux_prepare(dev, n, m, vstride, with_boxes):
    """B = 3 with a box-less middle sample (or no boxes at all); M = (0, 5, 3): an empty level, and the grid comes from N"""
    c = TC.prepare_case(n, n, m, vstride, with_boxes)
    got, ref = run_prepare(dev, c), TC.aux_prepare_ref(c)
    assert np.array_equal(bits(got["points"]), bits(ref["points"]))
    for k in range(3):
        assert got["known"][k].shape == (m[k], 4) and np.array_equal(bits(got["known"][k]), bits(ref["known"][k])), k
    assert np.array_equal(got["label"], ref["label"])
    assert np.array_equal(bits(got["target"]), bits(ref["target"]))
    assert got["npos"] == ref["npos"] and (ref["npos"] > 0) == with_boxes
    if with_boxes:
        i = c["planted"]["overlap"][0]
        assert got["label"][i] == 1 and got["target"][i, 0] == c["vfeat"][i, 0] - c["gt"][7, 0]      # the LAST containing box
        assert not got["label"][c["planted"]["foreign"] + c["planted"]["gate"]].any()


# ---- aux_head_fwd / _bwd --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fwd_refs(n, kind, positives):
    """(case, float64 reference, fp32 twin), computed once and shared by the forward and the backward tests"""
    c = TC.aux_case(n, n, kind, positives)
    return c, TC.aux_fwd_ref(c), TC.aux_fwd_ref(c, np.float32)


def dev_case(dev, c):
    t = {k: [torch.from_numpy(np.array(a)).to(dev) for a in c[k]] for k in ("feats", "nn_idx", "nn_d2")}
    for k in ("w1", "w2", "label", "target"):
        t[k] = torch.from_numpy(np.array(c[k])).to(dev)
    t["npos"] = torch.tensor([c["npos"]], dtype=torch.int32, device=dev)
    return t


FWD_KEYS = ("wgt", "h", "out", "gout", "sums")


@pytest.mark.parametrize("n", AUX_N)
@pytest.mark.parametrize("kind", ["tiny", "wide"])
def test_aux_head_fwd(dev, n, kind):
    """kind tiny: M = (3, 3, 3); wide: M = (N, N/2 + 3, N/4 + 3).  Point 0 has d2 = 0 at every scale, point N/2 three times the
    same neighbour.  Without positives (npos = 0) the smooth-L1 sum and gout[:, 1:] are exactly 0."""
    for positives in (True, False):
        c, ref, lo = fwd_refs(n, kind, positives)
        t = dev_case(dev, c)
        sums, wgt, h, out, gout = K.aux_head_fwd(t["feats"], t["nn_idx"], t["nn_d2"], t["w1"], t["w2"], t["label"], t["target"],
                                                 t["npos"])
        got = dict(wgt=wgt, h=h, out=out, gout=gout, sums=sums)
        got = {k: v.cpu().numpy() for k, v in got.items()}
        assert all(np.isfinite(v).all() for v in got.values())
        line = []
        for k in FWD_KEYS:
            if k == "sums":
                f32 = [TC.figure(lo[k][j], ref[k][j], ref["scale"][k][j]) for j in range(2)]
                fk = [TC.figure(got[k][j], ref[k][j], ref["scale"][k][j]) for j in range(2)]
            else:
                f32, fk = [TC.figure(lo[k], ref[k], ref["scale"][k])], [TC.figure(got[k], ref[k], ref["scale"][k])]
            line.append("%s %s / %s" % (k, " ".join("%.2e" % v for v in f32), " ".join("%.2e" % v for v in fk)))
            for a, b in zip(f32, fk):
                assert b <= TC.bar(a), (n, kind, positives, k, b, TC.bar(a))
        print("aux_head_fwd[n %d, %s, npos %d] fp32 / kernel: %s" % (n, kind, c["npos"], "; ".join(line)))
        assert abs(got["wgt"][c["zero"], 0] - 1) < 1e-6
        if not positives:
            assert got["sums"][1] == 0 and not got["gout"][:, 1:].any()
        else:
            pos = c["label"] > 0
            assert not got["gout"][~pos, 1:].any() and np.array_equal(np.sign(got["gout"][pos, 1:]), np.sign(ref["gout"][pos, 1:]))


def check_bwd(n, kind, gs, got, ref, lo, what):
    gf, dw1, dw2 = got
    line = []
    pairs = [("gf%d" % s, gf[s].cpu().numpy(), ref["gf"][s], lo["gf"][s], ref["scale"]["gf"][s]) for s in range(3)]
    pairs += [(k, v.cpu().numpy(), ref[k], lo[k], ref["scale"][k]) for k, v in (("dw1", dw1), ("dw2", dw2))]
    for name, x, r, l, sc in pairs:
        assert np.isfinite(x).all()
        a, b = TC.figure(l, r, sc), TC.figure(x, r, sc)           # (figure also holds rows nobody references to exactly 0)
        line.append("%s %.2e / %.2e" % (name, a, b))
        assert b <= TC.bar(a), (what, n, kind, gs, name, b, TC.bar(a))
    print("%s[n %d, %s, grad_sums %s] fp32 / kernel: %s" % (what, n, kind, gs, "; ".join(line)))


@functools.lru_cache(maxsize=None)
def bwd_refs(n, kind, gs):
    c, ref, _ = fwd_refs(n, kind, True)
    given = tuple(ref[k].astype(np.float32) for k in ("wgt", "h", "gout"))
    return c, given, TC.aux_bwd_ref(c, *given, gs), TC.aux_bwd_ref(c, *given, gs, np.float32)


def run_bwd(dev, c, given, gs, deterministic=False):
    t = dev_case(dev, c)
    wgt, h, gout = (torch.from_numpy(a).to(dev) for a in given)
    return K.aux_head_bwd(t["feats"], t["nn_idx"], t["w1"], t["w2"], wgt, h, gout, torch.tensor(gs, dtype=torch.float32, device=dev),
                          deterministic=deterministic)


@pytest.mark.parametrize("n", AUX_N)
@pytest.mark.parametrize("kind", ["tiny", "wide"])
def test_aux_head_bwd(dev, n, kind):
    """tiny: every atomic of a level lands in three rows; wide: rows nobody references stay exactly 0 (level 0's last row)"""
    for gs in ((1.0, 1.0), (0.37, -2.5)):
        c, given, ref, lo = bwd_refs(n, kind, gs)
        got = run_bwd(dev, c, given, gs)
        check_bwd(n, kind, gs, got, ref, lo, "aux_head_bwd")
        if kind == "wide" and n > 3:
            assert not got[0][0][-1].any().item()


def test_aux_head_bwd_det_cross_check(dev):
    """the deterministic twin on one case, held to the same bars (its bit-reproducibility is tested in test_gpu_determinism.py)"""
    for kind in ("tiny", "wide"):
        c, given, ref, lo = bwd_refs(257, kind, (0.37, -2.5))
        check_bwd(257, kind, (0.37, -2.5), run_bwd(dev, c, given, (0.37, -2.5), deterministic=True), ref, lo, "aux_head_bwd_det")
