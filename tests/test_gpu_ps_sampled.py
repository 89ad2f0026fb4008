"""-m gpu: the part-sensitive head at the pixels PSWarp samples (sassd_ps_pixel_list + sassd_ps_head_sampled) against what it
replaces, the dense 3x3 conv (sassd_conv2d_fwd) + the narrow 1x1 (sassd_conv1x1_narrow_fwd) in front of sassd_pswarp_sample:

  * the pixel list (counts, order, flags) int for int against a numpy model of the sampler's four-neighbour rule;
  * the sampled head BIT FOR BIT against the dense kernels at every listed pixel, and the logits sassd_pswarp_sample reads from
    either map (the unlisted pixels of the sampled map hold NaN: a read outside the list would show);
  * whole frames of an InferencePlan with and without ps_sampled, eager and as replayed graphs, bit for bit.

Shapes are the smallest that reach every path: two maps (W % 4 == 0 -> the dense kernel's DMA staging, W = 13 -> its register
staging), lists shorter than, not a multiple of and many times the 32-pixel workgroup block, Cin = 64 and 256 (2 and 8 of the
kernel's 4-chunk register buffers: the double buffer wraps)."""
import numpy as np
import pytest
import torch

from sassd import kernels as K
from sassd.pipeline import InferencePlan
import helpers as H
import test_bf16_infer_cpu as B16

pytestmark = pytest.mark.gpu
CAPK, PARTS = 16, 28
MAPS = [(24, 16), (21, 13)]
OFFS, SCALE = (0.0, 0.0), 1.0            # box coordinates are pixel coordinates: u = x, v = y


# ---- the numpy model of the four-neighbour rule ---------------------------------------------------------------------------
def _linspace(n):
    step = 1.0 / (n - 1)
    return [(-0.5 + step * i) if i < n // 2 else (0.5 - step * (n - i - 1)) for i in range(n)]


def _model_pixels(boxes, h, w):
    """pixels pswarp_kernel reads for these boxes [n, 7]: for each of the 4 x 7 grid points the in-map ones of its four bilinear
    neighbours.  float64; the hand-made boxes keep every sample coordinate 1e-3 away from an integer, so that the fp32 kernel
    floors to the same pixel (asserted)."""
    flags = np.zeros((h, w), bool)
    for xg, yg, _, wg, lg, _, rg in np.asarray(boxes, np.float64):
        ct, st = np.cos(rg), np.sin(rg)
        for ix, a in enumerate(_linspace(4)):
            for iy, c in enumerate(_linspace(7)):
                xx, yy = a * wg, c * lg
                fx = (xx * ct + yy * st + xg + OFFS[0]) * SCALE
                fy = (yy * ct - xx * st + yg + OFFS[1]) * SCALE
                for f in (fx, fy):
                    assert abs(f - round(f)) > 1e-3, "test design: a sample sits on a pixel boundary (%r)" % f
                x0, y0 = int(np.floor(fx)), int(np.floor(fy))
                for yy_, xx_ in ((y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)):
                    if 0 <= yy_ < h and 0 <= xx_ < w:
                        flags[yy_, xx_] = True
    return flags


def _boxes(h, w):
    """hand-made candidates (x, y, z, w, l, h, r), 17 rows: wholly inside, over each border and each corner (taps outside the map
    contribute no pixel), wholly outside, two identical, rotated by 0.7 rad, three more inside"""
    W1, H1 = w - 1, h - 1
    rows = [(7.37, 11.61, 0, 3.13, 6.29, 1.5, 0.0),                    # 0 inside
            (0.21, 10.43, 0, 3.13, 6.29, 1.5, 0.0),                    # 1 left border
            (W1 + 0.33, 9.57, 0, 3.13, 6.29, 1.5, 0.0),                # 2 right border
            (6.41, 0.36, 0, 3.13, 6.29, 1.5, 0.0),                     # 3 top border
            (5.59, H1 + 0.44, 0, 3.13, 6.29, 1.5, 0.0),                # 4 bottom border
            (0.27, 0.39, 0, 3.13, 6.29, 1.5, 0.0),                     # 5..8 corners
            (W1 + 0.23, 0.31, 0, 3.13, 6.29, 1.5, 0.0),
            (0.29, H1 + 0.37, 0, 3.13, 6.29, 1.5, 0.0),
            (W1 + 0.41, H1 + 0.28, 0, 3.13, 6.29, 1.5, 0.0),
            (-30.21, -30.73, 0, 3.13, 6.29, 1.5, 0.0),                 # 9 wholly outside
            (9.43, 14.27, 0, 2.87, 5.13, 1.5, 1.57),                   # 10, 11 identical
            (9.43, 14.27, 0, 2.87, 5.13, 1.5, 1.57),
            (6.13, 8.41, 0, 3.31, 6.83, 1.5, 0.7),                     # 12 rotated
            (3.77, 5.29, 0, 1.93, 4.11, 1.5, -2.9),                    # 13..15 more inside
            (8.19, 15.83, 0, 2.21, 3.57, 1.5, 0.31),
            (4.63, 17.17, 0, 1.71, 2.93, 1.5, 2.1),
            (2.47, 3.91, 0, 9.13, 11.29, 1.5, 0.45)]                   # 16 the row behind capK: never read
    return np.asarray(rows, np.float32)


def _run_list(dev, buf, guided, counts, h, w):
    g = torch.from_numpy(np.ascontiguousarray(guided)).to(dev)
    c = torch.tensor(counts, dtype=torch.int32, device=dev)
    K.ps_pixel_list(g, c, CAPK, len(counts), h, w, OFFS, SCALE, out=buf)
    torch.cuda.synchronize()
    return g, c


def _check_list(buf, want_flags, h, w):
    b = len(want_flags)
    cnt, pix, flags = (t.cpu().numpy() for t in K.ps_pixel_list_views(buf, b, h, w))
    for i, wf in enumerate(want_flags):
        want = np.flatnonzero(wf.reshape(-1))
        assert cnt[i] == len(want), (i, cnt[i], len(want))
        assert np.array_equal(pix[i, :len(want)], want), i            # the listed set AND its (ascending, row-major) order
        assert np.array_equal(flags[i], wf.reshape(-1).astype(np.uint8)), i      # no residue of another sample or frame
    return [int(c) for c in cnt]


@pytest.mark.parametrize("hw", MAPS)
def test_pixel_list_equals_the_four_neighbour_model(dev, hw):
    h, w = hw
    bx = _boxes(h, w)
    buf = K.ps_pixel_list_buffer(2, h, w, dev)
    buf.fill_(-7)                                                      # stale counts, list entries and flag bytes (0xF9)
    guided = np.zeros((2, CAPK, 7), np.float32)
    guided[0] = bx[:CAPK]                                              # sample 0: count == capK
    guided[1] = bx[1:CAPK + 1][::-1]                                   # sample 1: count above capK -> clamped to its capK rows
    _run_list(dev, buf, guided, [CAPK, CAPK + 4], h, w)
    want = [_model_pixels(guided[0], h, w), _model_pixels(guided[1], h, w)]
    n1 = _check_list(buf, want, h, w)
    only_outside = _model_pixels(bx[9:10], h, w)
    assert not only_outside.any() and 0 < n1[0] < h * w
    # a second frame on the same buffers: fewer candidates in sample 0, none in sample 1 -- it lists only its own pixels
    guided2 = guided.copy()
    guided2[0, :3] = bx[[12, 9, 5]]
    _run_list(dev, buf, guided2, [3, 0], h, w)
    n2 = _check_list(buf, [_model_pixels(guided2[0, :3], h, w), np.zeros((h, w), bool)], h, w)
    assert 0 < n2[0] < n1[0] and n2[1] == 0
    # a wholly outside box alone: an empty list
    guided3 = guided.copy()
    guided3[1, 0] = bx[9]
    _run_list(dev, buf, guided3, [0, 1], h, w)
    assert _check_list(buf, [np.zeros((h, w), bool)] * 2, h, w) == [0, 0]
    print("ps pixel list %s: %s pixels listed, second frame %s" % (hw, n1, n2))


# ---- the sampled head against the dense kernels ---------------------------------------------------------------------------
def _head(dev, cin, h, w):
    g = torch.Generator().manual_seed(100 * cin + h)
    x = torch.randn(2, cin, h, w, generator=g).to(dev)
    w0 = (torch.randn(PARTS, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5).to(dev)
    w1 = (torch.randn(PARTS, PARTS, 1, 1, generator=g) * (1.0 / PARTS) ** 0.5).to(dev)
    scale = (torch.rand(PARTS, generator=g) + 0.5).to(dev)
    shift = (torch.randn(PARTS, generator=g) * 0.1).to(dev)
    wp, w1t = K.conv2d_pack_weight(w0), K.conv1x1_narrow_pack_weight(w1)
    t0 = K.conv2d_fwd(x, wp, PARTS, 3, scale, shift, True)
    dense = K.conv1x1_narrow_fwd(t0, w1t, PARTS, None, None, False)          # computed once, shared, left unchanged
    return x, wp, w1t, scale, shift, dense


def _sampled(dev, head, buf, h, w):
    x, wp, w1t, scale, shift, _ = head
    y = torch.full((2, PARTS, h, w), float("nan"), device=dev)
    K.ps_head_sampled(x, wp, scale, shift, True, w1t, None, None, False, buf, y)
    torch.cuda.synchronize()
    return y


def _check_sampled(y, dense, lists, h, w):
    for b, px in enumerate(lists):
        on = torch.zeros(h * w, dtype=torch.bool, device=y.device)
        on[torch.as_tensor(px, dtype=torch.long, device=y.device)] = True
        ys, ds = y[b].reshape(PARTS, -1), dense[b].reshape(PARTS, -1)
        assert torch.equal(ys[:, on], ds[:, on]), ("listed pixels", b, (ys[:, on] - ds[:, on]).abs().max().item())
        assert torch.isnan(ys[:, ~on]).all(), ("a pixel outside the list was written", b)


@pytest.mark.parametrize("hw", MAPS)
@pytest.mark.parametrize("cin", [64, 256])
def test_sampled_head_equals_the_dense_kernels_bit_for_bit(dev, cin, hw):
    h, w = hw
    head = _head(dev, cin, h, w)
    dense = head[5]
    buf = K.ps_pixel_list_buffer(2, h, w, dev)
    # (a) the list of the hand-made candidates; sample 1 keeps three of them
    bx = _boxes(h, w)
    guided = np.zeros((2, CAPK, 7), np.float32)
    guided[0] = bx[:CAPK]
    guided[1, :3] = bx[[12, 2, 8]]
    g, c = _run_list(dev, buf, guided, [CAPK, 3], h, w)
    cnt, pix, _ = (t.cpu().numpy() for t in K.ps_pixel_list_views(buf, 2, h, w))
    assert cnt[0] > 64 and cnt[0] % 32 != 0 and 0 < cnt[1], cnt       # several workgroups, a ragged last one
    y = _sampled(dev, head, buf, h, w)
    _check_sampled(y, dense, [pix[b, :cnt[b]] for b in range(2)], h, w)
    lg_s = K.pswarp_sample(y, g, c, CAPK, OFFS, SCALE)
    lg_d = K.pswarp_sample(dense, g, c, CAPK, OFFS, SCALE)
    torch.cuda.synchronize()
    assert torch.isfinite(lg_s).all(), "the sampler read a pixel that is not in the list"
    assert torch.equal(lg_s, lg_d)
    # (b) hand-made lists: every pixel of sample 0 (the worst case the grid is sized for), none of sample 1;
    #     then 33 scattered pixels (one over the block) and a single one, image corners included
    counts, pixels, _ = K.ps_pixel_list_views(buf, 2, h, w)
    every = np.arange(h * w)
    rng = np.random.default_rng(cin + h)
    some = np.sort(np.concatenate([[0, w - 1, (h - 1) * w, h * w - 1], rng.permutation(np.arange(w, (h - 1) * w - 1))[:29]]))
    for lists in ([every, every[:0]], [some, every[-1:]]):
        pixels.fill_(-1)
        for b, px in enumerate(lists):
            counts[b] = len(px)
            pixels[b, :len(px)] = torch.from_numpy(px).int().to(dev)
        y = _sampled(dev, head, buf, h, w)
        _check_sampled(y, dense, lists, h, w)
    assert len(some) == 33


# ---- plan level ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def car():
    """the car model, three small frames (many candidates, few, none) and the thresholds the oracle picks away from every
    candidate score of the first two"""
    model, _ = B16.car_model()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    an, bv = B16.car_anchors()
    clouds = [H.frame("k17", 1), H.frame("small", 0), H.frame("small", 0)[:6]]
    _, rpn_thr, score_thr = H.oracle_forward_safe(sd, clouds[:2], an, bv, B16.CFG)
    return sd, an, bv, clouds, rpn_thr, score_thr


def _state(p):
    k = int(p.df["counts"][0].item())
    out = [p.df["counts"], p.df["guided"][0, :k], p.logits[0, :k]] + [p.det[n] for n in ("counts", "boxes", "scores", "labels")]
    return k, [t.clone() for t in out]


@pytest.mark.parametrize("overlap", [True, False])
def test_plan_with_and_without_ps_sampled_is_bit_identical(dev, car, overlap):
    """overlap=True: eager, then the two-branch graph; overlap=False: the one-branch graph bench.py keeps in flight.  Frames in
    the order many candidates -> few -> none -> many, so that a stale flag or list entry would show."""
    sd, an, bv, clouds, rpn_thr, score_thr = car
    kw = dict(batch_size=1, anchors=an, anchors_bv=bv, device=dev, rpn_thr=rpn_thr, score_thr=score_thr, overlap=overlap)
    sam, den = InferencePlan(sd, **kw), InferencePlan(sd, ps_sampled=False, **kw)
    assert sam.ps_sampled and not den.ps_sampled
    pts = [torch.from_numpy(c).to(dev) for c in clouds]
    order = (0, 1, 2, 0)

    def compare(form, run):
        ks = []
        for f in order:
            for p in (sam, den):
                run(p, pts[f])
            torch.cuda.synchronize()
            assert int(sam.status.item()) == 0 and int(den.status.item()) == 0
            (k, a), (_, b) = _state(sam), _state(den)
            for j, (u, v) in enumerate(zip(a, b)):
                assert u.shape == v.shape and torch.equal(u, v), (form, f, j)
            n = int(K.ps_pixel_list_views(sam.ps_list, 1, sam.H, sam.W)[0][0].item())
            assert (n > 0) == (k > 0) and n <= min(112 * k, sam.H * sam.W), (form, f, k, n)
            ks.append((k, n, int(sam.det["counts"][0].item())))
            assert torch.equal(sam.ps_t[1], den.ps_t[1]), (form, f)      # a read materialises the whole map of this frame
            assert torch.equal(sam.ps_t[0], den.ps_t[0]), (form, f)
        assert ks[0][0] > ks[1][0] > 0 and ks[2][0] == 0 and ks[3] == ks[0] and ks[0][2] >= 1, ks
        print("ps_sampled %s: (candidates, listed pixels, detections) per frame %s" % (form, ks))

    if overlap:
        compare("eager", lambda p, c: p.run_from_points([c]))
    cap = max(int(c.shape[0]) for c in pts) + 64
    for p in (sam, den):
        p.capture(cap)
    compare("two-branch graph" if overlap else "one-branch graph", lambda p, c: p.run_graph([c]))
