"""-m gpu: the Winograd F(4x4, 3x3) kernels alone, held PER ELEMENT.  F(4x4)'s B^T is not dyadic, so the kernels round; the rule is
the project's own: |y - y64| <= max(4 x figure of the fp32 twin, 4 x 2^-24) x scale_of at every element, with the twin
(tests/dense_conv_cases.py::wino4_twin: the kernel's own formulas in float32, channel sum in channel order) run on the case's own
inputs and scale_of = the float64 conv of |x| and |w| maximised over each 4x4 output tile, through the epilogue.  The whole-tensor
bar of test_gpu_wino4.py (1e-4 max|ref|) has 25-75x headroom over honest fp32 and passes a GEMM that loses the third bf16 piece
of V; this one does not (test_dense_conv_cases_cpu.py).  Every case prints the kernel's figure next to the twin's.

Inputs in turn: lattice operands (the reference is known exactly: only the transforms round), full-mantissa randn, one live input
channel.  x lies in NaN, y in 7.0, the workspace is NaN-filled; the bytes around x and y are checked."""
import numpy as np
import pytest
import torch

from sassd import kernels as K

import dense_conv_cases as DC

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _ids(table):
    return [c["name"] for c in table]


def _held(y, c, what):
    fig = DC.figure(y.cpu().numpy(), c["ref"], c["scale_of"])
    print("%s: kernel %.2e, fp32 twin %.2e, bar %.2e (of scale_of, per element)" % (what, fig, c["twin_figure"], c["bar"]))
    assert fig <= c["bar"], (what, fig, c["bar"])
    return fig


def _out(shape, dev):
    return DC.embed(torch.full(shape, 7.0), poison=7.0, device=dev)


def _fwd(dev, case):
    b, cin, cout, h, w = case["b"], case["cin"], case["cout"], case["h"], case["w"]
    c = DC.wino4_case(case["kind"], b, cin, cout, h, w, case["seed"])
    assert K.conv2d_wino4_supported(cin, cout, h, w)
    xb, x = DC.embed(c["x"], poison=NAN, device=dev)
    yb, y = _out((b, cout, h, w), dev)
    wp = K.conv2d_wino4_pack_weight(c["w"].to(dev))
    ws = K.conv2d_wino4_workspace(b, cin, cout, h, w, dev)
    ws.view(torch.float32).fill_(NAN)                              # stale columns must never reach a real tile
    K.conv2d_wino4_fwd(x, wp, cout, c["scale"].to(dev), c["shift"].to(dev), True, y, ws, cfg=K.wino4_cfg(case["geo"]))
    torch.cuda.synchronize()
    _held(y, c, "wino4 %s (%s, %s)" % (case["name"], case["kind"], case["edge"]))
    DC.check_surround(yb, y, 7.0)
    DC.check_surround(xb, x, NAN)


@pytest.mark.parametrize("case", DC.WINO4, ids=_ids(DC.WINO4))
def test_conv2d_wino4_fwd_every_geometry_word(dev, case):
    """words 1..6 (fp32 MFMA) and 11..16 (split operands) one by one, at T = 1, one below the word's column block, the block, one
    above, and with three images that end inside a block"""
    _fwd(dev, case)


@pytest.mark.parametrize("case", DC.WINO4_DEFAULT, ids=_ids(DC.WINO4_DEFAULT))
def test_conv2d_wino4_fwd_default_word_on_each_side_of_the_wide_tile(dev, case):
    """word 0 picks the 128 x 128 workgroup or the wide 256 x 192 one by w4_wide_pays: the last T before it pays, the first after"""
    assert DC.w4_wide_pays(case["T"], case["cout"]) == case["wide"]
    _fwd(dev, case)


def _tile_map(x, dev):
    """the active-tile map of the pixels where any channel of x is set, as sassd_wino4_tile_map builds it from sparse rows"""
    b, _, h, w = x.shape
    nz = (x != 0).any(1).nonzero()
    n = nz.shape[0]
    idx = torch.zeros(n + 5, 4, dtype=torch.int32)
    idx[:n, 0], idx[:n, 2], idx[:n, 3] = nz[:, 0].int(), nz[:, 1].int(), nz[:, 2].int()
    nptr = torch.tensor([n], dtype=torch.int32, device=dev)
    tmap = K.wino4_tile_map(idx.to(dev), nptr, n + 5, b, h, w)
    return tmap, int(tmap[0].item()), int(tmap[1].item())


@pytest.mark.parametrize("case", DC.CHAIN, ids=_ids(DC.CHAIN))
def test_conv2d_wino4_chain(dev, case):
    """one layer with its own output transform, and two layers with the map between them kept in the transform domain -- against
    float64 per element (ReLU is 1-Lipschitz and the comparison is on values: inputs near zero need no margin)"""
    b, cin, h, w = case["b"], case["cin"], case["h"], case["w"]
    c = DC.chain_case(case["kind"], b, cin, h, w, 31, case["layers"], band=case["tile_map"])
    assert K.conv2d_wino4_chain_supported(256, 256, h, w)
    xb, x = DC.embed(c["x"], poison=NAN, device=dev)
    yb, y = _out((b, 256, h, w), dev)
    wps = [K.conv2d_wino4_pack_weight(wt.to(dev)) for wt in c["ws"]]
    scs, shs = [t.to(dev) for t in c["scales"]], [t.to(dev) for t in c["shifts"]]
    wsb = K.conv2d_wino4_chain_workspace(b, 256, h, w, dev)
    wsb.view(torch.float32).fill_(NAN)
    tmap = None
    if case["tile_map"]:
        tmap, act, tot = _tile_map(c["x"], dev)
        assert 0 < act < tot, "the band leaves inactive tiles"
    last = case["layers"] == 1
    if not last:                                                    # the first layer's map from its own output transform
        ab, a1 = _out((b, 256, h, w), dev)
        K.conv2d_wino4_chain(x, None, wps[0], cin, 256, 256, b, h, w, scs[0], shs[0], True, a1, wsb, tile_map=tmap)
        torch.cuda.synchronize()
        wsb.view(torch.float32).fill_(NAN)
    K.conv2d_wino4_chain(x, None, wps[0], cin, 256, 256, b, h, w, scs[0], shs[0], True, y if last else None, wsb, tile_map=tmap)
    if not last:
        K.conv2d_wino4_chain(None, (scs[0], shs[0], True), wps[1], 256, 256, 256, b, h, w, scs[1], shs[1], True, y, wsb,
                             prev_tile_map=tmap)
    torch.cuda.synchronize()
    _held(y, c, "wino4 chain %s (%s)" % (case["name"], case["edge"]))
    if not last:
        # the second layer alone, on the map its own-transform launch stores (the fused transform forms the same values:
        # test_gpu_wino4.py holds them bit-equal), so that its bar is not diluted by the first layer's scale
        _held(a1, DC.chain_case(case["kind"], b, cin, h, w, 31, 1, band=case["tile_map"]), "wino4 chain %s, first layer" % case["name"])
        alone = DC.layer_alone(a1.cpu(), c["ws"][1], c["scales"][1], c["shifts"][1])
        _held(y, alone, "wino4 chain %s, the second layer on the first one's map" % case["name"])
        DC.check_surround(ab, a1, 7.0)
    DC.check_surround(yb, y, 7.0)
    DC.check_surround(xb, x, NAN)


@pytest.mark.parametrize("case", DC.TAIL, ids=_ids(DC.TAIL))
def test_conv2d_wino4_chain_tail(dev, case):
    """the narrow tail layer (<= 64 output channels on a 64-channel block) behind one chained layer"""
    b, cin, h, w, cout = case["b"], case["cin"], case["h"], case["w"], case["cout"]
    c = DC.chain_case(case["kind"], b, cin, h, w, 41, 1, tail_cout=cout)
    xb, x = DC.embed(c["x"], poison=NAN, device=dev)
    yb, y = _out((b, cout, h, w), dev)
    pb, yp = _out((b, 256, h, w), dev)
    wp0 = K.conv2d_wino4_pack_weight(c["ws"][0].to(dev))
    wpt = K.conv2d_wino4_pack_weight_narrow(c["ws"][1].to(dev))
    scs, shs = [t.to(dev) for t in c["scales"]], [t.to(dev) for t in c["shifts"]]
    wsb = K.conv2d_wino4_chain_workspace(b, 256, h, w, dev)
    wsb.view(torch.float32).fill_(NAN)
    K.conv2d_wino4_chain(x, None, wp0, cin, 256, 256, b, h, w, scs[0], shs[0], True, None, wsb)
    K.conv2d_wino4_chain_tail((scs[0], shs[0], True), yp, wpt, 256, cout, 256, b, h, w, scs[1], shs[1], True, y, wsb)
    torch.cuda.synchronize()
    _held(y, c, "wino4 chain tail %s, both layers" % case["name"])
    # y_prev is the previous layer's map as the fused transform itself formed it: that layer alone, and -- on exactly the map
    # it consumed -- the tail layer alone, whose bar is not diluted by the first layer's scale
    _held(yp, DC.chain_case(case["kind"], b, cin, h, w, 41, 1), "wino4 chain tail %s, y_prev" % case["name"])
    alone = DC.layer_alone(yp.cpu(), c["ws"][1], c["scales"][1], c["shifts"][1])
    _held(y, alone, "wino4 chain tail %s, the tail layer on y_prev" % case["name"])
    for buf, v in ((yb, y), (pb, yp)):
        DC.check_surround(buf, v, 7.0)
    DC.check_surround(xb, x, NAN)
