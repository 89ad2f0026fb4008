"""-m gpu: the wide wave tiles of the Winograd GEMM (cfg geometries 15 = 256 x 192 and 16 = 256 x 256 per workgroup, four waves
of 128 x 96 / 128 x 128) and the sliced epilogue (theirs, and geometry 14's) against geometry 12, the 128 x 128 workgroup of
64 x 64 waves.  Every tile shape issues the MFMAs of one output element in the same order over the same split operands, so the
results must be EQUAL bit for bit -- the BEV parity bars of the pipeline tests have little headroom, and equality is what lets
a plan change geometry under them.  256 -> 256 channels (the smallest layer the kernel takes) on maps of 4 to 240 tiles:
a single partial column block, blocks crossed inside an image and between images, and a compacted (active-tile) launch whose
last column blocks are never run."""
import pytest
import torch

import sassd
from sassd import kernels as K

pytestmark = pytest.mark.gpu

C = 256
REF, WIDE_A, WIDE_B, KC16 = 12, 15, 16, 14
SHAPES = [(1, 8, 8),        # 4 tiles: one partial column block
          (1, 40, 36),      # 90 tiles
          (1, 56, 56),      # 196 tiles: crosses a 192-column block, the second one partial
          (2, 48, 40)]      # 240 tiles: the batch inside the column index

_cache = {}


def _layer(dev, shape):
    """seeded input, packed weights, epilogue and geometry 12's output of one shape -- computed once, shared, never modified"""
    if shape not in _cache:
        b, h, w = shape
        g = torch.Generator().manual_seed(1000 * b + 10 * h + w)
        x = torch.randn(b, C, h, w, generator=g)
        x *= (torch.rand(b, C, h, w, generator=g) > 0.5).float()
        wt = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (C * 9)) ** 0.5
        sc, sh = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.1).to(dev)
        xd, wp = x.to(dev), K.conv2d_wino4_pack_weight(wt.to(dev))
        ref = K.conv2d_wino4_fwd(xd, wp, C, sc, sh, True, cfg=K.wino4_cfg(REF))
        torch.cuda.synchronize()
        assert torch.isfinite(ref).all() and ref.abs().max().item() > 0.1
        _cache[shape] = (xd, wp, sc, sh, ref)
    return _cache[shape]


def _fwd_equals_ref(dev, shape, geo):
    xd, wp, sc, sh, ref = _layer(dev, shape)
    b, h, w = shape
    ws = K.conv2d_wino4_workspace(b, C, C, h, w, dev)
    ws.view(torch.float32).fill_(float("nan"))               # columns past the tiles must never reach an output
    y = torch.full_like(ref, 7.0)
    K.conv2d_wino4_fwd(xd, wp, C, sc, sh, True, y, ws, cfg=K.wino4_cfg(geo))
    torch.cuda.synchronize()
    assert torch.equal(y, ref), (geo, shape, (y - ref).abs().max().item())


@pytest.mark.parametrize("shape", SHAPES)
def test_wide_tile_a_fwd_is_bit_identical(dev, shape):
    _fwd_equals_ref(dev, shape, WIDE_A)


def test_wide_tile_b_fwd_is_bit_identical(dev):
    _fwd_equals_ref(dev, (1, 56, 56), WIDE_B)


def test_kc16_sliced_epilogue_is_bit_identical(dev):
    """geometry 14 (128 x 128 workgroup, 16-channel chunks) stores its 64-row wave image in two 32-row slices"""
    _fwd_equals_ref(dev, (1, 56, 56), KC16)
    _fwd_equals_ref(dev, (2, 48, 40), KC16)


@pytest.mark.parametrize("geo", [WIDE_A, WIDE_B])
def test_wide_tile_chain_on_active_tiles_is_bit_identical(dev, geo):
    """Two chained layers on a compacted launch: 80 x 80 pixels = 400 tiles, the occupied pixels in the upper half of the map, so
    about half of the tiles are active and sit in the first columns -- the column blocks behind them are skipped by the device
    count (`ncols_dev`), and layer 2 reads layer 1's compacted products through the map (`prev_tile_map`).  The same two calls
    with geometry 12 are the reference; the tail layer of a chain follows the wide geometry's plane stride too."""
    b, h, w = 1, 80, 80
    g = torch.Generator().manual_seed(geo)
    occ = torch.rand(b, h, w, generator=g) < 0.3
    occ[:, h // 2 - 2:] = False
    x = torch.randn(b, C, h, w, generator=g) * occ.unsqueeze(1).float()
    nz = occ.nonzero()
    n = nz.shape[0]
    cap = n + 5
    idx = torch.zeros(cap, 4, dtype=torch.int32)
    idx[:n, 0], idx[:n, 2], idx[:n, 3] = nz[:, 0].int(), nz[:, 1].int(), nz[:, 2].int()
    tmap = K.wino4_tile_map(idx.to(dev), torch.tensor([n], dtype=torch.int32, device=dev), cap, b, h, w)
    T = b * (h // 4) * (w // 4)
    nact = int(tmap[0].item())
    assert 0.4 * T <= nact <= 0.6 * T and nact + 128 <= T        # about half, and whole column blocks without an active tile
    ws_ = [torch.randn(C, C, 3, 3, generator=g) * (2.0 / (C * 9)) ** 0.5 for _ in range(2)]
    wt = torch.randn(28, C, 3, 3, generator=g) * (2.0 / (C * 9)) ** 0.5
    scs = [(torch.rand(C, generator=g) + 0.5).to(dev) for _ in range(3)]
    shs = [(torch.randn(C, generator=g) * 0.1).to(dev) for _ in range(3)]
    wps = [K.conv2d_wino4_pack_weight(v.to(dev)) for v in ws_]
    wpt = K.conv2d_wino4_pack_weight_narrow(wt.to(dev))
    xd = x.to(dev)
    wsb = K.conv2d_wino4_chain_workspace(b, C, h, w, dev)

    def run(cfg, tail):
        y = torch.full((b, 28 if tail else C, h, w), 7.0, device=dev)
        wsb.view(torch.float32).fill_(float("nan"))
        K.conv2d_wino4_chain(xd, None, wps[0], C, C, C, b, h, w, scs[0], shs[0], True, None, wsb, cfg=cfg, tile_map=tmap)
        K.conv2d_wino4_chain(None, (scs[0], shs[0], True), wps[1], C, C, C, b, h, w, scs[1], shs[1], True, None if tail else y,
                             wsb, cfg=cfg, prev_tile_map=tmap)
        if tail:
            K.conv2d_wino4_chain_tail((scs[1], shs[1], True), None, wpt, C, 28, C, b, h, w, scs[2][:28].contiguous(),
                                      shs[2][:28].contiguous(), True, y, wsb, cfg=cfg)
        torch.cuda.synchronize()
        return y

    for tail in (False, True):
        ref, y = run(K.wino4_cfg(REF), tail), run(K.wino4_cfg(geo), tail)
        assert torch.isfinite(ref).all() and ref.abs().max().item() > 0.1
        assert torch.equal(y, ref), (geo, tail, (y - ref).abs().max().item())
