"""-m gpu: BEV conv0 straight from the sparse tensor (sassd_wino4_sparse_prepare + sassd_conv2d_wino4_chain_sparse) against the
sequence it replaces, sassd_densify(channel_order 1) + sassd_wino4_tile_map + sassd_conv2d_wino4_chain(tile_map): the conv0 output
and the transformed input V (columns in use) BIT FOR BIT, the rebuilt tile map int for int against a numpy restatement of its
definition, and a whole frame of an InferencePlan on either entry, eager and as replayed graphs.

Cout is 256 in every case: 128 output channels are refused by sassd_conv2d_wino4_supported (Cout % 256 == 0) on BOTH sides of the
comparison, so 256 is the smallest width at which there is anything to compare."""
import numpy as np
import pytest
import torch

from sassd import kernels as K
from sassd.pipeline import InferencePlan
import helpers as H
import test_bf16_infer_cpu as B16

pytestmark = pytest.mark.gpu
C, COUT = 64, 256


def _want_map(coords, b, h, w):
    """[0] active tiles, [1] T, tpos[T], tlist[:active]: a tile is active when a voxel lies in its patch rows / columns
    4 t - 1 .. 4 t + 4 (the kernel's comment)."""
    th, tw = h // 4, w // 4
    want = np.zeros((b, th, tw), bool)
    for bb, _, yy, xx in coords:
        for ty in {yy // 4, (yy - 1) // 4 if yy % 4 == 0 else yy // 4, (yy + 1) // 4 if yy % 4 == 3 else yy // 4}:
            for tx in {xx // 4, (xx - 1) // 4 if xx % 4 == 0 else xx // 4, (xx + 1) // 4 if xx % 4 == 3 else xx // 4}:
                if 0 <= ty < th and 0 <= tx < tw:
                    want[bb, ty, tx] = True
    act = np.flatnonzero(want.reshape(-1))
    pos = np.full(b * th * tw, -1, np.int64)
    pos[act] = np.arange(len(act))
    return act, pos


def _check_map(tmap, coords, b, h, w):
    t = b * (h // 4) * (w // 4)
    act, pos = _want_map(coords, b, h, w)
    tm = tmap.cpu().numpy()
    assert tm[0] == len(act) and tm[1] == t and tm[2] == 0 and tm[3] == 0, (tm[:4], len(act), t)
    assert np.array_equal(tm[4:4 + t], pos)
    assert np.array_equal(tm[4 + t:4 + t + len(act)], act)
    return len(act)


def _cases(b, d, h, w, rng):
    """name -> (coordinates [n, 4] (b, z, y, x), unique; rows handed over; value of the device count)"""
    def uniq(a):
        return np.unique(np.asarray(a, np.int64).reshape(-1, 4), axis=0)
    out = {}
    border = [(bb, zz, yy, xx) for bb in range(b) for zz in (0, d - 1) for yy in (0, h - 1) for xx in range(w)]
    border += [(bb, zz, yy, xx) for bb in range(b) for zz in (0, d - 1) for yy in range(h) for xx in (0, w - 1)]
    out["a_borders_and_corners"] = uniq(border)
    edge = [(bb, int(rng.integers(d)), yy, xx) for bb in range(b) for yy in range(h) for xx in range(w)
            if yy % 4 in (0, 3) and xx % 4 in (0, 3) and rng.random() < 0.3]
    edge += [(0, 0, 4, 4), (0, d - 1, 7, 3), (b - 1, 1, 3, 8)]       # 4 tiles, 4 tiles, 2 x 2 tiles at the seams
    out["b_tile_seams"] = uniq(edge)
    out["c_empty"] = np.zeros((0, 4), np.int64)
    full = uniq([(bb, zz, yy, xx) for bb in range(b) for zz in range(d) for yy in range(h) for xx in range(w)])
    out["d_count_above_cap"] = full[rng.permutation(len(full))[:min(len(full), 300)]]
    if b == 2:
        out["e_second_image_empty"] = uniq([(0, int(rng.integers(d)), int(rng.integers(h)), int(rng.integers(w)))
                                            for _ in range(60)])
    out["f_every_pixel_at_one_depth"] = uniq([(bb, d // 2, yy, xx) for bb in range(b) for yy in range(h) for xx in range(w)])
    out["g_single_voxel"] = uniq([(b - 1, d - 1, h // 2 + 1, w // 2 + 2)])
    return out


class _Layer:
    """one conv0 on either entry, through buffers that are REUSED from call to call (nothing is cleared in between)"""

    def __init__(self, dev, b, d, h, w, rows):
        g = torch.Generator().manual_seed(1000 * d + h)
        self.dev, self.b, self.d, self.h, self.w, self.rows = dev, b, d, h, w, rows
        self.cin = C * d
        self.cmax = max(self.cin, COUT)
        wt = torch.randn(COUT, self.cin, 3, 3, generator=g) * (2.0 / (self.cin * 9)) ** 0.5
        self.wp = K.conv2d_wino4_pack_weight(wt.to(dev))
        self.scale = (torch.rand(COUT, generator=g) + 0.5).to(dev)
        self.shift = (torch.randn(COUT, generator=g) * 0.1).to(dev)
        self.ws = [K.conv2d_wino4_chain_workspace(b, self.cmax, h, w, dev) for _ in range(2)]
        for ws_ in self.ws:
            ws_.view(torch.float32).fill_(float("nan"))               # a column that is read without being written shows
        self.grid = K.wino4_sparse_grid(b, d, h, w, dev)
        self.tmap = torch.zeros(K._C.lib().sassd_wino4_tile_map_ints(b, h, w), dtype=torch.int32, device=dev)
        self.tmap_ref = torch.zeros_like(self.tmap)
        self.dense = torch.empty(b, self.cin, h, w, device=dev)
        self.idx = torch.zeros(rows, 4, dtype=torch.int32, device=dev)
        self.t = b * (h // 4) * (w // 4)
        self.tp = (self.t + 127) // 128 * 128                         # plane stride of V: the default GEMM's 128-column block

    def run(self, coords, feats, count, cap):
        n = len(coords)
        idx = torch.tensor([0, 0, 1, 1], dtype=torch.int32).repeat(self.rows, 1)     # rows past the count must be ignored
        idx[:n] = torch.from_numpy(coords).int()
        self.idx.copy_(idx)
        nptr = torch.tensor([count], dtype=torch.int32, device=self.dev)
        b, d, h, w = self.b, self.d, self.h, self.w
        # the sequence it replaces
        K.densify(feats, self.idx, nptr, cap, (d, h, w), b, 1, out=self.dense)
        K.wino4_tile_map(self.idx, nptr, cap, b, h, w, out=self.tmap_ref)
        y_ref = torch.empty(b, COUT, h, w, device=self.dev)
        K.conv2d_wino4_chain(self.dense, None, self.wp, self.cin, COUT, self.cmax, b, h, w, self.scale, self.shift, True, y_ref,
                             self.ws[0], tile_map=self.tmap_ref)
        # the sparse entry
        K.wino4_sparse_prepare(self.idx, nptr, cap, b, d, h, w, self.grid, self.tmap)
        y = torch.empty(b, COUT, h, w, device=self.dev)
        K.conv2d_wino4_chain_sparse(feats, d, self.grid, self.wp, self.cin, COUT, self.cmax, b, h, w, self.scale, self.shift, True,
                                    y, self.ws[1], self.tmap)
        torch.cuda.synchronize()
        used = coords[:min(count, cap, n)]
        ncol = _check_map(self.tmap, used, b, h, w)
        _check_map(self.tmap_ref, used, b, h, w)
        grid = self.grid.view(b, d, h, w).cpu().numpy()
        want_grid = np.full((b, d, h, w), -1, np.int32)
        want_grid[tuple(used.T)] = np.arange(len(used))
        assert np.array_equal(grid, want_grid)
        v_ref, v = (ws_.view(torch.float32)[:36 * self.cin * self.tp].view(36, self.cin, self.tp)[:, :, :ncol] for ws_ in self.ws)
        assert torch.equal(v_ref, v), ("V", (v_ref - v).abs().max().item())
        assert torch.isfinite(y).all()
        assert torch.equal(y_ref, y), ("y", (y_ref - y).abs().max().item())
        return ncol


@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("hw", [(16, 16), (12, 20), (8, 36)])
@pytest.mark.parametrize("d", [2, 5])
def test_sparse_entry_equals_densify_plus_chain_bit_for_bit(dev, d, hw, b):
    h, w = hw
    rng = np.random.default_rng(100 * d + h + b)
    cases = _cases(b, d, h, w, rng)
    rows = max(len(c) for c in cases.values()) + 37
    L = _Layer(dev, b, d, h, w, rows)
    feats = torch.from_numpy(rng.standard_normal((rows, C)).astype(np.float32)).to(dev)
    seen = {}
    for name, coords in cases.items():
        coords = coords[rng.permutation(len(coords))]                 # rows arrive in no particular order
        count, cap = len(coords), rows
        if name.startswith("d_"):
            cap, count = len(coords) - 50, len(coords)                # the device count exceeds the capacity: clamped
        seen[name] = L.run(coords, feats, count, cap)
    t = L.t
    assert seen["c_empty"] == 0 and seen["f_every_pixel_at_one_depth"] == t and 0 < seen["g_single_voxel"] <= 4
    # (h) a second frame through the same buffers whose voxels are a strict subset of the first's: a grid entry, a tile flag or
    # a V column that was not rebuilt would show
    first = cases["a_borders_and_corners"]
    n1 = L.run(first, feats, len(first), rows)
    sub = first[rng.permutation(len(first))[:max(1, len(first) // 7)]]
    sub = sub[sub[:, 2] < h // 2]                                      # ... and only in the upper half of the image
    assert 0 < len(sub) < len(first)
    n2 = L.run(sub, feats, len(sub), rows)
    assert n2 < n1
    print("sparse entry %s: active tiles per case %s, then %d -> %d: y, V and the maps bit-identical" % ((b, d, hw), seen, n1, n2))


def test_tile_map_at_the_kitti_size(dev):
    """T = 2200 tiles: three workgroups of the ordered compaction, 13 000 rows in the flag pass"""
    b, d, h, w = 1, 5, 200, 176
    rng = np.random.default_rng(7)
    occ = rng.random((h, w)) < 0.17
    occ[: h // 3] = False                                              # clustered, as a KITTI frame is
    yx = np.argwhere(occ)
    coords = np.stack([np.zeros(len(yx), np.int64), rng.integers(0, d, len(yx)), yx[:, 0], yx[:, 1]], 1)
    coords = coords[rng.permutation(len(coords))]
    cap = len(coords) + 100
    idx = torch.zeros(cap, 4, dtype=torch.int32)
    idx[:len(coords)] = torch.from_numpy(coords).int()
    nptr = torch.tensor([len(coords)], dtype=torch.int32, device=dev)
    tmap = K.wino4_tile_map(idx.to(dev), nptr, cap, b, h, w)
    grid = K.wino4_sparse_grid(b, d, h, w, dev)
    tmap2 = torch.zeros_like(tmap)
    K.wino4_sparse_prepare(idx.to(dev), nptr, cap, b, d, h, w, grid, tmap2)
    torch.cuda.synchronize()
    n = _check_map(tmap, coords, b, h, w)
    assert _check_map(tmap2, coords, b, h, w) == n and 0 < n < 2200
    want = np.full((b, d, h, w), -1, np.int32)
    want[tuple(coords.T)] = np.arange(len(coords))
    assert np.array_equal(grid.view(b, d, h, w).cpu().numpy(), want)


def _frame_state(plan):
    k = int(plan.det["counts"][0].item())
    return [t.clone() for t in (plan.det["counts"], plan.det["boxes"][0, :k], plan.det["scores"][0, :k], plan.det["labels"][0, :k],
                                plan.x, plan.conv6)]


def test_whole_frame_on_either_entry_is_bit_identical(dev):
    """One seeded synthetic frame on the car grid (the grid every whole-frame test of the plan uses): a plan with
    dense_entry=True and a default plan leave the same BEV feature map and the same detections, eager and as replayed graphs
    (three replays with a device allocation and free in between).  The default plan holds no dense map until one is read."""
    model, _ = B16.car_model()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    an, bv = B16.car_anchors()
    pts = torch.from_numpy(H.frame("k21", 0)).to(dev)
    dense = InferencePlan(sd, batch_size=1, anchors=an, anchors_bv=bv, device=dev, dense_entry=True)
    sparse = InferencePlan(sd, batch_size=1, anchors=an, anchors_bv=bv, device=dev)
    assert sparse.sparse_entry and sparse._dense is None and not dense.sparse_entry and dense._dense is not None
    for p in (dense, sparse):
        p.run_from_points([pts])
    torch.cuda.synchronize()
    assert int(sparse.status.item()) == 0 and int(dense.status.item()) == 0
    want = _frame_state(dense)
    assert int(want[0].item()) >= 1, "the frame produced no detections"
    for j, (a, b_) in enumerate(zip(want, _frame_state(sparse))):
        assert a.shape == b_.shape and torch.equal(a, b_), ("eager", j)
    assert torch.equal(sparse.dense, dense.dense)                     # a read materialises the map of the current frame
    for overlap in (False, True):                                     # the one-branch graph bench.py keeps in flight, the two-branch one
        gd = InferencePlan(sd, batch_size=1, anchors=an, anchors_bv=bv, device=dev, overlap=overlap, dense_entry=True)
        gs = InferencePlan(sd, batch_size=1, anchors=an, anchors_bv=bv, device=dev, overlap=overlap)
        for p in (gd, gs):
            p.capture(int(pts.shape[0]) + 64)
        for nbytes in (2 << 20, 64 << 20, 256 << 20):
            junk = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            junk.fill_(255)
            torch.cuda.synchronize()
            del junk
            for p in (gd, gs):
                p.run_graph([pts])
            torch.cuda.synchronize()
            for j, (a, b_, c_) in enumerate(zip(want, _frame_state(gd), _frame_state(gs))):
                assert a.shape == c_.shape and torch.equal(a, b_) and torch.equal(a, c_), ("graph", overlap, nbytes, j)
