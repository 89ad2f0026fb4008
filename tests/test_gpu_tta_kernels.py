"""-m gpu: the two test-time augmentation kernels alone, against the numpy statement of their contract (sassd.tta.views_host /
pool_host; include/sassd.h "Test-time augmentation") -- bit for bit: the kernels only copy and apply the stated float32
arithmetic, and tests/test_tta_cpu.py holds the statement to the very header the kernels include."""
import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import _C, kernels as K, tta as T

import tta_cases as TC

pytestmark = pytest.mark.gpu

STALE = 0xA5A5A5A5          # what a destination holds before the launch: rows the kernel must leave alone keep it
CAP = 300                   # rows of every staging cloud: two workgroups of 256 floats and more at every width


def _dev_cloud(pts, dev, rows=CAP):
    buf = np.full((rows, pts.shape[1]), 0, np.uint32)
    buf[:] = 0x3F800000 + np.arange(rows * pts.shape[1], dtype=np.uint32).reshape(rows, -1)   # rows past n: not zeros
    buf[:len(pts)] = pts.view(np.uint32)
    return torch.from_numpy(buf.view(np.float32)).to(dev)


@pytest.mark.parametrize("ndim", [3, 4, 5, 8])
@pytest.mark.parametrize("n", [0, 1, 255, 257])
def test_tta_views_matches_views_host(dev, n, ndim):
    views = TC.V4_MIXED                                             # flip | rotate | flip + rotate + scale
    pts = TC.cloud(n, ndim, 100 * ndim + n)
    src = _dev_cloud(pts, dev)
    src_before = src.cpu().numpy().tobytes()
    n_src = torch.tensor([n], dtype=torch.int32, device=dev)
    guard = 16                                                      # stale rows under and over every destination
    bufs = [torch.from_numpy(np.full((CAP + 2 * guard, ndim), STALE, np.uint32).view(np.float32)).to(dev) for _ in range(3)]
    dst = [b[guard:guard + CAP] for b in bufs]
    cnt = torch.full((3,), -7, dtype=torch.int32, device=dev)
    K.tta_views(src, n_src, views, dst, [cnt[v:v + 1] for v in range(3)])
    torch.cuda.synchronize()
    want = T.views_host(pts, views)
    assert cnt.cpu().tolist() == [n, n, n]
    assert src.cpu().numpy().tobytes() == src_before and int(n_src.item()) == n          # the source is read only
    for v in range(3):
        got = bufs[v].cpu().numpy()
        assert TC.same_bits(got[guard:guard + n], want[v + 1]), (v, "view rows")
        rest = np.concatenate([got[:guard], got[guard + n:]]).view(np.uint32)
        assert (rest == STALE).all(), (v, "rows at or past n, or outside the destination, were written")
    if n >= 3 and ndim > 3:                                         # the bit patterns arithmetic would destroy
        u = bufs[2].cpu().numpy().view(np.uint32)
        assert u[guard + 2, 3] == TC.NAN_PAYLOAD and u[guard + 1, 2] == TC.INF


def test_tta_views_with_one_view_writes_nothing(dev):
    pts = TC.cloud(257, 4, 1)
    src = _dev_cloud(pts, dev)
    n_src = torch.tensor([257], dtype=torch.int32, device=dev)
    before = src.cpu().numpy().tobytes()
    assert K.tta_views(src, n_src, TC.V1, [], []) == ([], [])
    torch.cuda.synchronize()
    assert src.cpu().numpy().tobytes() == before and int(n_src.item()) == 257


def test_tta_views_clamps_a_count_above_the_capacity(dev):
    pts = TC.cloud(CAP, 5, 2)
    src = _dev_cloud(pts, dev)
    n_src = torch.tensor([CAP + 1000], dtype=torch.int32, device=dev)
    dst = [torch.zeros(CAP, 5, device=dev)]
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    K.tta_views(src, n_src, TC.V2, dst, [cnt])
    torch.cuda.synchronize()
    assert int(cnt.item()) == CAP and TC.same_bits(dst[0].cpu().numpy(), T.views_host(pts, TC.V2)[1])


def _pool(dev, cap_p, status0=0):
    g, lo, la, cnt = TC.candidates(2, 3, 8, [0, 8, 11, 3, 0, 8], 11)        # b = 2, V = 3, capK = 8; 11 is clamped to 8
    guard = 5
    gp = torch.from_numpy(np.full((2 * cap_p + 2 * guard, 7), STALE, np.uint32).view(np.float32)).to(dev)
    lp = torch.from_numpy(np.full(2 * cap_p + 2 * guard, STALE, np.uint32).view(np.float32)).to(dev)
    lb = torch.full((2 * cap_p + 2 * guard,), -77, dtype=torch.int32, device=dev)
    out = dict(guided=gp[guard:guard + 2 * cap_p].view(2, cap_p, 7), logits=lp[guard:guard + 2 * cap_p].view(2, cap_p),
               labels=lb[guard:guard + 2 * cap_p].view(2, cap_p), counts=torch.full((2,), -1, dtype=torch.int32, device=dev))
    status = torch.tensor([status0], dtype=torch.int32, device=dev)
    ins = [torch.from_numpy(a).to(dev) for a in (g, lo, la, cnt)]
    K.tta_pool(*ins, TC.V3, cap_p, out=out, status=status)
    torch.cuda.synchronize()
    want = T.pool_host(g, lo, la, cnt, TC.V3, cap_p)
    for a, t in zip((g, lo, la, cnt), ins):                                 # the inputs are read only
        assert TC.same_bits(t.cpu().numpy(), a)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert list(got["counts"]) == list(want["counts"])
    for s in range(2):
        k = int(want["counts"][s])
        assert TC.same_bits(got["guided"][s, :k], want["guided"][s, :k]), s
        assert TC.same_bits(got["logits"][s, :k], want["logits"][s, :k]) and TC.same_bits(got["labels"][s, :k], want["labels"][s, :k])
        # rows past the pooled count are left alone
        assert (got["guided"][s, k:].view(np.uint32) == STALE).all() and (got["logits"][s, k:].view(np.uint32) == STALE).all()
        assert (got["labels"][s, k:] == -77).all()
    for t, stale in ((gp, STALE), (lp, STALE)):                             # nothing outside the buffers
        u = t.cpu().numpy().view(np.uint32)
        assert (u[:guard] == stale).all() and (u[guard + 2 * cap_p:] == stale).all()
    assert (lb[:guard] == -77).all() and (lb[guard + 2 * cap_p:] == -77).all()
    return got, want, int(status.item())


def test_tta_pool_matches_pool_host(dev):
    got, want, status = _pool(dev, 24, status0=_C.ST_VOXEL_OVERFLOW)        # capP = V capK: every row fits
    assert list(got["counts"]) == [16, 11] and not want["overflow"]
    assert status == _C.ST_VOXEL_OVERFLOW                                   # OR-ed into only, and not set here
    assert got["guided"].view(np.uint32)[1, 0, 0] != STALE
    assert got["guided"][0].view(np.uint32)[0, 2] != TC.NAN_PAYLOAD         # sample 0's identity view is empty: row 0 is view 1's


def test_tta_pool_identity_rows_are_copied_as_bits(dev):
    g, lo, la, cnt = TC.candidates(1, 2, 8, [8, 8], 3)
    out = K.tta_pool(*[torch.from_numpy(a).to(dev) for a in (g, lo, la, cnt)], TC.V2, 16)
    torch.cuda.synchronize()
    got = out["guided"].cpu().numpy()
    assert TC.same_bits(got[0, :8], g[0]) and got.view(np.uint32)[0, 0, 2] == TC.NAN_PAYLOAD
    assert got.view(np.uint32)[0, 1, 1] == TC.NEG_ZERO


def test_tta_pool_overflow_keeps_the_prefix_and_sets_the_flag(dev):
    full, _, _ = _pool(dev, 24)
    got, want, status = _pool(dev, 12)                                      # sample 0 pools 16 rows: capP below the pooled sum
    assert want["overflow"] and status == _C.ST_BOX_OVERFLOW
    assert list(got["counts"]) == [12, 11]
    assert TC.same_bits(got["guided"][0], full["guided"][0, :12]) and TC.same_bits(got["logits"][0], full["logits"][0, :12])
    assert TC.same_bits(got["guided"][1, :11], full["guided"][1, :11])
