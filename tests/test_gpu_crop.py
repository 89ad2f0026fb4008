"""-m gpu: sassd_crop_polytope_dev against a numpy model of its contract (include/sassd.h "Frustum crop").

The model evaluates ((x*a + y*b) + z*c) + d for the six planes in float64 -- or in float32 with f32_math -- keeps a row when
no plane gives a value >= 0, and boolean-indexes: numpy neither contracts nor reorders, which is what `#pragma clang fp
contract(off)` gives inside_polytope.  The kernel only tests and copies, so every comparison is exact: rows byte for byte,
the count, the status word, and every byte the call must not touch."""
import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import _C, geometry as G, kernels as K

import augment_synth as A

pytestmark = pytest.mark.gpu

CAP_IN = 6144
SENTINEL = 0x5A5AA5A5                    # bit pattern of every float the call must leave alone
INSIDE = (20.0, 0.5, -0.5, 0.25)         # a point inside the frustum: what the rows past n hold (they must not be read as data)
_CACHE = {}


def frustum(shape=(375, 1242)):
    if shape not in _CACHE:
        c = A.calib_matrices()
        rect, trv2c, p2 = (A.extend(c[k]) for k in ("R0_rect", "Tr_velo_to_cam", "P2"))
        _CACHE[shape] = (G.frustum_planes(rect, trv2c, p2, shape)[0], (rect, trv2c, p2))
    return _CACHE[shape]


def sweep(n, ndim=4, seed=1):
    key = ("sweep", n, ndim, seed)
    if key not in _CACHE:
        pts = A.full_sweep(seed, n) if n else np.zeros((0, 4), np.float32)
        if ndim > 4:                     # extra columns: distinct values, copied like the rest
            extra = np.arange(n * (ndim - 4), dtype=np.float32).reshape(n, ndim - 4) + 0.5
            pts = np.concatenate([pts, extra], 1)
        _CACHE[key] = np.ascontiguousarray(pts, np.float32)
    return _CACHE[key]


def box_planes(lo, hi):
    """The six planes of the open box lo < (x, y, z) < hi."""
    pl = np.zeros((6, 4))
    for a in range(3):
        pl[2 * a, a], pl[2 * a, 3] = 1.0, -hi[a]          # x - hi < 0
        pl[2 * a + 1, a], pl[2 * a + 1, 3] = -1.0, lo[a]  # lo - x < 0
    return pl


def crop_model(pts, planes, f32_math):
    """-> the kept rows of `pts`, in order."""
    t = np.float32 if f32_math else np.float64
    x, y, z = (pts[:, i].astype(t) for i in range(3))
    pl = planes.astype(t)
    out = np.zeros(len(pts), bool)
    for k in range(6):
        s = ((x * pl[k, 0] + y * pl[k, 1]) + z * pl[k, 2]) + pl[k, 3]
        assert s.dtype == t
        out |= s >= 0
    return pts[~out]


class Buffers:
    """Device buffers of one call: `raw` [cap_in (+ guard)] holding the cloud and, past n, rows that WOULD be kept; `out`
    [cap_out + guard] pre-filled with the sentinel; count words and a status word."""

    def __init__(self, dev, cap_in, cap_out, ndim, guard=8):
        self.dev, self.cap_in, self.cap_out, self.ndim, self.guard = dev, cap_in, cap_out, ndim, guard
        self.raw_all = torch.empty(cap_in + guard, ndim, dtype=torch.float32, device=dev)
        self.out_all = torch.empty(cap_out + guard, ndim, dtype=torch.float32, device=dev)
        self.raw, self.out = self.raw_all[:cap_in], self.out_all[:cap_out]
        self.n_in = torch.zeros(1, dtype=torch.int32, device=dev)
        self.n_out = torch.full((1,), -77, dtype=torch.int32, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.planes = torch.zeros(6, 4, dtype=torch.float64, device=dev)

    def load(self, pts, n_in, planes, status=0):
        fill = np.tile(np.asarray(INSIDE + (1.0,) * (self.ndim - 4), np.float32)[:self.ndim], (self.cap_in + self.guard, 1))
        fill[:len(pts)] = pts
        self.raw_all.copy_(torch.from_numpy(fill))
        self.out_all.view(torch.int32).fill_(SENTINEL)
        self.n_in.fill_(n_in)
        self.n_out.fill_(-77)
        self.status.fill_(status)
        self.planes.copy_(torch.from_numpy(np.ascontiguousarray(planes, np.float64)))

    def call(self, f32_math):
        K.crop_polytope(self.raw, self.n_in, self.planes, f32_math, self.out, self.n_out, self.status)

    def check(self, want, tag, status=0, overflow=False):
        """`want`: every kept row, in order.  The call wrote min(len(want), cap_out) of them and nothing else."""
        torch.cuda.synchronize()
        got = self.out_all.cpu().numpy()
        k = min(len(want), self.cap_out)
        n_out, st = int(self.n_out.item()), int(self.status.item())
        print("%s: kept %d of cap_out %d, n_out %d, status 0x%x" % (tag, len(want), self.cap_out, n_out, st))
        assert n_out == k, (tag, n_out, k)
        assert got[:k].tobytes() == np.ascontiguousarray(want[:k]).tobytes(), tag
        assert (got[k:].view(np.uint32) == SENTINEL).all(), (tag, "rows at and beyond n_out, or the guard rows, were written")
        assert st == (status | (_C.ST_POINT_OVERFLOW if overflow else 0)), (tag, st)


def run(dev, pts, planes, f32_math=False, cap_in=CAP_IN, cap_out=None, n_in=None, status=0, tag=""):
    ndim = pts.shape[1]
    cap_out = cap_in if cap_out is None else cap_out
    b = Buffers(dev, cap_in, cap_out, ndim)
    b.load(pts, len(pts) if n_in is None else n_in, planes, status)
    b.call(f32_math)
    return b


KEPT = {0: 0, 1: 1, 63: 8, 64: 8, 65: 10, 1023: 207, 1024: 211, 1025: 214, 6000: 1224}     # full_sweep(1, n) in the frustum


@pytest.mark.parametrize("ndim", [4, 5])
@pytest.mark.parametrize("n", sorted(KEPT))
def test_sizes_across_a_wave_a_block_and_several_blocks(dev, n, ndim):
    planes, calib = frustum()
    pts = sweep(n, ndim)
    want = crop_model(pts, planes, False)
    assert len(want) == KEPT[n]                                         # the inputs are the ones the counts were taken on
    b = run(dev, pts, planes, tag="n %d ndim %d" % (n, ndim))
    b.check(want, ("sizes", n, ndim), status=0)
    if n == 6000 and ndim == 4:                                         # the same rows as today's path
        today = G.remove_outside_points(pts, *calib, (375, 1242))
        assert today.tobytes() == want.tobytes() and len(today) == 1224


def test_status_is_only_ored_into(dev):
    planes, _ = frustum()
    pts = sweep(1025)
    b = run(dev, pts, planes, status=_C.ST_BOX_OVERFLOW)
    b.check(crop_model(pts, planes, False), "status kept", status=_C.ST_BOX_OVERFLOW)


@pytest.mark.parametrize("f32_math", [False, True])
def test_points_on_a_face_are_outside(dev, f32_math):
    planes = box_planes((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    below, above = np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2))
    rows = [(0.0, 0.0, 0.0, 0.0)]
    for a in range(3):
        for sgn in (1.0, -1.0):
            for v in (1.0, below, above):
                p = [0.25, -0.5, 0.75, float(len(rows))]
                p[a] = sgn * float(v)
                rows.append(tuple(p))
    rows += [(1.0, 1.0, 1.0, 90.0), (below, -below, below, 91.0), (-0.0, 0.0, -0.0, 92.0)]
    pts = np.asarray(rows, np.float32)
    want = crop_model(pts, planes, f32_math)
    on_face = [i for i, r in enumerate(rows) if 1.0 in np.abs(np.asarray(r[:3], np.float32)).tolist()]
    assert len(on_face) == 7 and not set(pts[on_face, 3].tolist()) & set(want[:, 3].tolist())    # s == 0 is outside
    assert len(want) == 1 + 6 + 2                                       # the origin, the six just-inside points, two more
    run(dev, pts, planes, f32_math=f32_math, cap_in=64).check(want, ("faces", f32_math))


def test_f32_math_is_evaluated_in_float32(dev):
    """A plane on which the float32 and the float64 sums differ in sign for some points: each mode follows its own model."""
    planes = box_planes((-1e6, -1e6, -1e6), (1e6, 1e6, 1e6))
    planes[0] = (1.0, 1.0 / 3.0, 0.1, -30.0)                            # x + y/3 + z/10 < 30
    r = np.random.default_rng(5)
    y, z = r.uniform(-30, 30, 4000), r.uniform(-3, 3, 4000)
    x = 30.0 - y / 3.0 - z * 0.1 + r.choice([-1e-6, 0.0, 1e-6], 4000)     # on the plane to within float32 rounding
    pts = np.stack([x, y, z, np.arange(4000)], 1).astype(np.float32)
    w64, w32 = crop_model(pts, planes, False), crop_model(pts, planes, True)
    assert 100 < len(w64) < 3900 and w64.tobytes() != w32.tobytes()     # the two modes disagree on these inputs
    run(dev, pts, planes, f32_math=False).check(w64, "float64 mode")
    run(dev, pts, planes, f32_math=True).check(w32, "float32 mode")


def test_all_kept_and_none_kept(dev):
    pts = sweep(6000)
    huge = box_planes((-1e6, -1e6, -1e6), (1e6, 1e6, 1e6))
    run(dev, pts, huge).check(pts, "all kept")
    unit = box_planes((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))             # the sweep starts 2 m from the sensor
    none = crop_model(pts, unit, False)
    assert len(none) == 0
    run(dev, pts, unit).check(none, "none kept")


@pytest.mark.parametrize("ndim", [4, 5])
def test_overflow_writes_the_first_cap_out_rows(dev, ndim):
    planes, _ = frustum()
    pts = sweep(6000, ndim)
    want = crop_model(pts, planes, False)
    run(dev, pts, planes, cap_out=len(want) - 1).check(want, ("overflow", ndim), overflow=True)
    run(dev, pts, planes, cap_out=len(want)).check(want, ("exact fit", ndim), overflow=False)
    run(dev, pts, planes, cap_out=1).check(want, ("cap_out 1", ndim), overflow=True)


def test_input_count_above_capacity(dev):
    planes, _ = frustum()
    pts = sweep(6000)[:1024]
    want = crop_model(pts, planes, False)
    # the buffer holds cap_in = 1024 rows; the 8 guard rows behind it would be kept if they were read
    run(dev, pts, planes, cap_in=1024, n_in=1024 + 5).check(want, "n_in > cap_in", overflow=True)
    run(dev, pts, planes, cap_in=1024, n_in=-3).check(want[:0], "negative count")


def test_graph_replay_with_a_smaller_count_after_a_larger_one(dev):
    planes_a, _ = frustum()
    planes_b, _ = frustum((370, 1224))
    planes_c = box_planes((0.0, -10.0, -2.0), (40.0, 10.0, 1.0))
    b = Buffers(dev, CAP_IN, CAP_IN, 4)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        b.load(sweep(6000), 6000, planes_a)
        b.call(False)                                                   # warm-up: the workspace exists before the capture
        st.synchronize()
        graph = K.Graph().capture(lambda: b.call(False))
        for pts, planes in ((sweep(6000), planes_a), (sweep(65, seed=2), planes_b), (sweep(1025, seed=3), planes_c)):
            b.load(pts, len(pts), planes)
            graph.launch()
            st.synchronize()
            want = crop_model(pts, planes, False)
            assert len(want) > 0
            b.check(want, ("replay", len(pts)))


def test_batch_of_two_with_their_own_planes(dev):
    planes = np.stack([frustum()[0], frustum((370, 1224))[0]])
    clouds = [sweep(6000), sweep(1025, seed=2)]
    dplanes = torch.from_numpy(planes).to(dev)
    raw = torch.zeros(2, CAP_IN, 4, dtype=torch.float32, device=dev)
    out = torch.zeros(2, 2048, 4, dtype=torch.float32, device=dev)
    n_in = torch.tensor([6000, 1025], dtype=torch.int32, device=dev)
    n_out = torch.zeros(2, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    for b in range(2):
        raw[b, :len(clouds[b])].copy_(torch.from_numpy(clouds[b]))
    for b in range(2):                                                  # back to back on one stream, one shared workspace
        K.crop_polytope(raw[b], n_in[b:b + 1], dplanes[b], False, out[b], n_out[b:b + 1], status)
    torch.cuda.synchronize()
    counts = n_out.cpu().numpy()
    for b in range(2):
        want = crop_model(clouds[b], planes[b], False)
        assert counts[b] == len(want) > 0 and out[b, :len(want)].cpu().numpy().tobytes() == want.tobytes(), b
    assert counts[0] != counts[1] and int(status.item()) == 0


def test_wrapper_refuses_wrong_shapes_and_types(dev):
    b = Buffers(dev, 64, 64, 4)
    with pytest.raises(ValueError):
        K.crop_polytope(b.raw, b.n_in, b.planes.float(), False, b.out, b.n_out, b.status)
    with pytest.raises(ValueError):
        K.crop_polytope(b.raw, b.n_in, b.planes[:5], False, b.out, b.n_out, b.status)
    with pytest.raises(ValueError):
        K.crop_polytope(b.raw, b.n_in, b.planes, False, b.out[:, :3].contiguous(), b.n_out, b.status)
    with pytest.raises(ValueError):
        K.crop_polytope(b.raw, b.n_in.long(), b.planes, False, b.out, b.n_out, b.status)
