"""Test-time augmentation without a GPU: the view spec and where a bad one is refused, the error codes of the two entry points,
the numpy statement (sassd.tta.views_host / pool_host) against a CPU loop over the very headers the kernels include
(tests/tta_harness.hip) -- bit for bit --, the flip's inverse in closed form, and the sizes of the user-facing blocks of a plan
whose inner batch is b * V.  The kernels themselves: tests/test_gpu_tta_kernels.py; the frame: tests/test_gpu_tta.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import _C, tta as T
from sassd.pipeline import INPUT_WEIGHT_KEY, InferencePlan
from sassd.stream import FrameStream, decode_record, record_layout, stage_layout, stage_views

import tta_cases as TC

EINVAL, ENOSPC = -1, -2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return TC.harness(tmp_path_factory.mktemp("tta_harness"))


# ---- the spec ---------------------------------------------------------------------------------------------------------------
BAD_SPECS = [
    ([(1, 0.0, 1.0)], "identity"),                                  # the first view is not the identity
    ([(0, 0.1, 1.0), TC.ID], "identity"),
    ([TC.ID] * 9, r"1\.\.8 views"),                                 # nine views
    ([], r"1\.\.8 views"),
    ([TC.ID, (0, 0.0, 0.0)], "scale"),                              # scale <= 0
    ([TC.ID, (0, 0.0, -1.0)], "scale"),
    ([TC.ID, (0, 0.0, float("inf"))], "scale"),
    ([TC.ID, (0, float("nan"), 1.0)], "angle"),                     # an angle that is not finite
    ([TC.ID, (0, float("inf"), 1.0)], "angle"),
    ([TC.ID, (2, 0.0, 1.0)], "flip 0 / 1"),
    ([TC.ID, (0, 0.0)], "flip 0 / 1"),                              # malformed
    ("flip", "list"),
    (3, "list"),
]


@pytest.mark.parametrize("spec,what", BAD_SPECS)
def test_a_bad_spec_is_refused_everywhere_before_anything_is_allocated(spec, what):
    with pytest.raises(ValueError, match=what):
        T.check_views(spec)
    with pytest.raises(ValueError, match=what):                     # no state dict, no device: nothing was touched yet
        InferencePlan({}, batch_size=1, device="cuda:0", tta=spec)
    sd = {INPUT_WEIGHT_KEY: torch.zeros(3, 3, 3, 4, 16)}
    with pytest.raises(ValueError, match=what):
        FrameStream(sd, inflight=2, points_cap=1024, batch_size=1, device="cuda:0", tta=spec)


def test_a_good_spec_and_its_rounding():
    v = T.check_views([(False, 0, 1), (True, np.float32(0.5), 2)])
    assert v == ((0, 0.0, 1.0), (1, 0.5, 2.0))
    p = T.view_params(TC.V4)
    assert p["flip"].dtype == np.int32 and all(p[k].dtype == np.float32 for k in ("sin", "cos", "scale", "angle"))
    assert p["sin"][0] == 0 and p["cos"][0] == 1 and p["scale"][0] == 1 and p["angle"][0] == 0
    assert p["sin"][2] == np.float32(np.sin(np.pi / 8)) and p["cos"][3] == np.float32(np.cos(-np.pi / 8))   # PointAugmentor._global
    assert p["angle"][3] == np.float32(-np.pi / 8)


def test_an_inner_batch_the_plan_cannot_build_is_refused():
    # 40 x 1600 x 1408 voxels: 48 samples reach the 32-bit linear index (lin_fits of csrc/rulebook.hip)
    with pytest.raises(ValueError, match="inner batch of 48"):
        InferencePlan({}, batch_size=6, device="cuda:0", tta=[TC.ID] * 8)
    with pytest.raises(ValueError, match="inner batch"):
        InferencePlan({}, batch_size=0, device="cuda:0", tta=TC.V2)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def _host(views):
    p = T.view_params(views)
    return p, [p[k].ctypes.data for k in ("flip", "sin", "cos", "scale")]


def test_views_entry_point_error_codes():
    L = _C.lib()
    p16, null = C.c_void_p(16), None
    p, h = _host(TC.V3)
    dst = (C.c_void_p * 7)(*[32 + 16 * i for i in range(7)])
    cnt = (C.c_void_p * 7)(*[1024 + 16 * i for i in range(7)])
    d, c = C.addressof(dst), C.addressof(cnt)
    call = lambda src=p16, cap=64, n=p16, ndim=4, V=3, h=h, d=d, c=c, cap_dst=64: L.sassd_tta_views_dev(  # noqa: E731
        src, cap, n, ndim, V, *h, d, c, cap_dst, null)
    assert call(V=0) == EINVAL and call(V=9) == EINVAL
    assert call(ndim=2) == EINVAL and call(cap=0) == EINVAL
    assert call(src=null) == EINVAL and call(n=null) == EINVAL and call(d=null) == EINVAL and call(c=null) == EINVAL
    assert call(h=[null] + h[1:]) == EINVAL and call(h=h[:3] + [null]) == EINVAL
    assert call(src=C.c_void_p(18)) == EINVAL                                   # misaligned
    bad = (C.c_void_p * 7)(32, 0, 0, 0, 0, 0, 0)                                # a NULL destination among the V - 1
    assert call(d=C.addressof(bad)) == EINVAL
    alias = (C.c_void_p * 7)(32, 16, 0, 0, 0, 0, 0)                             # a destination that is the source
    assert call(d=C.addressof(alias)) == EINVAL
    _, hbad = _host(TC.V3)
    q = T.view_params(TC.V3)
    q["flip"][0] = 1                                                            # view 0 is not the identity
    assert call(h=[q["flip"].ctypes.data] + hbad[1:]) == EINVAL
    q = T.view_params(TC.V3)
    q["scale"][2] = 0.0
    assert call(h=hbad[:3] + [q["scale"].ctypes.data]) == EINVAL
    assert call(cap_dst=63) == ENOSPC                                           # a destination shorter than the source
    # V == 1: nothing to write, nothing launched -- no device needed, no destination either
    p1, h1 = _host(TC.V1)
    assert L.sassd_tta_views_dev(p16, 64, p16, 4, 1, *h1, null, null, 0, null) == 0
    del p, p1


def test_pool_entry_point_error_codes():
    L = _C.lib()
    p16, null = C.c_void_p(16), None
    p, h = _host(TC.V3)
    ang = p["angle"].ctypes.data
    ptrs = [p16] * 4
    outs = [p16] * 4

    def call(ptrs=ptrs, batch=2, V=3, capK=8, h=h, ang=ang, outs=outs, capP=24, status=p16):
        return L.sassd_tta_pool(*ptrs, batch, V, capK, *h, ang, *outs, capP, status, null)
    assert call(V=0) == EINVAL and call(V=9) == EINVAL
    assert call(batch=0) == EINVAL and call(capK=0) == EINVAL and call(capP=0) == EINVAL
    assert call(capP=4097) == EINVAL                                            # more than sassd_rescore_nms takes
    for i in range(4):
        assert call(ptrs=ptrs[:i] + [null] + ptrs[i + 1:]) == EINVAL
        assert call(outs=outs[:i] + [null] + outs[i + 1:]) == EINVAL
    assert call(status=null) == EINVAL and call(ang=null) == EINVAL and call(h=[null] + h[1:]) == EINVAL
    assert call(ptrs=[C.c_void_p(18)] + ptrs[1:]) == EINVAL
    q = T.view_params(TC.V3)
    q["angle"][1] = np.float32("nan")
    assert call(ang=q["angle"].ctypes.data) == EINVAL
    q = T.view_params(TC.V3)
    q["cos"][0] = 0.5                                                           # view 0 is not the identity
    assert call(h=h[:2] + [q["cos"].ctypes.data] + h[3:]) == EINVAL
    assert call(capP=7) == ENOSPC                                               # the pool cannot hold the identity view whole


def test_the_wrappers_exist_and_refuse_bad_shapes_on_the_host():
    from sassd import kernels as K
    with pytest.raises(ValueError, match="identity"):
        K.tta_views(torch.zeros(4, 4), torch.zeros(1, dtype=torch.int32), [(1, 0.0, 1.0)], [], [])
    with pytest.raises(ValueError, match="identity"):
        K.tta_pool(torch.zeros(2, 8, 7), torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.int32),
                   torch.zeros(2, dtype=torch.int32), [(0, 0.1, 1.0)], 16)


# ---- the numpy statement against the shared headers ---------------------------------------------------------------------
@pytest.mark.parametrize("ndim", [3, 4, 5, 8])
@pytest.mark.parametrize("views", [TC.V2, TC.V3, TC.V4, TC.V4_MIXED], ids=["V2", "V3", "V4", "V4mixed"])
def test_views_host_is_the_header_loop_bit_for_bit(lib, ndim, views):
    for n in (0, 1, 257, 5000):
        pts = TC.cloud(n, ndim, 10 * ndim + n)
        got, want = T.views_host(pts, views), TC.harness_views(lib, pts, views)
        assert len(got) == len(views) == len(want)
        assert TC.same_bits(got[0], pts)                                        # the identity view: the rows, untouched
        for v, (g, w) in enumerate(zip(got, want)):
            assert TC.same_bits(g, w), (n, v)
            assert TC.same_bits(g[:, 3:], pts[:, 3:]), (n, v)                   # further columns: copied as bits
        if n > 3 and ndim > 3:
            assert got[1].view(np.uint32)[2, 3] == TC.NAN_PAYLOAD and got[1].view(np.uint32)[1, 2] == TC.INF


def test_the_flip_view_is_y_negated_and_nothing_else():
    pts = TC.cloud(300, 4, 1)
    flipped = T.views_host(pts, TC.V2)[1]
    want = pts.copy()
    want[:, 1] = -pts[:, 1]
    keep = pts[:, 0] != 0                                                       # (x * 1 + (-y) * 0 turns -0.0 into +0.0)
    assert TC.same_bits(flipped[keep], want[keep])


@pytest.mark.parametrize("views", [TC.V2, TC.V3, TC.V4_MIXED], ids=["V2", "V3", "V4mixed"])
def test_unview_boxes_is_the_header_loop_bit_for_bit(lib, views):
    g, _, _, _ = TC.candidates(1, 1, 4000, [4000], 7)
    p = T.view_params(views)
    for v in range(1, len(views)):
        got = T.unview_boxes(g[0], p["flip"][v], p["sin"][v], p["cos"][v], p["scale"][v], p["angle"][v])
        assert TC.same_bits(got, TC.harness_unview(lib, g[0], views, v)), v


def test_a_flipped_box_maps_back_exactly(lib):
    r = np.random.default_rng(3)
    box = (r.standard_normal((500, 7)) * [20, 15, 1, 0.3, 0.6, 0.2, 1.5] + [35, 0, -1, 1.6, 3.9, 1.56, 0]).astype(np.float32)
    seen = box.copy()                                                           # the box as the flipped cloud shows it:
    seen[:, 1] = -box[:, 1]                                                     # (x, -y, z, w, l, h, y')
    want = box.copy()
    want[:, 6] = -seen[:, 6] + np.float32(np.pi)                                # (x, y, z, w, l, h, -y' + pi)
    p = T.view_params(TC.V2)
    got = T.unview_boxes(seen, p["flip"][1], p["sin"][1], p["cos"][1], p["scale"][1], p["angle"][1])
    assert TC.same_bits(got, want)
    assert TC.same_bits(TC.harness_unview(lib, seen, TC.V2, 1), want)


def test_the_inverse_undoes_the_forward_view_to_rounding():
    """Not a bit test: (rotate, scale, flip) and back is the identity up to float32 rounding of coordinates of ~70 m."""
    r = np.random.default_rng(5)
    ctr = (r.standard_normal((200, 4)) * [20, 15, 1, 1]).astype(np.float32)
    p = T.view_params(TC.V4_MIXED)
    for v in range(1, 4):
        seen = T.views_host(ctr, TC.V4_MIXED)[v]
        box = np.concatenate([seen[:, :3], np.ones((200, 4), np.float32)], 1)
        back = T.unview_boxes(box, p["flip"][v], p["sin"][v], p["cos"][v], p["scale"][v], p["angle"][v])
        assert np.abs(back[:, :3] - ctr[:, :3]).max() < 2e-5 * 70


CASE_COUNTS = [0, 8, 11, 3, 0, 8]                                               # b = 2, V = 3, capK = 8: 0, 8 and 11 (clamped)


def test_pool_host_is_the_header_walk_bit_for_bit(lib):
    g, lo, la, cnt = TC.candidates(2, 3, 8, CASE_COUNTS, 11)
    for cap, over in ((24, False), (16, False), (12, True), (8, True)):
        got, want = T.pool_host(g, lo, la, cnt, TC.V3, cap), TC.harness_pool(lib, g, lo, la, cnt, TC.V3, cap)
        for k in ("guided", "logits", "labels", "counts"):
            assert TC.same_bits(got[k], want[k]), (cap, k)
        assert got["overflow"] == want["overflow"] == over
        assert list(got["counts"]) == [min(16, cap), min(11, cap)]
    full = T.pool_host(g, lo, la, cnt, TC.V3, 24)
    # view-major, each view's rows in their order: sample 0 is 8 rows of view 1, then 8 of view 2 (11 clamped to capK)
    assert TC.same_bits(full["logits"][0, :8], lo[1, :8]) and TC.same_bits(full["logits"][0, 8:16], lo[2, :8])
    assert TC.same_bits(full["guided"][1, :3], g[3, :3])                        # the identity view: bits
    assert TC.same_bits(full["labels"][1, 3:11], la[5, :8]) and not full["guided"][1, 11:].any()
    cut = T.pool_host(g, lo, la, cnt, TC.V3, 12)                                # the prefix of the full pool
    assert TC.same_bits(cut["guided"][0], full["guided"][0, :12]) and TC.same_bits(cut["guided"][1, :11], full["guided"][1, :11])


# ---- the user-facing blocks of a plan whose inner batch is b * V ----------------------------------------------------------
@pytest.mark.parametrize("b,V", [(1, 4), (2, 3), (8, 2)])
def test_stage_and_record_layouts_are_those_of_b_samples(b, V):
    L = _C.lib()
    capD = 512
    R = record_layout(b, capD)
    assert R["total"] == L.sassd_frame_record_bytes(b, capD) < L.sassd_frame_record_bytes(b * V, capD)
    assert record_layout(b, capD, annos=True)["total"] == L.sassd_frame_record_kitti_bytes(b, capD)
    S = stage_layout(b, raw=True, annos=True, seal=True)
    assert S["total"] == 8 * 24 * b + 8 * 36 * b + 4 + 4 * b                    # planes, calib, seq, counts: per cloud, not per view
    views = stage_views(np.zeros(S["total"], np.uint8), b, S)
    assert views["counts"].shape == (b,) and views["planes"].shape == (b, 6, 4) and views["calib"].shape == (b, 36)
    assert stage_layout(b, seal=True, sweeps=3)["total"] == 8 * 12 * 3 * b + 4 + 4 * b + 16 * b * 3
    # a b-sample record decodes as b result sets; a decoder told b * V samples refuses it
    rec = np.zeros(R["total"], np.uint8)
    rec.view(np.int32)[:5] = (0x53460001, 9, 0, b, capD)
    assert decode_record(rec, b, capD, 9) == [(None, None, None)] * b
    with pytest.raises(RuntimeError, match="stale"):
        decode_record(np.zeros(record_layout(b * V, capD)["total"], np.uint8), b * V, capD, 9)
