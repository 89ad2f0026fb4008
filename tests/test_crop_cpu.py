"""The frustum crop without a GPU: geometry.frustum_planes against the chain of calls it wraps, the frustum plumbing of
FrameRing with a fake slot (frustums reach `stage` only when given; every refusal of a raw stream's inputs is a
ValueError with nothing queued), and the C-ABI error convention of the two new entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sassd  # noqa: F401
from sassd import _C, geometry as G, stream as S

import augment_synth as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _calib4():
    c = A.calib_matrices()
    return tuple(A.extend(c[k]) for k in ("R0_rect", "Tr_velo_to_cam", "P2"))


# ---- planes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(375, 1242), (370, 1224)])
def test_frustum_planes_are_the_planes_of_remove_outside_points(shape):
    rect, trv2c, p2 = _calib4()
    planes, f32 = G.frustum_planes(rect, trv2c, p2, shape)
    frustum = G.frustum_in_lidar(rect, trv2c, p2, shape)
    want, want_f32 = G.planes_of_surfaces(G.corner_to_surfaces_3d(frustum[np.newaxis, ...]))
    assert planes.shape == (6, 4) and planes.dtype == np.float64 and f32 is want_f32 is False
    assert planes.tobytes() == want[0].tobytes()
    assert np.isfinite(planes).all() and np.abs(planes[:, :3]).max() > 0


def test_frustum_planes_differ_between_image_shapes():
    rect, trv2c, p2 = _calib4()
    assert not np.array_equal(G.frustum_planes(rect, trv2c, p2, (375, 1242))[0], G.frustum_planes(rect, trv2c, p2, (370, 1224))[0])


def test_frustum_of_takes_a_calibration_object_a_dict_or_flat_rows():
    from sassd.kitti_common import Calibration
    rect, trv2c, p2 = _calib4()
    want = G.frustum_planes(rect, trv2c, p2, (375, 1242))[0]
    mats = A.calib_matrices()
    assert np.array_equal(S.frustum_of(Calibration(matrices=mats), (375, 1242)), want)
    assert np.array_equal(S.frustum_of(mats, (375, 1242, 3)), want)                         # flat rows, (h, w, channels)
    assert np.array_equal(S.frustum_of({"calib/P2": p2, "calib/R0_rect": rect, "calib/Tr_velo_to_cam": trv2c},
                                       np.array([375, 1242], np.int32)), want)              # the 4x4 matrices of a kitti info


# ---- FrameRing --------------------------------------------------------------------------------------------------------------
class FakeSlot:
    """A slot that checks its inputs with the stream's own host-side check, as _PlanSlot.stage does, and records calls."""

    def __init__(self, B=1, ndim=4, points_cap=100, raw_cap=None):
        self.B, self.ndim, self.points_cap, self.raw_cap = B, ndim, points_cap, raw_cap
        self.staged, self.launched, self.planes = [], 0, None

    def stage(self, *args):
        seq, clouds = args[0], args[1]
        frustums = args[2] if len(args) > 2 else None
        self.planes = S.check_frame_inputs(clouds, frustums, self.B, self.ndim, self.points_cap, self.raw_cap)
        self.staged.append(args)

    def launch(self):
        self.launched += 1

    def ready(self):
        return True

    def wait(self):
        pass

    def record(self):
        return self.staged[-1][0]


def _ring(**kw):
    slots = [FakeSlot(**kw) for _ in range(2)]
    return S.FrameRing(slots, lambda rec, seq: ("dets", rec)), slots


def test_ring_hands_frustums_to_stage_only_when_given():
    planes = G.frustum_planes(*_calib4(), (375, 1242))[0]
    cloud = np.zeros((150, 4), np.float32)
    ring, slots = _ring(raw_cap=200)
    t = ring.submit([cloud], [planes])
    assert t == 1 and len(slots[0].staged[0]) == 3 and slots[0].staged[0][2][0] is planes and slots[0].launched == 1
    assert slots[0].planes.shape == (1, 6, 4) and slots[0].planes.tobytes() == planes.tobytes()
    t = ring.submit([cloud], [dict(calib=A.calib_matrices(), img_shape=(375, 1242))])      # through frustum_of
    assert t == 2 and slots[1].planes.tobytes() == planes.tobytes()
    assert ring.collect(1) == ("dets", 1) and ring.collect(2) == ("dets", 2)
    # map: a raw stream's batch is the tuple (clouds, frustums)
    got = list(ring.map(([cloud], [planes]) for _ in range(3)))
    assert [t for t, _ in got] == [3, 4, 5] and all(len(a) == 3 for s in slots for a in s.staged)
    # without frustums the slot is called with two arguments, exactly as before
    ring, slots = _ring()
    assert ring.submit([cloud[:50]]) == 1 and len(slots[0].staged[0]) == 2
    assert [t for t, _ in ring.map([cloud[:50]] for _ in range(2))] == [2, 3]
    assert all(len(a) == 2 for s in slots for a in s.staged)


def test_every_refusal_is_a_value_error_with_nothing_queued():
    planes = G.frustum_planes(*_calib4(), (375, 1242))[0]
    cloud = np.zeros((150, 4), np.float32)
    bad_nan, bad_inf = planes.copy(), planes.copy()
    bad_nan[2, 1], bad_inf[5, 3] = np.nan, np.inf
    ring, slots = _ring(raw_cap=200)
    refused = [
        (([np.zeros((201, 4), np.float32)], [planes]), "201 points.*raw_cap"),              # a cloud above raw_cap
        (([cloud],), "needs one frustum per cloud"),                                         # frustums missing
        (([cloud], [planes, planes]), "2 frustums"),                                         # the wrong number of them
        (([cloud], []), "0 frustums"),
        (([cloud], [planes[:5]]), r"\[6, 4\]"),                                              # not [6,4]
        (([cloud], [planes.T.copy()]), r"\[6, 4\]"),
        (([cloud], [planes.astype(np.float32)]), "float64"),
        (([cloud], [bad_nan]), "finite"),                                                    # not finite
        (([cloud], [bad_inf]), "finite"),
        (([cloud], [dict(calib=A.calib_matrices())]), "img_shape"),
    ]
    for args, pattern in refused:
        with pytest.raises(ValueError, match=pattern):
            ring.submit(*args)
    assert ring.next_ticket == 1 and ring.in_flight() == 0 and not ring.done
    assert all(not s.staged and s.launched == 0 for s in slots)
    assert ring.submit([cloud], [planes]) == 1                                              # the refused frames took no ticket
    # points_cap does not bound a raw stream's clouds; raw_cap does
    assert ring.submit([np.zeros((200, 4), np.float32)], [planes]) == 2
    # frustums given to a stream that has no raw_cap
    ring, slots = _ring()
    with pytest.raises(ValueError, match="without raw_cap"):
        ring.submit([cloud[:50]], [planes])
    with pytest.raises(ValueError, match="101 points.*points_cap"):
        ring.submit([np.zeros((101, 4), np.float32)])
    assert ring.next_ticket == 1 and all(not s.staged and s.launched == 0 for s in slots)


def test_frame_stream_signatures_carry_raw_cap():
    import inspect
    from sassd import runner as R
    from sassd.detector import SingleStageDetector
    from sassd.pipeline import InferencePlan
    assert inspect.signature(S.FrameStream.__init__).parameters["raw_cap"].default is None
    assert inspect.signature(S.FrameStream.submit).parameters["frustums"].default is None
    assert inspect.signature(InferencePlan.capture).parameters["raw_cap"].default is None
    assert inspect.signature(SingleStageDetector.frame_stream).parameters["raw_cap"].default is None
    assert inspect.signature(R.single_test).parameters["raw_prefix"].default is None
    import test_runner_cpu as TR
    with pytest.raises(ValueError, match="raw_prefix needs inflight"):
        R.single_test(TR._Model(), TR._DS(2), rank=0, world=1, raw_prefix="/nowhere")


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_crop_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "sassd.h")).read()
    for name in ("sassd_crop_polytope_dev", "sassd_crop_polytope_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header), "%s is not declared in include/sassd.h" % name
        assert name in _C.EXPORTS, "%s is not bound in _C.py" % name
        assert getattr(C.CDLL(_C.LIB_PATH), name) is not None
    assert int(re.search(r"#define\s+SASSD_ST_POINT_OVERFLOW\s+(\d+)", header).group(1)) == 16 == _C.ST_POINT_OVERFLOW


def test_crop_argument_validation_returns_einval():
    L = _C.lib()
    crop, p16, null = L.sassd_crop_polytope_dev, C.c_void_p(16), None
    need = L.sassd_crop_polytope_workspace_bytes(6144)
    good = [p16, 6144, p16, 4, p16, 0, p16, 1024, p16, p16, p16, need, null]
    for i in (0, 2, 4, 6, 8, 9, 10):                                    # every pointer is required
        args = list(good)
        args[i] = null
        assert crop(*args) == EINVAL, i
    for i, v in ((3, 2), (3, 0), (1, -1), (7, 0), (7, -3), (11, need - 1), (11, 0)):        # ndim, cap_in, cap_out, ws_bytes
        args = list(good)
        args[i] = v
        assert crop(*args) == EINVAL, (i, v)
    args = list(good)
    args[4] = C.c_void_p(20)                                            # planes are float64: 8-byte aligned
    assert crop(*args) == EINVAL


def test_crop_workspace_query():
    L = _C.lib()
    caps = [0, 1, 255, 256, 1023, 1024, 1025, 6144, 122880, 1 << 20, (1 << 24) + 7]
    sizes = [L.sassd_crop_polytope_workspace_bytes(c) for c in caps]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert L.sassd_crop_polytope_workspace_bytes(-5) > 0
    assert sizes[8] >= 4 * (122880 // 1024)                             # at least one count per 1024-row block
