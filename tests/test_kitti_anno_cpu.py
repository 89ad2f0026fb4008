"""KITTI annotations inside the frame, without a GPU: the per-box arithmetic of csrc/kitti_anno_core.h (compiled for the
host) against kitti_common.kitti_bbox2results, the layout of the version 2 frame record against the library's size
queries, the decoder on hand-built records, result_anno_from_cam against the host annotation, and the ring / input checks
of sassd.stream with calibs.  Inputs, screening and bars: tests/kitti_anno_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest

import sassd  # noqa: F401
from sassd import _C, kitti_common as kc
import kitti_anno_cases as KA

EINVAL, ENOSPC = -1, -2


# ---- 1. the harness against the host ----------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(KA.HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("seed", [0, 1])
def test_core_arithmetic_matches_kitti_bbox2results(seed, tmp_path_factory):
    lib = KA.harness(tmp_path_factory.mktemp("kitti_anno"))
    S = KA.screened(seed)
    boxes = S["boxes"]
    print("seed %d: left out %d of %d; kept %d (clipped %d), dropped %d"
          % (seed, S["left_out"], KA.N_CAND, S["kept"].sum(), S["clipped"].sum(), S["dropped"].sum()))
    assert S["left_out"] <= 0.05 * KA.N_CAND
    assert S["kept"].sum() >= 100 and S["clipped"].sum() >= 10 and S["dropped"].sum() >= 40
    scores = np.linspace(0.99, 0.31, len(boxes)).astype(np.float32)
    labels = (np.arange(len(boxes)) % 3).astype(np.int64)
    cam = KA.harness_cam(lib, boxes, KA.calib_block())
    maxima = {}
    k = KA.compare(cam, boxes, scores, labels, maxima=maxima)
    print("seed %d maxima: %s" % (seed, maxima))
    assert k == S["kept"].sum() and np.array_equal(cam["index"], np.flatnonzero(S["kept"]))
    # the clip really happened and stays inside the image
    assert (cam["bbox"][:, :2] >= 0).all() and (cam["bbox"][:, 2] <= KA.IMG_SHAPE[1]).all() \
        and (cam["bbox"][:, 3] <= KA.IMG_SHAPE[0]).all()
    # the wrap: yaw spans several periods, rotation_y does not
    assert np.abs(boxes[:, 6]).max() > 2 * np.pi and np.abs(cam["rotation_y"]).max() <= np.float32(np.pi)


# ---- 2. layout --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,capD", [(1, 512), (1, 63), (2, 600), (3, 70), (3, 7), (8, 512)])
def test_v2_layout_keeps_v1_and_matches_the_library(B, capD):
    from sassd.stream import record_layout, FRAME_MAGIC_KITTI
    L1, L2 = record_layout(B, capD), record_layout(B, capD, annos=True)
    for key in L1:
        if key != "total":
            assert L2[key] == L1[key], key
    n = B * capD
    lib = _C.lib()
    at = (L1["total"] + 7) // 8 * 8
    assert L2["annos"] == L2["kept"] == at and at % 8 == 0 and at - L1["total"] in (0, 4)
    assert L2["bbox"] % 8 == 0
    assert L2["index"] >= L2["kept"] + 4 * B and L2["cam"] == L2["index"] + 4 * n and L2["alpha"] == L2["cam"] + 28 * n
    assert 0 <= L2["bbox"] - (L2["alpha"] + 4 * n) < 8
    assert L2["total"] == L2["bbox"] + 32 * n
    assert L2["total"] == at + lib.sassd_frame_annos_bytes(B, capD) == lib.sassd_frame_record_kitti_bytes(B, capD)
    assert lib.sassd_frame_record_bytes(B, capD) == L1["total"]
    header = open(os.path.join(KA.ROOT, "include", "sassd.h")).read()
    import re
    assert int(re.search(r"#define\s+SASSD_FRAME_MAGIC_KITTI\s+(0x[0-9a-fA-F]+)", header).group(1), 16) == FRAME_MAGIC_KITTI


def test_annos_abi_refusals():
    lib = _C.lib()
    for B, capD in ((0, 512), (1, 0), (1 << 13, 1 << 13)):
        assert lib.sassd_frame_annos_bytes(B, capD) == 0 and lib.sassd_frame_record_kitti_bytes(B, capD) == 0
    p16, null = C.c_void_p(16), None
    need = lib.sassd_frame_annos_bytes(2, 64)
    f = lib.sassd_frame_annos
    assert f(null, p16, 2, 64, p16, p16, need, null) == EINVAL
    assert f(p16, null, 2, 64, p16, p16, need, null) == EINVAL
    assert f(p16, p16, 2, 64, null, p16, need, null) == EINVAL
    assert f(p16, p16, 2, 64, p16, null, need, null) == EINVAL
    assert f(p16, p16, 0, 64, p16, p16, need, null) == EINVAL
    assert f(p16, p16, 2, 64, C.c_void_p(20), p16, need, null) == EINVAL        # the float64 calibration on 4 bytes
    assert f(p16, p16, 2, 64, p16, C.c_void_p(20), need, null) == EINVAL        # the block's float64 field needs 8
    assert f(p16, p16, 2, 64, p16, p16, need - 1, null) == ENOSPC
    g = lib.sassd_frame_seal_kitti
    need = lib.sassd_frame_record_kitti_bytes(1, 512)
    assert g(p16, p16, p16, p16, 1, 512, p16, p16, null, p16, need, null) == EINVAL
    assert g(p16, p16, p16, p16, 1, 512, p16, p16, p16, null, need, null) == EINVAL
    assert g(p16, p16, p16, p16, 1, 512, p16, p16, p16, C.c_void_p(20), need, null) == EINVAL
    assert g(p16, p16, p16, p16, 1, 512, p16, p16, p16, p16, need - 1, null) == ENOSPC


# ---- 3. the decoder on hand-built v2 records --------------------------------------------------------------------------------
def build_record_v2(B, capD, seq, counts, kept, status=0, magic=None, seed=0):
    """A version 2 record as the frame writes it (numpy model of the contract) + what decode_record must return."""
    from sassd.stream import record_layout, FRAME_MAGIC_KITTI
    L = record_layout(B, capD, annos=True)
    r = np.random.default_rng(seed)
    rec = np.zeros(L["total"], np.uint8)
    w = rec.view(np.int32)
    n = B * capD
    w[0], w[1], w[2], w[3], w[4] = FRAME_MAGIC_KITTI if magic is None else magic, seq, status, B, capD
    w[5:5 + B] = counts
    boxes = rec[L["boxes"]:L["scores"]].view(np.float32).reshape(B, capD, 7)
    scores = rec[L["scores"]:L["labels"]].view(np.float32).reshape(B, capD)
    labels = rec[L["labels"]:L["labels"] + 4 * n].view(np.int32).reshape(B, capD)
    w[L["kept"] // 4:L["kept"] // 4 + B] = kept
    index = rec[L["index"]:L["cam"]].view(np.int32).reshape(B, capD)
    cam = rec[L["cam"]:L["alpha"]].view(np.float32).reshape(B, capD, 7)
    alpha = rec[L["alpha"]:L["alpha"] + 4 * n].view(np.float32).reshape(B, capD)
    bbox = rec[L["bbox"]:L["total"]].view(np.float64).reshape(B, capD, 4)
    want = []
    for b, (k, m) in enumerate(zip(counts, kept)):
        boxes[b, :k] = r.standard_normal((k, 7)).astype(np.float32)
        scores[b, :k] = r.random(k, dtype=np.float32)
        labels[b, :k] = r.integers(0, 3, k)
        index[b, :m] = np.sort(r.choice(k, m, replace=False)) if m else []
        cam[b, :m] = r.standard_normal((m, 7)).astype(np.float32)
        alpha[b, :m] = r.standard_normal(m).astype(np.float32)
        bbox[b, :m] = r.uniform(0, 375, (m, 4))
        if k == 0:
            want.append((None,) * 4)
        else:
            want.append((boxes[b, :k].copy(), scores[b, :k].copy(), labels[b, :k].astype(np.int64),
                         dict(index=index[b, :m].astype(np.int64), location=cam[b, :m, :3].copy(),
                              dimensions=cam[b, :m, 3:6].copy(), rotation_y=cam[b, :m, 6].copy(),
                              alpha=alpha[b, :m].copy(), bbox=bbox[b, :m].copy())))
    return rec, want


CAM_DTYPES = dict(index=np.int64, location=np.float32, dimensions=np.float32, rotation_y=np.float32, alpha=np.float32,
                  bbox=np.float64)


def _same_v2(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == 4
        if w[0] is None:
            assert g == (None, None, None, None)
            continue
        for a, b in zip(g[:3], w[:3]):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
        assert set(g[3]) == set(CAM_DTYPES)
        for key, dt in CAM_DTYPES.items():
            assert g[3][key].dtype == dt and g[3][key].shape == w[3][key].shape and np.array_equal(g[3][key], w[3][key]), key


def test_decoder_v2_counts_zero_all_dropped_and_mixed():
    from sassd.stream import decode_record
    rec, want = build_record_v2(3, 70, 11, [0, 70, 17], [0, 0, 9])
    got = decode_record(rec, 3, 70, 11, annos=True)
    _same_v2(got, want)
    assert got[0] == (None, None, None, None)
    assert got[1][3]["index"].shape == (0,) and got[1][3]["bbox"].shape == (0, 4) and got[1][3]["location"].shape == (0, 3)
    assert len(got[2][3]["index"]) == 9
    got[2][3]["bbox"][:] = -1                          # copies: the pinned buffer is reused by the next frame
    got[2][0][:] = 0
    _same_v2(decode_record(rec, 3, 70, 11, annos=True), want)
    _same_v2(decode_record(rec.tobytes(), 3, 70, 11, annos=True), want)
    rec, want = build_record_v2(1, 63, 12, [63], [63])
    _same_v2(decode_record(rec, 1, 63, 12, annos=True), want)


def test_decoder_v2_rejects_stale_and_foreign_records():
    from sassd.stream import decode_record, FRAME_MAGIC
    rec, _ = build_record_v2(1, 32, 41, [4], [2])
    with pytest.raises(RuntimeError, match="stale frame record"):
        decode_record(rec, 1, 32, 42, annos=True)                  # another seq
    with pytest.raises(RuntimeError, match="stale frame record"):
        decode_record(rec, 1, 32, 41)                              # a v2 record read as v1
    rec, _ = build_record_v2(1, 32, 42, [4], [2], magic=FRAME_MAGIC)
    with pytest.raises(RuntimeError, match="stale frame record"):
        decode_record(rec, 1, 32, 42, annos=True)                  # a v1 magic where v2 is expected
    rec, _ = build_record_v2(2, 16, 42, [1, 1], [1, 0])
    with pytest.raises(RuntimeError, match="stale frame record"):
        decode_record(rec, 1, 32, 42, annos=True)                  # another B
    rec, _ = build_record_v2(1, 32, 42, [4], [2])
    with pytest.raises(RuntimeError, match="stale frame record"):
        decode_record(rec[:-8], 1, 32, 42, annos=True)             # shorter than the record
    with pytest.raises(RuntimeError, match="stale frame record"):
        decode_record(np.zeros_like(rec), 1, 32, 42, annos=True)


def test_decoder_v2_raises_the_status_error():
    from sassd.stream import decode_record, FrameStatusError
    rec, _ = build_record_v2(1, 32, 3, [4], [2], status=_C.ST_BOX_OVERFLOW)
    with pytest.raises(FrameStatusError) as e:
        decode_record(rec, 1, 32, 3, annos=True)
    assert e.value.status == _C.ST_BOX_OVERFLOW


# ---- 4. result_anno_from_cam ------------------------------------------------------------------------------------------------
def test_result_anno_from_cam_equals_the_host_annotation():
    S = KA.screened(0)
    boxes = S["boxes"]
    scores = np.linspace(0.99, 0.31, len(boxes)).astype(np.float32)
    labels = (np.arange(len(boxes)) % 3).astype(np.int64)
    want = kc.kitti_bbox2results(boxes.copy(), scores, labels, KA.meta(sample_idx=31), class_names=KA.CLASS_NAMES)
    # `cam` from the host's own intermediate values
    q = KA.host_quantities(boxes)
    idx = np.flatnonzero(q["keep"]).astype(np.int64)
    cam = dict(index=idx, location=want["location"], dimensions=want["dimensions"], rotation_y=want["rotation_y"],
               alpha=want["alpha"], bbox=want["bbox"])
    got = kc.result_anno_from_cam(cam, scores, labels, 31, KA.CLASS_NAMES)
    assert set(got) == set(want)
    for key in want:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert np.array_equal(got[key], want[key]), key
    empty = kc.empty_result_anno()
    for cam0 in (None, dict(cam, index=idx[:0])):
        got = kc.result_anno_from_cam(cam0, scores, labels, 31, KA.CLASS_NAMES)
        assert set(got) == set(empty)
        for key in empty:
            assert got[key].shape == empty[key].shape and got[key].dtype == empty[key].dtype, key


def test_detector_result_annos_uses_cam_when_it_is_there():
    from sassd import synth
    model, _ = synth.build_detector_for(synth.workload("car"), 0)
    model.class_names = KA.CLASS_NAMES
    S = KA.screened(1)
    boxes = S["boxes"][:40]
    scores = np.linspace(0.9, 0.4, 40).astype(np.float32)
    labels = np.zeros(40, np.int64)
    want = kc.kitti_bbox2results(boxes.copy(), scores, labels, KA.meta(5), class_names=KA.CLASS_NAMES)
    idx = np.flatnonzero(KA.host_quantities(boxes)["keep"]).astype(np.int64)
    cam = dict(index=idx, location=want["location"] + 1, dimensions=want["dimensions"], rotation_y=want["rotation_y"],
               alpha=want["alpha"], bbox=want["bbox"])
    out = model.result_annos([(boxes.copy(), scores, labels, cam), (None, None, None, None)], [KA.meta(5), KA.meta(6)])
    assert np.array_equal(out[0]["location"], want["location"] + 1)        # taken from cam, not recomputed
    assert np.array_equal(out[0]["score"], want["score"]) and len(out[1]["name"]) == 0
    out = model.result_annos([(boxes.copy(), scores, labels)], [KA.meta(5)])   # the 3-tuples keep the host path
    assert np.array_equal(out[0]["location"], want["location"])


# ---- 5. ring and input checks -----------------------------------------------------------------------------------------------
def test_ring_hands_calibs_through_and_omits_them_when_absent():
    from sassd.stream import FrameRing
    import test_frame_stream_cpu as TF
    calls = []

    class Slot(TF.FakeSlot):
        def stage(self, seq, clouds, *args, **kw):
            calls.append((args, kw))
            super().stage(seq, clouds)

    slots = [Slot(i, []) for i in range(2)]
    ring = FrameRing(slots, lambda rec, seq: rec)
    cloud = [np.zeros((3, 4), np.float32)]
    ring.submit(cloud)
    ring.submit(cloud, ["F"])
    ring.submit(cloud, None, ["C"])
    ring.submit(cloud, ["F"], ["C"])
    ring.submit(cloud, calibs=["C"])
    assert calls == [((), {}), ((["F"],), {}), ((), dict(calibs=["C"])), ((["F"],), dict(calibs=["C"])),
                     ((), dict(calibs=["C"]))]
    # the fake slot of the existing tests (stage(seq, clouds) only) keeps working
    ring2, _, _ = TF._ring(2)
    t = ring2.submit(cloud)
    TF._same(ring2.collect(t), TF._expected(3))
    got = list(ring.map([(cloud, None, ["C"])]))
    assert len(got) == 1 and calls[-1] == ((), dict(calibs=["C"]))


def test_check_frame_inputs_with_calibs():
    from sassd.stream import check_frame_inputs, calib_block_of, frustum_of
    cloud = [np.zeros((3, 4), np.float32)]
    cal = dict(calib=KA.calibration(), img_shape=(375, 1242, 3))
    mats = dict(P2=KA.AS.calib_matrices()["P2"], R0_rect=KA.AS.calib_matrices()["R0_rect"],
                Tr_velo_to_cam=KA.AS.calib_matrices()["Tr_velo_to_cam"])
    planes, block = check_frame_inputs(cloud, None, 1, 4, 100, None, [cal], True)
    assert planes is None and block.shape == (1, 36) and block.dtype == np.float64
    c = KA.calibration()
    assert np.array_equal(block[0, :12], c.V2C.ravel()) and np.array_equal(block[0, 12:21], c.R0.ravel())
    assert np.array_equal(block[0, 21:33], c.P2.ravel()) and tuple(block[0, 33:]) == (1242.0, 375.0, 0.0)
    # the dict form, flat rows and 4x4-extended matrices give the same block
    assert np.array_equal(calib_block_of(mats, (375, 1242)), block[0])
    ext = {k: KA.AS.extend(v) for k, v in mats.items()}
    assert np.array_equal(calib_block_of(ext, (375, 1242)), block[0])
    # a raw stream whose frustums are such dicts: calibs defaults to them
    planes, block2 = check_frame_inputs(cloud, [cal], 1, 4, 100, 200, None, True)
    assert np.array_equal(block2, block) and np.array_equal(planes[0], frustum_of(cal["calib"], cal["img_shape"]))
    # without annos nothing changes: the planes alone
    assert check_frame_inputs(cloud, None, 1, 4, 100) is None
    assert check_frame_inputs(cloud, [cal], 1, 4, 100, 200).shape == (1, 6, 4)
    with pytest.raises(ValueError, match="calibs"):
        check_frame_inputs(cloud, None, 1, 4, 100, None, None, True)                   # missing
    with pytest.raises(ValueError, match="calibs"):
        check_frame_inputs(cloud, [frustum_of(c, (375, 1242))], 1, 4, 100, 200, None, True)   # plane arrays: required
    with pytest.raises(ValueError, match="2 calibs"):
        check_frame_inputs(cloud, None, 1, 4, 100, None, [cal, cal], True)             # miscounted
    with pytest.raises(ValueError, match="without annos"):
        check_frame_inputs(cloud, None, 1, 4, 100, None, [cal], False)                 # given to a stream without annos
    bad = dict(mats, P2=np.where(np.arange(12) == 3, np.nan, mats["P2"]))
    with pytest.raises(ValueError, match="finite"):
        check_frame_inputs(cloud, None, 1, 4, 100, None, [dict(calib=bad, img_shape=(375, 1242))], True)
    bad = dict(mats, R0_rect=np.where(np.arange(9) == 0, np.inf, mats["R0_rect"]))
    with pytest.raises(ValueError, match="finite"):
        check_frame_inputs(cloud, None, 1, 4, 100, None, [dict(calib=bad, img_shape=(375, 1242))], True)
    for shape in ((0, 1242), (375, 0), (-1, 5)):
        with pytest.raises(ValueError, match="positive"):
            check_frame_inputs(cloud, None, 1, 4, 100, None, [dict(calib=mats, img_shape=shape)], True)
    with pytest.raises(ValueError, match="img_shape"):
        check_frame_inputs(cloud, None, 1, 4, 100, None, [dict(calib=mats)], True)
    with pytest.raises(ValueError):                                                    # the cloud checks still come first
        check_frame_inputs([np.zeros((101, 4), np.float32)], None, 1, 4, 100, None, [cal], True)


def test_capture_refuses_annos_without_seal_and_single_test_keyword():
    import inspect
    from sassd import runner as R
    from sassd.pipeline import InferencePlan
    assert inspect.signature(R.single_test).parameters["device_annos"].default is False
    assert inspect.signature(InferencePlan.capture).parameters["annos"].default is False
    src = inspect.getsource(InferencePlan.capture)
    assert "annos and not seal" in src
    with pytest.raises(ValueError, match="inflight"):
        import test_runner_cpu as TR
        R.single_test(TR._Model(), TR._DS(2), rank=0, world=1, device_annos=True)
