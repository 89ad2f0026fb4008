"""-m gpu: KITTI annotations inside the captured frame.  The annotation kernel against kitti_common.kitti_bbox2results on
the screened boxes of tests/kitti_anno_cases.py (its bars); FrameStream(annos=True) against the host function applied to
the SAME record's detections (no second stream is compared with frames in flight); the annos frame holds kernel nodes
only; single_test(device_annos=True) against the host path; refusals at submit queue nothing."""
import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import kernels as K, kitti_common as kc
from sassd.pipeline import InferencePlan
from sassd.stream import frustum_of, record_layout, stage_layout
import kitti_anno_cases as KA
import test_gpu_frame_stream as TS
import test_gpu_frame_stream_crop as TC

pytestmark = pytest.mark.gpu


# ---- 1. the kernel against the host -----------------------------------------------------------------------------------------
def _decode_block(raw, B, capD):
    """The annotation block alone (bytes of K.frame_annos) -> per sample (kept, index, cam, alpha, bbox), full capD rows."""
    L = record_layout(B, capD, annos=True)
    off = {k: L[k] - L["annos"] for k in ("kept", "index", "cam", "alpha", "bbox", "total")}
    n = B * capD
    kept = raw[off["kept"]:off["kept"] + 4 * B].view(np.int32)
    index = raw[off["index"]:off["cam"]].view(np.int32).reshape(B, capD)
    cam = raw[off["cam"]:off["alpha"]].view(np.float32).reshape(B, capD, 7)
    alpha = raw[off["alpha"]:off["alpha"] + 4 * n].view(np.float32).reshape(B, capD)
    bbox = raw[off["bbox"]:off["total"]].view(np.float64).reshape(B, capD, 4)
    return kept, index, cam, alpha, bbox


def _pool():
    """Screened boxes of both seeds, and those of them the host drops."""
    boxes, dropped = [], []
    for seed in (0, 1):
        S = KA.screened(seed)
        boxes.append(S["boxes"])
        dropped.append(S["boxes"][S["dropped"]])
    return np.concatenate(boxes), np.concatenate(dropped)


@pytest.mark.parametrize("B,capD,counts,all_dropped", [(1, 64, [37], None), (3, 70, [0, 70, 17], None),
                                                       (2, 600, [605, 259], None), (2, 96, [96, 50], 0)])
def test_annos_kernel_matches_kitti_bbox2results(dev, B, capD, counts, all_dropped):
    pool, dropped = _pool()
    assert len(dropped) >= 96
    r = np.random.default_rng(B * 1000 + capD)
    boxes = np.stack([pool[r.permutation(len(pool))[np.arange(capD) % len(pool)]] for _ in range(B)])    # every row is a real box:
    if all_dropped is not None:                                          # a wrong clamp would annotate the rows past count
        boxes[all_dropped] = dropped[r.permutation(len(dropped))[:capD]]
    boxes = np.ascontiguousarray(boxes, np.float32)
    cnt = np.asarray(counts, np.int32)
    det = dict(boxes=torch.from_numpy(boxes).to(dev), counts=torch.from_numpy(cnt).to(dev))
    calib = torch.from_numpy(np.stack([KA.calib_block()] * B)).to(dev)
    nbytes = K.frame_annos_bytes(B, capD)
    L = record_layout(B, capD, annos=True)
    assert nbytes == L["total"] - L["annos"]
    guard = 64
    buf = torch.full((nbytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)
    out = buf[guard:guard + nbytes]
    K.frame_annos(det, calib, out)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:guard] == 0xA5).all() and (got[guard + nbytes:] == 0xA5).all()      # nothing outside the block
    raw = got[guard:guard + nbytes].copy()
    kept, index, cam, alpha, bbox = _decode_block(raw, B, capD)
    maxima, total = {}, 0
    for b in range(B):
        k = max(0, min(int(cnt[b]), capD))
        m = int(kept[b])
        assert 0 <= m <= k
        scores = np.linspace(0.99, 0.31, capD).astype(np.float32)[:k]
        labels = (np.arange(k) % 3).astype(np.int64)
        c = dict(index=index[b, :m].astype(np.int64), location=cam[b, :m, :3], dimensions=cam[b, :m, 3:6],
                 rotation_y=cam[b, :m, 6], alpha=alpha[b, :m], bbox=bbox[b, :m])
        if k:
            total += KA.compare(c, boxes[b, :k], scores, labels, maxima=maxima)
        else:
            assert m == 0
        # rows at or past kept[b] are zero words
        assert not index[b, m:].any() and not cam[b, m:].view(np.uint32).any() and not alpha[b, m:].view(np.uint32).any()
        assert not bbox[b, m:].view(np.uint64).any()
    if all_dropped is not None:
        assert kept[all_dropped] == 0 and kept[1 - all_dropped] > 0
    print("B %d capD %d counts %s: kept %s, maxima %s" % (B, capD, counts, kept.tolist(), maxima))
    assert total > 0
    # every byte of the block is written, and two launches give identical bytes: a zeroed buffer ends up the same
    zero_fill = torch.zeros_like(buf)
    K.frame_annos(det, calib, zero_fill[guard:guard + nbytes])
    torch.cuda.synchronize()
    again = zero_fill.cpu().numpy()[guard:guard + nbytes]
    assert again.tobytes() == raw.tobytes(), "the block depends on what the buffer held before (or two launches differ)"
    # the inputs are read only
    assert det["boxes"].cpu().numpy().tobytes() == boxes.tobytes() and np.array_equal(det["counts"].cpu().numpy(), cnt)


# ---- 2..5: the stream --------------------------------------------------------------------------------------------------------
N_FRAMES = 4
CAL = dict(calib=KA.calibration(), img_shape=KA.IMG_SHAPE)


def _frames():
    return TS._car_frames()[:N_FRAMES]


def _annos_stream(dev, inflight):
    sd, w, _ = TS._workload(dev)
    return TS._stream(sd, w, dev, inflight, annos=True)


def _check_frame(dets, maxima):
    """One collected frame: the annotation of the record's cam against kitti_bbox2results on the record's own detections."""
    n = 0
    for boxes, scores, labels, cam in dets:
        if boxes is None:
            assert scores is None and labels is None and cam is None
            continue
        n += len(boxes)
        KA.compare(cam, boxes, scores, labels, maxima=maxima)
    return n


@pytest.mark.parametrize("inflight", [1, 3])
def test_stream_record_agrees_with_itself(dev, inflight):
    frames = _frames()
    maxima, n = {}, 0
    with _annos_stream(dev, inflight) as fs:
        assert fs.annos and len(fs.plans) == inflight
        got = [d for _, d in fs.map(([p], None, [CAL]) for p in frames)]
        tickets = [fs.submit([p], calibs=[CAL]) for p in frames]          # and through submit / collect
        got += [fs.collect(t) for t in tickets]
    for d in got:
        n += _check_frame(d, maxima)
    print("inflight %d: %d detections over %d frames, maxima %s" % (inflight, n, len(got), maxima))
    assert n > 0, "the frames detect nothing: the test is empty"
    if inflight == 1:                                                   # alone in flight, the detections are those of a
        sd, w, _ = TS._workload(dev)                                    # stream without annos, byte for byte
        with TS._stream(sd, w, dev, 1) as plain:
            want = [d for _, d in plain.map([p] for p in frames)]
        for i, (g, r) in enumerate(zip(got, want)):
            TS._same_dets([s[:3] for s in g], r, ("annos vs plain", i))


def test_annos_frame_holds_kernel_nodes_only(dev):
    KERNEL, MEMCPY, MEMSET = 0, 1, 2
    sd, w, _ = TS._workload(dev)
    with _annos_stream(dev, 1) as fs:
        plan = fs.plans[0]
        unsealed = InferencePlan(sd, batch_size=1, anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev,
                                 overlap=plan.overlap, **w["plan"])
        with pytest.raises(ValueError, match="seal"):
            unsealed.capture(w["points_cap"], annos=True)
        unsealed.capture(w["points_cap"])
        torch.cuda.synchronize()
        base, got = TS._node_types(unsealed, dev), TS._node_types(plan, dev)
        print("annos frame graph nodes by type:", got, "without seal and annos:", base)
        assert got.get(MEMSET, 0) == 0 and got.get(MEMCPY, 0) == 0 and set(got) == {KERNEL}, got
        assert got[KERNEL] == base[KERNEL] + 2                          # the seal and the annotation kernel
        t = fs.submit([_frames()[0]], calibs=[CAL])                     # the stream still works after the inspection
        assert _check_frame(fs.collect(t), {}) >= 0


def test_full_staging_block_at_batch_2(dev):
    """raw_cap + annos at batch 2: every part of the staging block present, per-sample offsets in play.  Each sample has its
    own sweep and image shape, hence its own planes and calibration block: a swapped or shifted sample index shows."""
    shapes = [(375, 1242), (370, 1224)]
    views = [dict(calib=KA.calibration(), img_shape=s) for s in shapes]
    raws = [TC.raw_sweep(b)[0] for b in range(2)]
    reds = [TC.reduce_on_host(raw, frustum_of(v["calib"], v["img_shape"])) for raw, v in zip(raws, views)]
    assert [len(r) for r in reds] == [14986, 14516] and max(len(r) for r in raws) <= TC.RAW_CAP
    sd, w, _ = TS._workload(dev)
    assert max(len(r) for r in reds) <= w["points_cap"]

    def aliases(plan, L, **parts):
        assert plan._stage_block.dtype == torch.uint8 and plan._stage_block.numel() == L["total"]
        for name, tensor in parts.items():
            assert tensor.data_ptr() == plan._stage_block.data_ptr() + L[name], name

    with TS._stream(sd, w, dev, 1, B=2) as ref:
        want = ref.collect(ref.submit(reds))
        p = ref.plans[0]
        aliases(p, stage_layout(2, seal=True), seq=p._seq, counts=p.npts)
    n_det = sum(len(s[0]) for s in want if s[0] is not None)
    print("batch 2, kept points %s: %d detections" % ([len(r) for r in reds], n_det))
    assert n_det >= 1, "the two sweeps detect nothing: the comparison would be empty"
    with TS._stream(sd, w, dev, 1, B=2, raw_cap=TC.RAW_CAP, annos=True) as fs:
        p = fs.plans[0]
        assert p.raw_cap == TC.RAW_CAP and p.crop_planes.shape == (2, 6, 4) and p.calib.shape == (2, 36)
        aliases(p, stage_layout(2, True, True, True), planes=p.crop_planes, calib=p.calib, seq=p._seq, counts=p.nraw)
        got = fs.collect(fs.submit(raws, views))                        # the frustum dicts serve as calibs too
        assert int(p.status.item()) == 0
    TS._same_dets([s[:3] for s in got], want, "raw + annos at batch 2")
    maxima = {}
    for (boxes, scores, labels, cam), shape in zip(got, shapes):
        if boxes is None:
            assert cam is None
            continue
        KA.compare(cam, boxes, scores, labels, img_shape=shape, maxima=maxima)
    print("maxima", maxima)


def test_single_test_device_annos_equals_the_host_path(dev, tmp_path):
    from sassd import runner as R
    from sassd.config import Config
    from sassd.kitti_dataset import get_dataset
    sd, w, model = TS._workload(dev)
    model = model.to(dev).eval()
    root = str(tmp_path / "kitti")
    frames = TS._car_frames()[:5]
    TS._write_kitti_tree(root, frames)
    c = Config.fromfile(w["cfg"])
    va = dict(c.data.val, root=root + '/training/', ann_file=root + '/ImageSets/val.txt', with_label=False)
    dv = get_dataset(va, device=dev)
    names = c.data.val.class_names
    base = R.single_test(model, dv, class_names=names, rank=0, world=1, inflight=1)
    out = str(tmp_path / "results")
    got = R.single_test(model, dv, class_names=names, rank=0, world=1, inflight=1, device_annos=True, saveto=out)
    assert len(base) == len(got) == len(frames)
    assert sum(len(a["name"]) for a in base) >= 3, "the synthetic split detects almost nothing"
    maxima = {}
    for a, b in zip(base, got):
        KA.compare_annos(b, a, maxima)
    print("single_test device_annos vs host: maxima", maxima)
    back = kc.get_label_annos(out, [i for i, a in enumerate(got) if len(a["name"])])
    assert [len(a["name"]) for a in back] == [len(a["name"]) for a in got if len(a["name"])]
    for a, b in zip(back, [a for a in got if len(a["name"])]):
        assert np.abs(a["bbox"] - b["bbox"]).max() <= 1e-4 and np.abs(a["location"] - b["location"]).max() <= 1e-4


def test_refusals_at_submit_queue_nothing(dev):
    frames = _frames()
    mats = KA.AS.calib_matrices()
    nan = dict(mats, P2=np.where(np.arange(12) == 0, np.nan, mats["P2"]))
    with _annos_stream(dev, 1) as fs:
        t0 = fs.submit([frames[0]], calibs=[CAL])
        fs.drain()                                   # the one slot is free again (its result parked): a submit that
        before = (fs._ring.next_ticket, fs._ring.in_flight())           # queued anything would show as a frame in flight
        for kw in (dict(), dict(calibs=[CAL, CAL]), dict(calibs=[dict(calib=nan, img_shape=KA.IMG_SHAPE)]),
                   dict(calibs=[dict(calib=mats, img_shape=(0, 1242))]), dict(calibs=[dict(calib=mats)])):
            with pytest.raises(ValueError):
                fs.submit([frames[1]], **kw)
            assert (fs._ring.next_ticket, fs._ring.in_flight()) == before, kw
        t1 = fs.submit([frames[1]], calibs=[CAL])
        assert t1 == t0 + 1
        assert _check_frame(fs.collect(t0), {}) >= 0 and _check_frame(fs.collect(t1), {}) >= 0
    sd, w, _ = TS._workload(dev)
    with TS._stream(sd, w, dev, 1) as plain:
        before = (plain._ring.next_ticket, plain._ring.in_flight())
        with pytest.raises(ValueError, match="without annos"):
            plain.submit([frames[0]], calibs=[CAL])
        assert (plain._ring.next_ticket, plain._ring.in_flight()) == before
        assert len(plain.collect(plain.submit([frames[0]]))[0]) == 3
