"""-m gpu: the frame seal kernel against a numpy model of its contract, and FrameStream against the eager plan -- bit for bit,
per frame and in order, for 1 / 2 / 3 frames in flight, host and device clouds, batch 8, the bf16 paths, after the host has
recycled device memory; the captured frame holds kernel nodes only; input and status errors stay with their ticket; the
detector and runner wiring give what forward_test / single_test(inflight=0) give.

Equality is the bar everywhere: the stream replays the kernels of the eager plan on the same inputs (the frame graph is
bit-equal to the eager frame, tests/test_gpu_pipeline.py; the bf16 paths are bit-reproducible, tests/test_gpu_bf16_infer.py),
and the seal kernel only copies."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import _C, kernels as K, synth
from sassd.pipeline import InferencePlan
from sassd.stream import FRAME_MAGIC, FrameStream, decode_record, record_layout

pytestmark = pytest.mark.gpu

_MODELS = {}


def _workload(dev, config="car"):
    """The bench.py workload: seeded weights with the classification head calibrated on the HIP pipeline."""
    if config not in _MODELS:
        import bench
        model, w = bench.build_model(0, dev, config)
        _MODELS[config] = ({k: v.clone() for k, v in model.state_dict().items()}, w, model)
    return _MODELS[config]


def _same_dets(got, want, tag):
    assert len(got) == len(want), tag
    for b, (g, w) in enumerate(zip(got, want)):
        if w[0] is None:
            assert g[0] is None and g[1] is None and g[2] is None, (tag, b)
            continue
        assert g[0] is not None, (tag, b)
        for j, (a, r) in enumerate(zip(g, w)):
            assert a.dtype == r.dtype and a.shape == r.shape, (tag, b, j, a.dtype, r.dtype, a.shape, r.shape)
            assert a.tobytes() == r.tobytes(), (tag, b, j)


def _eager(sd, w, dev, batches, overlap, **kw):
    """run_from_points + results(), one batch at a time, on a plan with the stream's `overlap` setting."""
    plan = InferencePlan(sd, batch_size=len(batches[0]), anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev,
                         overlap=overlap, **dict(w["plan"], **kw))
    out = []
    for clouds in batches:
        plan.run_from_points([torch.from_numpy(p).to(dev) for p in clouds])
        out.append(plan.results())
    return out


def _stream(sd, w, dev, inflight, B=1, **kw):
    return FrameStream(sd, inflight=inflight, points_cap=w["points_cap"], batch_size=B, anchors=w["anchors"],
                       anchors_bv=w["anchors_bv"], device=dev, **dict(w["plan"], **kw))


# ---- the seal kernel --------------------------------------------------------------------------------------------------------
def seal_model(boxes, scores, labels, counts, seq, status):
    B, capD = scores.shape
    L = record_layout(B, capD)
    rec = np.zeros(L["total"], np.uint8)
    words = rec.view(np.int32)
    words[0], words[1], words[2], words[3], words[4] = FRAME_MAGIC, seq, status, B, capD
    k = np.clip(counts, 0, capD)
    words[5:5 + B] = k
    live = np.arange(capD)[None, :] < k[:, None]
    rec[L["boxes"]:L["scores"]] = np.where(live[..., None], boxes, np.float32(0)).astype(np.float32).view(np.uint8).reshape(-1)
    rec[L["scores"]:L["labels"]] = np.where(live, scores, np.float32(0)).astype(np.float32).view(np.uint8).reshape(-1)
    rec[L["labels"]:L["total"]] = np.where(live, labels, 0).astype(np.int32).view(np.uint8).reshape(-1)
    return rec


@pytest.mark.parametrize("B,capD,counts", [(1, 512, [37]), (3, 64, [0, 64, 17]), (8, 1024, [1024, 0, 1, 5, 1023, 0, 300, 77]),
                                           (2, 5, [9, -3])])
def test_seal_kernel_matches_the_numpy_model(dev, B, capD, counts):
    r = np.random.default_rng(B * 1000 + capD)
    boxes = r.standard_normal((B, capD, 7)).astype(np.float32)
    boxes.view(np.uint32)[0, 0, :2] = (0x7FC00123, 0x80000000)          # a NaN payload and -0.0: copied as bits
    scores = r.random((B, capD), dtype=np.float32)
    labels = r.integers(-5, 1 << 30, (B, capD)).astype(np.int32)
    cnt = np.asarray(counts, np.int32)
    det = dict(boxes=torch.from_numpy(boxes).to(dev), scores=torch.from_numpy(scores).to(dev),
               labels=torch.from_numpy(labels).to(dev), counts=torch.from_numpy(cnt).to(dev))
    seq = torch.tensor([123456789], dtype=torch.int32, device=dev)
    status = torch.tensor([_C.ST_BOX_OVERFLOW | _C.ST_VOXEL_OVERFLOW], dtype=torch.int32, device=dev)   # a caller-set status word
    nbytes = K.frame_record_bytes(B, capD)
    assert nbytes == record_layout(B, capD)["total"]
    guard = 64
    buf = torch.full((nbytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)      # stale bytes under and around the record
    rec = buf[guard:guard + nbytes]
    K.frame_seal(det, seq, status, rec)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    want = seal_model(boxes, scores, labels, cnt, 123456789, 5)
    assert got[guard:guard + nbytes].tobytes() == want.tobytes()
    assert (got[:guard] == 0xA5).all() and (got[guard + nbytes:] == 0xA5).all()       # nothing outside the record
    # the inputs are read only
    assert det["boxes"].cpu().numpy().tobytes() == boxes.tobytes() and det["scores"].cpu().numpy().tobytes() == scores.tobytes()
    assert np.array_equal(det["labels"].cpu().numpy(), labels) and np.array_equal(det["counts"].cpu().numpy(), cnt)
    assert int(status.item()) == 5 and int(seq.item()) == 123456789
    # tail rows are zero, and the status word reaches the host decoder
    L = record_layout(B, capD)
    sc = want[L["scores"]:L["labels"]].view(np.float32).reshape(B, capD)
    for b in range(B):
        assert not sc[b, max(0, min(int(cnt[b]), capD)):].any()
    with pytest.raises(RuntimeError, match=r"status flags 0x5 \(capacity overflow / hash full\)"):
        decode_record(got[guard:guard + nbytes], B, capD, 123456789)
    status.fill_(0)
    K.frame_seal(det, seq, status, rec)
    torch.cuda.synchronize()
    dets = decode_record(rec.cpu().numpy(), B, capD, 123456789)
    for b in range(B):
        k = max(0, min(int(cnt[b]), capD))
        if k == 0:
            assert dets[b] == (None, None, None)
        else:
            assert dets[b][0].tobytes() == boxes[b, :k].tobytes() and dets[b][1].tobytes() == scores[b, :k].tobytes()
            assert np.array_equal(dets[b][2], labels[b, :k].astype(np.int64))


# ---- bit identity with the eager plan ---------------------------------------------------------------------------------------
N_FRAMES = 24
_REF = {}


def _car_frames():
    return [np.ascontiguousarray(synth.k21(500 + i)) for i in range(N_FRAMES)]


def _car_reference(dev, overlap):
    if overlap not in _REF:
        sd, w, _ = _workload(dev)
        _REF[overlap] = _eager(sd, w, dev, [[p] for p in _car_frames()], overlap)
        assert sum(r[0][0] is not None for r in _REF[overlap]) >= N_FRAMES // 2, "the frames detect almost nothing"
        assert len({r[0][0].tobytes() for r in _REF[overlap] if r[0][0] is not None}) > 1, "the frames are not distinct"
    return _REF[overlap]


@pytest.mark.parametrize("inflight", [1, 2, 3])
def test_stream_equals_the_eager_plan(dev, inflight):
    sd, w, _ = _workload(dev)
    frames = _car_frames()
    want = _car_reference(dev, overlap=inflight == 1)
    with _stream(sd, w, dev, inflight) as fs:
        assert len(fs.plans) == inflight and all(p.overlap == (inflight == 1) for p in fs.plans)
        assert all(p.side is None for p in fs.plans) or inflight == 1            # one stream per plan when frames are in flight
        # host clouds, through map
        got = list(fs.map([p] for p in frames))
        assert [t for t, _ in got] == list(range(1, N_FRAMES + 1))
        for i, (_, d) in enumerate(got):
            _same_dets(d, want[i], ("host clouds", inflight, i))
        # device clouds, through submit / collect with everything queued first
        dev_frames = [torch.from_numpy(p).to(dev) for p in frames]
        tickets = [fs.submit([p]) for p in dev_frames]
        for i, t in enumerate(tickets):
            _same_dets(fs.collect(t), want[i], ("device clouds", inflight, i))
        # CPU tensors are host clouds too
        t = fs.submit([torch.from_numpy(frames[5])])
        _same_dets(fs.collect(t), want[5], ("cpu tensor", inflight))
        for p in fs.plans:
            assert int(p.status.item()) == 0


def test_stream_equals_the_eager_plan_at_batch_8(dev):
    sd, w, _ = _workload(dev, "multi")
    B = 8
    assert w["batch"] == B
    batches = [[np.ascontiguousarray(synth.k21(900 + i * B + j)) for j in range(B)] for i in range(6)]
    want = _eager(sd, w, dev, batches, overlap=False)
    assert sum(s[0] is not None for r in want for s in r) >= 6
    with _stream(sd, w, dev, 3, B=B) as fs:
        got = list(fs.map(batches))
        for i, (_, d) in enumerate(got):
            _same_dets(d, want[i], ("multi host", i))
        got = list(fs.map([torch.from_numpy(p).to(dev) for p in clouds] for clouds in batches))
        for i, (_, d) in enumerate(got):
            _same_dets(d, want[i], ("multi device", i))


def test_stream_equals_the_eager_plan_in_bf16(dev):
    sd, w, _ = _workload(dev)
    frames = _car_frames()[:8]
    kw = dict(precision="bf16", sparse_precision="bf16")
    want = _eager(sd, w, dev, [[p] for p in frames], overlap=False, **kw)
    with _stream(sd, w, dev, 3, **kw) as fs:
        assert all(p.bf16 and p.sparse_bf16 for p in fs.plans)
        for i, (_, d) in enumerate(fs.map([p] for p in frames)):
            _same_dets(d, want[i], ("bf16", i))


# ---- graph contents ---------------------------------------------------------------------------------------------------------
def _node_types(plan, dev):
    """Capture the plan's frame once more into a plain hipGraph and count its nodes by hipGraphNodeType."""
    with open("/proc/self/maps") as f:                                 # the HIP runtime this process already runs on
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert len(paths) == 1, paths
    hip = C.CDLL(paths[0])
    st = torch.cuda.Stream(device=dev)
    graph = C.c_void_p()
    with torch.cuda.stream(st):
        raw = C.c_void_p(_C.stream())
        assert hip.hipStreamBeginCapture(raw, 1) == 0                   # hipStreamCaptureModeThreadLocal, as sassd_graph_begin
        try:
            plan._frame_fn()
        finally:
            rc = hip.hipStreamEndCapture(raw, C.byref(graph))
        assert rc == 0 and graph.value
    n = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and n.value > 0
    nodes = (C.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(graph, nodes, C.byref(n)) == 0
    counts = {}
    for node in nodes:
        t = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(t)) == 0
        counts[t.value] = counts.get(t.value, 0) + 1
    assert hip.hipGraphDestroy(graph) == 0
    return counts


@pytest.mark.parametrize("inflight", [1, 3])
def test_frame_graphs_hold_kernel_nodes_only(dev, inflight):
    KERNEL, MEMCPY, MEMSET = 0, 1, 2                                    # hipGraphNodeTypeKernel / Memcpy / Memset
    sd, w, _ = _workload(dev)
    with _stream(sd, w, dev, inflight) as fs:
        for plan in fs.plans:
            unsealed = InferencePlan(sd, batch_size=1, anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev,
                                     overlap=plan.overlap, **w["plan"])
            unsealed.capture(w["points_cap"])
            torch.cuda.synchronize()
            base, got = _node_types(unsealed, dev), _node_types(plan, dev)
            print("frame graph nodes by type (inflight %d):" % inflight, got, "without the seal:", base)
            assert got.get(MEMSET, 0) == 0 and got.get(MEMCPY, 0) == 0, got
            assert set(got) == {KERNEL}, got
            assert got[KERNEL] == base[KERNEL] + 1                      # the seal is ONE more kernel node
            break                                                       # the plans of a stream are built alike
        # the stream still works after its frame was captured a second time
        t = fs.submit([_car_frames()[0]])
        _same_dets(fs.collect(t), _car_reference(dev, overlap=inflight == 1)[0], "after the inspection")


# ---- recycled memory --------------------------------------------------------------------------------------------------------
def test_passes_are_bit_equal_after_the_host_recycled_memory(dev):
    sd, w, _ = _workload(dev)
    frames = _car_frames()[:9]
    want = _car_reference(dev, overlap=False)
    with _stream(sd, w, dev, 3) as fs:
        first = [d for _, d in fs.map([p] for p in frames)]
        for nbytes in (2 << 20, 8 << 20, 64 << 20, 1 << 30):           # as test_frame_graph_replays_equal_the_eager_frame
            junk = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            junk.fill_(255)
            torch.cuda.synchronize()
            del junk
            again = [d for _, d in fs.map([p] for p in frames)]
            for i in range(len(frames)):
                _same_dets(again[i], first[i], ("second pass", nbytes, i))
                _same_dets(again[i], want[i], ("second pass vs eager", nbytes, i))


# ---- errors stay with their ticket ------------------------------------------------------------------------------------------
def test_oversized_cloud_is_refused_at_submit(dev):
    sd, w, _ = _workload(dev)
    frames = _car_frames()
    want = _car_reference(dev, overlap=False)
    cap = w["points_cap"]
    with _stream(sd, w, dev, 3) as fs:
        a = fs.submit([frames[0]])
        big = np.zeros((cap + 1, 4), np.float32)
        with pytest.raises(ValueError, match="%d points" % (cap + 1)):
            fs.submit([big])
        with pytest.raises(ValueError):
            fs.submit([torch.from_numpy(big).to(dev)])
        with pytest.raises(ValueError):
            fs.submit([frames[0], frames[1]])                           # not a batch of this stream
        b = fs.submit([frames[1]])
        assert b == a + 1                                               # the refused frames took no ticket
        c = fs.submit([np.ascontiguousarray(frames[2][:cap])])
        _same_dets(fs.collect(a), want[0], "before the refusal")
        _same_dets(fs.collect(b), want[1], "after the refusal")
        _same_dets(fs.collect(c), want[2], "after the refusal, next slot")


def test_status_error_is_raised_for_its_ticket_only(dev):
    """No kernel is made to overflow: the test writes the plan's status word itself (a fill on the slot's stream)."""
    sd, w, _ = _workload(dev)
    frames = _car_frames()
    want = _car_reference(dev, overlap=False)
    with _stream(sd, w, dev, 3) as fs:
        slot = fs._slots[1]
        with torch.cuda.stream(slot.stream):
            fs.plans[1].status.fill_(_C.ST_BOX_OVERFLOW)
        ts = [fs.submit([frames[i]]) for i in range(3)]
        _same_dets(fs.collect(ts[0]), want[0], "ticket before")
        with pytest.raises(RuntimeError) as e:
            fs.collect(ts[1])
        assert str(e.value) == "sassd pipeline status flags 0x4 (capacity overflow / hash full)"
        _same_dets(fs.collect(ts[2]), want[2], "ticket after")
        ts = [fs.submit([frames[i]]) for i in range(3, 9)]               # slot 1 is used again: tickets 5 and 8
        for i, t in zip(range(3, 9), ts):
            _same_dets(fs.collect(t), want[i], ("later tickets", i))


# ---- detector and runner ----------------------------------------------------------------------------------------------------
def _forward_test_kwargs(model, w, dev, clouds):
    """model(...) keyword arguments as KittiLiDAR.collate builds them (test mode)."""
    cal = w["cal"]
    an = torch.from_numpy(w["anchors"]).to(dev)
    bv = torch.from_numpy(w["anchors_bv"]).to(dev)
    vs, cr = list(cal["voxel_size"]), list(cal["pc_range"])
    kw = dict(img=None, img_meta=[dict(sample_idx=i) for i in range(len(clouds))], return_loss=False, voxels=[],
              coordinates=[], num_points=[], anchors=[], anchors_mask=[])
    for p in clouds:
        r = K.voxelize(torch.from_numpy(p).to(dev), vs, cr, cal["max_points"], cal["max_voxels"], batch_idx=0, coors_cols=4,
                       want_mean=False)
        m = int(r["voxel_num"].item())
        kw["voxels"].append(r["voxels"][:m]); kw["coordinates"].append(r["coors"][:m, 1:])
        kw["num_points"].append(r["num_points"][:m]); kw["anchors"].append(an)
        zero = torch.zeros(1, dtype=torch.int32, device=dev)
        mask = K.anchor_mask(r["coors"], zero, r["voxel_num"], cal["grid_xyz"][1], cal["grid_xyz"][0], bv, vs, cr, 1)
        kw["anchors_mask"].append(mask.bool())
    return kw


def test_detector_frame_stream_equals_forward_test(dev):
    sd, w, model = _workload(dev)
    model = model.to(dev).eval()
    frames = _car_frames()[:4]
    want = []
    with torch.no_grad():
        for p in frames:
            want += model(**_forward_test_kwargs(model, w, dev, [p]))
    assert sum(r["boxes_lidar"] is not None for r in want) >= 2
    fs = model.frame_stream(w["anchors"], inflight=3, points_cap=w["points_cap"], cap_k=w["plan"]["cap_k"],
                            cap_d=w["plan"]["cap_d"])
    try:
        assert fs.plans[0].score_thr == model.plan(1, torch.from_numpy(w["anchors"]).to(dev), dev).score_thr
        got = [model.result_annos(d, [dict(sample_idx=i)])[0] for i, (_, d) in enumerate(fs.map([p] for p in frames))]
    finally:
        fs.close()
    for i, (g, r) in enumerate(zip(got, want)):
        _same_dets([(g["boxes_lidar"], g["scores"], g["labels"])], [(r["boxes_lidar"], r["scores"], r["labels"])],
                   ("frame_stream vs forward_test", i))


def _write_kitti_tree(root, clouds):
    """A KITTI-layout tree holding `clouds` as velodyne_reduced frames with one calibration; no images (the dataset then
    takes img_scale), no labels (test mode, with_label=False)."""
    import augment_synth as S
    for sub in ("velodyne_reduced", "calib", "label_2"):
        os.makedirs(os.path.join(root, "training", sub), exist_ok=True)
    os.makedirs(os.path.join(root, "ImageSets"), exist_ok=True)
    mats = S.calib_matrices()
    ids = list(range(len(clouds)))
    for i, p in zip(ids, clouds):
        np.ascontiguousarray(p, np.float32).tofile(os.path.join(root, "training", "velodyne_reduced", "%06d.bin" % i))
        with open(os.path.join(root, "training", "calib", "%06d.txt" % i), "w") as f:
            for key in ("P0", "P1", "P2", "P3"):
                f.write("%s: %s\n" % (key, " ".join("%.12e" % v for v in mats["P2"])))
            f.write("R0_rect: %s\n" % " ".join("%.12e" % v for v in mats["R0_rect"]))
            for key in ("Tr_velo_to_cam", "Tr_imu_to_velo"):
                f.write("%s: %s\n" % (key, " ".join("%.12e" % v for v in mats["Tr_velo_to_cam"])))
    with open(os.path.join(root, "ImageSets", "val.txt"), "w") as f:
        f.write("\n".join("%06d" % i for i in ids))
    return ids


def test_single_test_inflight_equals_the_default_path(dev, tmp_path):
    from sassd import runner as R
    from sassd.config import Config
    from sassd.kitti_dataset import get_dataset
    sd, w, model = _workload(dev)
    model = model.to(dev).eval()
    root = str(tmp_path)
    frames = _car_frames()[:7]
    frames[3] = frames[3][:3000]                                        # a small frame between full ones
    _write_kitti_tree(root, frames)
    c = Config.fromfile(w["cfg"])
    va = dict(c.data.val, root=root + '/training/', ann_file=root + '/ImageSets/val.txt', with_label=False)
    dv = get_dataset(va, device=dev)
    assert len(dv) == len(frames) and dv.test_mode
    base = R.single_test(model, dv, class_names=c.data.val.class_names, rank=0, world=1)
    got = R.single_test(model, dv, class_names=c.data.val.class_names, rank=0, world=1, inflight=3)
    assert len(base) == len(got) == len(frames)
    assert sum(len(a["name"]) for a in base) >= 3, "the synthetic split detects almost nothing"
    for i, (a, b) in enumerate(zip(base, got)):
        assert set(a) == set(b), i
        for k in a:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (i, k)
