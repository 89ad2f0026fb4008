"""-m gpu: FrameStream(raw_cap=...) -- raw 360-degree sweeps cropped to the camera frustum inside the captured frame --
against a stream without raw_cap that is fed the same sweeps reduced on the host with numpy.

Equality is the bar: the crop keeps the rows the numpy model keeps, in their order (tests/test_gpu_crop.py), the voxelizer's
result is a function of the rows and their order, and everything behind it replays the same kernels on the same inputs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import _C, synth
from sassd.pipeline import InferencePlan
from sassd.stream import FrameStatusError, FrameStream, frustum_of

import augment_synth as A

pytestmark = pytest.mark.gpu

RAW_CAP, POINTS_CAP = 122880, 16384
IMG_SHAPE = (375, 1242)
_MODELS, _SWEEPS = {}, {}


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
            assert np.array_equal(a, r) and a.tobytes() == r.tobytes(), (tag, b, j)


def _stream(sd, w, dev, inflight, points_cap=POINTS_CAP, raw_cap=None, **kw):
    return FrameStream(sd, inflight=inflight, points_cap=points_cap, batch_size=1, anchors=w["anchors"],
                       anchors_bv=w["anchors_bv"], device=dev, raw_cap=raw_cap, **dict(w["plan"], **kw))


def planes():
    if "planes" not in _SWEEPS:
        _SWEEPS["planes"] = frustum_of(A.calib_matrices(), IMG_SHAPE)
    return _SWEEPS["planes"]


def reduce_on_host(pts, pl):
    """The numpy model of the crop (tests/test_gpu_crop.py): float64, no contraction, boolean index."""
    x, y, z = (pts[:, i].astype(np.float64) for i in range(3))
    out = np.zeros(len(pts), bool)
    for k in range(6):
        out |= ((x * pl[k, 0] + y * pl[k, 1]) + z * pl[k, 2]) + pl[k, 3] >= 0
    return np.ascontiguousarray(pts[~out])


def raw_sweep(seed):
    """A 64-beam sweep all around the sensor, 2083 azimuths: seed 0 -> 121 746 rows, 14 986 of them in the frustum."""
    if seed not in _SWEEPS:
        az = np.deg2rad(np.linspace(-180, 180, 2083, endpoint=False))
        raw = synth._ray_cloud(seed, (2.0, -24.8), az, (5.0, 70.0), 80.0, (-80, -80, -3, 80, 80, 3))
        _SWEEPS[seed] = (raw, reduce_on_host(raw, planes()))
    return _SWEEPS[seed]


def test_the_sweeps_are_the_measured_ones():
    raw, red = raw_sweep(0)
    assert raw.shape == (121746, 4) and len(red) == 14986 and raw.dtype == np.float32
    assert len(raw) <= RAW_CAP and len(red) <= POINTS_CAP


@pytest.mark.parametrize("inflight", [1, 3])
def test_raw_sweeps_detect_what_their_reductions_detect(dev, inflight):
    sd, w, _ = _workload(dev)
    sweeps = [raw_sweep(s) for s in range(4)]
    with _stream(sd, w, dev, inflight) as ref:
        want = [d for _, d in ref.map([red] for _, red in sweeps)]
    n_det = sum(len(d[0][0]) for d in want if d[0][0] is not None)
    print("inflight %d: %d detections in %d frames, kept points %s" % (inflight, n_det, len(sweeps), [len(r) for _, r in sweeps]))
    assert n_det >= 1, "the frames detect nothing: the comparison would be empty"
    with _stream(sd, w, dev, inflight, raw_cap=RAW_CAP) as fs:
        assert fs.raw_cap == RAW_CAP and all(p.raw_cap == RAW_CAP for p in fs.plans)
        got = list(fs.map(([raw], [planes()]) for raw, _ in sweeps))                    # host clouds, plane arrays
        assert [t for t, _ in got] == [1, 2, 3, 4]
        for i, (_, d) in enumerate(got):
            _same_dets(d, want[i], ("raw host", inflight, i))
        assert all(int(p.status.item()) == 0 for p in fs.plans)
        if inflight != 1:               # the other input forms once, on the stream whose frames run alone
            return
        frustum = dict(calib=A.calib_matrices(), img_shape=IMG_SHAPE + (3,))
        tickets = [fs.submit([torch.from_numpy(raw).to(dev)], [frustum]) for raw, _ in sweeps]      # device clouds, calib dicts
        for i, t in enumerate(tickets):
            _same_dets(fs.collect(t), want[i], ("raw device", inflight, i))
        # a smaller sweep after larger ones: no stale rows, counts or planes
        small = np.ascontiguousarray(sweeps[1][0][:30000])
        t = fs.submit([small], [planes()])
        small_red = reduce_on_host(small, planes())
        with _stream(sd, w, dev, inflight) as ref:
            _same_dets(fs.collect(t), ref.collect(ref.submit([small_red])), ("small sweep", inflight))
        for p in fs.plans:                                              # the last frame of each slot: ticket 9, 7 or 8
            assert int(p.status.item()) == 0
            assert int(p.npts[0].item()) in (len(small_red), len(sweeps[2][1]), len(sweeps[3][1]))
        # refusals at submit, nothing queued
        nxt = fs._ring.next_ticket
        with pytest.raises(ValueError, match="raw_cap"):
            fs.submit([np.zeros((RAW_CAP + 1, 4), np.float32)], [planes()])
        with pytest.raises(ValueError, match="frustum"):
            fs.submit([small])
        assert fs._ring.next_ticket == nxt and fs._ring.in_flight() == 0


def test_raw_sweep_in_bf16_dense(dev):
    sd, w, _ = _workload(dev)
    raw, red = raw_sweep(0)
    with _stream(sd, w, dev, 3, precision="bf16") as ref:
        want = ref.collect(ref.submit([red]))
    assert want[0][0] is not None and len(want[0][0]) >= 1
    with _stream(sd, w, dev, 3, raw_cap=RAW_CAP, precision="bf16") as fs:
        assert all(p.bf16 for p in fs.plans)
        _same_dets(fs.collect(fs.submit([raw], [planes()])), want, "bf16 dense")


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


def test_the_cropping_frame_holds_kernel_nodes_only(dev):
    KERNEL, MEMCPY, MEMSET = 0, 1, 2                                    # hipGraphNodeTypeKernel / Memcpy / Memset
    sd, w, _ = _workload(dev)
    kw = dict(batch_size=1, anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev, overlap=False, **w["plan"])
    plain, cropping = InferencePlan(sd, **kw), InferencePlan(sd, **kw)
    plain.capture(POINTS_CAP, seal=True)
    cropping.capture(POINTS_CAP, seal=True, raw_cap=RAW_CAP)
    torch.cuda.synchronize()
    base, got = _node_types(plain, dev), _node_types(cropping, dev)
    print("frame graph kernel nodes: %d without raw_cap, %d with raw_cap (by type: %s / %s)"
          % (base.get(KERNEL, 0), got.get(KERNEL, 0), base, got))
    for counts in (base, got):
        assert counts.get(MEMSET, 0) == 0 and counts.get(MEMCPY, 0) == 0, counts
        assert set(counts) == {KERNEL}, counts
    assert got[KERNEL] > base[KERNEL]                                   # the crop is in the frame (the count is not pinned)


# ---- overflow ---------------------------------------------------------------------------------------------------------------
def test_point_overflow_belongs_to_its_ticket(dev):
    sd, w, _ = _workload(dev)
    raw, red = raw_sweep(0)
    small_raw = np.ascontiguousarray(raw[:30000])
    small_red = reduce_on_host(small_raw, planes())
    cap = 8192
    assert len(small_red) <= cap < len(red)
    with _stream(sd, w, dev, 3, points_cap=cap) as ref:
        want = ref.collect(ref.submit([small_red]))
    with _stream(sd, w, dev, 3, points_cap=cap, raw_cap=RAW_CAP) as fs:
        a = fs.submit([raw], [planes()])                                # slot 0: keeps 14 986 > 8 192 points
        b = fs.submit([small_raw], [planes()])                          # slot 1: fits
        with pytest.raises(FrameStatusError) as e:
            fs.collect(a)
        assert e.value.status & _C.ST_POINT_OVERFLOW, hex(e.value.status)
        _same_dets(fs.collect(b), want, "the next ticket")
        c = fs.submit([small_raw], [planes()])                          # slot 2
        d = fs.submit([small_raw], [planes()])                          # slot 0 again: recover() cleared its flag
        _same_dets(fs.collect(c), want, "slot 2")
        _same_dets(fs.collect(d), want, "slot 0 after recover()")
        assert all(int(p.status.item()) == 0 for p in fs.plans)


# ---- runner -----------------------------------------------------------------------------------------------------------------
def _write_kitti_tree(root, sweeps):
    """A KITTI-layout tree: raw sweeps under velodyne/, their reductions (as create_data writes them) under
    velodyne_reduced/, one calibration; no images (the dataset then takes img_scale = 1242 x 375), no labels."""
    from sassd.kitti_common import Calibration
    for sub in ("velodyne", "velodyne_reduced", "calib", "label_2"):
        os.makedirs(os.path.join(root, "training", sub), exist_ok=True)
    os.makedirs(os.path.join(root, "ImageSets"), exist_ok=True)
    mats = A.calib_matrices()
    for i, raw in enumerate(sweeps):
        path = os.path.join(root, "training", "calib", "%06d.txt" % i)
        with open(path, "w") as f:
            for key in ("P0", "P1", "P2", "P3"):
                f.write("%s: %s\n" % (key, " ".join("%.12e" % v for v in mats["P2"])))
            f.write("R0_rect: %s\n" % " ".join("%.12e" % v for v in mats["R0_rect"]))
            for key in ("Tr_velo_to_cam", "Tr_imu_to_velo"):
                f.write("%s: %s\n" % (key, " ".join("%.12e" % v for v in mats["Tr_velo_to_cam"])))
        red = reduce_on_host(raw, frustum_of(Calibration(path), IMG_SHAPE))
        raw.tofile(os.path.join(root, "training", "velodyne", "%06d.bin" % i))
        red.tofile(os.path.join(root, "training", "velodyne_reduced", "%06d.bin" % i))
    with open(os.path.join(root, "ImageSets", "val.txt"), "w") as f:
        f.write("\n".join("%06d" % i for i in range(len(sweeps))))


def test_single_test_on_raw_sweeps_equals_the_reduced_files(dev, tmp_path):
    from sassd import runner as R
    from sassd.config import Config
    from sassd.kitti_dataset import get_dataset
    sd, w, model = _workload(dev)
    model = model.to(dev).eval()
    root = str(tmp_path)
    sweeps = [raw_sweep(0)[0], np.ascontiguousarray(raw_sweep(1)[0][:40000]), raw_sweep(2)[0]]
    _write_kitti_tree(root, sweeps)
    c = Config.fromfile(w["cfg"])
    va = dict(c.data.val, root=root + '/training/', ann_file=root + '/ImageSets/val.txt', with_label=False)
    dv = get_dataset(va, device=dev)
    assert len(dv) == 3 and dv.test_mode
    base = R.single_test(model, dv, class_names=c.data.val.class_names, rank=0, world=1, inflight=3)
    got = R.single_test(model, dv, class_names=c.data.val.class_names, rank=0, world=1, inflight=3,
                        raw_prefix=os.path.join(root, "training", "velodyne"))      # points_cap defaults to raw_cap
    assert len(base) == len(got) == 3
    assert sum(len(a["name"]) for a in base) >= 1, "the synthetic split detects nothing"
    for i, (a, b) in enumerate(zip(base, got)):
        assert set(a) == set(b), i
        for k in a:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (i, k)
