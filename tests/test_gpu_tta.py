"""-m gpu: test-time augmentation inside the frame -- InferencePlan(tta=...) and FrameStream(tta=...) on bench.py's car workload,
batch 1 -- against a HOST STATEMENT made of parts that are each tested on their own: a plain batch-V plan run on the numpy views
of the cloud (sassd.tta.views_host), its candidate buffers pooled in numpy (sassd.tta.pool_host), and sassd_rescore_nms at
batch 1 on the pool.

Equality of bytes is the bar: the two new kernels only copy and apply the stated float32 arithmetic
(tests/test_gpu_tta_kernels.py), and everything else is the kernels of the plain plan on the same inputs.

Frames: the 4 seeded car frames, synth.k21(0..3) (the workload's frame(i)).  Views: V2 = identity + flip; V4 = identity + flip +
rotations of +-pi/8.  The conditions that keep the comparison from passing vacuously are asserted on the host statement."""
import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import kernels as K, tta as T
from sassd.pipeline import InferencePlan
from sassd.stream import FrameStream, calib_block_of, decode_record, merge_sweeps_host, sweep_transform

import tta_cases as TC
import test_gpu_frame_stream as TS
import test_gpu_frame_stream_crop as CROP
import augment_synth as A

pytestmark = pytest.mark.gpu

VIEWS = dict(V2=TC.V2, V4=TC.V4)
_STATEMENT, _PLAIN = {}, {}


def _frames(w):
    return [np.ascontiguousarray(w["frame"](i)) for i in range(4)]


def _plan(sd, w, dev, batch_size=1, **kw):
    return InferencePlan(sd, batch_size=batch_size, anchors=w["anchors"], anchors_bv=w["anchors_bv"], device=dev,
                         **dict(w["plan"], **kw))


def _plain(dev):
    """The plain batch-1 plan's detections on the 4 frames."""
    if not _PLAIN:
        sd, w, _ = TS._workload(dev)
        plan = _plan(sd, w, dev)
        out = []
        for p in _frames(w):
            plan.run_from_points([torch.from_numpy(p).to(dev)])
            out.append(plan.results())
        _PLAIN["dets"] = out
    return _PLAIN["dets"]


def host_statement(dev, clouds, views, overlap=True):
    """clouds (numpy, one per frame) -> per frame (results, pooled count, identity view's count): a plain batch-V plan on
    views_host clouds, pool_host on its candidate buffers, rescore / NMS at batch 1."""
    sd, w, _ = TS._workload(dev)
    V = len(views)
    plain = _plan(sd, w, dev, batch_size=V, overlap=overlap)
    assert plain.tta is None and plain.B == plain.b_user == V
    cap_p = min(V * plain.capK, 4096)
    out = []
    for pts in clouds:
        plain.run_from_points([torch.from_numpy(v).to(dev) for v in T.views_host(pts, views)])
        torch.cuda.synchronize()
        assert int(plain.status.item()) == 0
        df = {k: v.cpu().numpy() for k, v in plain.df.items()}
        pool = T.pool_host(df["guided"], plain.logits.cpu().numpy(), df["labels"], df["counts"], views, cap_p)
        assert not pool["overflow"]
        det = K.rescore_nms(*[torch.from_numpy(pool[k]).to(dev) for k in ("guided", "logits", "labels", "counts")],
                            plain.score_thr, plain.iou_thr, plain.capD)
        torch.cuda.synchronize()
        k = int(det["counts"][0].item())
        res = (None, None, None) if k == 0 else (det["boxes"][0, :k].cpu().numpy(), det["scores"][0, :k].cpu().numpy(),
                                                 det["labels"][0, :k].cpu().numpy().astype(np.int64))
        out.append(([res], int(pool["counts"][0]), int(min(df["counts"][0], plain.capK))))
    return out


def _statement(dev, name):
    if name not in _STATEMENT:
        _, w, _ = TS._workload(dev)
        _STATEMENT[name] = host_statement(dev, _frames(w), VIEWS[name])
    return _STATEMENT[name]


def _differs(a, b):
    if a[0] is None or b[0] is None:
        return (a[0] is None) != (b[0] is None)
    return a[0].shape != b[0].shape or a[0].tobytes() != b[0].tobytes() or a[1].tobytes() != b[1].tobytes()


# ---- 1: the identity spec is the plain plan -----------------------------------------------------------------------------
def test_identity_spec_gives_the_plain_detections(dev):
    sd, w, _ = TS._workload(dev)
    plan = _plan(sd, w, dev, tta=[TC.ID])
    assert plan.tta == (TC.ID,) and plan.V == 1 and plan.B == plan.b_user == 1 and plan.capP == plan.capK
    for i, p in enumerate(_frames(w)):
        plan.run_from_points([torch.from_numpy(p).to(dev)])
        TS._same_dets(plan.results(), _plain(dev)[i], ("identity spec", i))
    assert sum(r[0][0] is not None for r in _plain(dev)) == 4


# ---- 2: the tta plan is the host statement ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["V2", "V4"])
def test_tta_plan_equals_the_host_statement(dev, name):
    sd, w, _ = TS._workload(dev)
    views = VIEWS[name]
    want = _statement(dev, name)
    # the comparison is not empty: asserted on the statement, i.e. on the plain plan
    differ = 0
    for i, (res, pooled, own) in enumerate(want):
        print("%s frame %d: identity view %d candidates, pool %d, %d detections (plain plan: %d)"
              % (name, i, own, pooled, 0 if res[0][0] is None else len(res[0][0]),
                 0 if _plain(dev)[i][0][0] is None else len(_plain(dev)[i][0][0])))
        assert pooled > own, (name, i, "the other views add no candidate")
        assert res[0][0] is not None and len(res[0][0]) >= 1, (name, i, "no detection")
        differ += _differs(res[0], _plain(dev)[i][0])
    assert differ >= 1, "pooled detections equal the plain plan's on every frame: the views change nothing"
    plan = _plan(sd, w, dev, tta=views)
    V = len(views)
    assert plan.b_user == 1 and plan.B == V and plan.df["guided"].shape[0] == V and plan.det["boxes"].shape[0] == 1
    assert plan.capP == min(V * plan.capK, 4096) and plan.pool["guided"].shape == (1, plan.capP, 7)
    for i, p in enumerate(_frames(w)):
        plan.run_from_points([torch.from_numpy(p).to(dev)])
        got = plan.results()
        assert len(got) == 1
        TS._same_dets(got, want[i][0], (name, "eager", i))
        assert int(plan.pool["counts"][0].item()) == want[i][1]
    with pytest.raises(RuntimeError, match="no voxel entry"):
        plan.run_from_voxels(torch.zeros(1, 4, device=dev), torch.zeros(1, 4, dtype=torch.int32, device=dev))


# ---- 3: the captured frame ------------------------------------------------------------------------------------------------
def test_captured_frame_replays_the_eager_result_and_holds_kernel_nodes_only(dev):
    KERNEL = 0                                                          # hipGraphNodeTypeKernel
    sd, w, _ = TS._workload(dev)
    want = _statement(dev, "V4")
    plan = _plan(sd, w, dev, tta=TC.V4)
    plan.capture(w["points_cap"])
    assert len(plan.pts_in) == 1 and plan.npts.numel() == 1 and len(plan.pts_views[0]) == 3
    for i in (1, 0, 3, 2, 1):                                           # out of order, one frame twice: nothing carries over
        plan.run_graph([torch.from_numpy(_frames(w)[i]).to(dev)])
        TS._same_dets(plan.results(), want[i][0], ("graph", i))
    small = _frames(w)[2][:3000]                                        # a smaller cloud after larger ones: no stale view rows
    plan.run_graph([torch.from_numpy(small).to(dev)])
    got = plan.results()
    assert plan.npts_views.cpu().tolist() == [[3000, 3000, 3000]]
    TS._same_dets(got, host_statement(dev, [small], TC.V4)[0][0], "graph, small cloud")
    base = _plan(sd, w, dev)
    base.capture(w["points_cap"])
    torch.cuda.synchronize()
    n0, n1 = TS._node_types(base, dev), TS._node_types(plan, dev)
    print("frame graph nodes by type: plain", n0, "tta V4", n1)
    assert set(n1) == {KERNEL}, n1
    assert n1[KERNEL] > n0[KERNEL]
    plan.run_graph([torch.from_numpy(_frames(w)[0]).to(dev)])           # the plan still works after the second capture
    TS._same_dets(plan.results(), want[0][0], "graph after recapture")


# ---- 4: the stream --------------------------------------------------------------------------------------------------------
def _stream(sd, w, dev, inflight, points_cap=None, **kw):
    return FrameStream(sd, inflight=inflight, points_cap=points_cap or w["points_cap"], batch_size=1, anchors=w["anchors"],
                       anchors_bv=w["anchors_bv"], device=dev, **dict(w["plan"], **kw))


def test_stream_with_two_frames_in_flight_equals_the_plan(dev):
    sd, w, _ = TS._workload(dev)
    frames = _frames(w)
    want = host_statement(dev, frames, TC.V2, overlap=False)            # a stream in flight runs one-branch plans
    for i in range(4):                                                  # (the branch count does not change a bit)
        TS._same_dets(want[i][0], _statement(dev, "V2")[i][0], ("one-branch statement", i))
    with _stream(sd, w, dev, 2, tta=TC.V2) as fs:
        assert fs.batch_size == 1 and all(p.B == 2 and p.b_user == 1 and p.tta == tuple(TC.V2) for p in fs.plans)
        order = [0, 1, 2, 3, 3, 1]
        got = list(fs.map([frames[i]] for i in order))
        assert [t for t, _ in got] == list(range(1, len(order) + 1))
        for (_, d), i in zip(got, order):
            assert len(d) == 1
            TS._same_dets(d, want[i][0], ("stream inflight 2", i))
        tickets = [fs.submit([torch.from_numpy(frames[i]).to(dev)]) for i in order]      # device clouds
        for t, i in zip(tickets, order):
            TS._same_dets(fs.collect(t), want[i][0], ("stream inflight 2, device clouds", i))
        assert all(int(p.status.item()) == 0 for p in fs.plans)


def test_stream_with_raw_cap_and_annos_equals_the_plan(dev):
    sd, w, _ = TS._workload(dev)
    sweeps = [CROP.raw_sweep(s) for s in range(2)]
    calib = dict(calib=A.calib_matrices(), img_shape=CROP.IMG_SHAPE + (3,))
    plan = _plan(sd, w, dev, tta=TC.V2)
    block = torch.from_numpy(calib_block_of(calib["calib"], calib["img_shape"])).to(dev).view(1, -1)
    with _stream(sd, w, dev, 1, points_cap=CROP.POINTS_CAP, raw_cap=CROP.RAW_CAP, annos=True, tta=TC.V2) as fs:
        got = [d for _, d in fs.map(([raw], [calib]) for raw, _ in sweeps)]
        assert all(int(p.status.item()) == 0 for p in fs.plans)
        assert int(fs.plans[0].npts[0].item()) == len(sweeps[1][1]) == int(fs.plans[0].npts_views[0, 0].item())
    n_det = 0
    for i, (_, red) in enumerate(sweeps):
        plan.run_from_points([torch.from_numpy(red).to(dev)])           # the plan on the sweep reduced on the host ...
        seq = torch.tensor([i + 1], dtype=torch.int32, device=dev)
        rec = K.frame_seal_kitti(plan.det, seq, plan.status, block)     # ... and the annotations of ITS detections
        torch.cuda.synchronize()
        want = decode_record(rec.cpu().numpy(), 1, plan.capD, i + 1, annos=True)
        assert len(got[i]) == 1 and len(got[i][0]) == 4
        TS._same_dets([got[i][0][:3]], [want[0][:3]], ("raw + annos", i))
        if want[0][0] is not None:
            n_det += len(want[0][0])
            for k in want[0][3]:
                assert TC.same_bits(got[i][0][3][k], want[0][3][k]), (i, k)
    assert n_det >= 1


def test_stream_with_two_sweeps_equals_the_plan(dev):
    sd, w, _ = TS._workload(dev)
    scene = _frames(w)[0]

    def pose(yaw, t):
        m = np.eye(4)
        m[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
        m[:3, 3] = t
        return m
    poses = [pose(0.0, [0, 0, 0]), pose(0.02, [0.8, 0.1, 0]), pose(-0.01, [1.5, -0.2, 0]), pose(0.0, [2.1, 0.0, 0])]
    sweeps = []
    for p in poses:                                                     # one static scene seen from a moving sensor
        m = sweep_transform(p, poses[0])
        s = scene.copy()
        s[:, :3] = (scene[:, :3].astype(np.float64) @ m[:, :3].T + m[:, 3]).astype(np.float32)
        sweeps.append(s)
    merged = [merge_sweeps_host([(sweeps[t], None, 0.0)] + ([(sweeps[t - 1], sweep_transform(poses[t], poses[t - 1]), 0.1)]
                                                            if t else []), False) for t in range(4)]
    cap = 2 * len(scene) + 8
    plan = _plan(sd, w, dev, tta=TC.V2, overlap=False)
    want = []
    for m in merged:
        plan.run_from_points([torch.from_numpy(m).to(dev)])
        want.append(plan.results())
    assert sum(r[0][0] is not None for r in want) >= 2
    with _stream(sd, w, dev, 2, points_cap=cap, sweeps=2, sweep_cap=len(scene), time_feature=False, tta=TC.V2) as fs:
        got = [d for _, d in fs.map(([sweeps[t]], None, None, [dict(pose=poses[t], time=0.1 * t)]) for t in range(4))]
        for t in range(4):
            TS._same_dets(got[t], want[t], ("sweeps", t))
        assert all(int(p.status.item()) == 0 for p in fs.plans)


# ---- 5: the detector ------------------------------------------------------------------------------------------------------
def test_detector_plan_honours_test_cfg_tta(dev):
    sd, w, model = TS._workload(dev)
    model = model.to(dev).eval()
    an = torch.from_numpy(w["anchors"]).to(dev)
    kw = dict(cap_k=w["plan"]["cap_k"], cap_d=w["plan"]["cap_d"])
    had = "tta" in model.test_cfg
    old = model.test_cfg.get("tta")
    try:
        model.test_cfg.pop("tta", None)
        plain = model.plan(1, an, dev, **kw)
        assert plain.tta is None and plain.B == 1
        model.test_cfg["tta"] = TC.V2
        p2 = model.plan(1, an, dev, **kw)
        assert p2 is not plain and p2.tta == tuple(TC.V2) and p2.B == 2 and p2.b_user == 1
        assert model.plan(1, an, dev, **kw) is p2                       # the same spec: the cached plan
        model.test_cfg["tta"] = TC.V4
        p4 = model.plan(1, an, dev, **kw)                               # a changed spec rebuilds the plan
        assert p4 is not p2 and p4.tta == tuple((f, float(a), float(s)) for f, a, s in TC.V4) and p4.B == 4
        assert model.plan(1, an, dev, tta=None, **kw).tta is None       # an explicit tta= overrides test_cfg
        with pytest.raises(ValueError, match="identity"):
            model.test_cfg["tta"] = [(1, 0.0, 1.0)]
            model.plan(1, an, dev, **kw)
        # the plan the detector builds detects what the statement detects (the thresholds are the workload's: test_cfg's)
        model.test_cfg["tta"] = TC.V2
        plan = model.plan(1, an, dev, **kw)
        ref = _plan(sd, w, dev, tta=TC.V2, score_thr=plan.score_thr, iou_thr=plan.iou_thr, rpn_thr=plan.rpn_thr)
        pts = torch.from_numpy(_frames(w)[0]).to(dev)
        plan.run_from_points([pts])
        ref.run_from_points([pts])
        TS._same_dets(plan.results(), ref.results(), "detector plan")
    finally:
        model.test_cfg.pop("tta", None)
        if had:
            model.test_cfg["tta"] = old
        model._plan, model._plan_key = None, None
