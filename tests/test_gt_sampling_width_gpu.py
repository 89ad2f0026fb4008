"""-m gpu: GT-sampling at the cloud's width.  sassd_paste_objects_nd over the case table of tests/wide_cloud_cases.py
against the numpy contract (and, at 4 columns, against sassd_paste_objects); the projection property of PointAugmentor --
a widened database and a widened frame give, in their first four columns, the bits of the 4-wide call, with equal boxes,
types, labels and random state, and every extra column travels with its point (the tag column names the source row);
the refusal of a cloud of another width; and a 5-wide tree from disk through create_data, KittiLiDAR, collate and one
optimisation step of a 5-feature detector.  Every bar is equality."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import _C, create_data as CD, geometry as G, kitti_common as kc, point_augmentor as PA, train
from sassd.config import Config
from sassd.detector import build_detector
from sassd.kitti_dataset import get_dataset

import augment_synth as S
import helpers as H
import wide_cloud_cases as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------
def _launch(dev, case, entry="nd"):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    db, src, ostart, shift, lower = (t(case[k]) for k in ("db", "src_start", "out_start", "shift", "lower"))
    out = torch.full((case["n_out"], case["width"]), 7.0, dtype=torch.float32, device=dev)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    with torch.cuda.device(dev):
        if entry == "nd":
            rc = _C.lib().sassd_paste_objects_nd(p(db), case["width"], p(src), p(ostart), case["n_obj"], case["n_out"],
                                                 p(shift), p(lower), p(out), _C.stream())
        else:
            rc = _C.lib().sassd_paste_objects(p(db), p(src), p(ostart), case["n_obj"], case["n_out"], p(shift), p(lower),
                                              p(out), _C.stream())
    assert rc == 0, rc
    return out.cpu().numpy()


@pytest.mark.parametrize("width", W.WIDTHS)
def test_paste_objects_nd_gives_the_contract(dev, width):
    for case in W.cases(width):
        what = (case["name"], width, case["lower"] is not None)
        got = _launch(dev, case)
        assert W.same_bits(got, case["want"]), what
        if width == 4:                                             # the 4-column entry point: the same bytes
            assert W.same_bits(_launch(dev, case, "four"), got), what


# ---- 2. the projection property ----------------------------------------------------------------------------------------------
_DBS = {}


def _databases(tmp_path_factory):
    """the synthetic database written 4-wide and as its 5- and 8-wide twins: {width: (root, db)}"""
    if not _DBS:
        db4 = S.make_database()
        for width in (4, 5, 8):
            root = str(tmp_path_factory.mktemp("db_w%d" % width))
            db = W.widen_database(db4, width)
            S.write_database(db, root)
            _DBS[width] = (root, db)
    return _DBS


def _augmentor(dev, root, cfg):
    np.random.seed(1234)
    return PA.PointAugmentor(root_path=root, info_path=os.path.join(root, "kitti_dbinfos_train.pkl"), device=dev, **cfg)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _both(fn4, fnw, state):
    """the two calls from the same random state -> (4-wide result, wide result, the state after); the states must agree"""
    np.random.set_state(state)
    r4 = fn4()
    after = np.random.get_state()
    np.random.set_state(state)
    rw = fnw()
    assert _same_state(after, np.random.get_state()), "the wide call consumed other random numbers"
    return r4, rw, after


def _check_projection(p4, pw, sources, width):
    p4 = p4.cpu().numpy() if torch.is_tensor(p4) else p4
    pw = pw.cpu().numpy() if torch.is_tensor(pw) else pw
    assert pw.shape == (len(p4), width) and pw.dtype == np.float32
    assert W.same_bits(np.ascontiguousarray(pw[:, :4]), np.ascontiguousarray(p4))
    W.check_tags(pw, sources)


@pytest.mark.parametrize("width", [5, 8])
@pytest.mark.parametrize("cfg_name", ["car", "multi"])
def test_wide_augmentation_projects_onto_the_4_wide_call(dev, tmp_path_factory, cfg_name, width):
    dbs = _databases(tmp_path_factory)
    cfg = S.AUGMENTOR_CONFIGS[cfg_name]
    classes = cfg["sample_classes"]
    calib = kc.Calibration(matrices=S.calib_matrices())
    plane = S.PLANE if cfg_name == "multi" else None
    aug4, augw = _augmentor(dev, dbs[4][0], cfg), _augmentor(dev, dbs[width][0], cfg)          # fused recipe
    step4, stepw = _augmentor(dev, dbs[4][0], cfg), _augmentor(dev, dbs[width][0], cfg)        # method by method
    assert augw.num_point_features == width and tuple(augw.database_on_device().shape)[1] == width
    db_rows = W.database_sources(dbs[width][1])
    state = np.random.get_state()
    pasted = 0
    for f in range(3):
        pts4, gt_boxes, gt_types = S.frame(f)
        ptsw = W.widen_points(pts4, width, f)
        sources = np.concatenate([ptsw, db_rows])
        up = lambda a: torch.from_numpy(a).to(dev)

        # method by method, the numpy calling convention
        (b4, t4, s4), (bw, tw, sw), mid = _both(lambda: step4.sample_all(gt_boxes, gt_types, plane, calib),
                                                lambda: stepw.sample_all(gt_boxes, gt_types, plane, calib), state)
        assert np.array_equal(b4, bw) and t4 == tw and len(s4) > 0
        _check_projection(s4, sw, db_rows, width)
        pasted += len(s4)
        boxes = np.concatenate([gt_boxes, b4])
        p4, pw = np.concatenate([s4, pts4]), np.concatenate([sw, ptsw])

        def rest(step, boxes, p):
            step.noise_per_object_(boxes, p, num_try=100)
            moved = p.copy()
            boxes, p = step.random_flip(boxes, p)
            boxes, p = step.random_flip(boxes, p, probability=1.0)
            boxes, p = step.global_rotation(boxes, p)
            flipped_rotated = p.copy()
            boxes, p = step.global_scaling(boxes, p)
            return boxes, moved, flipped_rotated, p
        r4, rw, _ = _both(lambda: rest(step4, boxes.copy(), p4.copy()), lambda: rest(stepw, boxes.copy(), pw.copy()), mid)
        assert np.array_equal(r4[0], rw[0])
        for a, b in zip(r4[1:], rw[1:]):
            _check_projection(a, b, sources, width)
        assert not np.array_equal(r4[1][:, :3], p4[:, :3]) and not np.array_equal(r4[3][:, :3], r4[1][:, :3])

        # the fused recipe on device tensors
        o4, ow, state = _both(lambda: aug4.augment_frame(up(pts4), gt_boxes.copy(), gt_types, classes, plane, calib),
                              lambda: augw.augment_frame(up(ptsw), gt_boxes.copy(), gt_types, classes, plane, calib), state)
        assert ow[0].is_cuda and np.array_equal(o4[1], ow[1]) and o4[1].dtype == ow[1].dtype
        assert np.array_equal(o4[2], ow[2]) and np.array_equal(o4[3], ow[3])
        _check_projection(o4[0], ow[0], sources, width)
        tags = ow[0][:, 4].cpu().numpy()
        assert (tags >= W.DB_TAG_BASE * W.TAG_STRIDE).any() and (tags < 3 * W.TAG_STRIDE).any()   # pasted and scene rows
    assert pasted > 0


# ---- 3. a cloud of another width -----------------------------------------------------------------------------------------------
def test_a_cloud_of_another_width_is_refused_before_a_launch(dev, tmp_path_factory, monkeypatch):
    dbs = _databases(tmp_path_factory)
    cfg = S.AUGMENTOR_CONFIGS["car"]
    aug4, aug5 = _augmentor(dev, dbs[4][0], cfg), _augmentor(dev, dbs[5][0], cfg)
    aug5.database_on_device()

    def launched(*a, **k):
        raise AssertionError("a kernel was launched")
    for name in ("_paste_objects", "_paste_objects_nd", "_points_transform", "_points_global"):
        monkeypatch.setattr(PA, name, launched)
    monkeypatch.setattr(G, "points_in_polytopes", launched)
    pts4, gt_boxes, gt_types = S.frame(0)
    pts5 = W.widen_points(pts4, 5, 0)
    calib = kc.Calibration(matrices=S.calib_matrices())
    state = np.random.get_state()
    for aug, cloud, pattern in ((aug5, pts4, r"4 features.*database has 5"), (aug4, pts5, r"5 features.*database has 4")):
        for points in (cloud, torch.from_numpy(cloud).to(dev)):
            calls = [lambda: aug.augment_frame(points, gt_boxes.copy(), gt_types, ["Car"], None, calib),
                     lambda: aug.noise_per_object_(gt_boxes.copy(), points), lambda: aug.random_flip(gt_boxes.copy(), points),
                     lambda: aug.random_flip(gt_boxes.copy(), points, probability=1.0),
                     lambda: aug.global_rotation(gt_boxes.copy(), points), lambda: aug.global_scaling(gt_boxes.copy(), points)]
            for call in calls:
                with pytest.raises(ValueError, match=pattern):
                    call()
    assert _same_state(state, np.random.get_state()), "a refused call drew random numbers"


# ---- 4. from a 5-wide tree on disk to an optimisation step ---------------------------------------------------------------------
def _prepared(root, width, dev):
    S.write_kitti_tree(root)
    W.widen_tree(root, width)
    CD.create_kitti_info_file(root, device=dev, num_features=width)
    CD.create_reduced_point_cloud(root, device=dev)
    CD.create_groundtruth_database(root, device=dev)


def test_a_5_wide_tree_trains_a_5_feature_detector(dev, tmp_path):
    c = Config.fromfile(os.path.join(ROOT, "configs", "car_cfg.py"))
    sets = {}
    for width in (4, 5):
        root = str(tmp_path / ("w%d" % width))
        _prepared(root, width, dev)
        tr = dict(c.data.train, root=root + '/training/', ann_file=root + '/ImageSets/train.txt')
        tr['augmentor'] = dict(tr['augmentor'], root_path=root + '/', info_path=root + '/kitti_dbinfos_train.pkl',
                               sample_classes=['Van'], min_num_points=[2], sample_max_num=[4])
        if width != 4:
            tr['num_point_features'] = width
        np.random.seed(3)
        ds = get_dataset(tr, device=dev)
        assert ds.augmentor.num_point_features == width == ds.num_point_features
        sets[width] = (ds, [ds[0], ds[1]], np.random.get_state())
    (ds4, samples4, state4), (ds5, samples5, state5) = sets[4], sets[5]
    assert _same_state(state4, state5)
    foreign = 0
    for s4, s5 in zip(samples4, samples5):
        p4, p5 = s4['points'].cpu().numpy(), s5['points'].cpu().numpy()
        assert s5['points'].is_cuda and p5.shape == (len(p4), 5)
        assert W.same_bits(np.ascontiguousarray(p5[:, :4]), p4)
        assert torch.equal(s4['gt_bboxes'], s5['gt_bboxes']) and np.array_equal(s4['gt_types'], s5['gt_types'])
        frames = p5[:, 4].astype(np.int64) // W.TAG_STRIDE          # the tag column: rows of the sample's own sweep ...
        assert (frames == s5['img_meta']['sample_idx']).any()
        foreign += int((frames != s5['img_meta']['sample_idx']).sum())
    assert foreign > 0                                             # ... and, pasted from the database, of another frame's object

    c.model["backbone"]["num_input_features"] = 5
    c.model["neck"]["num_input_features"] = 5
    model = H.randomize_detector(build_detector(c.model, c.train_cfg, c.test_cfg), 3, cls_bias=-3.0).to(dev)
    assert tuple(model.neck.backbone.conv0[0].weight.shape) == (3, 3, 3, 5, 16)
    with pytest.raises(ValueError, match=r"4 features.*num_input_features is 5"):
        ds4.collate(samples4, model=model)
    opt = train.build_optimizer(model, c.optimizer, 1)
    sched = train.build_scheduler(opt, 10, 1, c.optimizer, c.lr_config)
    sync = train.GradSync(opt.flat)
    w0 = opt.flat.data.clone()
    batch = ds5.collate(samples5, model=model)
    assert len(batch['voxels']) == 2 and batch['voxels'][0].shape[2] == 5
    loss, terms = train.train_one_iter(model, opt, sched, sync, batch, 0)
    assert np.isfinite(float(loss)) and float((opt.flat.data - w0).abs().max()) > 0
