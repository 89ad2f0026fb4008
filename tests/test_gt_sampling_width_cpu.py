"""GT-sampling at the cloud's width, without a GPU: paste_point_nd / object_of_row looped on the CPU over the kernel's case
table (tests/wide_cloud_cases.py) against the numpy contract, the C-ABI error convention of sassd_paste_objects_nd, the
host half of PointAugmentor on 5-wide and legacy databases, and the data preparation of a widened KITTI tree (per-point
kernels replaced by the CPU harness, as test_create_data_cpu.py does).  Every bar is equality."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import _C, create_data as CD
from sassd.point_augmentor import PointAugmentor

import augment_synth as S
import harness
import wide_cloud_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL = 0, -1


# ---- 1. the arithmetic -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", W.WIDTHS)
def test_paste_point_nd_gives_the_contract(width, tmp_path_factory):
    lib = W.harness(tmp_path_factory.getbasetemp())
    for case in W.cases(width):
        got = W.harness_paste(lib, case)
        assert W.same_bits(got, case["want"]), (case["name"], width, case["lower"] is not None)


def test_the_case_table_covers_what_it_names():
    seen_obj, seen_out = set(), set()
    for width in W.WIDTHS:
        for case in W.cases(width):
            seen_obj.add(case["n_obj"])
            seen_out.add(case["n_out"])
            assert np.array_equal(np.diff(case["out_start"]), case["counts"])
    assert seen_obj == {1, 2, 37} and seen_out == {1, 255, 256, 257, 513}
    c37 = np.asarray(W.STRUCTURES["thirty_seven"])
    assert c37[0] == 0 and c37[-1] == 0 and ((c37[1:-2] == 0) & (c37[2:-1] == 0)).any() and (c37 == 1).any()
    assert list(W.STRUCTURES["zero_first"]) == [0, 1] and list(W.STRUCTURES["zero_last"]) == [1, 0]


# ---- 2. the ABI --------------------------------------------------------------------------------------------------------------
def test_paste_nd_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "sassd.h")).read()
    assert re.search(r"\bsassd_paste_objects_nd\s*\(", header), "sassd_paste_objects_nd is not declared in include/sassd.h"
    assert "sassd_paste_objects_nd" in _C.EXPORTS
    assert getattr(C.CDLL(_C.LIB_PATH), "sassd_paste_objects_nd") is not None


def test_paste_nd_argument_validation_returns_before_a_launch():
    """fake pointers throughout: a call that reached a launch could not return EINVAL or OK"""
    paste, p16, null = _C.lib().sassd_paste_objects_nd, C.c_void_p(16), None
    good = [p16, 5, p16, p16, 3, 100, p16, p16, p16, null]        # db, ndim, src_start, out_start, n_obj, n_out, shift, lower, out
    for ndim in (-1, 0, 1, 2, 9, 16):
        args = list(good)
        args[1] = ndim
        assert paste(*args) == EINVAL, ndim
    for i, v in ((4, -1), (5, -1), (5, -2 ** 40)):
        args = list(good)
        args[i] = v
        assert paste(*args) == EINVAL, (i, v)
    for ndim in (3, 4, 5, 6, 7, 8):                               # zero counts are fine, with or without arrays
        for i in (4, 5):
            args = list(good)
            args[1], args[i] = ndim, 0
            assert paste(*args) == OK, (ndim, i)
            assert paste(*[null if a is p16 else a for a in args]) == OK, (ndim, i)
    args = list(good)                                             # a bad width is refused even with zero counts
    args[1], args[4] = 9, 0
    assert paste(*args) == EINVAL
    for i in (0, 2, 3, 6, 8):                                     # every array but `lower` is required
        args = list(good)
        args[i] = null
        assert paste(*args) == EINVAL, i


# ---- 3. PointAugmentor, host half --------------------------------------------------------------------------------------------
def _small_db():
    """six cars; the first has exactly 4 points (so that its 5-wide file, 20 floats, is divisible by 4)"""
    db = S.make_database(seed=7, counts=(("Car", 6),))
    for info in db["Car"]:
        info["difficulty"] = 0
    first = db["Car"][0]
    first["points"] = np.ascontiguousarray(np.tile(first["points"], (3, 1))[:4])
    first["num_points_in_gt"] = 4
    return db


_CFG = dict(S.AUGMENTOR_CONFIGS["car"], min_num_points=[1])


def _augmentor(root, **kw):
    return PointAugmentor(str(root), str(root / "kitti_dbinfos_train.pkl"), device="cpu", **dict(_CFG, **kw))


def _check_packed(aug, root, width):
    infos = aug._samplers[0]._sampled_list
    assert aug.num_point_features == width and aug._db_points.dtype == np.float32
    assert aug._db_points.shape == (sum(i["num_points_in_gt"] for i in infos), width)
    for info in infos:
        rows = aug._db_points[info["_start"]:info["_start"] + info["_count"]]
        assert info["_count"] == info["num_points_in_gt"]
        assert rows.tobytes() == open(os.path.join(str(root), info["path"]), "rb").read(), info["path"]


def test_augmentor_takes_the_width_from_the_db_infos(tmp_path):
    wide = W.widen_database(_small_db(), 5)
    S.write_database(wide, str(tmp_path))
    aug = _augmentor(tmp_path)
    assert len(aug._samplers[0]._sampled_list) == 6
    _check_packed(aug, tmp_path, 5)
    assert np.array_equal(aug._db_points, W.database_sources(wide))
    assert _augmentor(tmp_path, num_point_features=5).num_point_features == 5
    with pytest.raises(ValueError, match=r"4 features.*database has 5"):              # a 4-wide cloud: both widths named
        aug.augment_frame(np.zeros((10, 4), np.float32), np.zeros((0, 7), np.float32), [], ["Car"])


def test_augmentor_refuses_a_file_of_another_width(tmp_path):
    S.write_database(W.widen_database(_small_db(), 5, key=False), str(tmp_path))      # 5-wide files, infos that do not say so
    first = re.escape(_small_db()["Car"][0]["path"])
    with pytest.raises(ValueError, match=first + r" holds 20 floats.*4 points x 4 features.*width 4"):
        _augmentor(tmp_path)                                       # 20 floats: divisible by 4, once parsed as 5 garbage rows
    with pytest.raises(ValueError, match=r"holds 20 floats.*width 4"):
        _augmentor(tmp_path, num_point_features=4)
    with pytest.raises(ValueError, match=r"holds 20 floats.*width 8"):
        _augmentor(tmp_path, num_point_features=8)
    _check_packed(_augmentor(tmp_path, num_point_features=5), tmp_path, 5)            # the stated width loads them
    with pytest.raises(ValueError, match="3..8"):
        _augmentor(tmp_path, num_point_features=9)
    # a truncated file of the right database: the count is not a whole number of rows
    db = W.widen_database(_small_db(), 5)
    S.write_database(db, str(tmp_path))
    path = os.path.join(str(tmp_path), db["Car"][2]["path"])
    blob = open(path, "rb").read()
    with open(path, "wb") as f:
        f.write(blob[:-4])
    with pytest.raises(ValueError, match=re.escape(db["Car"][2]["path"]) + r" holds %d floats.*width 5" % (len(blob) // 4 - 1)):
        _augmentor(tmp_path)


def test_a_legacy_database_without_the_key_loads_as_before(tmp_path):
    db = _small_db()
    S.write_database(db, str(tmp_path))
    assert all("num_point_features" not in i for i in W.load_pickle(str(tmp_path / "kitti_dbinfos_train.pkl"))["Car"])
    aug = _augmentor(tmp_path)
    _check_packed(aug, tmp_path, 4)
    assert np.array_equal(aug._db_points, W.database_sources(db))


# ---- 4. data preparation of a widened tree -------------------------------------------------------------------------------------
def _prepare(root, width, device):
    S.write_kitti_tree(root)
    W.widen_tree(root, width)
    CD.create_kitti_info_file(root, device=device, num_features=width)
    CD.create_reduced_point_cloud(root, device=device)
    return CD.create_groundtruth_database(root, device=device)


def test_data_preparation_keeps_the_width_and_the_four_columns(tmp_path, monkeypatch):
    harness.patch(monkeypatch)
    cpu = torch.device("cpu")
    base = str(tmp_path / "w4")
    db4 = _prepare(base, 4, cpu)
    assert all("num_point_features" not in i for infos in db4.values() for i in infos)
    files = [os.path.join(sub, fn) for sub in ("training/velodyne_reduced", "testing/velodyne_reduced", "gt_database")
             for fn in sorted(os.listdir(os.path.join(base, sub)))]
    assert len(files) > 10
    for width in (5, 8):
        root = str(tmp_path / ("w%d" % width))
        dbw = _prepare(root, width, cpu)
        for rel in files:
            narrow = np.fromfile(os.path.join(base, rel), dtype=np.float32).reshape(-1, 4)
            flat = np.fromfile(os.path.join(root, rel), dtype=np.float32)
            assert flat.size == len(narrow) * width, rel
            wide = flat.reshape(-1, width)
            assert np.ascontiguousarray(wide[:, :4]).tobytes() == narrow.tobytes(), rel
            if "velodyne_reduced" in rel:                         # the tag column: rows of this very frame, in file order
                frame = int(os.path.basename(rel).split(".")[0]) + (W.TREE_TESTING_FRAME if rel.startswith("testing") else 0)
                row = wide[:, 4].astype(np.int64) - frame * W.TAG_STRIDE
                assert (row >= 0).all() and (row < W.TAG_STRIDE).all() and (np.diff(row) > 0).all(), rel
        for name in ("train", "val", "trainval", "test"):
            a = W.load_pickle(os.path.join(base, "kitti_infos_%s.pkl" % name))
            b = W.load_pickle(os.path.join(root, "kitti_infos_%s.pkl" % name))
            assert len(a) == len(b)
            for ia, ib in zip(a, b):
                assert ia["pointcloud_num_features"] == 4 and ib["pointcloud_num_features"] == width
                if "annos" in ia:
                    assert np.array_equal(ia["annos"]["num_points_in_gt"], ib["annos"]["num_points_in_gt"])
        assert list(dbw) == list(db4)
        for cls in db4:
            assert len(dbw[cls]) == len(db4[cls])
            for ia, ib in zip(db4[cls], dbw[cls]):
                assert ib["num_point_features"] == width
                assert sorted(ib) == sorted(list(ia) + ["num_point_features"])
                assert ia["path"] == ib["path"] and ia["num_points_in_gt"] == ib["num_points_in_gt"]
                assert np.array_equal(ia["box3d_lidar"], ib["box3d_lidar"])
        on_disk = W.load_pickle(os.path.join(root, "kitti_dbinfos_train.pkl"))
        assert all(i["num_point_features"] == width for infos in on_disk.values() for i in infos)
        # the prepared wide tree feeds the augmentor at its own width
        np.random.seed(0)
        aug = PointAugmentor(root, os.path.join(root, "kitti_dbinfos_train.pkl"), **dict(
            S.AUGMENTOR_CONFIGS["car"], sample_classes=["Van"], min_num_points=[2], sample_max_num=[3]), device="cpu")
        assert aug.num_point_features == width and aug._db_points.shape[1] == width and len(aug._db_points) > 0
