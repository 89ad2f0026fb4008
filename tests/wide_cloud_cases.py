"""Inputs shared by test_gt_sampling_width_cpu.py and test_gt_sampling_width_gpu.py: the paste contract in numpy, the case
table of the wide paste kernel, and wideners for the synthetic clouds, databases and KITTI trees of augment_synth.

The contract of sassd_paste_objects_nd (include/sassd.h): x, y, z are moved, every other column is copied bit for bit.
  xyz   = (src[:, :3].astype(f64) + shift).astype(f32)
  z     = (z.astype(f64) - lower).astype(f32)              when lowered: a second rounding
  other = src                                              compared as uint32, so NaN payloads, -0.0 and denormals count
Every bar against it is equality.

Tags: a widened cloud's column 4 is `frame * 2**17 + row`, an integer below 2**24 (frame < 128, row < 2**17), so exact in
float32 and unique per source row; it names the row an output point was made from.  Further columns are seeded floats."""
import ctypes as C
import os
import pickle
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
WIDTHS = (3, 4, 5, 7, 8)
TAG_STRIDE = 2 ** 17
DB_TAG_BASE = 8                     # database object j is "frame" DB_TAG_BASE + j; scene frames are 0..7

# bit patterns the copied columns must carry through: quiet / signalling NaNs with payloads, -0.0, denormals, infinities
SPECIAL_BITS = np.array([0x7fc12345, 0x7f800001, 0xffc00001, 0xff8abcde, 0x80000000, 0x00000001, 0x807fffff, 0x00400000,
                         0x7f800000, 0xff800000], dtype=np.uint32)


# ---- the contract ------------------------------------------------------------------------------------------------------------
def rows_of(src_start, counts):
    """-> (database row, object) of every output row"""
    src_start, counts = np.asarray(src_start, np.int64), np.asarray(counts, np.int64)
    k = np.repeat(np.arange(len(counts)), counts)
    first = np.concatenate([[0], np.cumsum(counts)])[:-1]
    return src_start[k] + (np.arange(int(counts.sum())) - first[k]), k


def paste_contract(db, src_start, counts, shift, lower=None):
    """db [P,W] f32, shift [n_obj,3] f64, lower [n_obj] f64 or None -> [sum counts, W] f32"""
    rows, k = rows_of(src_start, counts)
    out = db.view(np.uint32)[rows].view(np.float32)                 # the copied columns, bit for bit
    xyz = (db[rows, :3].astype(np.float64) + shift[k]).astype(np.float32)
    if lower is not None:
        xyz[:, 2] = (xyz[:, 2].astype(np.float64) - lower[k]).astype(np.float32)
    out[:, :3] = xyz
    return out


def paste_float32(db, src_start, counts, shift, lower=None):
    """the WRONG arithmetic -- everything in float32 -- that a case must tell from the contract"""
    rows, k = rows_of(src_start, counts)
    out = db.view(np.uint32)[rows].view(np.float32)
    xyz = db[rows, :3] + shift.astype(np.float32)[k]
    if lower is not None:
        xyz[:, 2] = xyz[:, 2] - lower.astype(np.float32)[k]
    out[:, :3] = xyz
    return out


# ---- the kernel's case table -------------------------------------------------------------------------------------------------
def _counts37():
    """37 objects, 513 rows: zero-point objects first, in the middle (two in a row) and last, objects of one point"""
    c = np.array([0, 1, 30, 0, 0, 1, 1, 64, 17, 0, 5, 1, 40, 0, 23, 9, 1, 31, 0, 2, 30, 1, 1, 0, 12, 63, 3, 0, 28, 1, 44, 7,
                  0, 19, 1, 57, 0], dtype=np.int64)
    assert len(c) == 37
    c[7] += 513 - int(c.sum())
    assert c[7] > 0 and int(c.sum()) == 513
    return c


PASTED_TWICE = (2, 20)              # of "thirty_seven": two sampled objects of 30 points that name one database object

# name -> the objects' point counts; n_obj in {1, 2, 37}, n_out in {1, 255, 256, 257, 513}
STRUCTURES = {
    "one_point": [1],
    "one_object_255": [255],
    "zero_first": [0, 1],
    "zero_last": [1, 0],
    "one_and_255": [1, 255],
    "256_and_one": [256, 1],
    "two_blocks_and_one": [512, 1],
    "thirty_seven": _counts37(),
}


def make_case(name, width, lowered, seed=0):
    """-> dict(db [P,W] f32, src_start, out_start [n_obj+1], counts, shift, lower or None, want [n_out,W] f32).  The database
    holds one object per sampled object plus unused rows in front and between; the sampled objects name them out of order
    (src_start is not increasing), and in the 37-object case two of them name the SAME database object."""
    counts = np.asarray(STRUCTURES[name], dtype=np.int64)
    n_obj = len(counts)
    r = np.random.default_rng([seed, width, int(lowered), sorted(STRUCTURES).index(name)])
    order = r.permutation(n_obj)                                   # database position of every sampled object
    starts, at = np.zeros(n_obj, np.int64), 3
    for j in np.argsort(order):
        starts[j] = at
        at += int(counts[j]) + int(r.integers(0, 3))
    if name == "thirty_seven":                                     # one database object pasted twice
        i, j = PASTED_TWICE
        assert counts[i] == counts[j] > 1
        starts[j] = starts[i]
    P = at + 2
    db = r.uniform(-3, 3, (P, width)).astype(np.float32)
    if width > 3:                                                  # special bit patterns through the copied columns
        bits = db.view(np.uint32)
        ii, jj = np.meshgrid(np.arange(P), np.arange(3, width), indexing="ij")
        special = (ii + jj) % 3 == 0
        bits[:, 3:][special] = SPECIAL_BITS[((ii + 2 * jj) // 3 % len(SPECIAL_BITS))[special]]
    out_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    case = dict(name=name, width=width, db=db, src_start=starts, out_start=out_start, counts=counts, n_obj=n_obj,
                n_out=int(out_start[-1]))
    for attempt in range(64):                                      # float64 shifts whose add rounds unlike a float32 add
        shift = np.stack([r.uniform(4, 66, n_obj), r.uniform(-34, 34, n_obj), r.uniform(-1.9, -1.3, n_obj)], 1)
        lower = r.uniform(-0.4, 0.4, n_obj) if lowered else None
        want = paste_contract(db, starts, counts, shift, lower)
        if not np.array_equal(want.view(np.uint32), paste_float32(db, starts, counts, shift, lower).view(np.uint32)):
            break
    case.update(shift=shift, lower=lower, want=want)
    check_case(case)
    return case


def check_case(case):
    """what the table promises of every case, asserted so that no test passes on the wrong arithmetic or a lucky layout"""
    db, counts, starts = case["db"], case["counts"], case["src_start"]
    wrong = paste_float32(db, starts, counts, case["shift"], case["lower"])
    assert not np.array_equal(wrong[:, :3].view(np.uint32), case["want"][:, :3].view(np.uint32)), \
        "%s: a float32 add gives the contract's bytes" % case["name"]
    assert case["want"].shape == (case["n_out"], case["width"]) and case["n_out"] == int(counts.sum())
    assert (starts >= 0).all() and (starts + counts <= len(db)).all(), "an object reaches outside the database"
    if case["n_obj"] >= 3:
        assert (np.diff(starts) < 0).any(), "src_start is increasing"
        assert len(set(starts[counts > 0].tolist())) < int((counts > 0).sum()), "no object is pasted twice"
    if case["width"] > 3 and case["n_out"] >= 16:
        got = set(case["want"][:, 3:].view(np.uint32).ravel().tolist())
        assert got >= set(SPECIAL_BITS.tolist()), "a special bit pattern is not among the copied values"


_CASES = {}


def cases(width):
    """every structure x (lower null, lower given) at one width, built once"""
    if width not in _CASES:
        _CASES[width] = [make_case(n, width, lowered) for n in STRUCTURES for lowered in (False, True)]
    return _CASES[width]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the CPU harness over paste_point_nd / object_of_row ------------------------------------------------------------------------
_harness = None


def harness(tmp_dir):
    """tests/paste_nd_harness.hip, compiled once per process into `tmp_dir` (hipcc --cuda-host-only)"""
    global _harness
    if _harness is None:
        dst = os.path.join(str(tmp_dir), "libpaste_nd_harness.so")
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-fno-fast-math", "-ffp-contract=on", "-shared",
                               "-fPIC", "-o", dst, os.path.join(ROOT, "tests", "paste_nd_harness.hip")])
        _harness = C.CDLL(dst)
        _harness.hst_paste_objects_nd.restype = None
        _harness.hst_paste_objects_nd.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]
    return _harness


def harness_paste(lib, case):
    out = np.full((case["n_out"], case["width"]), 7.0, np.float32)
    lower = case["lower"]
    lib.hst_paste_objects_nd(case["db"].ctypes.data, case["width"], case["src_start"].ctypes.data,
                             case["out_start"].ctypes.data, case["n_obj"], case["n_out"], case["shift"].ctypes.data,
                             None if lower is None else lower.ctypes.data, out.ctypes.data)
    return out


# ---- wideners ------------------------------------------------------------------------------------------------------------------
def widen_points(pts, width, frame, seed=0):
    """[N,4] f32 -> [N,width] f32 (width 4..8): the four columns as they are, column 4 the tag frame * 2**17 + row, further
    columns floats seeded by (seed, frame)."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    assert pts.shape[1] == 4 and 4 <= width <= 8 and 0 <= frame < 128 and len(pts) < TAG_STRIDE
    if width == 4:
        return pts.copy()
    tag = (frame * TAG_STRIDE + np.arange(len(pts))).astype(np.float32)
    extra = np.random.default_rng([seed, frame]).uniform(-1, 1, (len(pts), width - 5)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([pts, tag[:, None], extra], 1))


def widen_database(db, width, key=True):
    """augment_synth.make_database's dict -> its twin at `width`: every object's points widened (object j of the whole
    database is tag frame DB_TAG_BASE + j), the db infos carrying 'num_point_features' as create_data writes it (for every
    width but 4) unless key=False."""
    out, j = {}, 0
    for name, infos in db.items():
        out[name] = []
        for info in infos:
            wide = dict(info, points=widen_points(info["points"], width, DB_TAG_BASE + j))
            if key and width != 4:
                wide["num_point_features"] = width
            out[name].append(wide)
            j += 1
    return out


def database_sources(db):
    """every point of a (widened) database, [P,W]"""
    return np.concatenate([info["points"] for infos in db.values() for info in infos])


def check_tags(out_points, sources):
    """column 4 of every output row names a source row whose intensity (column 3) the output row carries bit for bit"""
    tags = sources[:, 4]
    order = np.argsort(tags, kind="stable")
    assert len(np.unique(tags)) == len(tags), "the source tags are not unique"
    at = np.searchsorted(tags[order], out_points[:, 4])
    assert (at < len(tags)).all() and np.array_equal(tags[order][at], out_points[:, 4]), "a tag names no source row"
    src = sources[order][at]
    assert np.array_equal(src[:, 3].view(np.uint32), out_points[:, 3].view(np.uint32)), "a tag travelled with another point"
    if out_points.shape[1] > 5:                                    # the columns after the tag come from the same row
        assert np.array_equal(src[:, 5:].view(np.uint32), out_points[:, 5:].view(np.uint32))


TREE_TESTING_FRAME = 16             # tag frame of testing/velodyne/%06d.bin = TREE_TESTING_FRAME + idx


def widen_tree(root, width):
    """a tree written by augment_synth.write_kitti_tree -> the same tree with velodyne files of `width` floats per point"""
    for split, base in (("training", 0), ("testing", TREE_TESTING_FRAME)):
        d = os.path.join(root, split, "velodyne")
        for fn in sorted(os.listdir(d)):
            pts = np.fromfile(os.path.join(d, fn), dtype=np.float32).reshape(-1, 4)
            widen_points(pts, width, base + int(fn.split(".")[0])).tofile(os.path.join(d, fn))


def load_pickle(path):
    with open(path, "rb") as f:
        return pickle.load(f)
