"""Tracking without a GPU (include/sassd.h "Tracking"): the numpy statement sassd.track.track_host against a CPU loop over the
product's own rule (csrc/track_core.h through tests/track_harness.hip) on every seeded case, bit for bit over the whole state
and every output; that the cases' script really makes its events happen; properties of the statement; the switch; the ABI
surface, the record arithmetic and the argument errors of the entry point and its wrapper; the descriptor book; and the
submit-time errors on FrameRing with a fake slot."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sassd  # noqa: F401
from sassd import _C, track as T

import track_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSPC = -1, -2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not os.path.exists(TC.HIPCC):
        pytest.skip("hipcc not available")
    return TC.harness(tmp_path_factory.mktemp("track_harness"))


# ---- 1: the statement is the header -------------------------------------------------------------------------------------------
def _against_harness(lib, tr, cap):
    cur = tr["state0"]
    for t, (fr, want) in enumerate(zip(tr["seq"]["frames"], tr["steps"])):
        got = TC.harness_step(lib, cur, fr["det"], fr["desc"], TC.params(cap), fr["status"])
        assert TC.same_step(got, want) is None, (cap, t, TC.same_step(got, want))
        cur = want[0]


@pytest.mark.parametrize("seed,cap", TC.CASES)
def test_statement_equals_the_header_looped_on_the_cpu(lib, seed, cap):
    _against_harness(lib, TC.trace(seed, cap), cap)


@pytest.mark.parametrize("cap", TC.CROWD_CAPS)
def test_statement_equals_the_header_on_the_crowd(lib, cap):
    _against_harness(lib, TC.crowd_trace(0, cap), cap)


# ---- 2: the script of the cases happens ---------------------------------------------------------------------------------------
def _fields(state, b):
    return T.slot_fields(state["slots"][b])


def test_the_cases_make_their_events_happen():
    cap = 65
    tr = TC.trace(0, cap)
    frames, steps = tr["seq"]["frames"], tr["steps"]
    lo, hi = TC.TIE_SLOTS[cap]
    for b in range(TC.B):
        # frame 0: both tie slots hold live label-1 tracks at the same cost of the one label-1 detection; the lowest wins
        f0 = _fields(tr["state0"], b)
        det = frames[0]["det"]
        d = int(np.flatnonzero(det["labels"][b, :det["counts"][b]] == 1)[-1])
        c = [(float(det["boxes"][b, d, 0]) - float(f0["box"][i, 0])) ** 2 + (float(det["boxes"][b, d, 1]) - float(f0["box"][i, 1])) ** 2
             for i in (lo, hi)]
        assert c[0] == c[1] == 1.0 and frames[0]["desc"]["flags"][b] == 0
        assert np.array_equal(frames[0]["desc"]["T"][b], T.identity_desc(1)["T"][0]) and frames[0]["desc"]["dyaw"][b] == 0.0
        assert steps[0][1]["det_id"][b, d] == f0["id"][lo]
        f = _fields(steps[0][0], b)
        assert f["misses"][lo] == 0 and f["misses"][hi] == 1
        # a track coasts and is re-found with its id (object A: missed in frame 2)
        ids = [set(o["det_id"][b, :o["count"][b]].tolist()) - {-1} for _, o in steps]
        if b == 0:
            back = (ids[1] & ids[3]) - ids[2]
            assert back, "no track was re-found after a miss"
            f2 = _fields(steps[2][0], b)
            assert all(f2["misses"][np.flatnonzero(f2["id"] == i)[0]] == 1 for i in back)
        # a track dies of age between frames 3 and 6, and its object is born again later
        live = [set(_fields(st, b)["id"][_fields(st, b)["id"] >= 0].tolist()) for st, _ in steps]
        assert any(live[t - 1] - live[t] for t in range(3, 8)), "no track died"
        assert max(ids[7]) > max(ids[6]), "no birth in frame 7"
        # a detection below birth_score got no track
        s1 = frames[1]["det"]
        low = np.flatnonzero(s1["scores"][b, :s1["counts"][b]] < np.float32(TC.SPEC["birth_score"]))
        assert len(low) == 1 and steps[1][1]["det_id"][b, low[0]] == -1
        # the clamped count, the NaN, dt = 0, the reset, the second tie, the flagged frame, the empty frame
        assert frames[TC.OVER_FRAME]["det"]["counts"][b] > TC.CAP_D and steps[TC.OVER_FRAME][1]["count"][b] == TC.CAP_D
        assert steps[TC.FULL_FRAME][1]["count"][b] == TC.CAP_D == frames[TC.FULL_FRAME]["det"]["counts"][b]
        n5 = frames[TC.NAN_FRAME]["det"]
        assert np.isnan(n5["boxes"][b, :n5["counts"][b], 0]).sum() == 1
        assert frames[TC.DT0_FRAME]["desc"]["dt"][b] == 0.0 and frames[TC.DT0_FRAME - 1]["desc"]["dt"][b] > 0
        assert frames[TC.RESET_FRAME]["desc"]["flags"][b] == 1
        assert [int(f) for f in (fr["desc"]["flags"][b] for fr in frames)].count(1) == 1
        after = _fields(steps[TC.RESET_FRAME][0], b)
        assert (after["id"] >= 0).sum() == 3 and (after["id"][:3] >= 0).all(), "the reset's births take the lowest slots"
        t9 = steps[TC.RESET_FRAME + 1][1]
        assert t9["det_id"][b, 1] == after["id"][0], "the second tie: slot 0 wins over slot 2"
        assert steps[TC.STATUS_FRAME][1]["count"][b] == 0 and frames[TC.STATUS_FRAME]["status"] != 0
        assert steps[TC.EMPTY_FRAME[b]][1]["count"][b] == 0 and frames[TC.EMPTY_FRAME[b]]["det"]["counts"][b] == 0
    # two objects of different labels within max_dist of each other, each keeping its own track
    det4 = frames[4]["det"]
    n = int(det4["counts"][0])
    xy, la = det4["boxes"][0, :n, :2].astype(np.float64), det4["labels"][0, :n]
    close = [(i, j) for i in range(n) for j in range(n) if la[i] == 0 and la[j] == 1
             and np.hypot(*(xy[i] - xy[j])) < min(TC.SPEC["max_dist"])]
    assert close, "no two objects of different labels pass within max_dist"
    # births are dropped where the table is full, and only there
    assert sum(int(o["dropped"].sum()) for _, o in TC.trace(0, 1)["steps"]) > 0
    assert sum(int(o["dropped"].sum()) for _, o in TC.trace(0, 4)["steps"]) > 0
    assert sum(int(o["dropped"].sum()) for _, o in tr["steps"]) == 0
    # the statement leaves its inputs alone
    again = TC.initial_state(0, cap)
    assert TC.same_bits(again["slots"], tr["state0"]["slots"])


# ---- 3: properties of the statement -------------------------------------------------------------------------------------------
def test_ids_are_unique_and_ascending_in_birth_order():
    for cap in (4, 65):
        tr = TC.trace(0, cap)
        prev = tr["state0"]
        for t, (st, out) in enumerate(tr["steps"]):
            for b in range(TC.B):
                f, fp = _fields(st, b), _fields(prev, b)
                live = f["id"][f["id"] >= 0]
                assert len(set(live.tolist())) == len(live), (cap, t, b)
                born = sorted(set(live.tolist()) - set(fp["id"][fp["id"] >= 0].tolist()))
                assert born == list(range(int(prev["next_id"][b]), int(st["next_id"][b]))), (cap, t, b)
                n = int(out["count"][b])
                new = [i for i in out["det_id"][b, :n].tolist() if i in born]
                assert new == sorted(new), ("births follow the detector's order", cap, t, b)
            prev = st


def _pose(t):
    yaw = 0.04 * t
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0, 1.5 * t], [s, c, 0, 0.04 * t * t], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)


def _world_scene(moving, n_frames=8):
    """three objects at constant world velocity, exact detections in the sensor frame -> (frames, truth velocities per frame)"""
    p0 = np.array([[20.0, 4.0], [35.0, -8.0], [28.0, 12.0]])
    v = np.array([[6.0, -1.0], [-4.0, 2.5], [0.0, 0.0]])
    book = T.TrackBook(1)
    frames, truth = [], []
    for t in range(n_frames):
        pose = _pose(t) if moving else np.eye(4)
        R, o = pose[:2, :2], pose[:2, 3]
        xy = (p0 + v * (t * TC.DT) - o) @ R                                  # R^T (p - o), row-wise
        boxes = np.zeros((1, 4, 7), np.float32)
        boxes[0, :3, :2] = xy
        boxes[0, :3, 2:] = [-1.0, 1.6, 3.9, 1.56, 0.2]
        det = dict(boxes=boxes, scores=np.full((1, 4), 0.8, np.float32), labels=np.zeros((1, 4), np.int32), counts=np.array([3], np.int32))
        d = book.plan([dict(time=t * TC.DT, pose=pose)])
        book.commit(d)
        frames.append((det, d))
        truth.append(v @ R)
    return frames, truth


def test_velocity_of_a_constant_mover_seen_from_a_turning_ego():
    """From the second match on the velocity is the world velocity rotated into the sensor frame.  The bar is float32 rounding
    alone: a coordinate below 70 m is stored to half a spacing, the update divides a difference of such coordinates by dt, and
    the gain folds the error of the velocity before into the same bound -- one spacing of 70 m over dt, 7.6e-5 m/s."""
    bound = float(np.spacing(np.float32(70.0))) / TC.DT
    assert bound <= 1e-4
    frames, truth = _world_scene(moving=True)
    assert max(float(np.abs(f[0]["boxes"][0, :3, :2]).max()) for f in frames) < 70.0
    p = T.check_track(dict(max_dist=2.0, cap=8))
    st = T.empty_state(1, 8)
    worst = 0.0
    for t, (det, d) in enumerate(frames):
        st, out = T.track_host(st, det, d, p)
        assert out["det_id"][0, :3].tolist() == [0, 1, 2] and out["det_hits"][0, :3].tolist() == [t + 1] * 3
        if t >= 2:
            err = float(np.abs(out["det_vel"][0, :3].astype(np.float64) - truth[t]).max())
            worst = max(worst, err)
            assert err <= bound, (t, err, bound)
    print("largest velocity error %.2e m/s (bar %.2e)" % (worst, bound))
    assert float(np.abs(truth[-1] - truth[0]).max()) > 0.5, "the ego does not turn: the rotation of the velocity is untested"


def test_the_same_world_scene_with_and_without_ego_motion_gives_the_same_ids():
    p = T.check_track(dict(max_dist=2.0, cap=8))
    runs = []
    for moving in (False, True):
        st, ids = T.empty_state(1, 8), []
        for det, d in _world_scene(moving)[0]:
            st, out = T.track_host(st, det, d, p)
            ids.append(out["det_id"][0].tolist())
        runs.append(ids)
    assert runs[0] == runs[1] and runs[0][-1][:3] == [0, 1, 2]


def test_a_flagged_frame_changes_nothing_but_the_predicted_poses():
    cap = 65
    tr = TC.trace(0, cap)
    t = TC.STATUS_FRAME
    before, (after, out) = tr["steps"][t - 1][0], tr["steps"][t]
    fr = tr["seq"]["frames"][t]
    assert fr["status"] != 0 and fr["det"]["counts"].min() > 0
    empty = dict(fr["det"], counts=np.zeros(TC.B, np.int32))
    plain, _ = T.track_host(before, empty, fr["desc"], TC.params(cap), status=0)           # a step that only predicts and ages
    moved = 0
    for b in range(TC.B):
        fb, fa, fp = _fields(before, b), _fields(after, b), _fields(plain, b)
        for k in ("id", "label", "hits", "misses", "score"):
            assert TC.same_bits(fa[k], fb[k]), k
        assert TC.same_bits(fa["box"][:, 3:6], fb["box"][:, 3:6])
        live = fb["id"] >= 0
        assert live.sum() >= 2
        assert TC.same_bits(fa["box"][live], fp["box"][live]) and TC.same_bits(fa["vel"][live], fp["vel"][live])
        moved += int((fa["box"][live] != fb["box"][live]).any())
    assert moved >= 1, "the flagged frame predicts nothing: sample 0's ego moves"
    assert TC.same_bits(after["next_id"], before["next_id"])
    assert (out["det_id"] == -1).all() and not out["det_hits"].any() and not out["det_vel"].any()
    assert not out["dropped"].any() and not out["count"].any()


# ---- 4: the switch ------------------------------------------------------------------------------------------------------------
def test_check_track_normalises():
    assert T.check_track(None) is None
    p = T.check_track({})
    assert p == dict(max_dist=(2.0,) * 8, max_age=3, alpha=0.5, cap=256, birth_score=0.0)
    assert T.check_track(p) == p                                                            # idempotent
    q = T.check_track(dict(max_dist=[1, np.float32(0.1)], max_age=np.int64(0), alpha=1, cap=1024, birth_score=0.3))
    assert q["max_dist"] == (1.0, float(np.float32(0.1))) and q["max_age"] == 0 and q["alpha"] == 1.0 and q["cap"] == 1024
    assert q["birth_score"] == float(np.float32(0.3))
    assert T.check_track(dict(max_dist=np.array([0.0, 3.0])))["max_dist"] == (0.0, 3.0)


@pytest.mark.parametrize("spec", [
    "on", 3, [], dict(maxdist=2.0), dict(max_dist=-1.0), dict(max_dist=float("inf")), dict(max_dist=float("nan")),
    dict(max_dist=[]), dict(max_dist=[1.0] * 9), dict(max_dist=[1.0, -0.5]), dict(max_dist="2"), dict(max_dist=True),
    dict(max_dist=None), dict(max_dist=1e39), dict(max_age=-1), dict(max_age=1.5), dict(max_age="3"), dict(max_age=None),
    dict(alpha=0.0), dict(alpha=1.01), dict(alpha=float("nan")), dict(alpha=-0.5), dict(alpha=False), dict(cap=0), dict(cap=1025),
    dict(cap=2.5), dict(cap=True), dict(birth_score=float("nan")), dict(birth_score="0"),
])
def test_check_track_refuses_malformed_specs(spec):
    with pytest.raises(ValueError):
        T.check_track(spec)
    from sassd.stream import FrameStream
    with pytest.raises(ValueError):
        FrameStream({}, inflight=1, points_cap=100, track=spec)                            # refused before any plan is built


# ---- 5: ABI surface, record arithmetic, argument errors -------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "sassd.h")).read()
    for name in ("sassd_track_step", "sassd_track_record_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header), "%s is not declared in include/sassd.h" % name
        assert name in _C.EXPORTS and getattr(C.CDLL(_C.LIB_PATH), name) is not None
    for macro, value in (("SASSD_TRACK_MAGIC", T.TRACK_MAGIC), ("SASSD_TRACK_HEADER_WORDS", T.HEADER_WORDS),
                         ("SASSD_TRACK_SLOT_WORDS", T.SLOT_WORDS), ("SASSD_TRACK_DESC_BYTES", T.DESC_BYTES)):
        assert int(re.search(r"#define\s+%s\s+(\w+)" % macro, header).group(1), 0) == value
    assert "Tracking" in header and "sassd.track.track_host" in header


@pytest.mark.parametrize("B,capD,cap", [(1, 512, 256), (2, 8, 1), (3, 300, 1024), (8, 1, 65)])
def test_record_layout_matches_the_library(B, capD, cap):
    L = T.track_record_layout(B, capD, cap)
    order = ["magic", "seq", "status", "B", "capD", "cap", "count", "dropped", "next_id", "det_id", "det_hits", "det_vel", "slots"]
    size = dict(magic=4, seq=4, status=4, B=4, capD=4, cap=4, count=4 * B, dropped=4 * B, next_id=4 * B, det_id=4 * B * capD,
                det_hits=4 * B * capD, det_vel=8 * B * capD, slots=56 * B * cap)
    assert set(L) == set(order) | {"total"}
    end = 0
    for name in order:
        assert L[name] % 4 == 0 and L[name] >= end, (name, L)
        end = L[name] + size[name]
    assert L["count"] == 4 * T.HEADER_WORDS and L["total"] == end == _C.lib().sassd_track_record_bytes(B, capD, cap)


def test_record_layout_rejects_impossible_shapes():
    lib_ = _C.lib()
    for B, capD, cap in ((0, 8, 4), (1, 0, 4), (1, 8, 0), (1, 8, 1025), (1, T.MAX_CAP_D + 1, 4), (65536, 8, 4)):
        with pytest.raises(ValueError):
            T.track_record_layout(B, capD, cap)
        assert lib_.sassd_track_record_bytes(B, capD, cap) == 0


def test_record_round_trip_and_results():
    cap = 65
    tr = TC.trace(0, cap)
    st, out = tr["steps"][2]                                # frame 2: object A coasts
    rec = T.encode_track_record(st, out, TC.B, TC.CAP_D, cap, seq=3)
    dec = T.decode_track_record(rec, TC.B, TC.CAP_D, cap, 3)
    for k in ("det_id", "det_hits", "det_vel", "dropped", "count"):
        assert TC.same_bits(dec[k], out[k]), k
    assert TC.same_bits(dec["slots"], st["slots"]) and TC.same_bits(dec["next_id"], st["next_id"])
    assert dec["status"] == 0 and dec["seq"] == 3
    for bad in (dict(seq=4), dict(B=1), dict(capD=TC.CAP_D + 1), dict(cap=cap + 1)):
        kw = dict(dict(B=TC.B, capD=TC.CAP_D, cap=cap, seq=3), **bad)
        with pytest.raises((RuntimeError, ValueError), match="stale track record"):
            T.decode_track_record(rec, kw["B"], kw["capD"], kw["cap"], kw["seq"])
    with pytest.raises(RuntimeError, match="stale track record"):
        T.decode_track_record(np.zeros_like(rec), TC.B, TC.CAP_D, cap, 3)
    with pytest.raises(RuntimeError, match="stale track record"):
        T.decode_track_record(rec[:-4], TC.B, TC.CAP_D, cap, 3)
    r = T.results_of(dec, 0)
    k = int(out["count"][0])
    assert set(r) == {"ids", "vel", "hits", "dropped", "coast"} and len(r["ids"]) == k == len(r["hits"]) and r["vel"].shape == (k, 2)
    assert set(r["coast"]) == {"ids", "labels", "boxes", "vel", "misses", "scores"}
    f = _fields(st, 0)
    assert sorted(r["coast"]["ids"].tolist()) == sorted(f["id"][(f["id"] >= 0) & (f["misses"] > 0)].tolist())
    assert len(r["coast"]["ids"]) >= 1 and (r["coast"]["misses"] > 0).all() and r["coast"]["boxes"].shape[1] == 7
    assert not set(r["coast"]["ids"].tolist()) & set(r["ids"].tolist())


def test_entry_point_returns_its_argument_errors_without_a_gpu():
    L = _C.lib()
    p16, null = C.c_void_p(16), None
    md = (C.c_float * 2)(2.0, 1.5)
    need = L.sassd_track_record_bytes(1, 8, 4)

    def call(boxes=p16, scores=p16, labels=p16, counts=p16, B=1, capD=8, seq=p16, status=p16, desc=p16, slots=p16, next_id=p16,
             cap=4, max_dist=md, n=2, max_age=3, alpha=0.5, birth=0.0, record=p16, nbytes=need):
        return L.sassd_track_step(boxes, scores, labels, counts, B, capD, seq, status, desc, slots, next_id, cap, max_dist, n,
                                  max_age, alpha, birth, record, nbytes, null)
    for name in ("boxes", "scores", "labels", "counts", "seq", "status", "desc", "slots", "next_id", "max_dist", "record"):
        assert call(**{name: null}) == EINVAL, name
    for name in ("boxes", "scores", "labels", "counts", "seq", "status", "slots", "next_id", "record"):
        assert call(**{name: C.c_void_p(18)}) == EINVAL, name
    assert call(desc=C.c_void_p(20)) == EINVAL                                  # the descriptors hold float64
    for kw in (dict(B=0), dict(B=65536), dict(capD=0), dict(capD=T.MAX_CAP_D + 1), dict(cap=0), dict(cap=1025), dict(n=0),
               dict(n=9), dict(max_age=-1), dict(alpha=0.0), dict(alpha=1.5), dict(alpha=float("nan")),
               dict(birth=float("nan")), dict(max_dist=(C.c_float * 2)(2.0, -1.0)),
               dict(max_dist=(C.c_float * 2)(float("inf"), 1.0)), dict(max_dist=(C.c_float * 2)(float("nan"), 1.0))):
        assert call(**kw) == EINVAL, kw
    assert call(nbytes=need - 1) == ENOSPC


def test_wrapper_validates_like_its_neighbours():
    import torch
    from sassd import kernels as K
    B, capD, cap = 2, 8, 4
    p = T.check_track(dict(cap=cap))
    good = dict(det=dict(boxes=torch.zeros(B, capD, 7), scores=torch.zeros(B, capD), labels=torch.zeros(B, capD, dtype=torch.int32),
                         counts=torch.zeros(B, dtype=torch.int32)),
                seq=torch.zeros(1, dtype=torch.int32), status=torch.zeros(1, dtype=torch.int32),
                desc=torch.zeros(B * T.DESC_BYTES, dtype=torch.uint8), slots=torch.zeros(B, cap, T.SLOT_WORDS, dtype=torch.int32),
                next_id=torch.zeros(B, dtype=torch.int32), params=p,
                record=torch.zeros(T.track_record_layout(B, capD, cap)["total"], dtype=torch.uint8))
    assert K.track_record_bytes(B, capD, cap) == good["record"].numel()
    with pytest.raises(ValueError):
        K.track_record_bytes(B, capD, 0)
    bad = [dict(det=dict(good["det"], boxes=torch.zeros(B, capD, 6))), dict(det=dict(good["det"], scores=torch.zeros(B, capD + 1))),
           dict(det=dict(good["det"], labels=torch.zeros(B, capD, dtype=torch.int64))),
           dict(det=dict(good["det"], counts=torch.zeros(B + 1, dtype=torch.int32))),
           dict(det=dict(good["det"], boxes=torch.zeros(B, 7, capD).transpose(1, 2))),
           dict(seq=torch.zeros(2, dtype=torch.int32)), dict(status=torch.zeros(1, dtype=torch.int64)),
           dict(desc=torch.zeros(B * T.DESC_BYTES - 1, dtype=torch.uint8)),
           dict(slots=torch.zeros(B, cap + 1, T.SLOT_WORDS, dtype=torch.int32)), dict(next_id=torch.zeros(B, dtype=torch.int64)),
           dict(record=good["record"][:-1]), dict(record=good["record"].view(torch.int32)), dict(params=None),
           dict(params=dict(p, alpha=2.0)), dict(params=dict(p, cap=cap + 1))]
    for kw in bad:
        with pytest.raises(ValueError, match="track"):
            K.track_step(**dict(good, **kw))
    with pytest.raises(RuntimeError, match="CUDA"):                             # every shape is right: only the device is not
        K.track_step(**good)


# ---- 6: the descriptor book ---------------------------------------------------------------------------------------------------
def test_track_book_descriptors_and_commit():
    from sassd.stream import sweep_transform
    book = T.TrackBook(2)
    a, b = _pose(3), _pose(4)
    d0 = book.plan([dict(time=1.0, pose=a), dict(time=5.0)])
    assert d0["flags"].tolist() == [1, 1] and book.prev == [None, None]          # a sample's first frame resets; plan is pure
    assert np.array_equal(d0["T"], T.identity_desc(2)["T"]) and not d0["dyaw"].any() and not d0["dt"].any()
    book.commit(d0)
    d1 = book.plan([dict(time=1.1, pose=b), dict(time=5.25, first=False)])
    assert d1["flags"].tolist() == [0, 0]
    assert np.array_equal(d1["T"][0], sweep_transform(b, a)) and d1["dyaw"][0] == np.arctan2(d1["T"][0, 1, 0], d1["T"][0, 0, 0])
    assert d1["dt"][0] == 1.1 - 1.0 and d1["dt"][1] == 5.25 - 5.0
    assert np.array_equal(d1["T"][1], T.identity_desc(1)["T"][0]) and d1["dyaw"][1] == 0.0      # no pose: exactly [I|0]
    book.commit(d1)
    same = book.plan([dict(time=1.2, pose=b), dict(time=5.5, first=True)])
    assert np.array_equal(same["T"][0], T.identity_desc(1)["T"][0]) and same["dyaw"][0] == 0.0  # equal poses: exactly [I|0]
    assert same["flags"].tolist() == [0, 1] and same["dt"][1] == 0.0
    packed = T.pack_desc(d1)
    assert packed.dtype == np.uint8 and packed.shape == (2 * T.DESC_BYTES,)
    rows = packed.view(T.DESC_DTYPE)
    assert np.array_equal(rows["T"].reshape(2, 3, 4), d1["T"]) and np.array_equal(rows["dt"], d1["dt"])
    assert rows["flags"].tolist() == [0, 0] and not rows["pad"].any()
    prev = list(book.prev)
    for items in (None, [dict(time=1.3)], [dict(time=1.3)] * 3, [dict(time=float("nan")), dict(time=1.0)],
                  [dict(time=float("inf")), dict(time=1.0)], [dict(pose=a), dict(time=1.0)], [dict(time="x"), dict(time=1.0)],
                  [dict(time=1.3, pose=np.eye(3)), dict(time=1.0)], [dict(time=1.3, pose=np.full((4, 4), np.nan)), dict(time=1.0)],
                  [dict(time=1.3, pose="pose"), dict(time=1.0)], [1.3, 1.0], dict(time=1.3)):
        with pytest.raises(ValueError):
            book.plan(items)
    assert len(book.prev) == len(prev) and all(p is q for p, q in zip(book.prev, prev))          # the book is unchanged


# ---- 7: the submit-time errors on FrameRing with a fake slot ------------------------------------------------------------------
class FakeTrackSlot:
    """A slot that checks what _PlanSlot.stage checks for tracking, in its order: which dicts carry pose and time
    (sassd.track.track_items), then the book's plan; the book is committed only behind every check."""

    def __init__(self, log, book, has_sweeps=False):
        self.log, self.book, self.has_sweeps = log, book, has_sweeps
        self.arrived = False

    def stage(self, seq, clouds, frustums=None, calibs=None, sweeps=None, track=None):
        items = T.track_items(self.book is not None, self.has_sweeps, sweeps, track)
        plan = None if self.book is None else self.book.plan(items)
        if len(clouds[0]) > 100:
            raise ValueError("cloud 0 has %d points" % len(clouds[0]))          # a later check: the book must still be unchanged
        if plan is not None:
            self.book.commit(plan)
        self.log.append(("stage", seq, None if plan is None else plan["flags"].tolist()))
        self.seq = seq

    def launch(self):
        self.log.append(("launch", self.seq))

    def ready(self):
        return True

    def wait(self):
        pass

    def record(self):
        return self.seq


def _track_ring(n=2, tracking=True, has_sweeps=False):
    from sassd.stream import FrameRing
    log, book = [], (T.TrackBook(1) if tracking else None)
    return FrameRing([FakeTrackSlot(log, book, has_sweeps) for _ in range(n)], lambda rec, seq: rec), log, book


def test_submit_refuses_bad_track_inputs_before_anything_is_queued():
    ring, log, book = _track_ring()
    cloud = [np.zeros((3, 4), np.float32)]
    a = ring.submit(cloud, track=[dict(time=0.0)])
    assert a == 1 and log == [("stage", 1, [1]), ("launch", 1)]
    prev = list(book.prev)
    del log[:]
    for kw in (dict(), dict(track=[]), dict(track=[dict(time=0.1)] * 2), dict(track=[dict(time=float("nan"))]),
               dict(track=[dict(time=0.1, pose=np.eye(3))]), dict(track=[dict(time=0.1, pose=np.full((4, 4), np.inf))]),
               dict(track=[dict(pose=np.eye(4))])):
        with pytest.raises(ValueError):
            ring.submit(cloud, **kw)
    with pytest.raises(ValueError):
        ring.submit([np.zeros((101, 4), np.float32)], track=[dict(time=0.1)])     # refused by a later check
    assert log == [] and ring.next_ticket == 2 and ring.busy == [a, None]
    assert all(p is q for p, q in zip(book.prev, prev)), "a refused submit changed the book"
    b = ring.submit(cloud, track=[dict(time=0.1, pose=None, first=False)])
    assert b == 2 and log == [("stage", 2, [0]), ("launch", 2)] and book.prev[0][1] == 0.1
    assert ring.collect(a) == 1 and ring.collect(b) == 2


def test_track_given_to_a_stream_without_it_and_next_to_sweeps():
    ring, log, _ = _track_ring(tracking=False)
    cloud = [np.zeros((3, 4), np.float32)]
    with pytest.raises(ValueError, match="built without track"):
        ring.submit(cloud, track=[dict(time=0.0)])
    assert log == [] and ring.submit(cloud) == 1 and log[0] == ("stage", 1, None)
    # a stream with sweeps takes pose, time and `first` from the sweep dicts
    ring, log, book = _track_ring(has_sweeps=True)
    sw = [dict(pose=_pose(0), time=0.0)]
    with pytest.raises(ValueError, match="must not be given"):
        ring.submit(cloud, sweeps=sw, track=[dict(time=0.0)])
    with pytest.raises(ValueError):
        ring.submit(cloud)                                                      # no sweeps: nothing to track by
    assert log == [] and book.prev == [None]
    ring.submit(cloud, sweeps=sw)
    ring.submit(cloud, sweeps=[dict(pose=_pose(1), time=0.1)])
    ring.submit(cloud, sweeps=[dict(pose=_pose(2), time=0.2, first=True)])
    assert [e[2] for e in log if e[0] == "stage"] == [[1], [0], [1]]
    assert np.array_equal(book.prev[0][0], _pose(2)) and book.prev[0][1] == 0.2
