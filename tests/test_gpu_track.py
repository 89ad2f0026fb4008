"""-m gpu: tracking through the public interface -- FrameStream(track=...) -- on bench.py's car workload, batch 1.  The cloud
sequence is the 4 seeded car frames and then the same four shifted by 0.3 m along x, seen from an ego that backs off by 0.075 m
a frame while turning a little: a static world, so the tracks born on the first four frames coast for three frames and are
re-found on the shifted ones.

The bar is equality of bytes.  Everything in front of `trk` is what the stream without track= returns; `trk` is
sassd.track.track_host fed with the collected detections in ticket order and with the descriptors sassd.track.TrackBook makes
of the same poses and times; three frames in flight give what one frame in flight gives, which holds only if every step waits
for the one before it on another slot's stream.  A stream with sweeps=2 takes pose, time and `first` from its sweep dicts.
The kernel itself is held to the statement in tests/test_gpu_track_kernel.py."""
import numpy as np
import pytest

import sassd  # noqa: F401
from sassd import track as T
from sassd.stream import FrameStream

import track_cases as TC
import test_gpu_frame_stream as TS

pytestmark = pytest.mark.gpu

SPEC = dict(max_dist=2.0, max_age=3, alpha=0.5, cap=256, birth_score=0.0)
N, DT = 8, 0.1
_CACHE = {}


def _pose(t):
    yaw = 0.002 * t
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0, -0.075 * t], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)


def _items(t, **kw):
    return [dict(time=100.0 + DT * t, pose=_pose(t), **kw)]


def _clouds(w):
    base = [np.ascontiguousarray(w["frame"](i)) for i in range(4)]
    shifted = [p + np.float32([0.3, 0, 0, 0]) for p in base]
    return base + [np.ascontiguousarray(p, np.float32) for p in shifted]


def _stream(dev, inflight, **kw):
    sd, w, _ = TS._workload(dev)
    return FrameStream(sd, inflight=inflight, points_cap=w["points_cap"], batch_size=1, anchors=w["anchors"],
                       anchors_bv=w["anchors_bv"], device=dev, **dict(w["plan"], **kw))


def _plain(dev, inflight):
    """what the stream without track= returns for the 8 clouds (computed once per inflight)"""
    key = ("plain", inflight)
    if key not in _CACHE:
        _, w, _ = TS._workload(dev)
        with _stream(dev, inflight) as fs:
            assert fs.track is None and not hasattr(fs, "tracker")
            _CACHE[key] = [d for _, d in fs.map([p] for p in _clouds(w))]
    return _CACHE[key]


def _det_of(dets, cap_d):
    """collected detections of one frame (batch 1) -> the buffers track_host takes"""
    det = dict(boxes=np.zeros((1, cap_d, 7), np.float32), scores=np.zeros((1, cap_d), np.float32),
               labels=np.zeros((1, cap_d), np.int32), counts=np.zeros(1, np.int32))
    if dets[0][0] is not None:
        k = len(dets[0][0])
        det["boxes"][0, :k], det["scores"][0, :k], det["labels"][0, :k], det["counts"][0] = dets[0][0], dets[0][1], dets[0][2], k
    return det


def _statement(collected, items, cap_d, spec):
    """track_host over the collected frames in ticket order -> the `trk` element of every frame"""
    p = T.check_track(spec)
    book, st, out = T.TrackBook(1), T.empty_state(1, p["cap"]), []
    for dets, it in zip(collected, items):
        d = book.plan(it)
        book.commit(d)
        st, o = T.track_host(st, _det_of(dets, cap_d), d, p)
        out.append(T.results_of(dict(o, slots=st["slots"]), 0))
    return out


def _same_trk(got, want, tag):
    assert set(got) == set(want) == {"ids", "vel", "hits", "dropped", "coast"}, tag
    assert got["dropped"] == want["dropped"], tag
    for k in ("ids", "vel", "hits"):
        assert TC.same_bits(got[k], want[k]), (tag, k)
    for k in want["coast"]:
        assert TC.same_bits(got["coast"][k], want["coast"][k]), (tag, "coast", k)


def _tracked(dev, inflight):
    """the tracking stream over the 8 clouds, every frame checked against the plain stream and the statement"""
    key = ("tracked", inflight)
    if key in _CACHE:
        return _CACHE[key]
    _, w, _ = TS._workload(dev)
    clouds, plain = _clouds(w), _plain(dev, inflight)
    with _stream(dev, inflight, track=SPEC) as fs:
        cap_d = fs.plans[0].capD
        assert fs.track == T.check_track(SPEC) and fs.tracker.cap == SPEC["cap"] and fs.tracker.capD == cap_d
        tickets = []
        for t, p in enumerate(clouds):
            if t == 5:                                  # refusals in mid-sequence: nothing queued, the book as it was
                for kw in (dict(), dict(track=_items(t) * 2), dict(track=[dict(time=float("nan"))]),
                           dict(track=[dict(time=1.0, pose=np.eye(3))])):
                    with pytest.raises(ValueError):
                        fs.submit([p], **kw)
            tickets.append(fs.submit([p], track=_items(t)))
        got = [fs.collect(k) for k in tickets]
        assert tickets == list(range(1, N + 1))
        assert all(int(pl.status.item()) == 0 for pl in fs.plans)
    for t, (g, b) in enumerate(zip(got, plain)):
        assert len(g) == 1 and len(g[0]) == 4, t
        TS._same_dets([g[0][:3]], b, ("detections in front of trk", inflight, t))
    want = _statement(plain, [_items(t) for t in range(N)], cap_d, SPEC)
    for t, (g, r) in enumerate(zip(got, want)):
        _same_trk(g[0][3], r, (inflight, t))
    trks = [g[0][3] for g in got]
    n_det = [len(k["ids"]) for k in trks]
    refound = sum(int((k["hits"] >= 2).sum()) for k in trks[4:])
    coast = [len(k["coast"]["ids"]) for k in trks]
    print("inflight %d: detections per frame %s, re-found on the shifted frames %d, coasting per frame %s"
          % (inflight, n_det, refound, coast))
    assert sum(n_det) >= 4 and all((k["ids"] >= 0).all() for k in trks), "every detection has a track (birth_score 0, cap 256)"
    assert refound >= 1 and max(coast) >= 1, "no track was re-found or none coasts: the comparison is thin"
    moving = [k["vel"][k["hits"] >= 2] for k in trks[4:]]
    assert any(np.abs(v).max() > 0 for v in moving if v.size), "no re-found track has a velocity"
    _CACHE[key] = trks
    return trks


@pytest.mark.parametrize("inflight", [1, 3])
def test_tracking_stream_equals_the_plain_stream_and_the_statement(dev, inflight):
    _tracked(dev, inflight)


def test_three_frames_in_flight_track_as_one(dev):
    one, three = _tracked(dev, 1), _tracked(dev, 3)
    for t, (a, b) in enumerate(zip(one, three)):
        _same_trk(b, a, ("inflight 3 against inflight 1", t))


def test_sweeps_stream_tracks_by_its_sweep_dicts(dev):
    import test_gpu_sweeps as TSW
    sq = TSW._sequence()
    first_at, inflight = (0, 4), 2
    want_dets = TSW._want(dev, inflight, first_at)
    with TSW._sweeps_stream(dev, inflight, track=SPEC) as fs:
        cap_d = fs.plans[0].capD
        with pytest.raises(ValueError, match="must not be given"):
            fs.submit([sq["sweeps"][0]], sweeps=[TSW._descr(0, first_at)], track=_items(0))
        got = list(fs.map(([sq["sweeps"][t]], None, None, [TSW._descr(t, first_at)]) for t in range(TSW.N_SWEEPS)))
    for t, (_, d) in enumerate(got):
        TSW._same([d[0][:3]], want_dets[t], ("sweeps + track: detections", t))
    items = [[dict(time=sq["times"][t], pose=sq["poses"][t], first=t in first_at)] for t in range(TSW.N_SWEEPS)]
    want = _statement(want_dets, items, cap_d, SPEC)
    for t, ((_, d), r) in enumerate(zip(got, want)):
        _same_trk(d[0][3], r, ("sweeps", t))
    ids = [d[0][3]["ids"] for _, d in got]
    assert sum(len(i) for i in ids) >= 3, "the sweeps stream detects too little: the comparison would be empty"
    hits = np.concatenate([d[0][3]["hits"] for _, d in got])
    assert (hits >= 2).any(), "a static scene seen from a known drive: some track must be matched again"
    after = [i for i in ids[4:] if len(i)]
    before = [i for i in ids[:4] if len(i)]
    if after and before:                                # first=True at frame 4: ids run on, none comes back
        assert min(int(i.min()) for i in after) > max(int(i.max()) for i in before)
