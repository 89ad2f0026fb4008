"""-m gpu: the multi-sweep merge -- sassd_merge_sweeps_dev through ctypes against the numpy oracle of tests/sweeps_cases.py, and
FrameStream(sweeps=3) against a plain FrameStream(ndim=5) that is fed the oracle's merged cloud of every frame.

Equality is the bar everywhere: the merged cloud is defined bit for bit (include/sassd.h "Multi-sweep merge"), the voxelizer's
result is a function of the rows and their order, and everything behind it replays the same kernels on the same inputs."""
import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import _C
from sassd.pipeline import InferencePlan
from sassd.stream import FrameStatusError, FrameStream

import helpers as H
import sweeps_cases as SC

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)
SWEEP_CAP, R, S = 600, 5, 4


# ---- the kernel through the C ABI ---------------------------------------------------------------------------------------------
def _kernel_inputs(ndim, seed=0):
    g = np.random.default_rng(seed + 10 * ndim)
    ring = g.uniform(-70, 70, (R, SWEEP_CAP, ndim)).astype(np.float32)
    ring[2, 5, 0] = ring[2, 6, 2] = ring[2, 7, ndim - 1] = -0.0      # slot 2 is the entry that is copied
    ring[1, 0, 1] = -0.0
    T = np.stack([SC.seeded_transform(seed + s) for s in range(S)])
    dt = g.uniform(0, 0.5, S).astype(np.float32)
    return ring, T, dt


def _run(dev, ring_d, slot, count, xform, T, dt, tf, out_d, status_d):
    """one call on device copies of the descriptors -> (n, status word); `out_d` is written in place"""
    to = lambda a, dt_: torch.from_numpy(np.ascontiguousarray(a, dtype=dt_)).to(dev)      # noqa: E731
    d = [to(slot, np.int32), to(count, np.int32), to(xform, np.int32), to(T, np.float64), to(dt, np.float32)]
    n_d = torch.full((1,), -7, dtype=torch.int32, device=dev)
    rc = _C.lib().sassd_merge_sweeps_dev(_C.ptr(ring_d), ring_d.shape[0], ring_d.shape[1], ring_d.shape[2], _C.ptr(d[0]),
                                         _C.ptr(d[1]), _C.ptr(d[2]), _C.ptr(d[3]), _C.ptr(d[4]), len(slot), int(tf),
                                         _C.ptr(out_d), out_d.shape[0], _C.ptr(n_d), _C.ptr(status_d), _C.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return int(n_d.item()), int(status_d.item())


def _check(dev, ring, slot, count, xform, T, dt, tf, cap_out, out_d=None, before=None):
    """run the kernel and the oracle; `out_d` / `before`: a second call into a buffer whose earlier contents must survive"""
    nd_out = ring.shape[2] + tf
    if out_d is None:
        out_d = torch.full((cap_out, nd_out), float(SENTINEL), device=dev)
        before = np.full((cap_out, nd_out), SENTINEL, np.float32)
    status_d = torch.zeros(1, dtype=torch.int32, device=dev)
    n, st = _run(dev, torch.from_numpy(ring).to(dev), slot, count, xform, T, dt, tf, out_d, status_d)
    want, n_want, flag = SC.merge_oracle(ring, slot, count, xform, T, dt, tf, cap_out)
    got = out_d.cpu().numpy()
    assert n == n_want and st == flag, (n, n_want, st, flag)
    assert got[:n].tobytes() == want.tobytes()
    assert got[n:].tobytes() == before[n:].tobytes(), "rows at and beyond n were written"
    return out_d, got, n, st


CASES = [(nd, tf) for nd in (3, 4, 5) for tf in (0, 1)]


@pytest.mark.parametrize("ndim,tf", CASES)
def test_merge_equals_the_oracle(dev, ndim, tf):
    ring, T, dt = _kernel_inputs(ndim)
    count, xform = (600, 0, 257, 1), (0, 1, 1, 1)
    for third in (-1, 4):
        slot = (2, 0, third, 1)
        out_d, first, n, st = _check(dev, ring, slot, count, xform, T, dt, tf, 1000)
        assert n == (601 if third < 0 else 858) and st == 0
        assert np.signbit(first[5, 0]) and np.signbit(first[6, 2])              # -0.0 survives the copied entry
        if tf:
            assert (first[:600, -1] == dt[0]).all() and first[n - 1, -1] == dt[3]
        # a second call with smaller counts into the same buffer: the rows beyond the new n stay as the first call wrote them
        _, second, n2, _ = _check(dev, ring, slot, (100, 0, 31, 1), xform, T, dt, tf, 1000, out_d, first)
        assert n2 == (101 if third < 0 else 132)


@pytest.mark.parametrize("ndim,tf", CASES)
def test_merge_overflow_absent_slots_and_empty_frames(dev, ndim, tf):
    ring, T, dt = _kernel_inputs(ndim, seed=1)
    xform = (0, 1, 1, 1)
    # 858 rows into 700: the flag, and the first 700 rows of the oracle
    _, _, n, st = _check(dev, ring, (2, 0, 4, 1), (600, 0, 257, 1), xform, T, dt, tf, 700)
    assert n == 700 and st == _C.ST_POINT_OVERFLOW
    # a count above sweep_cap: the flag, 600 rows read
    _, _, n, st = _check(dev, ring, (2, 0, 4, 1), (601, 0, 257, 1), xform, T, dt, tf, 1000)
    assert n == 858 and st == _C.ST_POINT_OVERFLOW
    # slots outside the ring contribute nothing and set no flag
    _, _, n, st = _check(dev, ring, (2, 7, -3, 1), (600, 300, 257, 1), xform, T, dt, tf, 1000)
    assert n == 601 and st == 0
    # nothing at all
    _, got, n, st = _check(dev, ring, (2, 0, 4, 1), (0, 0, 0, 0), xform, T, dt, tf, 1000)
    assert n == 0 and st == 0 and (got == SENTINEL).all()


def test_merge_wrapper_validates_like_its_neighbours(dev):
    from sassd import kernels as K
    ring = torch.zeros(R, SWEEP_CAP, 4, device=dev)
    i32 = lambda: torch.zeros(S, dtype=torch.int32, device=dev)                                 # noqa: E731
    T, dt = torch.zeros(S, 3, 4, dtype=torch.float64, device=dev), torch.zeros(S, device=dev)
    out, one = torch.zeros(100, 5, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    K.merge_sweeps(ring, i32(), i32(), i32(), T, dt, True, out, one, one.clone())
    with pytest.raises(ValueError, match="out"):
        K.merge_sweeps(ring, i32(), i32(), i32(), T, dt, False, out, one, one)                  # 5 columns without a time feature
    with pytest.raises(ValueError, match="T must be"):
        K.merge_sweeps(ring, i32(), i32(), i32(), T.float(), dt, True, out, one, one)
    with pytest.raises(ValueError, match="count must be"):
        K.merge_sweeps(ring, i32(), i32()[:2], i32(), T, dt, True, out, one, one)
    with pytest.raises(ValueError, match="entries"):
        K.merge_sweeps(ring, *(torch.zeros(17, dtype=torch.int32, device=dev) for _ in range(3)),
                       torch.zeros(17, 3, 4, dtype=torch.float64, device=dev), torch.zeros(17, device=dev), True, out, one, one)


# ---- the stream -----------------------------------------------------------------------------------------------------------------
N_SWEEPS, S_STREAM = 7, 3
_SEQ, _WANT = {}, {}


def _case():
    import test_gpu_input_features as TIF
    return TIF._case()                      # a 5-feature car detector, its anchors and safe thresholds (shared with that file)


def _sequence():
    """7 sweeps of 4 columns: the k21 frame, a static scene, seen from a seeded smooth drive; times 0.05 s apart"""
    if not _SEQ:
        poses, times = SC.trajectory(N_SWEEPS, seed=0)
        sweeps = SC.sweeps_of_a_static_scene(H.frame("k21"), poses)
        assert len(sweeps) == N_SWEEPS and all(s.shape[1] == 4 and s.dtype == np.float32 for s in sweeps)
        _SEQ.update(sweeps=sweeps, poses=poses, times=times, sweep_cap=max(len(s) for s in sweeps) + 5)
    return _SEQ


def _starts(first_at):
    """per frame, the sweep its sequence began at"""
    out, start = [], 0
    for t in range(N_SWEEPS):
        if t in first_at:
            start = t
        out.append(start)
    return out


def _merged(first_at=()):
    sq = _sequence()
    return [SC.merge_entries_oracle(SC.frame_entries(sq["sweeps"], sq["poses"], sq["times"], t, S_STREAM, start), True)
            for t, start in enumerate(_starts(first_at))]


def _descr(t, first_at=()):
    sq = _sequence()
    return dict(pose=sq["poses"][t], time=sq["times"][t], first=t in first_at)


def _stream(dev, inflight, points_cap=None, **kw):
    cs, sq = _case(), _sequence()
    cap = 3 * sq["sweep_cap"] if points_cap is None else points_cap
    return FrameStream(cs["sd"], inflight=inflight, points_cap=cap, anchors=cs["an"], anchors_bv=cs["bv"], device=dev,
                       **dict(cs["thr"], **kw))


def _sweeps_stream(dev, inflight, **kw):
    return _stream(dev, inflight, ndim=4, sweeps=S_STREAM, sweep_cap=_sequence()["sweep_cap"], time_feature=True, **kw)


def _want(dev, inflight, first_at=(), annos=False):
    """what a plain FrameStream(ndim=5) returns for the oracle's merged cloud of every frame; computed once per key"""
    key = (inflight, tuple(first_at), annos)
    if key not in _WANT:
        with _stream(dev, inflight, ndim=5, annos=annos) as ref:
            if annos:
                _WANT[key] = [d for _, d in ref.map(([m], None, [_calib()]) for m in _merged(first_at))]
            else:
                _WANT[key] = [d for _, d in ref.map([m] for m in _merged(first_at))]
    return _WANT[key]


def _calib():
    import augment_synth as A
    return dict(calib=A.calib_matrices(), img_shape=(375, 1242))


def _same(got, want, tag):
    assert len(got) == len(want), tag
    for b, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (tag, b)
        if w[0] is None:
            assert all(x is None for x in g), (tag, b)
            continue
        assert g[0] is not None, (tag, b)
        for j, (a, r) in enumerate(zip(g, w)):
            if isinstance(r, dict):
                assert set(a) == set(r), (tag, b, j)
                pairs = [(a[k], r[k]) for k in sorted(r)]
            else:
                pairs = [(a, r)]
            for x, y in pairs:
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (tag, b, j)


@pytest.mark.parametrize("inflight", [1, 3])
def test_sweeps_stream_detects_what_the_merged_clouds_detect(dev, inflight):
    sq = _sequence()
    want, want_first = _want(dev, inflight), _want(dev, inflight, (0, 4))
    n_det = [0 if d[0][0] is None else len(d[0][0]) for d in want]
    print("inflight %d: detections per frame %s, sweeps of %s points" % (inflight, n_det, [len(s) for s in sq["sweeps"]]))
    assert sum(n >= 1 for n in n_det) >= 3, "the plain stream detects in fewer than three frames: the comparison would be empty"
    with _sweeps_stream(dev, inflight) as fs:
        assert fs.sweeps == S_STREAM and tuple(fs.sweep_ring.shape) == (1, S_STREAM + inflight - 1, sq["sweep_cap"], 4)
        assert all(p.sw_ring is fs.sweep_ring for p in fs.plans)
        got = list(fs.map(([sq["sweeps"][t]], None, None, [_descr(t)]) for t in range(N_SWEEPS)))
        assert [t for t, _ in got] == list(range(1, N_SWEEPS + 1))
        for t, (_, d) in enumerate(got):
            _same(d, want[t], ("sequence", inflight, t))
        # the same sweeps once more as two sequences: first=True at the first and at the fifth frame
        tickets = [fs.submit([sq["sweeps"][t]], sweeps=[_descr(t, (0, 4))]) for t in range(N_SWEEPS)]
        for t, ticket in enumerate(tickets):
            _same(fs.collect(ticket), want_first[t], ("first", inflight, t))
        assert all(int(p.status.item()) == 0 for p in fs.plans)


def test_device_clouds_and_a_refused_submit_in_mid_sequence(dev):
    sq = _sequence()
    want = _want(dev, 3, (0,))
    with _sweeps_stream(dev, 3) as fs:
        tickets = []
        for t in range(N_SWEEPS):
            if t == 3:                      # refusals in mid-sequence: nothing queued, no ticket used, the sequence as it was
                nxt, k = fs._ring.next_ticket, fs._book.k
                bad = dict(_descr(t), pose=np.full((4, 4), np.nan))
                for clouds, kw in (([sq["sweeps"][t]], dict(sweeps=[bad])), ([sq["sweeps"][t]], {}),
                                   ([sq["sweeps"][t][:, :3].copy()], dict(sweeps=[_descr(t)])),
                                   ([np.zeros((sq["sweep_cap"] + 1, 4), np.float32)], dict(sweeps=[_descr(t)])),
                                   ([sq["sweeps"][t]], dict(sweeps=[_descr(t), _descr(t)])),
                                   ([sq["sweeps"][t]], dict(sweeps=[dict(_descr(t), time=float("nan"))])),
                                   ([sq["sweeps"][t]], dict(frustums=[np.zeros((6, 4))], sweeps=[_descr(t)]))):
                    with pytest.raises(ValueError):
                        fs.submit(clouds, **kw)
                assert fs._ring.next_ticket == nxt and fs._book.k == k
            cloud = torch.from_numpy(sq["sweeps"][t]).to(dev) if t % 2 else sq["sweeps"][t]     # device and host clouds
            tickets.append(fs.submit([cloud], sweeps=[_descr(t, (0,))]))
        for t, ticket in enumerate(tickets):
            _same(fs.collect(ticket), want[t], ("device / refused", t))
    with _stream(dev, 1, ndim=5) as plain:
        with pytest.raises(ValueError, match="without sweeps"):
            plain.submit([_merged()[0]], sweeps=[_descr(0)])
    cs = _case()
    with pytest.raises(ValueError, match="raw_cap"):
        FrameStream(cs["sd"], inflight=1, points_cap=1024, anchors=cs["an"], anchors_bv=cs["bv"], device=dev, sweeps=3,
                    sweep_cap=512, raw_cap=2048)
    with pytest.raises(ValueError, match="too narrow"):
        FrameStream(cs["sd"], inflight=1, points_cap=1024, anchors=cs["an"], anchors_bv=cs["bv"], device=dev, sweeps=3,
                    sweep_cap=512, time_feature=False)


def test_two_samples_are_two_sequences(dev):
    """batch 2: sample 1 runs the sweeps two places on, on a clock of its own, and starts a new sequence at its fourth frame"""
    sq = _sequence()
    pick = [(t + 2) % N_SWEEPS for t in range(N_SWEEPS)]
    sweeps1, poses1 = [sq["sweeps"][j] for j in pick], [sq["poses"][j] for j in pick]
    times1 = [100.0 + 0.05 * t for t in range(N_SWEEPS)]
    merged0 = _merged()
    merged1 = [SC.merge_entries_oracle(SC.frame_entries(sweeps1, poses1, times1, t, S_STREAM, 3 if t >= 3 else 0), True)
               for t in range(N_SWEEPS)]
    with _stream(dev, 3, ndim=5, batch_size=2) as ref:
        want = [d for _, d in ref.map([merged0[t], merged1[t]] for t in range(N_SWEEPS))]
    assert any(d[1][0] is not None for d in want)
    with _sweeps_stream(dev, 3, batch_size=2) as fs:
        assert tuple(fs.sweep_ring.shape) == (2, S_STREAM + 2, sq["sweep_cap"], 4)
        got = [d for _, d in fs.map(([sq["sweeps"][t], sweeps1[t]], None, None,
                                     [_descr(t), dict(pose=poses1[t], time=times1[t], first=t == 3)]) for t in range(N_SWEEPS))]
    for t in range(N_SWEEPS):
        _same(got[t], want[t], ("batch 2", t))


def test_sweeps_compose_with_annos(dev):
    sq = _sequence()
    want = _want(dev, 3, annos=True)
    assert any(d[0][0] is not None for d in want)
    with _sweeps_stream(dev, 3, annos=True) as fs:
        got = list(fs.map(([sq["sweeps"][t]], None, [_calib()], [_descr(t)]) for t in range(N_SWEEPS)))
    for t, (_, d) in enumerate(got):
        assert len(d[0]) == 4
        _same(d, want[t], ("annos", t))


def test_the_sweeps_frame_holds_kernel_nodes_only(dev):
    import test_gpu_frame_stream_crop as TC
    KERNEL, MEMCPY, MEMSET = 0, 1, 2
    cs, sq = _case(), _sequence()
    kw = dict(batch_size=1, anchors=cs["an"], anchors_bv=cs["bv"], device=dev, overlap=False, **cs["thr"])
    plain, merging = InferencePlan(cs["sd"], **kw), InferencePlan(cs["sd"], **kw)
    cap = 3 * sq["sweep_cap"]
    plain.capture(cap, ndim=5, seal=True)
    ring = torch.zeros(1, 5, sq["sweep_cap"], 4, device=dev)
    merging.capture(cap, ndim=5, seal=True, sweeps=dict(ring=ring, S=S_STREAM, sweep_cap=sq["sweep_cap"], time_feature=True))
    torch.cuda.synchronize()
    base, got = TC._node_types(plain, dev), TC._node_types(merging, dev)
    print("frame graph kernel nodes: %d without sweeps, %d with sweeps" % (base.get(KERNEL, 0), got.get(KERNEL, 0)))
    for counts in (base, got):
        assert counts.get(MEMSET, 0) == 0 and counts.get(MEMCPY, 0) == 0, counts
        assert set(counts) == {KERNEL}, counts
    assert got[KERNEL] == base[KERNEL] + 1                              # one kernel per sample
    with pytest.raises(ValueError, match="raw_cap"):
        InferencePlan(cs["sd"], **kw).capture(cap, ndim=5, seal=True, raw_cap=4096,
                                              sweeps=dict(ring=ring, S=S_STREAM, sweep_cap=sq["sweep_cap"], time_feature=True))
    with pytest.raises(ValueError, match="columns"):
        InferencePlan(cs["sd"], **kw).capture(cap, ndim=6, seal=True,
                                              sweeps=dict(ring=ring, S=S_STREAM, sweep_cap=sq["sweep_cap"], time_feature=True))


def test_point_overflow_belongs_to_its_ticket_and_its_sweep_stays(dev):
    """sweeps of 1000 rows behind one of 3000: the third frame merges 5000 rows into 4999, the fourth 3000 -- and reads the
    sweep that the overflowing frame brought"""
    sq = _sequence()
    sweeps = [np.ascontiguousarray(s[:3000 if t == 0 else 1000]) for t, s in enumerate(sq["sweeps"][:5])]
    assert [len(s) for s in sweeps] == [3000, 1000, 1000, 1000, 1000]
    cap = 4999
    merged = [SC.merge_entries_oracle(SC.frame_entries(sweeps, sq["poses"], sq["times"], t, S_STREAM), True) for t in range(5)]
    assert [len(m) for m in merged] == [3000, 4000, 5000, 3000, 3000]
    with _stream(dev, 3, points_cap=cap, ndim=5) as ref:
        want = {t: ref.collect(ref.submit([merged[t]])) for t in (0, 1, 3, 4)}
    with _sweeps_stream(dev, 3, points_cap=cap) as fs:
        tickets = [fs.submit([sweeps[t]], sweeps=[_descr(t)]) for t in range(5)]
        for t in (0, 1):
            _same(fs.collect(tickets[t]), want[t], ("before", t))
        with pytest.raises(FrameStatusError) as e:
            fs.collect(tickets[2])
        assert e.value.status & _C.ST_POINT_OVERFLOW, hex(e.value.status)
        for t in (3, 4):                                                # ticket 4 runs on slot 0, ticket 5 on slot 1
            _same(fs.collect(tickets[t]), want[t], ("after", t))
        t6 = fs.submit([sweeps[1]], sweeps=[_descr(5, (5,))])           # slot 2 again: recover() cleared its flag
        assert fs.collect(t6) is not None
        assert all(int(p.status.item()) == 0 for p in fs.plans)
