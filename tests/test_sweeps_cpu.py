"""No GPU: the multi-sweep merge's host side -- the staging block with sweeps, sweep_transform, merge_sweeps_host against the
tests' own oracle (tests/sweeps_cases.py), the descriptor bookkeeping through FrameRing with a fake slot, and the argument
validation of sassd_merge_sweeps_dev.  Every bar is equality except sweep_transform against inv(A) @ B (1e-12 relative: both
are float64 products of a handful of terms)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import sassd  # noqa: F401
from sassd import _C
from sassd import stream as S

import sweeps_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


# ---- staging block ----------------------------------------------------------------------------------------------------------
def _todays_layout(B, raw, annos, seal):
    """stage_layout as it was before sweeps, written out"""
    calib = 192 * B if raw else 0
    words = calib + (8 * 36 * B if annos else 0)
    counts = words + (4 if seal else 0)
    return dict(planes=0, calib=calib, words=words, seq=words if seal else None, counts=counts, total=counts + 4 * B)


@pytest.mark.parametrize("B", [1, 3])
def test_layout_without_sweeps_is_todays(B):
    for raw, annos, seal in itertools.product((False, True), repeat=3):
        want = _todays_layout(B, raw, annos, seal)
        assert S.stage_layout(B, raw, annos, seal, sweeps=0) == want
        assert S.stage_layout(B, raw, annos, seal) == want


@pytest.mark.parametrize("B", [1, 3])
def test_layout_with_sweeps_is_aligned_disjoint_and_covered(B):
    n = 4
    for raw, annos, seal in itertools.product((False, True), repeat=3):
        L = S.stage_layout(B, raw, annos, seal, sweeps=n)
        base = _todays_layout(B, raw, annos, seal)
        size = dict(planes=192 * B * raw, calib=288 * B * annos, sweep_T=96 * B * n, seq=4 * seal, counts=4 * B,
                    sweep_slot=4 * B * n, sweep_count=4 * B * n, sweep_xform=4 * B * n, sweep_dt=4 * B * n)
        for k in ("planes", "calib", "sweep_T"):
            assert L[k] % 8 == 0, (k, L[k])
        assert L["planes"] == base["planes"] and L["calib"] == base["calib"]
        spans = sorted((L[k] if L[k] is not None else L["counts"], size[k]) for k in size)
        at = 0
        for lo, ln in spans:
            assert lo % 4 == 0 and lo >= at, spans          # no two parts overlap
            at = lo + ln
        assert at == L["total"] == sum(size.values())       # and total covers them, without holes
        assert L["words"] == L["sweep_T"] + size["sweep_T"] and (L["seq"] == L["words"] if seal else L["seq"] is None)
    for bad in (-1, 17):
        with pytest.raises(ValueError):
            S.stage_layout(B, sweeps=bad)


def test_stage_views_of_a_sweeps_block():
    B, n, guard = 3, 4, 64
    L = S.stage_layout(B, False, True, True, sweeps=n)
    whole = np.full(L["total"] + 2 * guard, 0xA5, np.uint8)
    buf = whole[guard:guard + L["total"]]
    V = S.stage_views(buf, B, L)
    want = dict(calib=((B, 36), np.float64), seq=((1,), np.int32), counts=((B,), np.int32), sweep_T=((B, n, 3, 4), np.float64),
                sweep_slot=((B, n), np.int32), sweep_count=((B, n), np.int32), sweep_xform=((B, n), np.int32),
                sweep_dt=((B, n), np.float32))
    assert V["planes"] is None and set(V) == set(want) | {"planes"}
    for i, (k, (shape, dt)) in enumerate(want.items()):
        assert V[k].shape == shape and V[k].dtype == dt, k
        V[k][...] = i + 1
    for i, k in enumerate(want):                            # each view aliases its own bytes and nobody else's
        assert (V[k] == i + 1).all(), k
        lo = L[k]
        assert buf[lo:lo + V[k].nbytes].tobytes() == V[k].tobytes(), k
    assert (whole[:guard] == 0xA5).all() and (whole[guard + L["total"]:] == 0xA5).all()
    plain = S.stage_views(np.zeros(64, np.uint8), 1, S.stage_layout(1, seal=True))
    assert set(plain) == {"planes", "calib", "seq", "counts"}


# ---- sweep_transform --------------------------------------------------------------------------------------------------------
def test_sweep_transform_of_equal_poses_is_exactly_the_identity():
    want = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    for seed in range(5):
        P = SC.seeded_pose(seed)
        got = S.sweep_transform(P, P.copy())
        assert got.shape == (3, 4) and got.dtype == np.float64 and got.tobytes() == want.tobytes(), seed


def test_sweep_transform_agrees_with_the_matrix_inverse():
    g = np.random.default_rng(5)
    pts = g.uniform(-80, 80, (200, 3))
    for seed in range(8):
        A, B = SC.seeded_pose(100 + seed), SC.seeded_pose(200 + seed)
        T = S.sweep_transform(A, B)
        assert T.shape == (3, 4) and T.dtype == np.float64
        M = np.linalg.inv(A) @ B
        got, want = pts @ T[:, :3].T + T[:, 3], pts @ M[:3, :3].T + M[:3, 3]
        err = np.abs(got - want).max() / np.abs(want).max()
        assert err <= 1e-12, (seed, err)
    with pytest.raises(ValueError):
        S.sweep_transform(np.eye(3), np.eye(4))


# ---- merge_sweeps_host ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndim,time_feature", [(3, False), (4, True), (4, False), (5, True)])
def test_merge_sweeps_host_equals_the_oracle(ndim, time_feature):
    g = np.random.default_rng(ndim * 2 + time_feature)
    sizes = (257, 0, 64, 1)
    clouds = [g.uniform(-70, 70, (n, ndim)).astype(np.float32) for n in sizes]
    clouds[0][3, 0] = -0.0                                  # the current sweep is copied, not multiplied by an identity
    clouds[0][4, 2] = -0.0
    poses, times = SC.trajectory(4, seed=3)
    ent = [(clouds[0], None, 0.0)] + [(clouds[j], S.sweep_transform(poses[3], poses[3 - j]), np.float32(times[3] - times[3 - j]))
                                      for j in (1, 2, 3)]
    got = S.merge_sweeps_host(ent, time_feature)
    want = SC.merge_entries_oracle(ent, time_feature)
    assert got.dtype == np.float32 and got.shape == want.shape == (sum(sizes), ndim + time_feature)
    assert got.tobytes() == want.tobytes()
    assert np.signbit(got[3, 0]) and np.signbit(got[4, 2])
    if time_feature:
        assert (got[:257, -1] == 0).all() and got[-1, -1] == np.float32(times[3] - times[0])


# ---- descriptor bookkeeping through FrameRing -------------------------------------------------------------------------------
class FakeSweepSlot:
    """A slot that stages the way _PlanSlot does on a sweeps stream -- SweepBook.plan, then commit -- and records the
    descriptors; its frame is over at once."""

    def __init__(self, book, staged):
        self.book, self.staged = book, staged

    def stage(self, seq, clouds, sweeps=None):
        d = self.book.plan(clouds, sweeps)
        self.book.commit(d)
        self.staged.append(dict(d, seq=seq))

    def launch(self):
        pass

    def ready(self):
        return True

    def wait(self):
        pass

    def record(self):
        return None


def _sweeps_ring(S_=3, inflight=2, B=1, cap=100, ndim=4):
    staged = []
    book = S.SweepBook(B, S_, S_ + inflight - 1, cap, ndim, inflight)
    ring = S.FrameRing([FakeSweepSlot(book, staged) for _ in range(inflight)], lambda rec, seq: seq)
    return ring, book, staged


def _submit(ring, poses, times, i, n=None, **kw):
    return ring.submit([np.zeros((10 + i if n is None else n, 4), np.float32)], sweeps=[dict(pose=poses[i], time=times[i], **kw)])


def _check_frame(d, poses, times, i, start, S_=3, R=4, sizes=None):
    """frame of sweep i of a sequence that began at sweep `start` (sweep i sits in ring slot i % R)"""
    past = list(range(i - 1, max(start, i - S_ + 1) - 1, -1))
    size = (lambda j: 10 + j) if sizes is None else sizes
    assert d["write"] == i % R
    assert d["slot"][0].tolist() == [i % R] + [j % R for j in past] + [-1] * (S_ - 1 - len(past)), (i, d["slot"])
    assert d["count"][0].tolist() == [size(i)] + [size(j) for j in past] + [0] * (S_ - 1 - len(past))
    assert d["xform"][0].tolist() == [0] + [1] * len(past) + [0] * (S_ - 1 - len(past))
    assert d["dt"].dtype == np.float32 and d["dt"][0, 0] == 0
    for s, j in enumerate(past, 1):
        assert d["T"][0, s].tobytes() == S.sweep_transform(poses[i], poses[j]).tobytes(), (i, j)
        assert d["dt"][0, s] == np.float32(times[i] - times[j])
    assert d["reads"] == sorted({j % R for j in past})


def test_descriptors_of_a_sequence():
    ring, book, staged = _sweeps_ring()
    poses, times = SC.trajectory(6, seed=1)
    assert [_submit(ring, poses, times, i) for i in range(6)] == [1, 2, 3, 4, 5, 6]
    assert book.R == 4 and len(staged) == 6
    for i, d in enumerate(staged):
        assert d["seq"] == i + 1 and d["k"] == i
        _check_frame(d, poses, times, i, 0)


def test_first_starts_a_new_sequence():
    ring, book, staged = _sweeps_ring()
    poses, times = SC.trajectory(6, seed=2)
    for i in range(6):
        _submit(ring, poses, times, i, **(dict(first=True) if i == 3 else {}))
    for i, d in enumerate(staged):
        _check_frame(d, poses, times, i, 3 if i >= 3 else 0)
    assert staged[3]["slot"][0].tolist() == [3, -1, -1] and staged[3]["reads"] == []


def test_a_refused_submit_leaves_the_sequence_as_it_was():
    ring, book, staged = _sweeps_ring(cap=50)
    poses, times = SC.trajectory(6, seed=3)
    bad_pose = poses[3].copy()
    bad_pose[1, 2] = np.nan
    for i in range(3):
        _submit(ring, poses, times, i)
    state = lambda: (book.k, [[(e[0], e[1].tobytes(), e[2], e[3]) for e in h] for h in book.hist], ring.next_ticket)  # noqa: E731
    before = state()
    cloud = np.zeros((13, 4), np.float32)
    good = dict(pose=poses[3], time=times[3])
    refusals = [
        lambda: ring.submit([cloud], sweeps=[]),                                            # miscounted
        lambda: ring.submit([cloud], sweeps=[good, good]),
        lambda: ring.submit([cloud, cloud], sweeps=[good]),
        lambda: ring.submit([cloud], sweeps=[dict(pose=bad_pose, time=times[3])]),          # not finite
        lambda: ring.submit([cloud], sweeps=[dict(pose=np.eye(3), time=times[3])]),         # not 4x4
        lambda: ring.submit([cloud], sweeps=[dict(pose=poses[3], time=float("inf"))]),
        lambda: ring.submit([cloud], sweeps=[dict(pose=poses[3])]),                         # no time
        lambda: ring.submit([np.zeros((51, 4), np.float32)], sweeps=[good]),                # above sweep_cap
        lambda: ring.submit([np.zeros((13, 5), np.float32)], sweeps=[good]),                # the wrong width
        lambda: ring.submit([cloud]),                                                       # missing
    ]
    for i, refuse in enumerate(refusals):
        with pytest.raises(ValueError):
            refuse()
        assert state() == before and len(staged) == 3, i
    for i in range(3, 6):
        _submit(ring, poses, times, i)
    assert [d["seq"] for d in staged] == [1, 2, 3, 4, 5, 6]
    for i, d in enumerate(staged):
        _check_frame(d, poses, times, i, 0)


def test_samples_are_sequences_of_their_own():
    ring, book, staged = _sweeps_ring(B=2)
    pa, ta = SC.trajectory(4, seed=4)
    pb, tb = SC.trajectory(4, seed=5)
    for i in range(4):
        ring.submit([np.zeros((10 + i, 4), np.float32), np.zeros((20 + i, 4), np.float32)],
                    sweeps=[dict(pose=pa[i], time=ta[i]), dict(pose=pb[i], time=tb[i], first=i == 2)])
    d = staged[3]
    assert d["slot"].tolist() == [[3, 2, 1], [3, 2, -1]] and d["count"].tolist() == [[13, 12, 11], [23, 22, 0]]
    assert d["T"][1, 1].tobytes() == S.sweep_transform(pb[3], pb[2]).tobytes()
    assert d["T"][0, 2].tobytes() == S.sweep_transform(pa[3], pa[1]).tobytes()


def test_the_ring_passes_sweeps_as_a_keyword_and_only_when_given():
    calls = []

    class Slot(FakeSweepSlot):
        def stage(self, seq, *a, **kw):
            calls.append((a, kw))

    ring = S.FrameRing([Slot(None, None)], lambda rec, seq: seq)
    ring.submit(["c"])
    ring.submit(["c"], None, None, "sw")
    got = list(ring.map([(["c"], None, None, "sw2"), ["d"]]))
    assert [t for t, _ in got] == [3, 4]
    assert calls == [((["c"],), {}), ((["c"],), dict(sweeps="sw")), ((["c"],), dict(sweeps="sw2")), ((["d"],), {})]


def test_a_ring_that_is_too_short_is_refused():
    with pytest.raises(AssertionError):
        S.SweepBook(1, 3, 4, 100, 4, inflight=3)            # needs 3 + 3 - 1 = 5 slots
    S.SweepBook(1, 3, 5, 100, 4, inflight=3)
    for bad in (0, 17):
        with pytest.raises(ValueError):
            S.SweepBook(1, bad, 20, 100, 4)


def test_frame_stream_signature_carries_sweeps():
    import inspect
    from sassd.pipeline import InferencePlan
    p = inspect.signature(S.FrameStream.__init__).parameters
    assert p["sweeps"].default is None and p["sweep_cap"].default is None and p["time_feature"].default is True
    assert inspect.signature(S.FrameStream.submit).parameters["sweeps"].default is None
    assert inspect.signature(InferencePlan.capture).parameters["sweeps"].default is None


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_merge_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "sassd.h")).read()
    name = "sassd_merge_sweeps_dev"
    assert re.search(r"\b%s\s*\(" % name, header), "%s is not declared in include/sassd.h" % name
    assert name in _C.EXPORTS, "%s is not bound in _C.py" % name
    assert getattr(C.CDLL(_C.LIB_PATH), name) is not None


def test_merge_argument_validation_returns_einval():
    merge, p16, null = _C.lib().sassd_merge_sweeps_dev, C.c_void_p(16), None
    #       ring R  sweep_cap ndim slot count xform T    dt   S  tf out  cap_out n_out status stream
    good = [p16, 5, 600,      4,   p16, p16,  p16,  p16, p16, 4, 1, p16, 1000,   p16,  p16,   null]
    for i in (0, 4, 5, 6, 7, 8, 11, 13, 14):                            # every pointer is required
        args = list(good)
        args[i] = null
        assert merge(*args) == EINVAL, i
    for i, v in ((9, 0), (9, 17), (9, -1), (1, 0), (2, 0), (12, 0), (12, -5), (3, 2)):     # S, R, sweep_cap, cap_out, ndim_in
        args = list(good)
        args[i] = v
        assert merge(*args) == EINVAL, (i, v)
    args = list(good)
    args[7] = C.c_void_p(20)                                            # T is float64: 8-byte aligned
    assert merge(*args) == EINVAL
    for i in (0, 4, 5, 6, 8, 11, 13, 14):                               # every other pointer: 4-byte aligned
        args = list(good)
        args[i] = C.c_void_p(18)
        assert merge(*args) == EINVAL, i
