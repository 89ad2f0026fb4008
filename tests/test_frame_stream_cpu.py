"""FrameStream without a GPU: the ABI surface of the frame seal (header, library, binding), the record arithmetic of
sassd.stream.record_layout against the library's own size query, the host decoder on hand-built records, the ring / ordering /
back-pressure / error rules of FrameRing with a fake slot, the seal kernel's device assembly (no float atomics, no scalar
memory writes), and the opt-in wiring of runner.single_test."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import sassd  # noqa: F401
from sassd import _C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
EINVAL, ENOSPC = -1, -2


# ---- ABI surface ------------------------------------------------------------------------------------------------------------
def test_seal_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "sassd.h")).read()
    for name in ("sassd_frame_seal", "sassd_frame_record_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header), "%s is not declared in include/sassd.h" % name
        assert name in _C.EXPORTS, "%s is not bound in _C.py" % name
        assert getattr(C.CDLL(_C.LIB_PATH), name) is not None          # exported by the cross-compiled library
    assert "SASSD_FRAME_MAGIC" in header and "SASSD_FRAME_HEADER_WORDS" in header
    L = _C.lib()
    assert L.sassd_frame_record_bytes(0, 512) == 0 and L.sassd_frame_record_bytes(1, 0) == 0
    assert L.sassd_frame_record_bytes(1 << 13, 1 << 13) == 0           # more rows than a record indexes
    p16, null = C.c_void_p(16), None
    need = L.sassd_frame_record_bytes(1, 512)
    seal = L.sassd_frame_seal
    assert seal(null, p16, p16, p16, 1, 512, p16, p16, p16, need, null) == EINVAL
    assert seal(p16, p16, p16, p16, 1, 512, null, p16, p16, need, null) == EINVAL          # seq comes from memory
    assert seal(p16, p16, p16, p16, 1, 512, p16, null, p16, need, null) == EINVAL          # so does the status snapshot
    assert seal(p16, p16, p16, p16, 1, 512, p16, p16, null, need, null) == EINVAL
    assert seal(p16, p16, p16, p16, 0, 512, p16, p16, p16, need, null) == EINVAL
    assert seal(p16, p16, p16, p16, 1, 512, p16, p16, C.c_void_p(18), need, null) == EINVAL    # record not 4-byte aligned
    assert seal(p16, p16, p16, p16, 1, 512, p16, p16, p16, need - 1, null) == ENOSPC


# ---- record arithmetic ------------------------------------------------------------------------------------------------------
def _plan_cap_d(config):
    from sassd import synth
    return synth.workload(config)["plan"]["cap_d"]


@pytest.mark.parametrize("B", [1, 2, 8])
@pytest.mark.parametrize("config", ["car", "multi"])
def test_record_layout_matches_the_library(B, config):
    from sassd.stream import record_layout, FRAME_MAGIC
    capD = _plan_cap_d(config)
    L = record_layout(B, capD)
    order = ["magic", "seq", "status", "B", "capD", "counts", "boxes", "scores", "labels"]
    size = dict(magic=4, seq=4, status=4, B=4, capD=4, counts=4 * B, boxes=28 * B * capD, scores=4 * B * capD,
                labels=4 * B * capD)
    assert set(L) == set(order) | {"total"}
    end = 0
    for name in order:                       # the header's documented order, 4-byte aligned, nothing overlaps
        assert L[name] % 4 == 0 and L[name] >= end, (name, L)
        end = L[name] + size[name]
    assert [L[k] for k in order[:6]] == [0, 4, 8, 12, 16, 20]
    assert L["boxes"] % 16 == 0 and L["boxes"] - (20 + 4 * B) < 16         # only the header's padding in front of the body
    assert L["scores"] == L["boxes"] + size["boxes"] and L["labels"] == L["scores"] + size["scores"]   # the body is packed
    assert L["total"] == end == _C.lib().sassd_frame_record_bytes(B, capD)
    header = open(os.path.join(ROOT, "include", "sassd.h")).read()
    assert int(re.search(r"#define\s+SASSD_FRAME_MAGIC\s+(0x[0-9a-fA-F]+)", header).group(1), 16) == FRAME_MAGIC


def test_record_layout_rejects_impossible_shapes():
    from sassd.stream import record_layout
    for B, capD in ((0, 512), (1, 0), (1 << 13, 1 << 13)):
        with pytest.raises(ValueError):
            record_layout(B, capD)


# ---- staging block arithmetic -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 3, 8])
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("annos", [False, True])
@pytest.mark.parametrize("seal", [False, True])
def test_stage_layout_arithmetic(B, raw, annos, seal):
    from sassd.stream import stage_layout, CALIB_DOUBLES
    assert CALIB_DOUBLES == 36
    L = stage_layout(B, raw, annos, seal)
    assert set(L) == {"planes", "calib", "words", "seq", "counts", "total"}
    assert L["planes"] == 0
    assert L["calib"] == 192 * B * raw
    assert L["words"] == L["calib"] + 288 * B * annos
    assert L["seq"] == (L["words"] if seal else None)
    assert L["counts"] == L["words"] + 4 * seal
    assert L["total"] == 192 * B * raw + 288 * B * annos + 4 * (B + seal)
    assert L["planes"] % 8 == 0 and L["calib"] % 8 == 0 and L["words"] % 4 == 0
    assert stage_layout(B, raw=raw, annos=annos, seal=seal) == L


def test_stage_layout_rejects_an_empty_batch():
    from sassd.stream import stage_layout
    for B in (0, -1):
        with pytest.raises(ValueError):
            stage_layout(B, True, True, True)


def test_stage_views_alias_the_buffer_at_the_layouts_offsets():
    from sassd.stream import stage_layout, stage_views
    B, guard = 3, 64
    L = stage_layout(B, True, True, True)
    whole = np.full(L["total"] + 2 * guard, 0xA5, np.uint8)
    buf = whole[guard:guard + L["total"]]
    V = stage_views(buf, B, L)
    assert set(V) == {"planes", "calib", "seq", "counts"}
    assert V["planes"].shape == (B, 6, 4) and V["planes"].dtype == np.float64
    assert V["calib"].shape == (B, 36) and V["calib"].dtype == np.float64
    assert V["seq"].shape == (1,) and V["seq"].dtype == np.int32
    assert V["counts"].shape == (B,) and V["counts"].dtype == np.int32
    for v in V.values():
        assert np.shares_memory(v, buf) and np.shares_memory(v, whole)
    planes = 1000.5 + np.arange(B * 24, dtype=np.float64).reshape(B, 6, 4)
    calib = -7.25 - np.arange(B * 36, dtype=np.float64).reshape(B, 36)
    counts = np.asarray([70001, 70002, 70003], np.int32)
    V["planes"][...], V["calib"][...], V["seq"][0], V["counts"][...] = planes, calib, 0x12345678, counts
    raw = whole.tobytes()
    assert np.array_equal(np.frombuffer(raw, np.float64, B * 24, offset=guard + L["planes"]), planes.ravel())
    assert np.array_equal(np.frombuffer(raw, np.float64, B * 36, offset=guard + L["calib"]), calib.ravel())
    assert np.frombuffer(raw, np.int32, 1, offset=guard + L["seq"])[0] == 0x12345678
    assert np.array_equal(np.frombuffer(raw, np.int32, B, offset=guard + L["counts"]), counts)
    assert (whole[:guard] == 0xA5).all() and (whole[guard + L["total"]:] == 0xA5).all()      # nothing outside the block
    assert not (buf == 0xA5).all()
    # the four parts tile the block: every byte of it belongs to exactly one view
    assert sum(v.nbytes for v in V.values()) == L["total"]
    # lesser forms: the absent parts are None, the present ones keep their shapes
    for raw_, annos, seal in ((False, False, False), (False, False, True), (True, False, False), (False, True, True)):
        Lf = stage_layout(B, raw_, annos, seal)
        Vf = stage_views(np.zeros(Lf["total"] + 8, np.uint8), B, Lf)         # a longer buffer is fine
        assert (Vf["planes"] is not None) == raw_ and (Vf["calib"] is not None) == annos and (Vf["seq"] is not None) == seal
        assert Vf["counts"].shape == (B,) and Vf["counts"].dtype == np.int32
        assert raw_ is False or Vf["planes"].shape == (B, 6, 4)
        assert annos is False or Vf["calib"].shape == (B, 36)


# ---- the decoder on hand-built records --------------------------------------------------------------------------------------
def build_record(B, capD, seq, counts, status=0, magic=None, seed=0):
    """A record as the seal kernel writes it (numpy model of the contract) + the detections it holds."""
    from sassd.stream import record_layout, FRAME_MAGIC
    L = record_layout(B, capD)
    r = np.random.default_rng(seed)
    rec = np.zeros(L["total"], np.uint8)
    w = rec.view(np.int32)
    w[0], w[1], w[2], w[3], w[4] = FRAME_MAGIC if magic is None else magic, seq, status, B, capD
    w[5:5 + B] = counts
    boxes = rec[L["boxes"]:L["scores"]].view(np.float32).reshape(B, capD, 7)
    scores = rec[L["scores"]:L["labels"]].view(np.float32).reshape(B, capD)
    labels = rec[L["labels"]:L["total"]].view(np.int32).reshape(B, capD)
    dets = []
    for b, k in enumerate(counts):
        boxes[b, :k] = r.standard_normal((k, 7)).astype(np.float32)
        scores[b, :k] = r.random(k, dtype=np.float32)
        labels[b, :k] = r.integers(0, 3, k)
        dets.append((boxes[b, :k].copy(), scores[b, :k].copy(), labels[b, :k].astype(np.int64)) if k else (None,) * 3)
    return rec, dets


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if w[0] is None:
            assert g == (None, None, None)
            continue
        for a, b in zip(g, w):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
        assert g[0].dtype == np.float32 and g[1].dtype == np.float32 and g[2].dtype == np.int64


def test_decoder_normal_and_zero_detections():
    from sassd.stream import decode_record
    rec, dets = build_record(2, 64, 7, [5, 64])
    got = decode_record(rec, 2, 64, 7)
    _same(got, dets)
    got[0][0][:] = 0                                   # copies: the pinned buffer is reused by the next frame
    _same(decode_record(rec, 2, 64, 7), dets)
    _same(decode_record(rec.tobytes(), 2, 64, 7), dets)
    rec, dets = build_record(2, 64, 8, [0, 3])
    got = decode_record(rec, 2, 64, 8)
    assert got[0] == (None, None, None)
    _same(got, dets)
    rec, dets = build_record(1, 512, 9, [0])
    assert decode_record(rec, 1, 512, 9) == [(None, None, None)]


def test_decoder_rejects_stale_and_foreign_records():
    from sassd.stream import decode_record
    rec, _ = build_record(1, 32, 41, [4])
    with pytest.raises(RuntimeError, match="stale frame record"):
        decode_record(rec, 1, 32, 42)                  # the previous frame's record
    rec, _ = build_record(1, 32, 42, [4], magic=0x12345678)
    with pytest.raises(RuntimeError, match="stale frame record"):
        decode_record(rec, 1, 32, 42)
    with pytest.raises(RuntimeError, match="stale frame record"):
        decode_record(np.zeros_like(rec), 1, 32, 42)   # a buffer nothing was copied into
    rec, _ = build_record(2, 16, 42, [1, 1])
    with pytest.raises(RuntimeError, match="stale frame record"):
        decode_record(rec, 1, 32, 42)                  # a record of another shape
    rec, _ = build_record(1, 32, 42, [4])
    with pytest.raises(RuntimeError, match="stale frame record"):
        decode_record(rec[:-4], 1, 32, 42)             # a buffer shorter than the record
    with pytest.raises(RuntimeError, match="stale frame record"):
        decode_record(b"", 1, 32, 42)


def test_decoder_raises_the_status_error_of_plan_results():
    from sassd.stream import decode_record
    rec, _ = build_record(1, 32, 3, [4], status=_C.ST_BOX_OVERFLOW)
    with pytest.raises(RuntimeError) as e:
        decode_record(rec, 1, 32, 3)
    assert str(e.value) == "sassd pipeline status flags 0x4 (capacity overflow / hash full)"
    src = open(os.path.join(ROOT, "sa-ssd_amd", "pipeline.py")).read()
    assert '"sassd pipeline status flags 0x%x (capacity overflow / hash full)"' in src      # the text results() raises


# ---- ring logic with a fake slot --------------------------------------------------------------------------------------------
class FakeSlot:
    """A slot whose "GPU" finishes a frame when the test says so.  log: the calls, in order, over all slots."""

    def __init__(self, name, log, capD=8, cap=100):
        self.name, self.log, self.capD, self.cap = name, log, capD, cap
        self.rec, self.pending, self.arrived = None, None, False
        self.status, self.recovered, self.closed = 0, 0, False

    def stage(self, seq, clouds):
        if len(clouds[0]) > self.cap:
            raise ValueError("cloud 0 has %d points" % len(clouds[0]))
        self.log.append(("stage", self.name, seq))
        self.seq, self.payload = seq, clouds

    def launch(self):
        self.log.append(("launch", self.name, self.seq))
        n = len(self.payload[0]) % self.capD            # "detections": a function of the input
        self.pending, _ = build_record(1, self.capD, self.seq, [n], status=self.status, seed=len(self.payload[0]))
        self.arrived = False

    def finish(self):
        self.rec, self.arrived = self.pending, True

    def ready(self):
        return self.arrived

    def wait(self):
        self.log.append(("wait", self.name, self.seq))
        self.finish()

    def record(self):
        assert self.arrived
        return self.rec

    def recover(self):
        self.recovered += 1
        self.status = 0

    def close(self):
        self.closed = True


def _ring(n, **kw):
    from sassd.stream import FrameRing, decode_record
    log = []
    slots = [FakeSlot(i, log, **kw) for i in range(n)]
    return FrameRing(slots, lambda rec, seq: decode_record(rec, 1, slots[0].capD, seq)), slots, log


def _expected(npts, capD=8):
    return build_record(1, capD, 0, [npts % capD], seed=npts)[1]


@pytest.mark.parametrize("inflight", [1, 2, 3, 4])
def test_results_come_back_in_submit_order(inflight):
    ring, slots, log = _ring(inflight)
    sizes = [3, 9, 16, 4, 5, 30, 7, 8, 1, 12, 13]
    tickets = [ring.submit([np.zeros((n, 4), np.float32)]) for n in sizes]
    assert tickets == list(range(1, len(sizes) + 1))
    assert ring.in_flight() == inflight
    for t, n in zip(tickets, sizes):
        _same(ring.collect(t), _expected(n))
    assert ring.in_flight() == 0 and not ring.done
    with pytest.raises(KeyError):
        ring.collect(tickets[0])                        # collected already
    # map: the same, lazily
    got = list(ring.map([np.zeros((n, 4), np.float32)] for n in sizes))
    assert [t for t, _ in got] == list(range(len(sizes) + 1, 2 * len(sizes) + 1))
    for (_, d), n in zip(got, sizes):
        _same(d, _expected(n))


def test_inflight_is_limited_to_the_hardware_queues():
    from sassd.stream import FrameRing, FrameStream, MAX_INFLIGHT
    assert MAX_INFLIGHT == 4
    for n in (0, 5):
        with pytest.raises(ValueError):
            FrameRing([FakeSlot(i, []) for i in range(n)], None)
        with pytest.raises(ValueError):
            FrameStream({}, inflight=n, points_cap=100)            # refused before any plan is built
    with pytest.raises(ValueError):
        FrameStream({}, inflight=3, points_cap=None)


def test_submit_on_a_busy_slot_harvests_before_it_restages():
    ring, slots, log = _ring(2)
    t1 = ring.submit([np.zeros((3, 4), np.float32)])
    t2 = ring.submit([np.zeros((5, 4), np.float32)])
    del log[:]
    t3 = ring.submit([np.zeros((6, 4), np.float32)])               # slot 0 again: still busy with ticket 1
    assert log == [("wait", 0, t1), ("stage", 0, t3), ("launch", 0, t3)]
    assert ring.busy == [t3, t2] and list(ring.done) == [t1]
    _same(ring.collect(t1), _expected(3))                          # not overwritten by ticket 3, not skipped
    _same(ring.collect(t3), _expected(6))
    _same(ring.collect(t2), _expected(5))


def test_poll_harvests_only_what_has_arrived():
    ring, slots, log = _ring(3)
    ts = [ring.submit([np.zeros((n, 4), np.float32)]) for n in (1, 2, 3)]
    assert ring.poll() == []
    slots[1].finish()
    del log[:]
    assert ring.poll() == [ts[1]] and ("wait", 1, ts[1]) in log and len(log) == 1
    assert ring.busy == [ts[0], None, ts[2]]
    _same(ring.collect(ts[1]), _expected(2))
    ring.drain()
    assert ring.in_flight() == 0 and sorted(ring.done) == [ts[0], ts[2]]
    assert [c for c in log if c[0] == "wait"][1:] == [("wait", 0, ts[0]), ("wait", 2, ts[2])]     # oldest first


def test_map_never_holds_more_than_inflight_frames():
    for inflight in (1, 2, 3, 4):
        ring, slots, log = _ring(inflight)
        produced, peak = [0], [0]

        def batches():
            for n in range(1, 12):
                produced[0] += 1
                yield [np.zeros((n, 4), np.float32)]

        yielded = 0
        for t, d in ring.map(batches()):
            held = ring.next_ticket - 1 - yielded                   # submitted and not yet handed over, this one included
            assert produced[0] == ring.next_ticket - 1 and held <= inflight and ring.in_flight() <= inflight
            peak[0] = max(peak[0], held)
            yielded += 1
            assert t == yielded
            _same(d, _expected(t))
        assert yielded == 11 and peak[0] == inflight and ring.in_flight() == 0 and not ring.done


def test_an_error_belongs_to_its_ticket():
    ring, slots, log = _ring(3)
    a = ring.submit([np.zeros((3, 4), np.float32)])
    slots[1].status = _C.ST_VOXEL_OVERFLOW                           # the frame on slot 1 ends with a status flag
    b = ring.submit([np.zeros((4, 4), np.float32)])
    c = ring.submit([np.zeros((5, 4), np.float32)])
    _same(ring.collect(a), _expected(3))
    with pytest.raises(RuntimeError, match=r"status flags 0x1 \(capacity overflow / hash full\)"):
        ring.collect(b)
    _same(ring.collect(c), _expected(5))
    assert slots[1].recovered == 1 and slots[0].recovered == slots[2].recovered == 0
    with pytest.raises(KeyError):
        ring.collect(b)                                              # raised once, for that ticket
    d = ring.submit([np.zeros((6, 4), np.float32)])
    e = ring.submit([np.zeros((7, 4), np.float32)])                 # slot 1 again: unaffected
    _same(ring.collect(e), _expected(7))
    _same(ring.collect(d), _expected(6))
    # a stale record: the slot hands back the previous frame's record
    f = ring.submit([np.zeros((2, 4), np.float32)])
    slots[2].pending = build_record(1, 8, f - 1, [1])[0]
    g = ring.submit([np.zeros((1, 4), np.float32)])
    with pytest.raises(RuntimeError, match="stale frame record"):
        ring.collect(f)
    _same(ring.collect(g), _expected(1))
    assert slots[2].recovered == 0 and slots[1].recovered == 1      # only a status flag clears the status word


def test_a_rejected_cloud_queues_nothing_and_costs_no_ticket():
    ring, slots, log = _ring(2, cap=10)
    a = ring.submit([np.zeros((3, 4), np.float32)])
    del log[:]
    with pytest.raises(ValueError):
        ring.submit([np.zeros((11, 4), np.float32)])
    assert not [c for c in log if c[0] in ("stage", "launch")] and ring.busy == [a, None]
    b = ring.submit([np.zeros((4, 4), np.float32)])
    assert b == a + 1 and log[-2:] == [("stage", 1, b), ("launch", 1, b)]
    _same(ring.collect(a), _expected(3))
    _same(ring.collect(b), _expected(4))


def test_close_drains():
    ring, slots, log = _ring(3)
    ts = [ring.submit([np.zeros((n, 4), np.float32)]) for n in (1, 2, 3, 4)]
    ring.close()
    assert ring.in_flight() == 0 and all(s.closed for s in slots) and all(s.arrived for s in slots)
    for t, n in zip(ts, (1, 2, 3, 4)):
        _same(ring.collect(t), _expected(n))                        # what was in flight stays collectable
    with pytest.raises(RuntimeError, match="closed"):
        ring.submit([np.zeros((1, 4), np.float32)])
    ring.close()                                                     # idempotent


def test_map_left_early_leaves_nothing_in_flight():
    ring, slots, log = _ring(3)
    it = ring.map([np.zeros((n, 4), np.float32)] for n in range(1, 9))
    next(it), next(it)
    it.close()
    assert ring.in_flight() == 0 and not ring.done


# ---- the device assembly of the seal kernel ---------------------------------------------------------------------------------
FLOAT_ATOMICS = re.compile(r"global_atomic_add_f32|global_atomic_pk_add_|flat_atomic_add_f32|buffer_atomic_add_f32")
ANY_ATOMIC = re.compile(r"^\s*\w*atomic\w*", re.M)
# a memory write issued by the scalar unit: a scalar mnemonic (s_...) that stores, is an atomic, or writes back / discards the
# scalar data cache
SCALAR_WRITE = re.compile(r"^\s*s_\w*(?:store|atomic|dcache)\w*", re.M)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_seal_kernel_assembly(tmp_path):
    path = os.path.join(ROOT, "sa-ssd_amd", "csrc", "heads.hip")
    asm = str(tmp_path / "heads.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math",
             "-fhip-fp32-correctly-rounded-divide-sqrt", "-ffp-contract=on"]
    subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", path, "-o", asm], check=True, cwd=os.path.dirname(path),
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(asm).read()
    bodies = {}
    for m in re.finditer(r"^(_Z\S+):\s*;", text, re.M):
        bodies[m.group(1)] = text[m.end():text.find(".Lfunc_end", m.end())]
    hits = [s for s in bodies if "frame_seal_kernel" in s]
    assert len(hits) == 1, "frame_seal_kernel not found in heads.hip"
    body = bodies[hits[0]]
    assert not FLOAT_ATOMICS.search(body) and not ANY_ATOMIC.search(body), "the seal kernel holds an atomic"
    assert not SCALAR_WRITE.search(body), "the seal kernel writes memory from the scalar unit"
    assert re.search(r"^\s*global_store_dword", body, re.M), "the seal kernel's vector stores were not found"
    # the guards can see what they look for: the atomic kernels next door hold float atomics
    assert any(FLOAT_ATOMICS.search(b) and ANY_ATOMIC.search(b) for b in bodies.values())


# ---- runner / detector wiring -----------------------------------------------------------------------------------------------
def test_single_test_inflight_defaults_to_zero_and_stays_off_the_stream_module(tmp_path):
    import test_runner_cpu as TR
    from sassd import runner as R
    sig = inspect.signature(R.single_test)
    assert sig.parameters["inflight"].default == 0
    assert "sassd.stream" not in inspect.getsource(R) and "from .stream" not in inspect.getsource(R) \
        and "import stream" not in inspect.getsource(R)
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import sassd, test_runner_cpu as TR\n"
            "from sassd import runner as R\n"
            "out = R.single_test(TR._Model(), TR._DS(5), rank=0, world=1)\n"
            "assert [len(a['name']) for a in out] == [1, 1, 0, 1, 1]\n"
            "assert 'sassd.stream' not in sys.modules, 'the inflight=0 path imported sassd.stream'\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)


def test_single_test_inflight_goes_through_frame_stream(monkeypatch):
    """inflight > 0: raw points of this rank's frames -> model.frame_stream(...).map -> model.result_annos, dataset order."""
    import types
    import test_runner_cpu as TR
    from sassd import kitti_common as kc, runner as R
    seen = {}

    class DS(TR._DS):
        with_point, anchors, anchors_bv, anchor_area_threshold = True, np.zeros((4, 7), np.float32), None, 1
        lidar_prefix = None
        generator = types.SimpleNamespace(voxel_size=[0.05, 0.05, 0.1], point_cloud_range=[0, -40., -3., 70.4, 40., 1.],
                                          max_num_points_per_voxel=5, _max_voxels=20000)

        def _dev(self):
            return "cpu"

        def load_frame(self, idx, with_label=True):
            assert with_label is False
            return dict(sample_idx=idx, img_shape=(375, 1242, 3), calib=None, points=np.full((idx + 1, 4), idx, np.float32))

    class FS:
        def __init__(self, **kw):
            seen.update(kw)
            self.closed = False

        def map(self, batches):
            for t, clouds in enumerate(batches, 1):
                yield t, [(clouds[0], None, None)]

        def close(self):
            self.closed = True

    class Model(TR._Model):
        def frame_stream(self, anchors, **kw):
            seen["anchors"] = anchors
            self.fs = FS(**kw)
            return self.fs

        def result_annos(self, results, img_meta):
            i = img_meta[0]['sample_idx']
            assert results[0][0].shape == (i + 1, 4) and float(results[0][0][0, 0]) == i
            return [dict(kc.empty_result_anno(), tag=i)]

    model = Model()
    out = R.single_test(model, DS(5), rank=0, world=1, inflight=3, points_cap=64, workers=2)
    assert [a["tag"] for a in out] == [0, 1, 2, 3, 4] and model.fs.closed
    assert seen["inflight"] == 3 and seen["points_cap"] == 64 and seen["batch_size"] == 1 and seen["max_voxels"] == 20000
    assert seen["max_num_points"] == 5 and tuple(seen["voxel_size"]) == (0.05, 0.05, 0.1)


def test_detector_frame_stream_takes_its_settings_from_test_cfg(monkeypatch):
    from sassd import stream as S, synth
    model, cfg = synth.build_detector_for(synth.workload("car"), 0)
    seen = {}
    monkeypatch.setattr(S, "FrameStream", lambda sd, **kw: seen.update(kw, n_weights=len(sd)) or "fs")
    an = synth.workload("car")["anchors"]
    assert model.frame_stream(an, points_cap=1000) == "fs"
    tc = model.test_cfg.get('extra', model.test_cfg)
    assert seen["inflight"] == 3 and seen["batch_size"] == 1 and seen["points_cap"] == 1000
    assert seen["score_thr"] == tc.get('score_thr', 0.3) and seen["iou_thr"] == tc.get('nms', {}).get('iou_thr', 0.1)
    assert seen["precision"] == "fp32" and seen["sparse_precision"] == "fp32" and seen["anchors"].shape == (len(an), 7)
    assert seen["num_class"] == 1 and tuple(seen["sparse_shape"]) == tuple(model._cfg["sparse_shape"])
    model.test_cfg['precision'] = "bf16"
    model.frame_stream(an, inflight=2, points_cap=1000, sparse_precision="bf16", score_thr=0.5)
    assert (seen["precision"], seen["sparse_precision"], seen["inflight"], seen["score_thr"]) == ("bf16", "bf16", 2, 0.5)
