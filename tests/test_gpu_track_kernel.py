"""-m gpu: sassd_track_step alone (include/sassd.h "Tracking") on the seeded sequences of tests/track_cases.py: every case --
slot capacities 1, 4, 64, 65 and 257, with coasting, re-found and dying tracks, births, dropped births, two cost ties, a NaN
x, dt = 0, a reset in mid-sequence, a flagged frame, D = 0, D = capD, a count above capD -- and the crowd (capD = 300, D = 290,
cap = 257 and 1024: more detections than one chunk of 256 threads, more slots than one pass).

The bar is equality of bytes, frame by frame: the device state (slots, next_id) and the whole record equal
sassd.track.track_host's state and sassd.track.encode_track_record of its outputs.  The slot table and the record carry guard
words behind them, which must stay untouched; the detection buffers are only read."""
import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import kernels as K, track as T

import track_cases as TC

pytestmark = pytest.mark.gpu

GUARD_WORDS, SENTINEL = 3 * T.SLOT_WORDS, -0x5A5A5A5B


def _run(dev, tr, cap):
    """the sequence through the kernel, compared with the trace after every frame -> the number of frames compared"""
    p = TC.params(cap)
    frames = tr["seq"]["frames"]
    nb, cap_d = frames[0]["det"]["boxes"].shape[:2]
    n_slots = nb * cap * T.SLOT_WORDS
    slots_buf = torch.full((n_slots + GUARD_WORDS,), SENTINEL, dtype=torch.int32, device=dev)
    slots = slots_buf[:n_slots].view(nb, cap, T.SLOT_WORDS)
    slots.copy_(torch.from_numpy(tr["state0"]["slots"]))
    next_buf = torch.full((nb + 4,), SENTINEL, dtype=torch.int32, device=dev)
    next_id = next_buf[:nb]
    next_id.copy_(torch.from_numpy(tr["state0"]["next_id"]))
    need = K.track_record_bytes(nb, cap_d, cap)
    assert need == T.track_record_layout(nb, cap_d, cap)["total"]
    rec_buf = torch.full((need + 4 * GUARD_WORDS,), 0xA5, dtype=torch.uint8, device=dev)
    record = rec_buf[:need]
    for t, (fr, (st, out)) in enumerate(zip(frames, tr["steps"])):
        det = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in fr["det"].items()}
        seq = torch.tensor([t + 1], dtype=torch.int32, device=dev)
        status = torch.tensor([fr["status"]], dtype=torch.int32, device=dev)
        desc = torch.from_numpy(T.pack_desc(fr["desc"])).to(dev)
        assert K.track_step(det, seq, status, desc, slots, next_id, p, record) is record
        torch.cuda.synchronize()
        tag = (cap, t)
        assert TC.same_bits(slots.cpu().numpy(), st["slots"]), ("slots", tag)
        assert TC.same_bits(next_id.cpu().numpy(), st["next_id"]), ("next_id", tag)
        got = record.cpu().numpy()
        want = T.encode_track_record(st, out, nb, cap_d, cap, seq=t + 1, status=fr["status"])
        if not TC.same_bits(got, want):
            dec = T.decode_track_record(got, nb, cap_d, cap, t + 1)
            ref = T.decode_track_record(want, nb, cap_d, cap, t + 1)
            bad = [k for k in ref if not TC.same_bits(np.asarray(dec[k]), np.asarray(ref[k]))]
            raise AssertionError(("record", tag, bad))
        for k, v in fr["det"].items():
            assert TC.same_bits(det[k].cpu().numpy(), np.ascontiguousarray(v)), ("the detections were written", k, tag)
        assert (slots_buf[n_slots:] == SENTINEL).all() and (next_buf[nb:] == SENTINEL).all(), ("guard words behind the state", tag)
        assert (rec_buf[need:] == 0xA5).all(), ("guard bytes behind the record", tag)
    return len(frames)


@pytest.mark.parametrize("seed,cap", TC.CASES)
def test_kernel_equals_the_statement_frame_by_frame(dev, seed, cap):
    assert _run(dev, TC.trace(seed, cap), cap) == TC.N_FRAMES


@pytest.mark.parametrize("cap", TC.CROWD_CAPS)
def test_crowd_of_more_detections_than_threads(dev, cap):
    tr = TC.crowd_trace(0, cap)
    assert max(int(o["count"].max()) for _, o in tr["steps"]) > 256                     # a second chunk of detections
    assert (cap == 257) == any(int(o["dropped"].sum()) > 0 for _, o in tr["steps"])
    assert _run(dev, tr, cap) == TC.CROWD_FRAMES


def test_tracker_object_steps_and_resets(dev):
    """sassd.track.Tracker: the same bytes through the object, and reset() frees every slot while next_id runs on."""
    seed, cap = 0, 65
    tr = TC.trace(seed, cap)
    trk = T.Tracker(TC.B, TC.CAP_D, dev, **TC.params(cap))
    assert trk.state()["slots"].shape == (TC.B, cap, T.SLOT_WORDS) and (trk.state()["slots"][:, :, T.ID] == -1).all()
    trk.load_state(tr["state0"])
    for t in range(3):
        fr, (st, out) = tr["seq"]["frames"][t], tr["steps"][t]
        det = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in fr["det"].items()}
        rec = trk.step(det, torch.zeros(1, dtype=torch.int32, device=dev), fr["desc"])
        torch.cuda.synchronize()
        assert TC.same_bits(rec.cpu().numpy(), T.encode_track_record(st, out, TC.B, TC.CAP_D, cap))
    before = trk.state()["next_id"].copy()
    trk.reset()
    state = trk.state()
    assert (state["slots"][:, :, T.ID] == -1).all() and TC.same_bits(state["next_id"], before)
