"""FrameStream: frames in flight, detections on the host, in order, the pipeline status checked per frame.

The rate README publishes for car_cfg batch 1 comes from three one-branch frame graphs (InferencePlan(overlap=False)) replayed
round-robin on three HIP streams.  This module is that recipe behind a public call, with what a user
needs added: the result leaves the GPU.  Per frame and slot:

  submit   pinned staging block [seq, npts[B] | points] -> one H2D copy per cloud + one for the int block (no fill launches)
           graph.launch()            the captured frame; its last node, sassd_frame_seal, writes the frame record
           one D2H copy              the record -> a pinned host buffer; an event behind it
  collect  event.synchronize()       then decode the record: magic, seq == ticket, status, counts, boxes / scores / labels

The record layout is the contract of include/sassd.h ("Frame record"); `record_layout` is its only Python statement and the
decoder reads nothing else.  Ring order, back-pressure and the error rules live in `FrameRing`, which drives any "slot" with
stage / launch / ready / wait / record -- the CPU tests hand it a fake one.

    fs = FrameStream(state_dict, inflight=3, points_cap=21504, batch_size=1, anchors=an, device=dev)
    for ticket, dets in fs.map(batches):     # dets: what plan.results() returns for that batch
        ...
    fs.close()
"""
from collections import deque

import numpy as np

FRAME_MAGIC = 0x53460001            # SASSD_FRAME_MAGIC: 'S' 'F', layout version 1
MAX_INFLIGHT = 4                    # one HIP stream per frame in flight; the runtime multiplexes a process onto 4 hardware queues
_SEQ_MASK = 0x7FFFFFFF


def record_layout(B, capD):
    """Byte offsets of the frame record for `B` samples x `capD` detection rows (include/sassd.h "Frame record"):
    dict(magic, seq, status, B, capD, counts, boxes, scores, labels, total) -- every field 4-byte aligned, in this order."""
    B, capD = int(B), int(capD)
    if B < 1 or capD < 1 or B * capD > (1 << 24):
        raise ValueError("no frame record for batch %d x capD %d" % (B, capD))
    hdr = (5 + B + 3) // 4 * 4                  # SASSD_FRAME_HEADER_WORDS
    n = B * capD
    boxes = 4 * hdr
    scores = boxes + 4 * 7 * n
    labels = scores + 4 * n
    return dict(magic=0, seq=4, status=8, B=12, capD=16, counts=20, boxes=boxes, scores=scores, labels=labels,
                total=labels + 4 * n)


class FrameStatusError(RuntimeError):
    """A frame whose status word was not zero: the RuntimeError of InferencePlan.results(), with the word in `.status`."""

    def __init__(self, st):
        super().__init__("sassd pipeline status flags 0x%x (capacity overflow / hash full)" % st)
        self.status = int(st)


def status_error(st):
    """The error InferencePlan.results() raises for a non-zero status word."""
    return FrameStatusError(st)


def decode_record(buf, B, capD, seq):
    """One frame record (bytes-like / uint8 array of record_layout(B, capD)['total'] bytes) -> what plan.results() returns:
    per sample (boxes [k,7] f32, scores [k] f32, labels [k] i64), or (None, None, None) for a sample without detections.
    The arrays are copies.  RuntimeError("stale frame record") unless the record carries the magic word, this B / capD and
    `seq`; the status error of plan.results() when its status word is not zero."""
    L = record_layout(B, capD)
    if memoryview(buf).nbytes < L["total"]:
        raise RuntimeError("stale frame record")
    raw = np.frombuffer(buf, dtype=np.uint8, count=L["total"])
    words = raw.view(np.int32)
    n = B * capD
    if (int(words[0]) != FRAME_MAGIC or int(words[3]) != B or int(words[4]) != capD
            or int(words[1]) != (int(seq) & _SEQ_MASK)):
        raise RuntimeError("stale frame record")
    st = int(words[2])
    if st:
        raise status_error(st)
    counts = words[L["counts"] // 4:L["counts"] // 4 + B]
    boxes = raw[L["boxes"]:L["scores"]].view(np.float32).reshape(B, capD, 7)
    scores = raw[L["scores"]:L["labels"]].view(np.float32).reshape(B, capD)
    labels = words[L["labels"] // 4:L["labels"] // 4 + n].reshape(B, capD)
    out = []
    for b in range(B):
        k = min(max(int(counts[b]), 0), capD)
        if k == 0:
            out.append((None, None, None))
        else:
            out.append((boxes[b, :k].copy(), scores[b, :k].copy(), labels[b, :k].astype(np.int64)))
    return out


class FrameRing:
    """Tickets over a ring of slots.  Ticket t (1, 2, ...) runs on slot (t - 1) % len(slots); a slot is

        stage(seq, clouds)   check and queue the inputs of one frame (ValueError for inputs it cannot take: nothing queued)
        launch()             queue the frame and the copy of its record
        ready() / wait()     has the record arrived / block until it has
        record()             the arrived record, valid until the next stage()
        recover()            (optional) called after a record that carried a status flag (FrameStatusError), before the slot
                             is used again

    `decode(record, seq)` turns a record into a result or raises.  A busy slot is harvested -- waited for, decoded, its
    result (or its error) parked under its ticket -- before it is staged again, so a result is neither overwritten nor
    skipped; an error belongs to its ticket alone and is raised by that ticket's collect()."""

    def __init__(self, slots, decode):
        if not 1 <= len(slots) <= MAX_INFLIGHT:
            raise ValueError("inflight must be 1..%d, got %d" % (MAX_INFLIGHT, len(slots)))
        self.slots, self.decode = list(slots), decode
        self.busy = [None] * len(self.slots)        # ticket in flight on each slot
        self.done = {}                              # ticket -> (result, None) | (None, exception)
        self.next_ticket = 1
        self.closed = False

    def in_flight(self):
        return sum(t is not None for t in self.busy)

    def _harvest(self, i):
        slot, t = self.slots[i], self.busy[i]
        slot.wait()
        try:
            self.done[t] = (self.decode(slot.record(), t), None)
        except RuntimeError as e:
            self.done[t] = (None, e)
            recover = getattr(slot, "recover", None)
            if isinstance(e, FrameStatusError) and recover is not None:     # a stale record says nothing about the status word
                recover()
        self.busy[i] = None

    def submit(self, clouds):
        if self.closed:
            raise RuntimeError("FrameStream is closed")
        t = self.next_ticket
        i = (t - 1) % len(self.slots)
        if self.busy[i] is not None:
            self._harvest(i)
        self.slots[i].stage(t & _SEQ_MASK, clouds)     # a ValueError leaves the ticket unused and the slot free
        self.slots[i].launch()
        self.busy[i] = t
        self.next_ticket = t + 1
        return t

    def poll(self):
        """Harvest every frame whose record has arrived -> the tickets that collect() now returns without waiting."""
        for i in sorted(range(len(self.slots)), key=lambda j: self.busy[j] or 0):
            if self.busy[i] is not None and self.slots[i].ready():
                self._harvest(i)
        return sorted(self.done)

    def collect(self, ticket):
        if ticket not in self.done:
            if ticket not in self.busy:
                raise KeyError("ticket %r is unknown or was collected already" % (ticket,))
            self._harvest(self.busy.index(ticket))
        result, err = self.done.pop(ticket)
        if err is not None:
            raise err
        return result

    def drain(self):
        """Wait for everything in flight (oldest first); the results stay collectable."""
        for i in sorted(range(len(self.slots)), key=lambda j: self.busy[j] or 0):
            if self.busy[i] is not None:
                self._harvest(i)

    def map(self, batches):
        """(ticket, result) per batch of `batches`, in order, with at most len(slots) frames submitted and not yet yielded."""
        pending = deque()
        try:
            batches = iter(batches)
            while True:
                if len(pending) == len(self.slots):
                    t = pending.popleft()
                    yield t, self.collect(t)
                try:
                    clouds = next(batches)
                except StopIteration:
                    break
                pending.append(self.submit(clouds))
            while pending:
                t = pending.popleft()
                yield t, self.collect(t)
        finally:
            for t in pending:                           # left early (an error, a break): nothing stays in flight or parked
                try:
                    self.collect(t)
                except RuntimeError:
                    pass

    def close(self):
        if not self.closed:
            self.drain()
            self.closed = True
            for s in self.slots:
                fin = getattr(s, "close", None)
                if fin is not None:
                    fin()


class _PlanSlot:
    """One frame in flight: an InferencePlan captured with the seal as its last node, its HIP stream, a pinned staging block
    [seq, npts[B] | B x points_cap x ndim f32], a pinned record buffer and the event behind the record's copy."""

    def __init__(self, plan, points_cap, ndim):
        import torch
        self.torch, self.plan = torch, plan
        dev, B = plan.dev, plan.B
        self.stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(self.stream):
            plan.capture(points_cap, ndim=ndim, seal=True)
        self.stream.synchronize()
        self.cap, self.ndim = int(points_cap), int(ndim)
        nwords = 1 + B
        self.pin_words = torch.zeros(nwords, dtype=torch.int32).pin_memory()
        self.pin_pts = torch.zeros(B, self.cap, self.ndim, dtype=torch.float32).pin_memory()
        self.pin_rec = torch.zeros(plan.record.numel(), dtype=torch.uint8).pin_memory()
        self.np_words, self.np_pts, self.np_rec = self.pin_words.numpy(), self.pin_pts.numpy(), self.pin_rec.numpy()
        self.event = torch.cuda.Event()
        self.feed = torch.cuda.Event()          # orders device-tensor clouds (produced on the caller's stream) before their copy

    def stage(self, seq, clouds):
        torch, plan = self.torch, self.plan
        if len(clouds) != plan.B:
            raise ValueError("a batch of %d clouds for a stream of batch_size %d" % (len(clouds), plan.B))
        for b, pts in enumerate(clouds):        # never detect on a silently truncated cloud; nothing is queued before this check
            if pts.ndim != 2 or pts.shape[1] != self.ndim:
                raise ValueError("cloud %d has shape %s, expected [N, %d]" % (b, tuple(pts.shape), self.ndim))
            if pts.shape[0] > self.cap:
                raise ValueError("cloud %d has %d points, the stream was sized for %d (points_cap)" % (b, pts.shape[0], self.cap))
        on_dev = [torch.is_tensor(p) and p.is_cuda for p in clouds]
        if any(on_dev):
            self.feed.record(torch.cuda.current_stream(plan.dev))
            self.stream.wait_event(self.feed)
        self.np_words[0] = seq
        with torch.cuda.stream(self.stream):
            for b, pts in enumerate(clouds):
                n = int(pts.shape[0])
                self.np_words[1 + b] = n
                if n == 0:
                    continue
                if on_dev[b]:
                    plan.pts_in[b][:n].copy_(pts, non_blocking=True)
                    pts.record_stream(self.stream)      # the caller may drop the cloud now: its memory is not handed out
                                                        # again before this copy has run
                else:
                    self.np_pts[b, :n] = pts.numpy() if torch.is_tensor(pts) else pts
                    plan.pts_in[b][:n].copy_(self.pin_pts[b, :n], non_blocking=True)
            plan._stage_words.copy_(self.pin_words, non_blocking=True)

    def launch(self):
        torch = self.torch
        with torch.cuda.stream(self.stream):
            self.plan.graph.launch()
            self.pin_rec.copy_(self.plan.record, non_blocking=True)
            self.event.record(self.stream)

    def ready(self):
        return self.event.query()

    def wait(self):
        self.event.synchronize()

    def record(self):
        return self.np_rec

    def recover(self):
        """InferencePlan's status word is sticky and the plan, its kernels and the seal leave it so.  The STREAM clears it, and
        only here: after a frame whose record carried a flag (that frame's collect() raises it), on the slot's stream, in
        front of the slot's next frame -- so that the flag is reported once, by its ticket, and later tickets start clean."""
        with self.torch.cuda.stream(self.stream):
            self.plan.status.fill_(0)

    def close(self):
        self.stream.synchronize()


class FrameStream:
    """`inflight` frames in flight over `inflight` InferencePlans, each captured once with the frame seal as its last node,
    each on its own HIP stream (and no other stream: with inflight > 1 the plans are one-branch, overlap=False; inflight == 1
    keeps the default two-branch plan, which is the faster form for a frame that runs alone -- INTEGRATION section 6).

    submit(clouds) -> ticket; collect(ticket) -> per sample (boxes, scores, labels) exactly as plan.results() returns them;
    map(batches) yields (ticket, detections) in order and keeps `inflight` frames queued; poll() harvests what has arrived;
    drain() waits for everything in flight; close() drains and ends the stream.  `clouds` is a list of batch_size point clouds
    [N, ndim] f32: numpy arrays / CPU tensors (copied through the pinned staging block) or device tensors (copied on the
    slot's stream, after the work queued on the caller's current stream).  Lifetime: a host cloud has been copied out when
    submit() returns; a device cloud is read by a copy that may still be pending then -- the caller may DROP it at once (it is
    recorded on the slot's stream, so the allocator keeps its memory until the copy has run) but must not WRITE into it before
    the ticket has been collected.  A cloud of more than points_cap points raises
    ValueError at submit, before anything is queued.  A frame whose status word is not zero raises plan.results()'s
    RuntimeError from ITS collect(); a record that is not the ticket's own raises RuntimeError("stale frame record").
    `plans` are the InferencePlans (for tools); plan_kwargs go to InferencePlan (precision, sparse_precision, ...)."""

    def __init__(self, state_dict, inflight=3, points_cap=None, batch_size=1, anchors=None, device=None, ndim=4,
                 **plan_kwargs):
        from .pipeline import InferencePlan
        inflight = int(inflight)
        if not 1 <= inflight <= MAX_INFLIGHT:
            raise ValueError("inflight must be 1..%d, got %d" % (MAX_INFLIGHT, inflight))
        if points_cap is None or int(points_cap) < 1:
            raise ValueError("points_cap (the largest cloud the stream accepts) is required")
        if "overlap" in plan_kwargs:
            raise ValueError("FrameStream chooses `overlap` itself: one-branch plans in flight, the two-branch plan alone")
        self.inflight, self.points_cap, self.batch_size = inflight, int(points_cap), int(batch_size)
        self.plans = [InferencePlan(state_dict, batch_size=batch_size, anchors=anchors, device=device,
                                    overlap=inflight == 1, **plan_kwargs) for _ in range(inflight)]
        B, capD = self.plans[0].B, self.plans[0].capD
        self._slots = [_PlanSlot(p, self.points_cap, ndim) for p in self.plans]
        self._ring = FrameRing(self._slots, lambda rec, seq: decode_record(rec, B, capD, seq))

    def submit(self, clouds):
        return self._ring.submit(clouds)

    def collect(self, ticket):
        return self._ring.collect(ticket)

    def map(self, batches):
        return self._ring.map(batches)

    def poll(self):
        return self._ring.poll()

    def drain(self):
        self._ring.drain()

    def close(self):
        self._ring.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
