"""k_replay_fast's uniform loop (replay_fast.inc, CDR_FAST_UNI): slices whose rows carry one
type_flags word on every lane, the hand-over to the per-lane loop where a lane starts to differ,
a lane that fails while the rows stay uniform, missing lanes, and the TASKS instantiation.  One
fast slice per launch, <= 64 workflows of <= 40 events, against the CPU restatement."""
import ctypes as C
import functools

import numpy as np
import pytest

from cadence_amd import abi, engine, ndc
from .test_operand_hints_gpu import T0, Hist, build, check, run_sliced

gpu = pytest.mark.gpu
FD = 2  # replay_fast.inc CDR_FDEPTH: the loops run groups of FD rows
N = 11  # rows of the hand-over slice: its last group (rows 9, 10) is a whole group


class UHist(Hist):
    """A Hist whose timestamps, task ids, first event id and activity names are the lane's own;
    `ver` is the version of the events added next, `gap_row` the row whose id skips two."""

    def __init__(self, lane=0, base=0, gap_row=None):
        self.lane, self.base, self.ver, self.gap_row, self.aid = lane, base, 1, gap_row, None
        super().__init__()

    def add(self, name, gap=0, same_call=False, **attrs):
        if not self.calls:
            self.id = self.base
        if self.n == self.gap_row:
            gap += 2
        if name == "ActivityTaskScheduled":
            self.aid = attrs["activityId"] = f"L{self.lane}-{attrs['activityId']}"
        self.id += 1 + gap
        e = dict(eventId=self.id, version=self.ver, timestamp=T0 + self.lane * 1000 + self.id * 10 ** 9,
                 taskId=100 + self.id + 7 * self.lane, eventType=name,
                 **{name[0].lower() + name[1:] + "EventAttributes": attrs})
        if same_call and self.calls:
            self.calls[-1].append(e)
        else:
            self.calls.append([e])
        return self.id

    def done_decision(self, checksum="ck", **kw):
        s, st = self.decision(**kw)
        return self.complete_decision(s, st, checksum=checksum)

    def cut(self, n):
        """Keep the first n events."""
        calls, left = [], n
        for c in self.calls:
            if left <= 0:
                break
            calls.append(c[:left])
            left -= len(c)
        self.calls = calls
        self.id = calls[-1][-1]["eventId"]
        return self


# ---------------------------------------------------------------- 1. shapes that stay uniform
def s_signal_cancel_marker(h):
    h.done_decision()
    h.add("WorkflowExecutionSignaled")
    h.add("WorkflowExecutionCancelRequested")
    h.add("MarkerRecorded")
    h.activity()
    h.add("WorkflowExecutionCompleted")


def _transient(h, name, **attrs):
    s, st = h.decision()
    h.add(name, scheduledEventId=s, startedEventId=st, **attrs)
    s, st = h.decision(attempt=1)  # the transient decision's real events
    h.complete_decision(s, st)


def s_decision_failed(h):
    _transient(h, "DecisionTaskFailed")
    h.activity(close="ActivityTaskFailed")
    h.add("WorkflowExecutionFailed")


def s_decision_timed_out(h):
    _transient(h, "DecisionTaskTimedOut", timeoutType="START_TO_CLOSE")
    h.activity(close="ActivityTaskTimedOut")
    h.add("WorkflowExecutionTimedOut")


def s_activity_canceled(h):
    h.done_decision()
    s = h.activity(close=None)
    h.add("ActivityTaskCancelRequested", activityId=h.aid)
    h.add("ActivityTaskCanceled", scheduledEventId=s, startedEventId=s + 1)
    h.add("WorkflowExecutionCancelRequested")
    h.add("WorkflowExecutionCanceled")


def s_pending_heartbeat(h):
    h.done_decision()
    h.activity()
    h.done_decision()
    h.activity(close=None, hb=3)


def s_terminated(h):
    h.done_decision()
    h.activity(signals=2)
    h.add("WorkflowExecutionTerminated")


def s_version_bump(h):  # a new VersionHistory item on every lane in one row
    h.done_decision()
    h.ver = 2
    h.activity()
    h.ver = 5
    h.done_decision()
    h.add("WorkflowExecutionSignaled")


def s_id_gap(h):
    h.done_decision()
    h.activity(gap=2)
    h.done_decision(gap=3)
    h.activity()


def s_checksums(h):  # more distinct checksums than the kernel caches: the deep lookup, and a repeat
    for j in range(11):
        h.done_decision(checksum=f"ck{j}")
    h.done_decision(checksum="ck9")


def _pad(n):
    def f(h):
        h.pad_to(n)
    f.__name__ = f"s_len{n}"
    return f


def s_even_rows(h):  # srows - 1 at the other residue mod FD than s_pending_heartbeat's
    s_pending_heartbeat(h)
    h.add("WorkflowExecutionSignaled")


SHAPES = [s_signal_cancel_marker, s_decision_failed, s_decision_timed_out, s_activity_canceled, s_pending_heartbeat,
          s_even_rows, s_terminated, s_version_bump, s_id_gap, s_checksums, _pad(2), _pad(3), _pad(4), _pad(5)]


def lanes(shape, n=64, base=lambda i: 0):
    hs = []
    for i in range(n):
        h = UHist(lane=i, base=base(i))
        shape(h)
        hs.append(h)
    assert max(h.n for h in hs) <= 40
    return hs


class Case:
    def __init__(self, hists):
        import oracle
        self.batch = build(hists)
        self.pl = engine.plan(self.batch)
        self.ref = oracle.replay(self.batch, self.pl, tasks=True)


@functools.lru_cache(maxsize=None)
def uniform_case(i):
    # every fourth shape with a first event id of the lane's own (not the transient decisions':
    # an attempt of 1 is a hinted operand at some ids and not at others); the cancel request's
    # operand is a string handle, a small number: ids from a million keep it (and the arena offsets) from looking hinted
    base = (lambda l: 3 * l) if i % 4 == 0 else (lambda l: 10 ** 6) if SHAPES[i] is s_activity_canceled else (lambda l: 0)
    return Case(lanes(SHAPES[i], base=base))


def run_and_check(eng, c, tasks, skip=None, masked=()):
    got = run_sliced(eng, c.batch, c.pl, tasks=tasks, skip=skip, want_fast=(1, 1))
    check(c, got, skip=masked)
    if tasks:
        bad = [m for m in engine.compare_tasks(c.batch, got, c.ref) if int(m.split()[1].rstrip(":")) not in masked]
        assert not bad, "\n".join(bad[:8])
        assert sum(got.tasks["n"]) > 0
    return got


def host_type_flags(c):
    """(fast slices, slices, type_flags[rows, 64], lane_wf) of the case as the host planner and
    packer lay it out (no device)."""
    L = abi.lib()
    b, n = c.batch, c.batch.n_wfs
    ns, rows, nw = C.c_uint32(), C.c_uint64(), C.c_uint32()
    assert L.cdr_plan_slices_ex(b.wfs, c.pl.caps, n, 0, None, None, None, None, C.byref(ns), C.byref(rows), C.byref(nw)) == 0
    lane, slen = np.zeros(ns.value * 64, np.int32), np.zeros(ns.value, np.uint32)
    row0, flags = np.zeros(ns.value, np.uint64), np.zeros(ns.value, np.uint32)
    L.cdr_plan_slices_ex(b.wfs, c.pl.caps, n, 0, lane.ctypes.data, slen.ctypes.data, row0.ctypes.data, flags.ctypes.data,
                         C.byref(ns), C.byref(rows), C.byref(nw))
    bs = b.cstruct()
    slab = np.zeros(int(rows.value) * abi.ROW_BYTES, np.uint8)
    arena = np.zeros(max(1, L.cdr_plan_arena_words(C.byref(bs))), np.uint64)
    s = abi.CdrSlices(n_slices=ns.value, n_rows=rows.value, arena_words=len(arena))
    s.slice_row0, s.slice_len, s.lane_wf = row0.ctypes.data, slen.ctypes.data, lane.ctypes.data
    s.slab, s.arena, s.slice_flags = slab.ctypes.data, arena.ctypes.data, flags.ctypes.data
    assert L.cdr_pack_slices(C.byref(bs), C.byref(s), 0) == 0
    sc = [np.zeros(ns.value, dt) for dt in (np.uint64, np.uint32, np.uint32)]
    words, nf = C.c_uint64(), C.c_uint32()
    assert L.cdr_plan_scratch(c.pl.caps, lane.ctypes.data, ns.value, sc[0].ctypes.data, sc[1].ctypes.data, sc[2].ctypes.data,
                              flags.ctypes.data, C.byref(words), C.byref(nf)) == 0
    tf = abi.slab_columns(slab, row0, slen, ("type_flags",))["type_flags"].reshape(-1, 64)
    return nf.value, ns.value, tf, lane


def test_the_shapes_pack_to_uniform_rows():
    """The premise of the GPU cases below, on the host: each shape is one fast slice whose every
    row after the first carries one type_flags word on all 64 lanes; between them the rows hold
    every fast-path event type, both residues of srows - 1 mod FD, and histories of 2 to 5 events."""
    types, residues, lens = set(), set(), set()
    for i in range(len(SHAPES)):
        nf, ns, tf, _ = host_type_flags(uniform_case(i))
        assert (nf, ns) == (1, 1), SHAPES[i].__name__
        assert (tf[1:] == tf[1:, :1]).all(), SHAPES[i].__name__  # (row 0, Started, is peeled off the loops)
        types |= set((tf[:, 0] & 0xFF).tolist())
        residues.add((len(tf) - 1) % FD)
        lens.add(len(tf))
    want = ["WorkflowExecutionSignaled", "WorkflowExecutionCancelRequested", "MarkerRecorded", "DecisionTaskFailed",
            "DecisionTaskTimedOut", "ActivityTaskCancelRequested", "ActivityTaskCanceled", "ActivityTaskFailed",
            "ActivityTaskTimedOut", "ActivityTaskCompleted", "WorkflowExecutionCompleted", "WorkflowExecutionFailed",
            "WorkflowExecutionTimedOut", "WorkflowExecutionCanceled", "WorkflowExecutionTerminated"]
    assert {abi.EV[t] for t in want} <= types
    assert residues == set(range(FD)) and {2, 3, 4, 5} <= lens


@gpu
@pytest.mark.parametrize("tasks", [False, True], ids=["states", "tasks"])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[s.__name__ for s in SHAPES])
def test_uniform_to_the_end(engine_gpu, i, tasks):
    c = uniform_case(i)
    assert all(c.ref.result[w].code == abi.OK for w in range(64))
    run_and_check(engine_gpu, c, tasks)


def run_with_last_decision(eng, c):
    """run_sliced with cdr_out.last_decision set: the kernel then writes applyEvents' lastDecision
    (the capture before a clearing event inside the loop, and the record after it)."""
    dev = ndc._Dev()
    try:
        n = c.batch.n_wfs
        db = ndc.upload_batch(dev, c.batch, c.pl.caps, 0, False)
        assert (db.n_fast_slices, db.ev.n_slices) == (1, 1)
        o = ndc.alloc_out(dev, n, c.pl.totals)
        o.last_decision = dev.alloc(n * C.sizeof(abi.CdrLastDecision))
        assert abi.lib().cdr_replay_sliced_async(eng.ctx, C.byref(db), C.byref(o), None) == 0
        out = ndc.download_out(dev, o, n, c.pl)  # (synchronises)
        dev.down(out.last_decision, o.last_decision)
        return out
    finally:
        dev.close()


def _sched(h, **kw):
    return h.add("DecisionTaskScheduled", attempt=0, startToCloseTimeoutSeconds=10, taskList={"name": "tl"}, **kw)


def s_ld_scheduled(h):  # the last call is a DecisionTaskScheduled
    h.done_decision()
    h.activity()
    _sched(h)


def s_ld_started(h):  # ... a DecisionTaskStarted
    h.done_decision()
    h.activity()
    h.decision()


def s_ld_captured(h):  # Scheduled, Started and the clearing Completed in one call: the in-loop capture
    h.done_decision()
    s = _sched(h)
    st = h.add("DecisionTaskStarted", same_call=True, scheduledEventId=s, requestId="rq")
    h.add("DecisionTaskCompleted", same_call=True, scheduledEventId=s, startedEventId=st, binaryChecksum="ck")
    h.add("WorkflowExecutionSignaled", same_call=True)


def s_ld_transient(h):  # DecisionTaskFailed last in its call: the transient decision
    h.done_decision()
    s = _sched(h)
    st = h.add("DecisionTaskStarted", same_call=True, scheduledEventId=s, requestId="rq")
    h.add("DecisionTaskFailed", same_call=True, scheduledEventId=s, startedEventId=st)


def s_ld_reset(h):  # a decision in the call before the last: the call boundary clears it
    h.done_decision()
    h.decision()
    h.add("WorkflowExecutionSignaled")


LD_SHAPES = [s_ld_scheduled, s_ld_started, s_ld_captured, s_ld_transient, s_ld_reset]
LD_SOURCES = {"s_ld_scheduled": abi.LD_SCHEDULED, "s_ld_started": abi.LD_STARTED, "s_ld_captured": abi.LD_STARTED,
              "s_ld_transient": abi.LD_TRANSIENT, "s_ld_reset": 0}


@functools.lru_cache(maxsize=None)
def ld_case(i):
    return Case(lanes(LD_SHAPES[i]))


def test_the_last_decision_shapes_pack_to_uniform_rows():
    for i, shape in enumerate(LD_SHAPES):
        c = ld_case(i)
        nf, ns, tf, _ = host_type_flags(c)
        assert (nf, ns) == (1, 1) and (tf[1:] == tf[1:, :1]).all(), shape.__name__
        assert {c.ref.last_decision[w].source for w in range(64)} == {LD_SOURCES[shape.__name__]}, shape.__name__


@gpu
@pytest.mark.parametrize("i", range(len(LD_SHAPES)), ids=[s.__name__ for s in LD_SHAPES])
def test_last_decision_in_uniform_rows(engine_gpu, i):
    """The uniform step's call-boundary reset of the lastDecision bookkeeping, its sources and its
    capture before a clearing event: states and lastDecision records equal the oracle's."""
    c = ld_case(i)
    got = run_with_last_decision(engine_gpu, c)
    bad = engine.compare(c.batch, got, c.ref, limit=10 ** 6)
    assert not bad, "\n".join(bad[:8])


# ---------------------------------------------------------------- 2. where the hand-over happens
def s_base(h):  # Started, decision (3 rows), activity (3 rows), signals
    h.done_decision()
    h.activity()
    h.pad_to(N)


def differing(kind, lane, r):
    """The lane's history, equal to the others' on rows < r and different from row r on; as long
    as theirs and with an activity too unless it ends at r, so that the planner leaves it in its
    lane (it orders a slice's lanes by working slots, then length, and is stable)."""
    if kind == "gap":
        h = UHist(lane=lane, gap_row=r)
        s_base(h)
        return h
    h = UHist(lane=lane)
    s_base(h)
    h.cut(r)  # "ends": the history stops before row r
    if kind == "type":
        while h.n < (N - 3 if r <= 4 else N):
            h.add("MarkerRecorded")
        if r <= 4:
            h.activity()
    return h


KINDS = ("type", "gap", "ends")
# (the planner puts the shortest history of a slice in its last lane)
HANDOVER = [(r, kind, 63 if kind == "ends" else (0, 37, 63)[(j + ki) % 3])
            for j, r in enumerate((1, 2, 3, 4, 5, 6, N - 2, N - 1)) for ki, kind in enumerate(KINDS)]


@functools.lru_cache(maxsize=None)
def handover_case(r, kind, lane):
    hs = lanes(s_base)
    hs[lane] = differing(kind, lane, r)
    return Case(hs)


def test_the_handover_lane_differs_from_its_row_on():
    for r, kind, lane in HANDOVER:
        nf, ns, tf, lane_wf = host_type_flags(handover_case(r, kind, lane))
        assert (nf, ns) == (1, 1) and lane_wf[lane] == lane
        other = tf[:, (lane + 1) % 64]
        assert (tf[1:r] == other[1:r, None]).all() and tf[r, lane] != other[r], (r, kind, lane)


@gpu
@pytest.mark.parametrize("tasks", [False, True], ids=["states", "tasks"])
@pytest.mark.parametrize("r,kind,lane", HANDOVER, ids=[f"row{r}-{k}-lane{l}" for r, k, l in HANDOVER])
def test_handover_at_every_slot_phase(engine_gpu, r, kind, lane, tasks):
    """One lane differs from row r on — another type, an id gap, or its history ends — so the
    uniform loop is left before its first step (r <= 2 FD), in mid-slice, and at the last rows."""
    run_and_check(engine_gpu, handover_case(r, kind, lane), tasks)


# ---------------------------------------------------------------- 3. a lane fails, the rows stay uniform
def s_unhinted(h, bad=False):
    h.done_decision()
    s = h.activity(signals=8, close=None)  # operand distances 9 and 10: no hint, the key is loaded
    h.add("ActivityTaskCompleted", same_call=True, scheduledEventId=s - 1 if bad else s, startedEventId=h.id)
    h.done_decision()
    h.activity(signals=8)


@functools.lru_cache(maxsize=None)
def failing_case():
    hs = lanes(s_unhinted)
    hs[21] = UHist(lane=21)
    s_unhinted(hs[21], bad=True)
    return Case(hs)


def test_the_failing_lane_keeps_the_rows_uniform():
    nf, ns, tf, _ = host_type_flags(failing_case())
    assert (nf, ns) == (1, 1) and (tf[1:] == tf[1:, :1]).all()


@gpu
@pytest.mark.parametrize("tasks", [False, True], ids=["states", "tasks"])
def test_a_lane_fails_while_rows_stay_uniform(engine_gpu, tasks):
    """The failed entry's code, fail id and fail index equal the oracle's (engine.compare), and
    the other 63 entries are unaffected."""
    c = failing_case()
    codes = [abi.STATUS[c.ref.result[w].code] for w in range(64)]
    assert codes[21] == "E_ACTIVITY_NOT_FOUND" and codes.count("OK") == 63
    assert c.ref.result[21].fail_index == 14
    run_and_check(engine_gpu, c, tasks)


# ---------------------------------------------------------------- 4. lanes missing
@gpu
@pytest.mark.parametrize("n", [1, 63])
def test_fewer_than_64_workflows(engine_gpu, n):
    run_and_check(engine_gpu, Case(lanes(s_signal_cancel_marker, n=n)), False)


@gpu
def test_a_skip_mask_with_lane_0(engine_gpu):
    c = uniform_case(0)
    skip = np.zeros(64, np.uint8)
    skip[[0, 1, 37, 63]] = 1
    masked = set(np.nonzero(skip)[0].tolist())
    got = run_and_check(engine_gpu, c, False, skip=skip, masked=masked)
    for w in masked:  # a masked entry's records are untouched
        assert bytes(got.result[w]) == bytes(C.sizeof(abi.CdrWfResult))
        assert bytes(got.exec[w]) == bytes(C.sizeof(abi.CdrExecInfo))
