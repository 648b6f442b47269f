"""Operand hint fields of the packed type_flags word (cdr.h CDR_SEF_KEY_BACK / CDR_SEF_AUX_IMPL):
set by the shared packer (pack_event.h cdr_put_event) from an event's own values, only for a
column its type reads, with the cell keeping its full value and every other bit of the word as
cdr_type_flags gives it.  Hand-made histories through cadence_amd.history; host packer only."""
import ctypes as C

import numpy as np

from cadence_amd import abi
from cadence_amd.history import HistoryBuilder

PAD = 0xFF
HINTS = abi.SEF_KEY_BACK | abi.SEF_AUX_IMPL

# cdr.h CDR_NEED_*: the event types that read each operand column
NEED = {
    abi.SEF_NEED_TS: ("WorkflowExecutionStarted", "DecisionTaskScheduled", "DecisionTaskStarted", "ActivityTaskScheduled",
                      "ActivityTaskStarted", "TimerStarted", "WorkflowExecutionCompleted", "WorkflowExecutionFailed",
                      "WorkflowExecutionTimedOut", "WorkflowExecutionCanceled", "WorkflowExecutionTerminated",
                      "WorkflowExecutionContinuedAsNew"),
    abi.SEF_NEED_KEY: ("DecisionTaskStarted", "ActivityTaskScheduled", "ActivityTaskStarted", "ActivityTaskCompleted",
                       "ActivityTaskFailed", "ActivityTaskTimedOut", "ActivityTaskCanceled", "ActivityTaskCancelRequested",
                       "TimerStarted", "TimerFired", "TimerCanceled", "StartChildWorkflowExecutionInitiated",
                       "ChildWorkflowExecutionStarted", "StartChildWorkflowExecutionFailed",
                       "ChildWorkflowExecutionCompleted", "ChildWorkflowExecutionFailed", "ChildWorkflowExecutionCanceled",
                       "ChildWorkflowExecutionTimedOut", "ChildWorkflowExecutionTerminated",
                       "RequestCancelExternalWorkflowExecutionFailed", "ExternalWorkflowExecutionCancelRequested",
                       "SignalExternalWorkflowExecutionFailed", "ExternalWorkflowExecutionSignaled",
                       "RequestCancelExternalWorkflowExecutionInitiated", "SignalExternalWorkflowExecutionInitiated"),
    abi.SEF_NEED_AUX: ("WorkflowExecutionStarted", "DecisionTaskScheduled", "DecisionTaskCompleted", "ActivityTaskScheduled",
                       "TimerStarted", "StartChildWorkflowExecutionInitiated", "SignalExternalWorkflowExecutionInitiated",
                       "UpsertWorkflowSearchAttributes"),
    abi.SEF_NEED_H: ("DecisionTaskStarted", "DecisionTaskCompleted", "ActivityTaskScheduled", "ActivityTaskStarted",
                     "StartChildWorkflowExecutionInitiated", "ChildWorkflowExecutionStarted",
                     "SignalExternalWorkflowExecutionInitiated", "UpsertWorkflowSearchAttributes"),
    abi.SEF_NEED_N: ("DecisionTaskScheduled", "DecisionTaskTimedOut", "ActivityTaskScheduled",
                     "StartChildWorkflowExecutionInitiated"),
}
M64 = (1 << 64) - 1


def type_flags(ty: int, flags: int) -> int:
    """cdr.h cdr_type_flags: type, flags and the type's column-need bits."""
    tf = (ty & 0xFF) | flags
    for bit, names in NEED.items():
        if any(abi.EV[n] == ty for n in names):
            tf |= bit
    return tf


def operand_hints(tf: int, eid: int, key: int, aux: int) -> int:
    """cdr.h cdr_operand_hints, from the cell values (uint64 arithmetic, wrapping)."""
    h = 0
    if tf & abi.SEF_NEED_KEY:
        d = (eid - key) & M64
        if 1 <= d <= 7:
            h |= d << abi.SEF_KEY_BACK_SHIFT
    if tf & abi.SEF_NEED_AUX:
        d = (eid - aux) & M64
        if aux == 0:
            h |= abi.SEF_AUX_ZERO << abi.SEF_AUX_IMPL_SHIFT
        elif 1 <= d <= 6:
            h |= d << abi.SEF_AUX_IMPL_SHIFT
    return h


def pack(batch):
    """Host plan + pack (lane slices): columns, and each entry's (slice, lane)."""
    L = abi.lib()
    ns, rows = C.c_uint32(), C.c_uint64()
    assert L.cdr_plan_slices(batch.wfs, batch.n_wfs, None, None, None, C.byref(ns), C.byref(rows)) == 0
    lane = np.zeros(ns.value * 64, np.int32)
    slen = np.zeros(ns.value, np.uint32)
    row0 = np.zeros(ns.value, np.uint64)
    assert L.cdr_plan_slices(batch.wfs, batch.n_wfs, lane.ctypes.data, slen.ctypes.data, row0.ctypes.data, C.byref(ns),
                             C.byref(rows)) == 0
    slab = np.zeros(rows.value * 64 * abi.EL_BYTES, np.uint8)
    aw = L.cdr_plan_arena_words(C.byref(batch.cstruct()))
    arena = np.zeros(max(1, aw), np.uint64)
    s = abi.CdrSlices(n_slices=ns.value, n_rows=rows.value, arena_words=aw)
    s.slice_row0, s.slice_len, s.lane_wf = row0.ctypes.data, slen.ctypes.data, lane.ctypes.data
    s.slab, s.arena = slab.ctypes.data, arena.ctypes.data
    assert L.cdr_pack_slices(C.byref(batch.cstruct()), C.byref(s), 1) == 0
    return abi.slab_columns(slab, row0, slen), lane, slen, row0


def cells(batch, packed):
    """(entry, k, event or None for padding, cell index) of every cell of the occupied lanes."""
    cols, lane, slen, row0 = packed
    for i, w in enumerate(lane):
        if w < 0:
            continue
        sl, l = divmod(i, 64)
        d = batch.wfs[w]
        for k in range(int(slen[sl])):
            j = (int(row0[sl]) + k) * 64 + l
            yield int(w), k, (batch.events[d.ev_off + k] if k < d.ev_len else None), j


def operands(e):
    """(key, aux) the packer stores for the event types these tests use (cdr.h "operand columns")."""
    name = abi.EVENT_TYPES[e.type]
    if name == "DecisionTaskScheduled":
        return 0, e.a.dt_sched.attempt
    if name == "DecisionTaskStarted":
        return e.a.dt.scheduled_event_id, 0
    if name == "DecisionTaskCompleted":
        return e.a.dt.scheduled_event_id, e.a.dt.started_event_id
    if name in ("ActivityTaskStarted", "ActivityTaskCompleted", "ActivityTaskFailed"):
        return e.a.at.scheduled_event_id, 0
    if name in ("WorkflowExecutionSignaled", "MarkerRecorded", "DecisionTaskFailed"):
        return 0, 0
    return None


def check_all(batch, packed):
    """The checks every case shares; returns {(entry, k): hint bits}."""
    cols = packed[0]
    tf, eid, key, aux = cols["type_flags"], cols["event_id"], cols["key"], cols["aux"]
    got = {}
    for w, k, e, j in cells(batch, packed):
        if e is None:  # padding: PAD and zero columns, as before
            assert int(tf[j]) == PAD, (w, k)
            assert all(int(cols[c][j]) == 0 for c in cols if c != "type_flags"), (w, k)
            continue
        p = batch.events[batch.wfs[w].ev_off + k - 1] if k > 0 else None
        flags = abi.SEF_BATCH_FIRST if (e.flags & abi.EVF_BATCH_FIRST or k == 0) else 0
        if p is not None:
            flags |= abi.SEF_ID_NEXT if e.event_id == p.event_id + 1 else 0
            flags |= abi.SEF_VER_SAME if e.version == p.version else 0
        word = int(tf[j])
        base = type_flags(e.type, flags)
        assert word & ~HINTS == base, (w, k, hex(word), hex(base))  # type, batch-first, delta and need bits
        assert int(eid[j]) == e.event_id
        ops = operands(e)
        if ops is not None:  # a hinted cell still holds its full value
            assert (int(key[j]), int(aux[j])) == ops, (w, k)
        assert word & HINTS == operand_hints(base, int(eid[j]), int(key[j]), int(aux[j])), (w, k, hex(word))
        if not base & abi.SEF_NEED_KEY:
            assert not word & abi.SEF_KEY_BACK, (w, k)
        if not base & abi.SEF_NEED_AUX:
            assert not word & abi.SEF_AUX_IMPL, (w, k)
        got[(w, k)] = word & HINTS
    return got


def started(eid=1, **kw):
    return dict(eventId=eid, version=1, timestamp=10 ** 18, eventType="WorkflowExecutionStarted",
                workflowExecutionStartedEventAttributes={"taskList": {"name": "tl"}}, **kw)


def ev(eid, name, **attrs):
    return dict(eventId=eid, version=1, timestamp=10 ** 18 + eid, eventType=name,
                **{name[0].lower() + name[1:] + "EventAttributes": attrs})


def kb(d):
    return d << abi.SEF_KEY_BACK_SHIFT


def ai(d):
    return d << abi.SEF_AUX_IMPL_SHIFT


def one(events):
    hb = HistoryBuilder()
    hb.workflow(workflow_id="w", run_id="r", request_id="q").calls = [events]
    return hb.build()


def test_key_back_distances():
    """key == id - d for d = 0, 1, 7, 8: none, set, set, none."""
    for d, want in ((0, 0), (1, kb(1)), (7, kb(7)), (8, 0)):
        b = one([started(), ev(2, "WorkflowExecutionSignaled"), ev(20, "ActivityTaskCompleted", scheduledEventId=20 - d)])
        got = check_all(b, pack(b))
        assert got[(0, 2)] == want, d
        assert got[(0, 1)] == 0


def test_key_back_wraps_like_the_delta_bits():
    """uint64 arithmetic: a negative id whose key is id - 2 is hinted, a key far away is not."""
    b = one([started(), ev(-5, "ActivityTaskCompleted", scheduledEventId=-7),
             ev(3, "ActivityTaskCompleted", scheduledEventId=(1 << 62))])
    got = check_all(b, pack(b))
    assert got[(0, 1)] == kb(2) and got[(0, 2)] == 0


def test_aux_implied():
    """aux == id - 1 (DecisionTaskCompleted's startedEventId), aux == 0 and aux == 5 (attempts)."""
    b = one([started(), ev(20, "DecisionTaskCompleted", scheduledEventId=18, startedEventId=19),
             ev(21, "DecisionTaskScheduled", attempt=0), ev(22, "DecisionTaskScheduled", attempt=5),
             ev(23, "DecisionTaskCompleted", scheduledEventId=21, startedEventId=17),
             ev(24, "DecisionTaskCompleted", scheduledEventId=21, startedEventId=17),
             ev(3, "DecisionTaskScheduled", attempt=0), ev(7, "DecisionTaskScheduled", attempt=5)])
    got = check_all(b, pack(b))
    assert got[(0, 1)] == ai(1)   # started = id - 1; its key is id - 2 but the type does not read key
    assert got[(0, 2)] == ai(abi.SEF_AUX_ZERO)
    assert got[(0, 3)] == 0       # 22 - 5 = 17 > 6
    assert got[(0, 4)] == ai(6)   # the largest distance
    assert got[(0, 5)] == 0       # 7 would collide with "aux == 0": not a distance
    assert got[(0, 6)] == ai(abi.SEF_AUX_ZERO)  # aux == 0 wins over id - 3
    assert got[(0, 7)] == ai(2)   # attempt 5 == 7 - 2: value-based


def test_hint_without_id_next():
    """Non-contiguous event ids: the hint is about the event's own id, whatever the previous one."""
    b = one([started(), ev(5, "ActivityTaskStarted", scheduledEventId=4), ev(9, "ActivityTaskCompleted", scheduledEventId=8),
             ev(10, "ActivityTaskCompleted", scheduledEventId=8)])
    packed = pack(b)
    got = check_all(b, packed)
    tf = packed[0]["type_flags"]
    idx = {(w, k): j for w, k, e, j in cells(b, packed) if e is not None}
    assert not int(tf[idx[(0, 1)]]) & abi.SEF_ID_NEXT and not int(tf[idx[(0, 2)]]) & abi.SEF_ID_NEXT
    assert int(tf[idx[(0, 3)]]) & abi.SEF_ID_NEXT
    assert [got[(0, k)] for k in (1, 2, 3)] == [kb(1), kb(1), kb(2)]


def test_first_event_of_an_entry():
    """An entry's first event (no delta bits): hinted from its own values like any other — the
    first Started's arena offset is 0, the next entry's is not."""
    hb = HistoryBuilder()
    hb.workflow(workflow_id="a", run_id="r", request_id="q").calls = [[started(), ev(2, "DecisionTaskScheduled")]]
    hb.workflow(workflow_id="b", run_id="r", request_id="q").calls = [[ev(3, "ActivityTaskStarted", scheduledEventId=2),
                                                                       ev(4, "DecisionTaskScheduled", attempt=1)]]
    hb.workflow(workflow_id="c", run_id="r", request_id="q").calls = [[started(eid=1000)]]
    b = hb.build()
    packed = pack(b)
    got = check_all(b, packed)
    aux = packed[0]["aux"]
    idx = {(w, k): j for w, k, e, j in cells(b, packed) if e is not None}
    offs = sorted(int(aux[idx[(w, 0)]]) for w in (0, 2))
    assert offs[0] == 0 and offs[1] > 6  # the two Started records in the arena
    for w in (0, 2):
        assert got[(w, 0)] == (ai(abi.SEF_AUX_ZERO) if int(aux[idx[(w, 0)]]) == 0 else 0)
    assert got[(1, 0)] == kb(1)
    assert got[(1, 1)] == ai(3)  # attempt 1 == 4 - 3


def test_types_without_the_need_bit():
    """No hint on a column the type does not read, whatever the cell holds."""
    b = one([started(), ev(2, "WorkflowExecutionSignaled"), ev(3, "MarkerRecorded"),
             ev(4, "DecisionTaskStarted", scheduledEventId=3),           # aux cell 0, not read
             ev(5, "DecisionTaskCompleted", scheduledEventId=3, startedEventId=4),  # key == id - 2, not read
             ev(6, "DecisionTaskFailed", scheduledEventId=5, startedEventId=5)])
    got = check_all(b, pack(b))
    assert [got[(0, k)] for k in range(1, 6)] == [0, 0, kb(1), ai(1), 0]


def test_encoded_bytes_do_not_price_hinted_columns():
    """synth.encoded_event_bytes (the bench's achieved_basis): 8 B less per hinted column."""
    from cadence_amd import synth
    T = abi.EV["ActivityTaskCompleted"]
    base = type_flags(T, abi.SEF_ID_NEXT | abi.SEF_VER_SAME)
    assert synth.encoded_event_bytes(np.array([base], np.uint32)) == 12
    assert synth.encoded_event_bytes(np.array([base | kb(2)], np.uint32)) == 4
    D = type_flags(abi.EV["DecisionTaskCompleted"], abi.SEF_ID_NEXT | abi.SEF_VER_SAME)
    assert synth.encoded_event_bytes(np.array([D, D | ai(1), D | kb(1)], np.uint32)) == 16 + 8 + 16
