"""k_replay_fast with the operand hint fields (cdr.h CDR_SEF_KEY_BACK / CDR_SEF_AUX_IMPL) and
the launch of fast slices alone that skips k_tables: hand-made sequential-activity histories
(<= 64 per slice, <= 40 events) through cdr_replay_sliced_async against the CPU restatement."""
import ctypes as C
import random

import numpy as np
import pytest

from cadence_amd import abi, engine, ndc
from cadence_amd.history import HistoryBuilder

pytestmark = pytest.mark.gpu

T0 = 10 ** 18
COL_OFF = {}
_off = 0
for _name, _dt in abi.SLAB_COLS:
    COL_OFF[_name] = _off * abi.SLICE_WIDTH
    _off += np.dtype(_dt).itemsize
# a recognisable value no event id minus 1..7 and no attempt equals (compared, never dereferenced:
# the cells of WorkflowExecutionStarted / ActivityTaskScheduled, whose aux is an arena offset that
# the pending activity's emission reads from the cell itself, are left alone)
GARBAGE = 0x5A5A5A5A5A5A5A5A
ARENA_TYPES = (abi.EV["WorkflowExecutionStarted"], abi.EV["ActivityTaskScheduled"])


class Hist:
    """One workflow's events: ids advance by 1 unless `gap` is given; every event its own call
    unless `same_call`."""

    def __init__(self, sa=None):
        self.calls, self.id = [], 0
        attrs = {"taskList": {"name": "tl"}, "taskStartToCloseTimeoutSeconds": 10,
                 "executionStartToCloseTimeoutSeconds": 3600}
        if sa is not None:
            attrs["searchAttributes"] = {"indexedFields": sa}
        self.add("WorkflowExecutionStarted", **attrs)

    def add(self, name, gap=0, same_call=False, **attrs):
        self.id += 1 + gap
        e = dict(eventId=self.id, version=1, timestamp=T0 + self.id * 10 ** 9, taskId=100 + self.id, eventType=name,
                 **{name[0].lower() + name[1:] + "EventAttributes": attrs})
        if same_call and self.calls:
            self.calls[-1].append(e)
        else:
            self.calls.append([e])
        return self.id

    def decision(self, attempt=0, gap=0, checksum="", bad_sched=None):
        s = self.add("DecisionTaskScheduled", gap=gap, attempt=attempt, startToCloseTimeoutSeconds=10,
                     taskList={"name": "tl"})
        st = self.add("DecisionTaskStarted", scheduledEventId=s if bad_sched is None else bad_sched, requestId="rq")
        return s, st

    def complete_decision(self, s, st, checksum=""):
        return self.add("DecisionTaskCompleted", scheduledEventId=s, startedEventId=st, binaryChecksum=checksum)

    def activity(self, signals=0, gap=0, close="ActivityTaskCompleted", bad_close=None, hb=0):
        """Scheduled, `signals` WorkflowExecutionSignaled, Started, close: the Started / close events'
        scheduledEventId is 1 + signals / 2 + signals behind their own id (+ gap)."""
        s = self.add("ActivityTaskScheduled", same_call=True, activityId=f"a{self.id}", taskList={"name": "atl"},
                     scheduleToStartTimeoutSeconds=5, scheduleToCloseTimeoutSeconds=50, startToCloseTimeoutSeconds=20,
                     heartbeatTimeoutSeconds=hb)
        for _ in range(signals):
            self.add("WorkflowExecutionSignaled")
        st = self.add("ActivityTaskStarted", gap=gap, scheduledEventId=s, requestId="arq")
        if close:
            self.add(close, same_call=True, scheduledEventId=s if bad_close is None else bad_close, startedEventId=st)
        return s

    def pad_to(self, n):
        while self.n < n:
            self.add("WorkflowExecutionSignaled")
        assert self.n == n, (self.n, n)
        return self

    @property
    def n(self):
        return sum(len(c) for c in self.calls)


def chain(acts=2, signals=(0, 0), gap_at=None, **kw):
    """The activity-chain shape: Started, then per activity decision - activity."""
    h = Hist(**kw)
    for i in range(acts):
        s, st = h.decision(gap=2 if gap_at == i else 0)
        h.complete_decision(s, st, checksum=f"ck{i % 2}")
        h.activity(signals=signals[i % len(signals)])
    return h


def build(hists):
    hb = HistoryBuilder()
    for i, h in enumerate(hists):
        hb.workflow(workflow_id=f"w{i}", run_id=f"r{i}", request_id=f"q{i}").calls = h.calls
    return hb.build()


def quick_lanes(n=64, length=38):
    """Contiguous ids, one version, equal lengths: every row is the wave-uniform quick row.  The
    lanes still disagree on type and on the hint distance at the same step."""
    sig = [(0, 0), (1, 0), (0, 8), (2, 3), (7, 0), (6, 1)]
    return [chain(acts=2, signals=sig[i % len(sig)]).pad_to(length) for i in range(n)]


def mixed_lanes():
    """Hinted beside unhinted events, id gaps, transient decisions, wrong scheduledEventIds (hinted
    and not), histories shorter than the slice, one of a single event."""
    hs = []
    for i in range(40):
        hs.append(chain(acts=1 + i % 3, signals=[(0, 1), (5, 0), (8, 2), (6, 3)][i % 4], gap_at=(i % 3) if i % 5 == 0 else None))
    for i in range(4):  # a transient decision: DecisionTaskFailed, then Scheduled with attempt 1
        h = Hist()
        for _ in range(i):
            h.add("WorkflowExecutionSignaled")
        s, st = h.decision()
        h.add("DecisionTaskFailed", scheduledEventId=s, startedEventId=st)
        s, st = h.decision(attempt=1)
        h.complete_decision(s, st)
        h.activity(signals=i)
        hs.append(h)
    for i, (sig, back) in enumerate(((0, 1), (0, 3), (2, 9), (0, 30))):  # a close naming another event
        h = chain(acts=1)
        s, st = h.decision()
        h.complete_decision(s, st)
        sid = h.activity(signals=sig, close=None)
        wrong = h.id + 1 - back
        assert wrong != sid
        h.add("ActivityTaskCompleted", scheduledEventId=wrong, startedEventId=h.id)
        h.add("WorkflowExecutionSignaled")
        hs.append(h)
    for back in (2, 20):  # a DecisionTaskStarted naming another event
        h = chain(acts=1)
        h.decision(bad_sched=h.id + 2 - back)
        hs.append(h)
    h = chain(acts=1)  # an ActivityTaskStarted for no activity (hinted: id - 1)
    h.add("ActivityTaskStarted", scheduledEventId=h.id, requestId="x")
    hs.append(h)
    h = chain(acts=1)  # a still-pending, started activity with a heartbeat
    s, st = h.decision()
    h.complete_decision(s, st)
    h.activity(close=None, hb=3)
    hs.append(h)
    for n in (1, 2, 3, 5):  # shorter than the slice; a history of length 1
        hs.append(Hist().pad_to(n))
    assert len(hs) <= 64 and max(h.n for h in hs) <= 40
    return hs


def slab_views(dev, db):
    """The device slab's bytes and (row0, slen) of its slices, downloaded."""
    ns = db.ev.n_slices
    slab = np.zeros(int(db.ev.n_rows) * abi.ROW_BYTES, np.uint8)
    row0, slen = np.zeros(ns, np.uint64), np.zeros(ns, np.uint32)
    for arr, p in ((slab, db.ev.slab), (row0, db.ev.slice_row0), (slen, db.ev.slice_len)):
        assert dev.hip.hipMemcpy(C.c_void_p(arr.ctypes.data), C.c_void_p(p), C.c_size_t(arr.nbytes), 2) == 0
    return slab, row0, slen


def garble_hinted(dev, db):
    """Overwrite every hinted key / aux cell of the device slab; returns how many of each."""
    slab, row0, slen = slab_views(dev, db)
    tf = abi.slab_columns(slab, row0, slen, ("type_flags",))["type_flags"]
    g = np.frombuffer(np.uint64(GARBAGE).tobytes(), np.uint8)
    cnt = {"key": 0, "aux": 0}
    for j in np.nonzero(tf & (abi.SEF_KEY_BACK | abi.SEF_AUX_IMPL))[0]:
        r, l = divmod(int(j), 64)
        for col, mask in (("key", abi.SEF_KEY_BACK), ("aux", abi.SEF_AUX_IMPL)):
            if int(tf[j]) & mask and not (col == "aux" and int(tf[j]) & 0xFF in ARENA_TYPES):
                o = r * abi.ROW_BYTES + COL_OFF[col] + l * 8
                slab[o:o + 8] = g
                cnt[col] += 1
    assert dev.hip.hipMemcpy(C.c_void_p(db.ev.slab), C.c_void_p(slab.ctypes.data), C.c_size_t(slab.nbytes), 1) == 0
    return cnt


def run_sliced(eng, batch, pl, tasks=False, garble=False, skip=None, want_fast=None):
    """`batch` through cdr_replay_sliced_async (host plan + pack, lane slices) and back; want_fast:
    (fast slices, slices) the plan must have."""
    L = abi.lib()
    dev = ndc._Dev()
    try:
        db = ndc.upload_batch(dev, batch, pl.caps, 0, False)
        if want_fast is not None:
            assert (db.n_fast_slices, db.ev.n_slices) == want_fast
        info = garble_hinted(dev, db) if garble else None
        if skip is not None:
            db.skip = dev.up(np.asarray(skip, np.uint8))
        o = ndc.alloc_out(dev, batch.n_wfs, pl.totals, tasks)
        assert L.cdr_replay_sliced_async(eng.ctx, C.byref(db), C.byref(o), None) == 0
        out = ndc.download_out(dev, o, batch.n_wfs, pl, tasks)  # (synchronises)
        return (out, info) if garble else out
    finally:
        dev.close()


class Case:
    def __init__(self, hists, tasks=False):
        import oracle
        self.batch = build(hists)
        self.pl = engine.plan(self.batch)
        self.ref = oracle.replay(self.batch, self.pl, tasks=tasks)


@pytest.fixture(scope="module")
def mixed():
    return Case(mixed_lanes(), tasks=True)


def check(case, got, skip=()):
    bad = [m for m in engine.compare(case.batch, got, case.ref, limit=10 ** 6, last_decision=False)
           if int(m.split()[1].rstrip(":")) not in skip]
    assert not bad, "\n".join(bad[:8])


def test_mixed_slice_matches_the_oracle(engine_gpu, mixed):
    """Lanes that disagree at the same step — hint distances 1..7 beside unhinted events, id gaps,
    transient decisions, wrong scheduledEventIds, short histories — equal the oracle, failed
    entries' code, fail id and fail index included."""
    ref = mixed.ref
    codes = {ref.result[w].code for w in range(mixed.batch.n_wfs)}
    assert {"OK", "E_ACTIVITY_NOT_FOUND", "E_DECISION_NOT_FOUND", "P_ACTIVITY_STARTED_NIL"} <= {abi.STATUS[c] for c in codes}
    assert any(ref.result[w].code == abi.OK and ref.result[w].n_activity == 1 for w in range(mixed.batch.n_wfs))
    check(mixed, run_sliced(engine_gpu, mixed.batch, mixed.pl, want_fast=(1, 1)))


def test_quick_rows_and_one_general_lane(engine_gpu):
    """A slice whose every row is the quick row, and the same slice with one lane whose id gap
    forces the general row."""
    quick = quick_lanes()
    check(Case(quick), run_sliced(engine_gpu, build(quick), engine.plan(build(quick)), want_fast=(1, 1)))
    one = quick_lanes()
    one[37] = chain(acts=2, signals=(1, 0), gap_at=1).pad_to(38)
    c = Case(one)
    check(c, run_sliced(engine_gpu, c.batch, c.pl, want_fast=(1, 1)))


def test_hinted_cells_are_not_loaded(engine_gpu, mixed):
    """With every hinted key / aux cell of the device slab overwritten, the fast kernel's results
    still equal the oracle's: it rebuilds those operands and never loads them."""
    got, cnt = run_sliced(engine_gpu, mixed.batch, mixed.pl, garble=True, want_fast=(1, 1))
    assert cnt["key"] >= 100 and cnt["aux"] >= 100, cnt
    check(mixed, got)


def test_tasks_instantiation(engine_gpu, mixed):
    """k_replay_fast<TASKS> on the mixed slice: states and task lists equal the oracle's."""
    got = run_sliced(engine_gpu, mixed.batch, mixed.pl, tasks=True, want_fast=(1, 1))
    check(mixed, got)
    bad = engine.compare_tasks(mixed.batch, got, mixed.ref)
    assert not bad, "\n".join(bad[:8])
    assert sum(got.tasks["n"]) == sum(mixed.ref.tasks["n"]) > 0


# ---------------------------------------------------------------- launches of fast slices alone
SA_SHAPES = ([], [0], [1, 0], [0, 1], [4, 3, 2, 1, 0], [2, 4, 0, 3, 1], [3, 0, 4, 1, 2])


def sa_lanes(n=64):
    """Started events with 0, 1, 2 and 5 search attributes in ascending, descending and shuffled
    key order (a key is its interned handle: the names are interned in ascending order first)."""
    hb = HistoryBuilder()
    names = [f"Custom{k}Field" for k in range(5)]
    for k in names:
        hb.intern(k)
    rnd = random.Random(7)
    for i in range(n):
        order = list(SA_SHAPES[i % len(SA_SHAPES)])
        if i >= 2 * len(SA_SHAPES) and len(order) == 5:
            rnd.shuffle(order)
        h = chain(acts=1 + i % 2, sa={names[k]: f"v{i}-{k}" for k in order} if order or i % 2 else None)
        hb.workflow(workflow_id=f"w{i}", run_id=f"r{i}", request_id=f"q{i}").calls = h.calls
    return hb


def with_timers(hb, n=3):
    """Entries the fast kernel does not take (a user timer), with search attributes too."""
    for i in range(n):
        h = chain(acts=1, sa={"Custom3Field": "x", "Custom1Field": "y"})
        h.add("TimerStarted", timerId=f"t{i}", startToFireTimeoutSeconds=5)
        hb.workflow(workflow_id=f"t{i}", run_id=f"tr{i}", request_id=f"tq{i}").calls = h.calls
    return hb


def sa_case(hb):
    import oracle
    c = Case.__new__(Case)
    c.batch = hb.build()
    c.pl = engine.plan(c.batch)
    c.ref = oracle.replay(c.batch, c.pl)
    return c


def check_sa_sorted(case, got, skip=()):
    seen = set()
    for w in range(case.batch.n_wfs):
        if w in skip:
            continue
        keys = [r.key for r in got.rows(w, "sa")]
        assert keys == sorted(keys) == [r.key for r in case.ref.rows(w, "sa")], w
        seen.add(len(keys))
    return seen


def test_all_fast_launch_orders_search_attributes(engine_gpu):
    c = sa_case(sa_lanes())
    got = run_sliced(engine_gpu, c.batch, c.pl, want_fast=(1, 1))
    check(c, got)
    assert check_sa_sorted(c, got) == {0, 1, 2, 5}


def test_mixed_launch_keeps_the_table_pass(engine_gpu):
    """The same entries beside a slice of another class: k_tables runs (its sort a no-op on the
    fast entries), and the other class's rows are ordered by it."""
    c = sa_case(with_timers(sa_lanes()))
    got = run_sliced(engine_gpu, c.batch, c.pl, want_fast=(1, 2))
    check(c, got)
    assert check_sa_sorted(c, got) == {0, 1, 2, 5}
    assert any(c.ref.result[w].n_timer == 1 for w in range(c.batch.n_wfs))


def test_all_fast_launch_with_a_skip_mask(engine_gpu):
    c = sa_case(sa_lanes())
    skip = np.zeros(c.batch.n_wfs, np.uint8)
    skip[[0, 5, 11, 63]] = 1
    masked = set(np.nonzero(skip)[0].tolist())
    got = run_sliced(engine_gpu, c.batch, c.pl, skip=skip, want_fast=(1, 1))
    check(c, got, skip=masked)
    check_sa_sorted(c, got, skip=masked)
    for w in masked:  # a masked entry's records are untouched
        assert bytes(got.result[w]) == bytes(C.sizeof(abi.CdrWfResult))
