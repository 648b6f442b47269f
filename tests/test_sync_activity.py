"""Batched SyncActivity on loaded states (cdr_sync_activity_async / cdr_sync_activity_batch):
historyReplicator.SyncActivity (service/history/historyReplicator.go:160-295) per request —
its exits, resetActivityTimerTaskStatus, ReplicateActivityInfo on the pending-activity row and
the activity timer pick.

The reference is tests/sync_ref.py, a plain-Python restatement over engine.Outputs rows.  CPU:
the reference gives the reference test suite's answers (the TestSyncActivity_* cases of
historyReplicator_test.go:221-706 as data), its pick equals the oracle's refreshTasks pick,
and the fixtures hold every exit and every kind of applied request.  GPU: the kernel equals
the reference on those fixtures and on hand-made states (row counts around the group size and
the wave width, ties, schedule ids around 2^31, failed and version-history-less records),
writes nothing outside the rows it touches, and a synced state carries into a replay.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from cadence_amd import abi, engine, sync
from tests import sync_ref as ref

FILL = 0xA5
SEC = sync.SEC
T0 = 1_600_000_000 * SEC
BUILDERS = (abi.BUILDER_LOCAL, abi.BUILDER_2DC, abi.BUILDER_NDC)


# ---------------------------------------------------------------- hand-made states
def _act(sched, version=100, attempt=0, started=False, sched_time=T0, s2c=600, s2s=60, stc=120, hb=0,
         status=0, hb_time=None, activity_id=0, expiration=None):
    """A pending-activity row; every field the sync path leaves alone gets a value derived
    from the schedule id, so a stray write shows."""
    a = abi.CdrActivityInfo(
        version=version, schedule_id=sched, scheduled_event_batch_id=sched - 1, scheduled_time=sched_time,
        started_id=sched + 1 if started else abi.EMPTY_EVENT_ID, started_time=sched_time + SEC if started else 0,
        last_heartbeat_time=(hb_time if hb_time is not None else sched_time + SEC) if started or hb_time else 0,
        expiration_time=expiration if expiration is not None else sched_time + s2c * SEC,
        cancel_request_id=abi.EMPTY_EVENT_ID, activity_id=activity_id or (sched & 0xFFFF) + 7,
        request_id=(sched & 0xFFF) + 3, task_list=5, nonretriable=0, s2s=s2s, s2c=s2c, stc=stc, hb=hb,
        timer_task_status=status, attempt=attempt, initial_interval=1, maximum_interval=9, maximum_attempts=4,
        flags=abi.AI_HAS_RETRY | (abi.AI_STARTED_TIME_SET if started else 0), backoff_coefficient=2.0)
    return a


def _entry(rows=(), kind=abi.BUILDER_2DC, lwv=100, nxt=154, state=abi.STATE_RUNNING, code=abi.OK, n_vh=1):
    return dict(rows=list(rows), kind=kind, lwv=lwv, nxt=nxt, state=state, code=code, n_vh=n_vh)


def _state(entries, slack=lambda w: 0, fill=0):
    """An Outputs of hand-made records: entry w's activity slice is slack(w) rows larger than
    its row count, and the whole act table is pre-filled with `fill`."""
    n = len(entries)
    caps = (abi.CdrWfCaps * n)()
    tot = abi.CdrTotals()
    for w, e in enumerate(entries):
        caps[w].act_off, caps[w].act_cap = tot.act, len(e["rows"]) + slack(w)
        tot.act += caps[w].act_cap
        caps[w].vh_off, caps[w].vh_cap = tot.vh, 2
        tot.vh += 2
    fake = engine.Batch(events=(abi.CdrEvent * 0)(), wfs=(abi.CdrWfDesc * n)(), kvs=(abi.CdrKV * 0)(),
                        rps=(abi.CdrResetPoint * 0)(), cluster=engine.default_cluster())
    st = engine.Outputs(fake, engine.Plan(caps=caps, totals=tot))
    if fill:
        C.memset(st.tables["act"], fill, C.sizeof(st.tables["act"]))
    for w, e in enumerate(entries):
        st.result[w].code = e["code"]
        st.result[w].n_activity = len(e["rows"])
        st.exec[w].state, st.exec[w].next_event_id = e["state"], e["nxt"]
        if e["kind"] == abi.BUILDER_2DC:
            st.repl[w].present, st.repl[w].last_write_version = 1, e["lwv"]
        elif e["kind"] == abi.BUILDER_NDC:
            st.exec[w].flags |= abi.XI_VH_BRANCH
            st.result[w].n_vh = e["n_vh"]
            for k in range(e["n_vh"]):
                st.tables["vh"][caps[w].vh_off + k] = abi.CdrVHItem(event_id=e["nxt"] - 1, version=e["lwv"])
        for j, r in enumerate(e["rows"]):
            st.tables["act"][caps[w].act_off + j] = r
    return st


# the TestSyncActivity_* cases of historyReplicator_test.go:221-706: scheduleID 144, version 100
# (name, state, nextEventID, lastWriteVersion, the pending row or None, request attempt,
#  expected action, expected resetActivityTimerTaskStatus)
KATS = [
    ("WorkflowClosed", abi.STATE_COMPLETED, 154, 100, None, 0, abi.SYNC_SKIP_NOT_RUNNING, None),
    ("IncomingScheduleIDLarger_IncomingVersionSmaller", abi.STATE_RUNNING, 134, 200, None, 0,
     abi.SYNC_SKIP_STALE_VERSION, None),
    ("IncomingScheduleIDLarger_IncomingVersionLarger", abi.STATE_RUNNING, 134, 0, None, 0, abi.SYNC_RETRY_2DC, None),
    ("ActivityCompleted", abi.STATE_RUNNING, 154, 100, None, 0, abi.SYNC_SKIP_NO_ACTIVITY, None),
    ("LocalActivityVersionLarger", abi.STATE_RUNNING, 154, 110, (109, 0), 0, abi.SYNC_SKIP_LOCAL_VERSION_LARGER, None),
    ("Update_SameVersionSameAttempt", abi.STATE_RUNNING, 154, 100, (100, 0), 0, abi.SYNC_APPLIED, False),
    ("Update_SameVersionLargerAttempt", abi.STATE_RUNNING, 154, 100, (100, 0), 1, abi.SYNC_APPLIED, True),
    ("Update_LargerVersion", abi.STATE_RUNNING, 154, 100, (99, 1), 0, abi.SYNC_APPLIED, True),
]


def _kat_batch():
    entries, reqs = [], []
    for w, (_, state, nxt, lwv, row, attempt, _, _) in enumerate(KATS):
        rows = [_act(144, version=row[0], attempt=row[1])] if row else []
        if row:  # Go's ActivityInfo{Version, ScheduleID, Attempt}: the times are zero
            rows[0].flags = 0
            rows[0].last_heartbeat_time = 0
        entries.append(_entry(rows, abi.BUILDER_2DC, lwv, nxt, state))
        reqs.append(sync.request(w, 144, 100, attempt, T0, 145, T0 + 60 * SEC, T0 + 120 * SEC, tag=1000 + w))
    return _state(entries), sync.Requests(reqs)


def _check_kats(results):
    for (name, _, nxt, lwv, _, _, action, reset), r in zip(KATS, results):
        assert (r.action, r.code) == (action, abi.OK), name
        assert (r.next_event_id, r.last_write_version) == (nxt, lwv), name  # the 2DC hint is nextEventID
        if reset is not None:
            assert bool(r.flags & abi.SYNC_RESET_TIMER_STATUS) == reset, name
            assert r.event_time == T0 + 120 * SEC, name


def _results_equal(got, want, where=""):
    assert len(got) >= len(want)
    bad = []
    for i, (g, w) in enumerate(zip(got, want)):
        if ref.rbytes(g) != ref.rbytes(w):
            fields = [f for f, _ in abi.CdrSyncResult._fields_ if ref.rbytes(g)[getattr(abi.CdrSyncResult, f).offset:][
                :getattr(abi.CdrSyncResult, f).size] != ref.rbytes(w)[getattr(abi.CdrSyncResult, f).offset:][
                :getattr(abi.CdrSyncResult, f).size]]
            bad.append((i, abi.SYNC_ACTIONS.get(g.action, g.action), abi.SYNC_ACTIONS.get(w.action, w.action), fields))
    assert not bad, (where, len(bad), bad[:5])


def _run(eng, state, reqs, via="batch", cluster=None):
    """The kernel on a copy of `state`: (results, the copy)."""
    st = ref.copy_state(state)
    return eng.sync_activity(st, reqs, via=via, cluster=cluster), st


# ---------------------------------------------------------------- fixtures
@functools.lru_cache(maxsize=None)
def _fixture(cfg, builder):
    """split_batch's prefix states of a 300-workflow batch, oracle-replayed, with synthetic
    requests and the reference's answer: (batch, prefix, cut, state, requests, the reference's
    state, the reference's results)."""
    import oracle
    b = engine.synth_batch(cfg, 300, seed=0x5EED0300 + cfg, builder=builder, error_rate=0.1 if cfg == 3 else 0.0)
    pre, cut = engine.split_batch(b, 2)
    st = oracle.replay(pre)
    inc = b.cluster.failover_version_increment
    reqs = sync.synth_requests(st, seed=77 + 10 * cfg + builder, per_wf=4, increment=inc)
    want_state = ref.copy_state(st)
    return b, pre, cut, st, reqs, want_state, ref.sync(want_state, reqs, inc)


FIXTURES = [(cfg, bld) for cfg in (3, 5) for bld in BUILDERS]


# ---------------------------------------------------------------- CPU
def test_reference_kats():
    st, reqs = _kat_batch()
    _check_kats(ref.sync(st, reqs))


@pytest.mark.parametrize("cfg", [3, 5])
def test_reference_pick_matches_oracle_refresh(cfg):
    """With the statuses cleared, the reference's pick is refreshTasks' activity timer task."""
    import oracle
    b = engine.synth_batch(cfg, 300, seed=0x5EED0300 + cfg)
    out = oracle.rebuild(b)
    n = 0
    for w in range(b.n_wfs):
        if out.result[w].code != abi.OK or out.result[w].n_activity == 0:
            continue
        want = [t for t in out.task_rows(w, "ttask") if t.type == abi.TT_ACTIVITY_TIMEOUT]
        rows = [abi.CdrActivityInfo.from_buffer_copy(r) for r in out.rows(w, "act")]
        status = [r.timer_task_status for r in rows]
        for r in rows:
            r.timer_task_status = 0
        head = ref.pick(rows)
        assert head is not None and len(want) == 1, w
        j, t, ty = head
        assert (ty, rows[j].schedule_id, t, rows[j].attempt) == (
            want[0].timeout_type, want[0].event_id, want[0].visibility_ts, want[0].attempt), w
        assert [r.timer_task_status for r in rows] == status, w  # the same bit on the same row
        n += 1
    assert n >= 20


def test_fixture_coverage():
    """A condition on the reference alone: the fixtures reach every exit, and every kind of
    applied request, often enough that a kernel that mishandles one cannot pass parity."""
    actions = np.zeros(11, np.int64)
    applied = dict(reset=0, no_reset=0, task=0, no_task=0, other_row=0, unstarted=0)
    total = 0
    for cfg, bld in FIXTURES:
        _, _, _, _, reqs, _, results = _fixture(cfg, bld)
        total += len(reqs)
        for q, r in zip(reqs, results):
            actions[r.action] += 1
            if r.action != abi.SYNC_APPLIED:
                continue
            applied["reset" if r.flags & abi.SYNC_RESET_TIMER_STATUS else "no_reset"] += 1
            applied["task" if r.flags & abi.SYNC_HAS_TIMER_TASK else "no_task"] += 1
            applied["other_row"] += bool(r.flags & abi.SYNC_HAS_TIMER_TASK) and r.task_row != r.act_row
            applied["unstarted"] += q.started_id == abi.EMPTY_EVENT_ID
    print({abi.SYNC_ACTIONS[a]: int(c) for a, c in enumerate(actions)}, applied, total)
    for a in range(11):
        if a != abi.SYNC_E_STATE:
            assert actions[a] >= 5, abi.SYNC_ACTIONS[a]
    assert actions[abi.SYNC_APPLIED] >= 0.2 * total
    assert all(v > 0 for v in applied.values()), applied


def test_abi_mirrors():
    L = abi.lib()
    assert C.sizeof(abi.CdrSyncActivity) == 64 == L.cdr_struct_size(b"cdr_sync_activity")
    assert C.sizeof(abi.CdrSyncResult) == 128 == L.cdr_struct_size(b"cdr_sync_result")
    assert abi.CdrSyncResult.timer_task.offset == 64
    assert (abi.SYNC_SKIP_NO_WORKFLOW, abi.SYNC_APPLIED, abi.SYNC_E_STATE) == (0, 9, 10)
    assert abi.SYNC_GROUP in abi.SYNC_GROUPS
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cdr",
                            "cdr.h")).read()
    assert int(re.search(r"#define CDR_SYNC_GROUP (\d+)", hdr).group(1)) == abi.SYNC_GROUP
    abi.check_layouts()


def test_plan_sync_is_stable_and_groups_strangers_last():
    rng = np.random.default_rng(5)
    n_states = 7
    wfs = rng.integers(-2, n_states + 3, 200)
    reqs = sync.Requests(sync.request(int(w), 1, 1, tag=i) for i, w in enumerate(wfs))
    order, off = sync.plan(reqs, n_states)
    assert len(off) == n_states + 2 and off[0] == 0 and off[-1] == 200
    assert sorted(order.tolist()) == list(range(200))
    for s in range(n_states):
        mine = order[off[s]:off[s + 1]].tolist()
        assert mine == [i for i in range(200) if wfs[i] == s]  # arrival order kept
    assert order[off[n_states]:].tolist() == [i for i in range(200) if wfs[i] < 0 or wfs[i] >= n_states]
    order, off = sync.plan(sync.Requests(), 3)
    assert len(order) == 0 and off.tolist() == [0] * 5


def test_edge_shapes_hold_what_they_claim():
    """The hand-made batch of the GPU edge test, through the reference alone (CPU)."""
    entries, reqs = _edge_batch(abi.SYNC_GROUP)
    assert len(entries) == 65
    st = _state(entries, slack=lambda w: (w + 1) % 3, fill=FILL)
    before = ref.rbytes(st.tables["act"])
    want = ref.sync(st, reqs)
    assert {r.action for r in want} >= {
        abi.SYNC_SKIP_NO_WORKFLOW, abi.SYNC_SKIP_NOT_RUNNING, abi.SYNC_SKIP_HEARTBEAT_OLDER, abi.SYNC_APPLIED,
        abi.SYNC_E_STATE, abi.SYNC_SKIP_NO_ACTIVITY, abi.SYNC_RETRY_NDC}
    assert {r.code for r in want} >= {abi.OK, abi.E_VH_EMPTY, abi.P_UNKNOWN_WF_STATE}
    by_tag = {r.tag: r for r in want}
    assert [by_tag[t].action for t in (1, 2, 3, 4, 5)] == [
        abi.SYNC_APPLIED, abi.SYNC_SKIP_HEARTBEAT_OLDER, abi.SYNC_APPLIED, abi.SYNC_SKIP_HEARTBEAT_OLDER,
        abi.SYNC_APPLIED]
    # ties: across rows the smaller schedule id, within a row ScheduleToClose first
    assert by_tag[6].timer_task.event_id == 20 and by_tag[6].task_row != by_tag[6].act_row
    assert by_tag[6].timer_task.timeout_type == abi.TIMEOUT_SCHEDULE_TO_CLOSE
    assert not by_tag[7].flags & abi.SYNC_HAS_TIMER_TASK  # the head's bit is set already
    assert by_tag[8].flags & abi.SYNC_RESET_TIMER_STATUS and by_tag[8].flags & abi.SYNC_HAS_TIMER_TASK
    assert by_tag[10].timer_task.timeout_type == abi.TIMEOUT_SCHEDULE_TO_CLOSE
    # the NDC state without items: schedule id 12 >= next 12 asks for the last write version,
    # schedule id 10 does not
    assert (by_tag[12].action, by_tag[12].code) == (abi.SYNC_SKIP_STALE_VERSION, abi.E_VH_EMPTY)
    assert (by_tag[13].action, by_tag[13].code) == (abi.SYNC_APPLIED, abi.OK)
    # an entry without a request, and the slack rows, keep their fill
    after = ref.rbytes(st.tables["act"])
    sz = C.sizeof(abi.CdrActivityInfo)
    last = st.plan.caps[len(entries) - 1]
    assert after[last.act_off * sz:] == before[last.act_off * sz:]
    assert after != before and before[-sz:] == bytes([FILL]) * sz


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_gpu_kats(engine_gpu):
    st, reqs = _kat_batch()
    want_state = ref.copy_state(st)
    want = ref.sync(want_state, reqs)
    got, got_state = _run(engine_gpu, st, reqs)
    _check_kats(got)
    _results_equal(got, want)
    assert ref.rbytes(got_state.tables["act"]) == ref.rbytes(want_state.tables["act"])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,builder", FIXTURES)
def test_gpu_matches_reference(engine_gpu, cfg, builder):
    """Results and every byte of state.act equal the reference, through both entry points,
    and a second run from the same input gives the same bytes; then once more with every
    other group size the kernel is built for."""
    b, _, _, st, reqs, want_state, want = _fixture(cfg, builder)
    raw = []
    for via in ("batch", "async", "batch"):
        got, got_state = _run(engine_gpu, st, reqs, via, b.cluster)
        _results_equal(got, want, via)
        assert ref.rbytes(got_state.tables["act"]) == ref.rbytes(want_state.tables["act"]), via
        raw.append(b"".join(ref.rbytes(r) for r in got))
    assert raw[0] == raw[1] == raw[2]
    for G in abi.SYNC_GROUPS:
        if G == abi.SYNC_GROUP:
            continue
        prev = engine_gpu.set_sync_group(G)
        try:
            got, got_state = _run(engine_gpu, st, reqs, "batch", b.cluster)
        finally:
            engine_gpu.set_sync_group(prev)
        _results_equal(got, want, G)
        assert ref.rbytes(got_state.tables["act"]) == ref.rbytes(want_state.tables["act"]), G


def _edge_batch(G):
    """Hand-made neighbours: row counts around the group size G and the wave width, request
    counts 0 / 1 / 2 / 40, ties, large schedule ids, failed and odd records."""
    big = (1 << 31) - 3
    entries, reqs = [], []

    def rows(n, first=10, **kw):
        return [_act(first + 2 * j, hb=30 if j % 3 == 0 else 0, started=j % 2 == 1, attempt=j % 3, **kw)
                for j in range(n)]

    def req(w, a, dv=0, da=0, started=None, hb=None, tag=0):
        started = (a.started_id != abi.EMPTY_EVENT_ID) if started is None else started
        return sync.request(w, a.schedule_id, a.version + dv, a.attempt + da, a.scheduled_time,
                            a.schedule_id + 1 if started else abi.EMPTY_EVENT_ID,
                            a.scheduled_time + SEC if started else 0,
                            hb if hb is not None else a.scheduled_time + 2 * SEC, tag)
    counts = [0, 1, G - 1, G, G + 1, 63, 64, 65, 130]
    per_state = [0, 1, 2, 40]
    for i, n in enumerate(counts):  # every count with every request count, as neighbours
        for k in per_state:
            w = len(entries)
            rr = rows(n, first=big if i % 2 else 10)
            nxt = (rr[-1].schedule_id if rr else 20) + 10
            entries.append(_entry(rr, BUILDERS[w % 3], 100, nxt))
            for t in range(k):
                if not rr:
                    reqs.append(sync.request(w, 12 + t, 100, tag=w * 100 + t))
                    continue
                a = rr[(t * 7) % n]
                reqs.append(req(w, a, dv=(0, 10, 1, 0)[t % 4], da=(0, 1, 0, -1)[t % 4], started=t % 3 != 0,
                                hb=a.scheduled_time + (2 + t % 5) * SEC, tag=w * 100 + t))
    # the same activity twice, the second heartbeat older; then an unstarted activity with a
    # heartbeat followed by an older one (only the new flag bit tells it is set)
    w = len(entries)
    rr = rows(5)
    entries.append(_entry(rr, abi.BUILDER_NDC, 100, 40))
    reqs += [req(w, rr[1], hb=T0 + 50 * SEC, tag=1), req(w, rr[1], hb=T0 + 40 * SEC, tag=2),
             req(w, rr[2], started=False, hb=T0 + 50 * SEC, tag=3), req(w, rr[2], started=False, hb=T0 + 40 * SEC, tag=4),
             req(w, rr[2], started=False, hb=T0 + 50 * SEC, tag=5)]
    # exact ties in the pick: within a row (ScheduleToClose == ScheduleToStart, and == Heartbeat)
    # and across rows (same time, the smaller schedule id wins); a head whose bit is set already
    w = len(entries)
    tie = [_act(30, s2c=60, s2s=60), _act(20, s2c=60, s2s=90), _act(40, s2c=61, stc=60, hb=60, started=True),
           _act(50, s2c=60, s2s=60)]
    tie.sort(key=lambda a: a.schedule_id)
    entries.append(_entry(tie, abi.BUILDER_2DC, 100, 100))
    reqs += [req(w, tie[3], tag=6), req(w, tie[1], tag=7), req(w, tie[0], da=1, tag=8), req(w, tie[0], da=1, tag=9)]
    w = len(entries)
    one = [_act(70, s2c=61, stc=60, hb=60, started=True)]
    one[0].last_heartbeat_time = one[0].started_time  # StartToClose == Heartbeat; ScheduleToClose == both
    entries.append(_entry(one, abi.BUILDER_LOCAL, 100, 100))
    reqs += [sync.request(w, 70, 100, 0, T0, 71, T0 + SEC, T0 + SEC, tag=10)]
    # a failed record, an NDC state without version-history items, an unknown workflow state,
    # closed and zombie ones, a workflow that is not found and one past the states
    w = len(entries)
    entries.append(_entry(rows(3), code=abi.E_HISTORY_EMPTY))
    entries.append(_entry(rows(3), abi.BUILDER_NDC, n_vh=0, nxt=12))
    entries.append(_entry(rows(3), state=abi.STATE_VOID))
    entries.append(_entry(rows(3), state=abi.STATE_ZOMBIE))
    reqs += [sync.request(w, 10, 100, tag=11), sync.request(w + 1, 12, 100, tag=12),
             sync.request(w + 1, 10, 100, tag=13), sync.request(w + 2, 10, 100, tag=14), sync.request(w + 3, 10, 100, tag=15),
             sync.request(-1, 10, 100, tag=16), sync.request(10_000, 10, 100, tag=17)]
    # more neighbours of mixed sizes up to 64 records, one request each (more than one
    # wavefront of groups at every group size), then a state no request addresses
    while len(entries) < 64:
        w = len(entries)
        rr = rows(1 + (5 * w) % 23)
        entries.append(_entry(rr, BUILDERS[w % 3], 100, rr[-1].schedule_id + 5))
        reqs.append(req(w, rr[w % len(rr)], da=w % 2, tag=w * 100))
    entries.append(_entry(rows(G + 2)))
    order = np.random.default_rng(G).permutation(len(reqs))
    by_wf = {}
    for q in reqs:  # shuffle the arrival order, each workflow's requests staying in order
        by_wf.setdefault(q.wf, []).append(q)
    cursor = {k: 0 for k in by_wf}
    mixed = []
    for i in order:
        k = reqs[int(i)].wf
        mixed.append(by_wf[k][cursor[k]])
        cursor[k] += 1
    return entries, mixed


@pytest.mark.gpu
@pytest.mark.parametrize("n_states", [1, 9, 65])
@pytest.mark.parametrize("G", abi.SYNC_GROUPS)
def test_gpu_edge_shapes_and_containment(engine_gpu, G, n_states):
    """The hand-made shapes with every group size the kernel is built for (the shipped one
    among them), on the first n_states records (65: all of them and more than one wavefront
    of groups).  Rows past each entry's count and whole entries without a request were
    pre-filled with 0xA5 and come back untouched — state.act equals the reference's bytes."""
    entries, reqs = _edge_batch(G)
    if n_states < 65:
        entries = entries[:n_states]
        reqs = [q for q in reqs if q.wf < n_states]  # wf = -1 stays
    assert len(entries) == n_states
    st = _state(entries, slack=lambda w: (w + 1) % 3, fill=FILL)
    reqs = sync.Requests(reqs)
    want_state = ref.copy_state(st)
    want = ref.sync(want_state, reqs)
    prev = engine_gpu.set_sync_group(G)
    try:
        got, got_state = _run(engine_gpu, st, reqs)
    finally:
        engine_gpu.set_sync_group(prev)
    _results_equal(got, want)
    assert ref.rbytes(got_state.tables["act"]) == ref.rbytes(want_state.tables["act"])


@pytest.mark.gpu
def test_gpu_synced_state_carries_into_a_replay(engine_gpu):
    """A state synced on the GPU, used as cdr_carry.state for its suffix replay, equals the
    oracle's replay of the same suffix onto the reference-synced state.

    The oracle does not know CDR_AI_HEARTBEAT_TIME_SET (schema.h): it loads such a row's
    heartbeat time as zero unless CDR_AI_STARTED_TIME_SET is set, and writes neither back,
    while the replay kernels carry a row they do not touch byte for byte.  So the kernels'
    rows are read the oracle's way before the comparison — the bit cleared, and the heartbeat
    time zero where the started-time bit is clear; every other byte must be equal."""
    import oracle
    b, pre, cut, st, reqs, want_state, _ = _fixture(3, abi.BUILDER_NDC)
    _, got_state = _run(engine_gpu, st, reqs, "batch", b.cluster)
    sb_gpu = engine.suffix_batch(b, cut, pre, got_state)
    sb_ref = engine.suffix_batch(b, cut, pre, want_state)
    assert int((sb_gpu.carry.src >= 0).sum()) > 100
    got = engine_gpu.replay(sb_gpu)
    want = oracle.replay(sb_ref)
    carried = 0
    for w in range(sb_gpu.n_wfs):
        if got.result[w].code != abi.OK:
            continue
        for a in got.rows(w, "act"):  # references into the table
            if a.flags & abi.AI_HEARTBEAT_TIME_SET:
                carried += 1
                a.flags &= ~abi.AI_HEARTBEAT_TIME_SET
                if not a.flags & abi.AI_STARTED_TIME_SET:
                    a.last_heartbeat_time = 0
    assert carried > 0  # synced rows did pass through the replay
    bad = engine.compare(sb_gpu, got, want)
    assert not bad, bad[:5]


@pytest.mark.gpu
def test_gpu_argument_errors(engine_gpu):
    L = abi.lib()
    st, reqs = _kat_batch()
    order, off = sync.plan(reqs, st.n_wfs)
    res = (abi.CdrSyncResult * len(reqs))()
    cl = engine.default_cluster()
    args = lambda cluster, state: (engine_gpu.ctx, C.addressof(reqs.arr), off.ctypes.data, len(reqs), st.n_wfs,  # noqa: E731
                                   C.addressof(st.plan.caps), C.byref(st.plan.totals), state, cluster,
                                   C.addressof(res), None)
    bad = engine.default_cluster()
    bad.failover_version_increment = 0
    assert L.cdr_sync_activity_batch(*args(C.byref(bad), C.byref(st.cstruct()))) == -1
    assert L.cdr_sync_activity_batch(*args(None, C.byref(st.cstruct()))) == -1
    assert L.cdr_sync_activity_batch(*args(C.byref(cl), None)) == -1
    assert L.cdr_sync_activity_async(engine_gpu.ctx, None, off.ctypes.data, len(reqs), st.n_wfs,
                                     C.addressof(st.plan.caps), C.byref(st.cstruct()), C.byref(cl),
                                     C.addressof(res), None) == -1
    with pytest.raises(ValueError):
        engine_gpu.set_sync_group(5)
    fresh = engine.Engine(0)  # the library's default is the mirror's
    try:
        assert fresh.set_sync_group(abi.SYNC_GROUP) == abi.SYNC_GROUP
    finally:
        fresh.close()
