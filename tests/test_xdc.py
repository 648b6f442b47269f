"""Batched 2DC replication rounds: historyReplicator.ApplyEvents on the device
(cdr_xdc_admit_host / cdr_xdc_admit_async / cdr_xdc_replicate_async;
service/history/historyReplicator.go:339-763, conflictResolver.go:66-184).

The reference is tests/xdc_ref.py: a plain-Python restatement of the decision tree and of the
round over oracle.replay.  CPU: both the reference and cdr_xdc_admit_host give the answers of
the reference project's own suite (historyReplicator_test.go, as data: inputs, verdict,
checkpoint, CAS triple); hand-made tasks reach every action, reason and new error code; 10k
tasks drawn around every comparison's boundary agree field for field; and the reference round
on config-3 histories cut at a checkpoint equals the replay of checkpoint prefix + incoming
suffix.  GPU: k_xdc_admit equals the host function byte for byte; the round equals the reference
round in decisions, both replay outputs and the whole state, over two rounds on device-resident
states, without allocating once warm.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from cadence_amd import abi, engine, xdc
from tests import xdc_ref as ref

FILL = 0xA5
CUR, ALT = 0, 1
RUN, DONE = abi.STATE_RUNNING, abi.STATE_COMPLETED
DT = abi.EV["DecisionTaskScheduled"]
STARTED = abi.EV["WorkflowExecutionStarted"]


def _cluster(inc=10, initial=(0, 1), current=CUR):
    m = abi.CdrClusterMeta(failover_version_increment=inc, current_cluster=current, n_clusters=len(initial))
    for i, v in enumerate(initial):
        m.initial_version[i] = v
    return m


class _N:
    def __init__(self, n):
        self.n_wfs = n


def _states(rows):
    """Hand-made target records: one dict per workflow (None: no state — its record is left
    zero) with lwv, lweid, lri {cluster: (version, last_event_id)}, state, next, code, present."""
    n = len(rows)
    out = engine.Outputs(_N(n), engine.Plan(caps=(abi.CdrWfCaps * max(1, n))(), totals=abi.CdrTotals()))
    for w, s in enumerate(rows):
        if s is None:
            continue
        out.result[w].code = s.get("code", abi.OK)
        out.exec[w].state = s.get("state", RUN)
        out.exec[w].next_event_id = s.get("next", 99)
        rs = out.repl[w]
        rs.present = s.get("present", 1)
        rs.current_version = rs.start_version = rs.last_write_version = s.get("lwv", 0)
        rs.last_write_event_id = s.get("lweid", 98)
        for c, (v, e) in s.get("lri", {}).items():
            rs.lri_mask |= 1 << c
            rs.lri_version[c], rs.lri_last_event_id[c] = v, e
    return out


def _tasks(rows, states):
    tasks = xdc.new_tasks(len(rows))
    for w, t in enumerate(rows):
        t = dict(t)
        flags = t.pop("flags", 0) | (abi.XDC_NO_STATE if states[w] is None else 0)
        xdc.fill_task(tasks[w], flags=flags, **t)
    return tasks


# ------------------------------------------------------------------------------- KATs
# historyReplicator_test.go, one row per test: (test name, :line, cluster, state, task, expected fields)
_RUNNING_CUR = dict(running=True, last_write_version=124, next_event_id=2333)
_ACTIVE = dict(lwv=10, lweid=98, state=RUN)
KATS = [
    ("ApplyOtherEventsMissingMutableState_MissingCurrent", 712, _cluster(), None, dict(version=123),
     dict(action="RETRY", reason="MISSING_NO_CURRENT", hint_run=0, hint_next_event_id=1)),
    ("ApplyOtherEventsMissingMutableState_IncomingLessThanCurrent_NoEventsReapplication", 738, _cluster(), None,
     dict(version=123, cur=_RUNNING_CUR), dict(action="REAPPLY", reason="MISSING_STALE", reapply_to=1)),
    ("ApplyOtherEventsMissingMutableState_IncomingLessThanCurrent_EventsReapplication_PendingDecision", 798,
     _cluster(), None, dict(version=123, cur=_RUNNING_CUR),
     dict(action="REAPPLY", reason="MISSING_STALE", reapply_to=1)),
    ("ApplyOtherEventsMissingMutableState_IncomingLessThanCurrent_EventsReapplication_NoPendingDecision", 883,
     _cluster(), None, dict(version=123, cur=_RUNNING_CUR),
     dict(action="REAPPLY", reason="MISSING_STALE", reapply_to=1)),
    ("ApplyOtherEventsMissingMutableState_IncomingEqualToCurrent_CurrentRunning", 987, _cluster(), None,
     dict(version=123, cur=dict(running=True, last_write_version=123, next_event_id=2333)),
     dict(action="RETRY", reason="MISSING_SAME_RUNNING", hint_run=1, hint_next_event_id=2333)),
    ("ApplyOtherEventsMissingMutableState_IncomingEqualToCurrent_CurrentRunning_OutOfOrder", 1055, _cluster(), None,
     dict(version=123, last_event_task_id=5667,
          cur=dict(running=True, last_write_version=123, next_event_id=2333, last_event_task_id=5677)),
     dict(action="DROP", reason="MISSING_SAME_OLDER_TASK")),
    ("ApplyOtherEventsMissingMutableState_IncomingLargerThanCurrent_CurrentRunning", 1127, _cluster(), None,
     dict(version=123, cur=dict(running=True, last_write_version=23, next_event_id=2333)),
     dict(action="RETRY", reason="MISSING_NEWER", terminate_current_first=1, hint_run=0, hint_next_event_id=1)),
    ("ApplyOtherEventsMissingMutableState_IncomingNotLessThanCurrent_CurrentFinished", 1203, _cluster(), None,
     dict(version=123, cur=dict(running=False, last_write_version=23, next_event_id=2333)),
     dict(action="RETRY", reason="MISSING_NEWER", terminate_current_first=0, hint_run=0, hint_next_event_id=1)),
    ("WorkflowReset", 1271, _cluster(), None,
     dict(version=123, flags=abi.XDC_RESET_WORKFLOW, cur=dict(running=False, last_write_version=23, next_event_id=2333)),
     dict(action="APPLY_RESET_EVENT", reason="MISSING_NEWER_RESET", terminate_current_first=0)),
    ("ApplyOtherEventsMissingMutableState_IncomingLessThanCurrent", 1344, _cluster(), None,
     dict(version=123, cur=dict(running=False, last_write_version=223)),
     dict(action="REAPPLY", reason="MISSING_STALE", reapply_to=1)),
    ("ApplyOtherEventsVersionChecking_IncomingLessThanCurrent_WorkflowClosed_WorkflowIsCurrent_NoEventsReapplication",
     1409, _cluster(), dict(lwv=123, state=DONE), dict(version=110, cur=dict(is_self=True, last_write_version=123)),
     dict(action="REAPPLY", reason="STALE_SELF", reapply_to=0)),
] + [
    ("ApplyOtherEventsVersionChecking_IncomingLessThanCurrent_WorkflowClosed_WorkflowIsNotCurrent_" + name, line,
     _cluster(), dict(lwv=123, state=DONE), dict(version=110, cur=dict(running=True, last_write_version=123)),
     dict(action="REAPPLY", reason="STALE_OTHER", reapply_to=1))
    for name, line in (("NoEventsReapplication", 1454), ("EventsReapplication_PendingDecision", 1516),
                       ("EventsReapplication_NoPendingDecision", 1604))
] + [
    ("ApplyOtherEventsVersionChecking_IncomingLessThanCurrent_WorkflowRunning_" + name, line, _cluster(),
     dict(lwv=123, state=RUN), dict(version=110), dict(action="REAPPLY", reason="STALE_RUNNING", reapply_to=0))
    for name, line in (("NoEventsReapplication", 1703), ("EventsReapplication_PendingDecision", 1732),
                       ("EventsReapplication_NoPendingDecision", 1783))
] + [
    ("ApplyOtherEventsVersionChecking_IncomingEqualToCurrent", 1846, _cluster(), dict(lwv=110, next=99),
     dict(version=110, first_event_id=99), dict(action="APPLY", via=abi.XDV_SAME_VERSION)),
    ("ApplyOtherEventsVersionChecking_IncomingGreaterThanCurrent_CurrentWasNotActive_SameCluster", 1867,
     _cluster(10, (1, 0)), dict(lwv=10, next=99), dict(version=20, first_event_id=99),
     dict(action="APPLY", via=abi.XDV_SAME_CLUSTER)),
    ("ApplyOtherEventsVersionChecking_IncomingGreaterThanCurrent_CurrentWasNotActive_DiffCluster", 1895,
     _cluster(20, (1, 10)), dict(lwv=10), dict(version=20),
     dict(action="DROP", reason="E_MORE_THAN_2DC", code=abi.E_XDC_MORE_THAN_2DC)),
    ("ApplyOtherEventsVersionChecking_IncomingGreaterThanCurrent_CurrentWasActive_MissingReplicationInfo", 1923,
     _cluster(), dict(_ACTIVE, lri={ALT: (0, 87)}), dict(version=20),
     dict(action="RESET_APPLY", reason="RESET_REJECTED", reset_event_id=87, cas_prev_is_self=1,
          cas_prev_last_write_version=10, cas_prev_state=RUN)),
    ("ApplyOtherEventsVersionChecking_IncomingGreaterThanCurrent_CurrentWasActive_ReplicationInfoVersionLocalLarger",
     1989, _cluster(), dict(lwv=120, lweid=980, state=RUN, lri={ALT: (100, 965)}),
     dict(version=130, replication_info={CUR: (90, 945)}),
     dict(action="RESET_APPLY", reason="RESET_REJECTED", reset_event_id=965, cas_prev_is_self=1,
          cas_prev_last_write_version=120, cas_prev_state=RUN)),
    ("ApplyOtherEventsVersionChecking_IncomingGreaterThanCurrent_CurrentWasActive_ReplicationInfoVersionLocalSmaller",
     2062, _cluster(), _ACTIVE, dict(version=20, replication_info={CUR: (20, 98)}),
     dict(action="DROP", reason="E_REMOTE_HIGHER_VERSION", code=abi.E_XDC_REMOTE_HIGHER_VERSION)),
    ("ApplyOtherEventsVersionChecking_IncomingGreaterThanCurrent_CurrentWasActive_ReplicationInfoVersionEqual_"
     "ResolveConflict", 2098, _cluster(), _ACTIVE, dict(version=20, replication_info={CUR: (10, 88)}),
     dict(action="RESET_APPLY", reason="RESET_CONFLICT", reset_event_id=88, cas_prev_is_self=1,
          cas_prev_last_write_version=10, cas_prev_state=RUN)),
    ("ApplyOtherEventsVersionChecking_IncomingGreaterThanCurrent_CurrentWasActive_ReplicationInfoVersionEqual_"
     "Corrputed", 2163, _cluster(), _ACTIVE, dict(version=20, replication_info={CUR: (10, 108)}),
     dict(action="DROP", reason="E_CORRUPTED_REPL_INFO", code=abi.E_XDC_CORRUPTED_REPL_INFO)),
    ("ApplyOtherEventsVersionChecking_IncomingGreaterThanCurrent_CurrentWasActive_ReplicationInfoVersionEqual_"
     "NoBufferedEvent_NoOp", 2203, _cluster(), dict(_ACTIVE, next=99),
     dict(version=20, first_event_id=99, replication_info={CUR: (10, 98)}),
     dict(action="APPLY", via=abi.XDV_EVENT_ID_MATCH)),
    # the reference flushes the buffer itself (a DecisionTaskFailed event: LastWriteEventID 98 -> 100) and goes
    # on; here the caller flushes and resubmits: two calls
    ("ApplyOtherEventsVersionChecking_IncomingGreaterThanCurrent_CurrentWasActive_ReplicationInfoVersionEqual_"
     "BufferedEvent_ResolveConflict", 2243, _cluster(), _ACTIVE,
     dict(version=20, flags=abi.XDC_HAS_BUFFERED, replication_info={CUR: (10, 98)}),
     dict(action="FLUSH_BUFFER", reason="FLUSH_BUFFER")),
    ("ApplyOtherEventsVersionChecking_IncomingGreaterThanCurrent_CurrentWasActive_ReplicationInfoVersionEqual_"
     "BufferedEvent_ResolveConflict (resubmitted)", 2243, _cluster(), dict(_ACTIVE, lweid=100),
     dict(version=20, replication_info={CUR: (10, 98)}),
     dict(action="RESET_APPLY", reason="RESET_CONFLICT", reset_event_id=98, cas_prev_is_self=1,
          cas_prev_last_write_version=10, cas_prev_state=RUN)),
    ("ApplyOtherEvents_IncomingLessThanCurrent", 2345, _cluster(), dict(lwv=4096, next=10),
     dict(version=4096, first_event_id=6), dict(action="DROP", reason="DUPLICATE")),
    ("ApplyOtherEvents_IncomingGreaterThanCurrent", 2369, _cluster(), dict(lwv=8192, next=10, state=RUN),
     dict(version=8192, first_event_id=14, n_events=4),
     dict(action="RETRY", reason="BUFFER", hint_run=0, hint_next_event_id=10)),
    ("ApplyReplicationTask_WorkflowClosed", 2411, _cluster(), dict(lwv=8192, next=14, state=DONE),
     dict(version=8192, first_event_id=14, n_events=4), dict(action="DROP", reason="CLOSED")),
    # conflictResolutionTerminateCurrentRunningIfNotSelf, reached through a rejected-by-remote reset
    # (the local map's checkpoint: version 1390, event 50; 1394 % 10 = 4 is this cluster's)
    ("ConflictResolutionTerminateCurrentRunningIfNotSelf_TargetRunning", 4245, _cluster(10, (4, 6)),
     dict(lwv=1394, state=RUN, lri={ALT: (1386, 50)}), dict(version=4096),
     dict(action="RESET_APPLY", reset_event_id=50, cas_prev_is_self=1, cas_prev_last_write_version=1394,
          cas_prev_state=RUN, terminate_current_first=0)),
    ("ConflictResolutionTerminateCurrentRunningIfNotSelf_TargetClosed_CurrentClosed", 4273, _cluster(10, (4, 6)),
     dict(lwv=1384, state=DONE, lri={ALT: (1376, 50)}),
     dict(version=4096, cur=dict(last_write_version=1394, state=DONE, close_status=abi.CLOSE_COMPLETED)),
     dict(action="RESET_APPLY", reset_event_id=50, cas_prev_is_self=0, cas_prev_last_write_version=1394,
          cas_prev_state=DONE, terminate_current_first=0, flags=0)),
    ("ConflictResolutionTerminateCurrentRunningIfNotSelf_TargetClosed_CurrentRunning_LowerVersion", 4318,
     _cluster(10, (4, 6)), dict(lwv=1384, state=DONE, lri={ALT: (1376, 50)}),
     dict(version=4096, cur=dict(running=True, last_write_version=4086)),
     dict(action="RESET_APPLY", reset_event_id=50, cas_prev_is_self=0, cas_prev_last_write_version=4086,
          cas_prev_state=DONE, terminate_current_first=1, flags=abi.XDD_CAS_VERSION_FROM_TERMINATE)),
    ("ConflictResolutionTerminateCurrentRunningIfNotSelf_TargetClosed_CurrentRunning_NotLowerVersion", 4388,
     _cluster(10, (4, 6)), dict(lwv=1384, state=DONE, lri={ALT: (1376, 50)}),
     dict(version=4096, cur=dict(running=True, last_write_version=4096)),
     dict(action="DROP", reason="RESET_ABANDONED")),
]

# hand-made: the exits the reference suite does not visit
EXTRA = [
    ("empty task", _cluster(), _ACTIVE, dict(version=20, n_events=0), dict(action="DROP", reason="EMPTY_TASK")),
    ("duplicate start", _cluster(), _ACTIVE, dict(version=20, first_event_type=STARTED),
     dict(action="DROP", reason="DUPLICATE_START")),
    ("start", _cluster(), None, dict(version=20, first_event_type=STARTED),
     dict(action="APPLY_FRESH", reason="START")),
    ("missing, same version, closed, reset", _cluster(), None,
     dict(version=20, flags=abi.XDC_RESET_WORKFLOW, cur=dict(last_write_version=20)),
     dict(action="APPLY_RESET_EVENT", reason="MISSING_SAME_RESET")),
    ("missing, same version, closed", _cluster(), None, dict(version=20, cur=dict(last_write_version=20)),
     dict(action="RETRY", reason="MISSING_SAME_CLOSED", hint_run=0, hint_next_event_id=1)),
    ("missing, newer, running, reset", _cluster(), None,
     dict(version=20, flags=abi.XDC_RESET_WORKFLOW, cur=dict(running=True, last_write_version=10)),
     dict(action="APPLY_RESET_EVENT", reason="MISSING_NEWER_RESET", terminate_current_first=1)),
    ("a gap, closed", _cluster(), dict(lwv=20, next=10, state=DONE), dict(version=20, first_event_id=12),
     dict(action="DROP", reason="CLOSED_AHEAD")),
    ("apply", _cluster(), dict(lwv=20, next=10), dict(version=20, first_event_id=10),
     dict(action="APPLY", reason="APPLY", via=abi.XDV_SAME_VERSION)),
    ("failed state", _cluster(), dict(_ACTIVE, code=abi.E_BAD_INPUT), dict(version=20),
     dict(action="DROP", reason="E_STATE", code=abi.E_BAD_INPUT)),
    ("no replication state", _cluster(), dict(_ACTIVE, present=0), dict(version=20),
     dict(action="DROP", reason="E_STATE", code=abi.E_BAD_INPUT)),
    ("closed target needs a reset, no current run", _cluster(), dict(_ACTIVE, state=DONE, lri={ALT: (1, 50)}),
     dict(version=20), dict(action="DROP", reason="E_NO_CURRENT", code=abi.E_BAD_INPUT)),
    ("unknown workflow state", _cluster(), dict(lwv=20, next=10, state=abi.STATE_VOID),
     dict(version=20, first_event_id=10), dict(action="DROP", reason="E_WF_STATE", code=abi.P_UNKNOWN_WF_STATE)),
    ("unowned version", _cluster(), dict(_ACTIVE, lwv=15), dict(version=20),
     dict(action="DROP", reason="E_CLUSTER", code=abi.P_UNKNOWN_CLUSTER)),
    ("no checkpoint", _cluster(), _ACTIVE, dict(version=20),
     dict(action="DROP", reason="E_MISSING_REPL_INFO", code=abi.E_XDC_MISSING_REPL_INFO)),
    # getLatestCheckpoint's order: remote before local, a later entry only on a strictly greater version
    ("checkpoint: remote wins a tie", _cluster(10, (0, 1, 2)), dict(_ACTIVE, lri={ALT: (5, 70)}),
     dict(version=20, replication_info={ALT: (5, 60), 2: (4, 40)}),
     dict(action="RESET_APPLY", reason="RESET_REJECTED", reset_event_id=60)),
]


def _expect(got, want, what):
    for k, v in want.items():
        g = getattr(got, k)
        if k == "action":
            g, v = abi.XDC_ACTIONS[g], v
        elif k == "reason":
            g = abi.XDC_REASONS[g]
        assert g == v, (what, k, g, v)
    if "code" not in want:
        assert got.code == abi.OK, (what, abi.STATUS.get(got.code))


def _run_cases(cases, fn):
    """fn(tasks, n, states, cluster) over the cases, grouped by cluster metadata"""
    got = [None] * len(cases)
    groups = {}
    for i, c in enumerate(cases):
        groups.setdefault(bytes(c[-4]), []).append(i)
    for idx in groups.values():
        st_rows = [cases[i][-3] for i in idx]
        states = _states(st_rows)
        tasks = _tasks([cases[i][-2] for i in idx], st_rows)
        dec = fn(tasks, len(idx), states, cases[idx[0]][-4])
        for j, i in enumerate(idx):
            got[i] = abi.CdrXdcDecision.from_buffer_copy(dec[j])
    return got


@pytest.mark.parametrize("side", ["reference", "host"])
def test_reference_suite_cases(side):
    """historyReplicator_test.go's cases as data: the reference restatement and
    cdr_xdc_admit_host both give the reference's verdict, checkpoint and CAS triple."""
    fn = ref.admit if side == "reference" else xdc.admit_host
    got = _run_cases(KATS, fn)
    for c, g in zip(KATS, got):
        _expect(g, c[-1], f"{c[0]} (:{c[1]})")


def test_every_action_reason_and_code_is_reached():
    """KATs + hand-made tasks: host == reference, every expectation holds, and no enumerator of
    cdr_xdc_action / cdr_xdc_reason (the round's two aside) or new status is left out."""
    cases = [c[:1] + c[2:] for c in KATS] + EXTRA
    host = _run_cases(cases, xdc.admit_host)
    py = _run_cases(cases, ref.admit)
    for c, h, p in zip(cases, host, py):
        assert not ref.diff(h, p), (c[0], ref.diff(h, p))
        _expect(h, c[-1], c[0])
    missing = [a for i, a in enumerate(abi.XDC_ACTIONS) if i not in {h.action for h in host}]
    missing += [r for i, r in enumerate(abi.XDC_REASONS)
                if i not in {h.reason for h in host} and r not in abi.XDR_ROUND_ONLY]
    missing += [abi.STATUS[c] for c in (26, 27, 28, 29, abi.P_UNKNOWN_CLUSTER, abi.E_BAD_INPUT)
                if c not in {h.code for h in host}]
    assert not missing, missing
    assert len(abi.XDC_REASONS) == 33 and len(abi.XDC_ACTIONS) == 8


@functools.lru_cache(maxsize=None)
def _random_cases(n=10000, seed=0xD2C):
    """Tasks drawn around each comparison's boundary (versions +-1 and +-increment, event ids
    +-1, every flag), cluster metadata (increment 10, initial versions 0 and 1)."""
    rng = np.random.default_rng(seed)
    m = _cluster()
    pick = lambda xs, p=None: xs[int(rng.choice(len(xs), p=p))]  # noqa: E731
    st_rows, t_rows = [], []
    for _ in range(n):
        lwv = pick([10, 11, 20, 21, 13, -10, -9, abi.EMPTY_VERSION])
        lweid = int(rng.integers(5, 200))
        nxt = lweid + 1
        s = dict(lwv=lwv, lweid=lweid, next=nxt, state=pick([0, 1, 2, 3, 4], [.1, .4, .3, .1, .1]),
                 code=pick([abi.OK, abi.E_BAD_INPUT], [.95, .05]), present=pick([1, 0], [.95, .05]),
                 lri={c: (lwv + pick([-20, -10, -9, -1]), lweid + pick([-7, -3, -1])) for c in (0, 1) if rng.random() < .5})
        version = lwv + pick([-10, -1, 0, 1, 9, 10, 20])
        lev = version + pick([-1, 0, 1], [.1, .8, .1])
        task_id = int(rng.integers(100, 200))
        flags = 0
        for f in (abi.XDC_RESET_WORKFLOW, abi.XDC_HAS_BUFFERED):
            flags |= f if rng.random() < .3 else 0
        cur = None
        if rng.random() < .7:
            cur = dict(is_self=rng.random() < .3, running=rng.random() < .5,
                       last_write_version=pick([lev, version]) + pick([-1, 0, 1]),
                       last_event_task_id=task_id + pick([-1, 0, 1]), next_event_id=int(rng.integers(1, 500)),
                       state=pick([0, 1, 2, 3]), close_status=pick([0, 1, 4], [.5, .3, .2]))
        t = dict(version=version, first_event_id=nxt + pick([-1, 0, 1]), n_events=pick([0, 1, 5], [.03, .47, .5]),
                 first_event_type=pick([STARTED, DT], [.05, .95]), last_event_version=lev,
                 last_event_task_id=task_id, flags=flags, cur=cur,
                 replication_info={c: (lwv + pick([-10, -1, 0, 1, 10]), lweid + pick([-1, 0, 1]))
                                   for c in (0, 1) if rng.random() < .6})
        st_rows.append(None if rng.random() < .15 else s)
        t_rows.append(t)
    states = _states(st_rows)
    return _tasks(t_rows, st_rows), states, m, n


def test_random_tasks_host_equals_reference():
    tasks, states, m, n = _random_cases()
    host = xdc.admit_host(tasks, n, states, m)
    py = ref.admit(tasks, n, states, m)
    bad = [(w, ref.diff(host[w], py[w])) for w in range(n) if bytes(host[w]) != bytes(py[w])]
    assert not bad, bad[:5]
    seen = {abi.XDC_REASONS[host[w].reason] for w in range(n)}
    want = set(abi.XDC_REASONS) - set(abi.XDR_ROUND_ONLY)
    assert seen == want, want - seen


def test_admit_host_rejects_bad_arguments():
    tasks, states, m, n = _random_cases()
    L = abi.lib()
    dec = xdc.new_decisions(4)
    for bad in (_cluster(0), _cluster(10, ()), _cluster(10, (0, 1), current=2)):
        assert L.cdr_xdc_admit_host(C.addressof(tasks), 4, None, C.byref(states.cstruct()), C.byref(bad),
                                    C.addressof(dec)) == -1
    assert L.cdr_xdc_admit_host(None, 4, None, C.byref(states.cstruct()), C.byref(m), C.addressof(dec)) == -1
    assert L.cdr_xdc_admit_host(None, 0, None, None, C.byref(m), None) == 0


# ------------------------------------------------------------------------------ rounds
V_LOCAL, V_REMOTE, V_THIRD = 1, 12, 13  # default cluster metadata: increment 10, clusters 0 (current), 1, 2
KINDS = ("apply", "fresh", "reset", "reset_retry", "reset_drop", "bad_prefix", "more_than_2dc", "no_checkpoint",
         "remote_higher", "corrupted", "failed_state", "stale", "small_caps")


def _ev_cols(events):
    a = np.frombuffer(events, dtype=np.uint8).reshape(-1, C.sizeof(abi.CdrEvent))
    col = lambda f, dt: a[:, f.offset:f.offset + f.size].view(dt)[:, 0]  # noqa: E731
    return col(abi.CdrEvent.event_id, np.int64), col(abi.CdrEvent.version, np.int64), col(abi.CdrEvent.type, np.uint32)


def _copy_events(events):
    ev = (abi.CdrEvent * len(events))()
    C.memmove(ev, events, C.sizeof(ev))
    return ev


def _with(batch, events=None, wfs=None):
    return engine.Batch(events=batch.events if events is None else events, wfs=batch.wfs if wfs is None else wfs,
                        kvs=batch.kvs, rps=batch.rps, cluster=batch.cluster, now_ns=batch.now_ns,
                        uuid_seed=batch.uuid_seed, empty_uuid=batch.empty_uuid)


def _copy_wfs(wfs):
    out = (abi.CdrWfDesc * len(wfs))()
    C.memmove(out, wfs, C.sizeof(out))
    return out


class Fixture:
    """n config-3 histories (2DC builder; workflows 16, 48, ... long enough for a two-page reset
    prefix), each cut at a call boundary — the checkpoint — into the events both clusters agree
    on and the rest.  Workflow w plays KINDS[w % len(KINDS)] (the long ones: "reset"):
      base    what the state buffer holds before the rounds: the whole history written by this
              cluster (version 1) for the reset kinds; the prefix at the task's version otherwise
      reset   events 1 .. checkpoint, version 1, page calls
      apply   the rest at the remote's version 12 (APPLY_FRESH: the whole history)
    round 1 resubmits round 0's tasks, the buffered ones with the event id they waited for."""

    def __init__(self, n, kinds=KINDS, seed=0x2DC):
        whole = engine.synth_batch(3, n, seed, builder=abi.BUILDER_2DC, max_len=1500, long_stride=32)
        assert whole.n_wfs == n  # no continue-as-new links
        self.n, self.cluster = n, whole.cluster
        self.kind = [("reset" if w % 32 == 16 else kinds[w % len(kinds)]) for w in range(n)]
        cut = np.zeros(n, np.int64)
        self.bad_cut = np.zeros(n, np.int64)
        for w in range(n):
            calls = engine._calls(whole, w)
            assert len(calls) >= 4
            k = len(calls) // 2
            if whole.wfs[w].ev_len > 1200:
                k = next(i for i, c in enumerate(calls) if c > 1100)
            elif self.kind[w] == "small_caps":
                k = 2  # a small state, so that the applied one outgrows its capacities
            cut[w], self.bad_cut[w] = calls[k], calls[k - 1]
        self.cut = cut
        # event arrays: `mixed` = prefix at the local version + the rest at the remote's
        base_ev, mixed_ev = _copy_events(whole.events), _copy_events(whole.events)
        _, bver, btype = _ev_cols(base_ev)
        mid, mver, _ = _ev_cols(mixed_ev)
        base_wfs, pre_wfs, suf_wfs = _copy_wfs(whole.wfs), _copy_wfs(whole.wfs), _copy_wfs(whole.wfs)
        self.tasks = [xdc.new_tasks(n), xdc.new_tasks(n)]
        for w in range(n):
            d, c, kind = whole.wfs[w], int(cut[w]), self.kind[w]
            lo, mid_, hi = d.ev_off, d.ev_off + c, d.ev_off + d.ev_len
            mver[lo:mid_], mver[mid_:hi] = V_LOCAL, V_REMOTE
            pre_wfs[w].ev_len = c
            suf_wfs[w].ev_off, suf_wfs[w].ev_len = mid_, d.ev_len - c
            e_c = int(mid[mid_ - 1])  # the checkpoint's event id
            ri, flags, first = {CUR: (V_LOCAL, e_c)}, 0, None
            if kind in ("reset", "reset_retry", "reset_drop", "bad_prefix", "no_checkpoint", "remote_higher",
                        "corrupted"):
                bver[lo:hi] = V_LOCAL  # the whole history, written here
                if kind == "bad_prefix":
                    pre_wfs[w].ev_len = int(self.bad_cut[w])
                ri = {"no_checkpoint": {}, "remote_higher": {CUR: (V_LOCAL + 10, e_c)},
                      "corrupted": {CUR: (V_LOCAL, int(mid[hi - 1]) + 5)}}.get(kind, ri)
                first = {"reset_retry": e_c + 2, "reset_drop": e_c}.get(kind)
            elif kind == "fresh":
                flags = abi.XDC_NO_STATE
                mver[lo:hi] = V_REMOTE
                suf_wfs[w].ev_off, suf_wfs[w].ev_len = lo, d.ev_len
                base_wfs[w].ev_len = c
                bver[lo:hi] = V_REMOTE
            else:  # the prefix alone is the state
                base_wfs[w].ev_len = c
                bver[lo:hi] = {"more_than_2dc": 2, "stale": V_REMOTE + 10}.get(kind, V_REMOTE)
                if kind == "failed_state":
                    btype[lo + c // 2] = 200  # no such event type: the base replay fails
            for k in (0, 1):
                # the target run is the current one; where it has closed, GetCurrentExecution says so
                t = xdc.task_from_entry(self.tasks[k][w], _with(whole, mixed_ev, suf_wfs), w, flags=flags,
                                        replication_info=ri, version=V_THIRD if kind == "more_than_2dc" else V_REMOTE,
                                        cur=dict(is_self=True, last_write_version=V_LOCAL, state=DONE,
                                                 close_status=abi.CLOSE_COMPLETED))
                if first is not None and k == 0:
                    t.first_event_id = first
        self.base = _with(whole, base_ev, base_wfs)
        self.reset = xdc.paged(_with(whole, mixed_ev, pre_wfs))
        self.apply = _with(whole, mixed_ev, suf_wfs)
        self.straight = _with(whole, mixed_ev)            # the original applyEvents calls
        self.page_called = _with(whole, self.reset.events)  # the prefix in page calls, then the task's
        rounds = [(self.reset, self.apply, self.tasks[0]), (self.reset, self.apply, self.tasks[1])]
        self.state_plan = xdc.state_caps_for(self.base, rounds)
        self.reset_plan = engine.plan(self.reset)
        self.apply_plan = xdc.plan_apply(self.apply, xdc.state_caps_for(self.base, rounds, live_sum=True).caps)
        self.rounds = rounds

    def squeeze(self, ref_run):
        """Under-size one table of one "small_caps" workflow: room for its base state, not for
        the state the apply leaves.  Returns the workflow, or None."""
        own = engine.plan(self.base)  # what the base replay itself needs
        final = ref_run[0]
        for w in range(self.n):
            if self.kind[w] != "small_caps":
                continue
            for t in ("act", "timer", "child", "signal", "cancel"):
                nb, nf = getattr(own.caps[w], t + "_cap"), getattr(final.result[w], engine.TABLE_COUNT[t])
                if nf > nb:
                    from cadence_amd import ndc
                    setattr(self.state_plan.caps[w], t + "_cap", nb)
                    self.state_plan.totals = ndc.offsets_from_caps(self.state_plan.caps, self.n)
                    return w
        return None

    def reference(self):
        """(final state, [(dec, reset Outputs, apply Outputs) per round]) by tests/xdc_ref.py"""
        import oracle
        state = oracle.replay(self.base, self.state_plan)
        per = []
        for reset, apply, tasks in self.rounds:
            per.append(ref.round_(state, tasks, reset, self.reset_plan, apply, self.apply_plan, self.cluster))
        return state, per


def _names(dec, n):
    return [(abi.XDC_ACTIONS[dec[w].action], abi.XDC_REASONS[dec[w].reason]) for w in range(n)]


def test_reference_round_equals_straight_replay():
    """Reset to the checkpoint, then apply, leaves the state a replay of checkpoint prefix +
    incoming suffix leaves: always the one with the prefix in page calls; the one with the
    original calls too, but for the BatchID fields a page boundary changes."""
    import oracle
    fx = Fixture(17, kinds=("reset",))
    state, per = fx.reference()
    dec = per[0][0]
    assert _names(dec, fx.n) == [("APPLY", "APPLY")] * fx.n
    assert all(dec[w].flags & abi.XDD_RESET_RAN and dec[w].via == abi.XDV_RESET for w in range(fx.n))
    assert fx.reset.wfs[16].ev_len > xdc.PAGE_SIZE and len(engine._calls(fx.reset, 16)) == 2
    paged = oracle.replay(fx.page_called, fx.state_plan)
    assert engine.status_histogram(paged) == {"OK": fx.n}
    bad = engine.compare(fx.page_called, state, paged, last_decision=False)
    assert not bad, bad[:5]
    straight = oracle.replay(fx.straight, fx.state_plan)
    same = 0
    for w in range(fx.n):
        diffs = {f for f, _ in abi.CdrExecInfo._fields_ if getattr(state.exec[w], f) != getattr(straight.exec[w], f)}
        assert bytes(state.result[w]) == bytes(straight.result[w]) and bytes(state.repl[w]) == bytes(straight.repl[w])
        for t in engine.TABLES:
            for p, q in zip(state.rows(w, t), straight.rows(w, t)):
                diffs |= {f for f, _ in type(p)._fields_ if getattr(p, f) != getattr(q, f)}
        assert all("batch_id" in f for f in diffs), (w, diffs)
        same += not diffs
    assert same > 0
    # the second round finds every task applied
    assert _names(per[1][0], fx.n) == [("DROP", "DUPLICATE")] * fx.n


@functools.lru_cache(maxsize=None)
def _mixed_fixture():
    fx = Fixture(65)
    first = fx.reference()
    fx.small = fx.squeeze(first)
    assert fx.small is not None
    return fx, fx.reference()


def test_reference_round_mixed_cases():
    """The 65-workflow mix the GPU test replays, on the reference alone: every kind takes the
    exit it was built for, in both rounds."""
    fx, (state, per) = _mixed_fixture()
    want0 = {"apply": ("APPLY", "APPLY"), "fresh": ("APPLY_FRESH", "START"), "reset": ("APPLY", "APPLY"),
             "reset_retry": ("RETRY", "BUFFER"), "reset_drop": ("DROP", "DUPLICATE"),
             "bad_prefix": ("DROP", "E_RESET_PREFIX"), "more_than_2dc": ("DROP", "E_MORE_THAN_2DC"),
             "no_checkpoint": ("DROP", "E_MISSING_REPL_INFO"), "remote_higher": ("DROP", "E_REMOTE_HIGHER_VERSION"),
             "corrupted": ("DROP", "E_CORRUPTED_REPL_INFO"), "failed_state": ("DROP", "E_STATE"),
             "stale": ("REAPPLY", "STALE_RUNNING"), "small_caps": ("APPLY", "APPLY")}
    want1 = dict(want0, apply=("DROP", "DUPLICATE"), fresh=("APPLY_FRESH", "START"), reset=("DROP", "DUPLICATE"),
                 reset_retry=("APPLY", "APPLY"), reset_drop=("APPLY", "APPLY"), bad_prefix=("DROP", "E_STATE"),
                 small_caps=("DROP", "DUPLICATE"))
    d0, d1 = per[0][0], per[1][0]
    for w in range(fx.n):
        k = fx.kind[w]
        if w == fx.small:
            assert _names(d0, fx.n)[w] == ("APPLY", "APPLY") and state.result[w].code == abi.E_BAD_INPUT
            assert _names(d1, fx.n)[w] == ("DROP", "E_STATE")
            continue
        assert _names(d0, fx.n)[w] == want0[k], (w, k, _names(d0, fx.n)[w])
        assert _names(d1, fx.n)[w] == want1[k], (w, k, _names(d1, fx.n)[w])
        ran = k in ("reset", "reset_retry", "reset_drop")
        assert bool(d0[w].flags & abi.XDD_RESET_RAN) == ran, (w, k)
        if k in ("apply", "fresh", "reset", "reset_retry", "reset_drop", "small_caps"):
            assert state.result[w].code == abi.OK, (w, k, state.result[w].code)
    assert d0[next(w for w in range(fx.n) if fx.kind[w] == "bad_prefix")].code == abi.E_BAD_INPUT
    # the reset emits the stateBuilder's task lists
    w = fx.kind.index("reset")
    assert per[0][1].tasks["n"][2 * w] + per[0][1].tasks["n"][2 * w + 1] > 0


# --------------------------------------------------------------------------------- GPU
def _with_every_action(n):
    """n hand-made tasks cycling through KATs + EXTRA rows of one cluster configuration"""
    m = _cluster()
    rows = [c for c in ([k[:1] + k[2:] for k in KATS] + EXTRA) if bytes(c[1]) == bytes(m)]
    assert {c[-1]["action"] for c in rows} == set(abi.XDC_ACTIONS)
    pick = [rows[i % len(rows)] for i in range(max(n, len(rows)))]
    st_rows = [c[2] for c in pick]
    return _tasks([c[3] for c in pick], st_rows), _states(st_rows), m, len(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_admit_kernel_equals_host_gpu(engine_gpu, n):
    """k_xdc_admit == cdr_xdc_admit_host byte for byte, the decision buffer pre-filled with 0xA5."""
    tasks, states, m, n_rows = _with_every_action(n)
    host = xdc.admit_host(tasks, n, states, m)
    got = xdc.admit(engine_gpu, tasks, n, states, m, fill=FILL)
    assert bytes(got)[:n * 64] == bytes(host)[:n * 64]
    if n >= n_rows:
        assert {host[w].action for w in range(n)} == set(range(len(abi.XDC_ACTIONS)))


@pytest.mark.gpu
def test_admit_kernel_random_tasks_gpu(engine_gpu):
    tasks, states, m, n = _random_cases()
    host = xdc.admit_host(tasks, n, states, m)
    got = xdc.admit(engine_gpu, tasks, n, states, m, fill=FILL)
    bad = [(w, ref.diff(got[w], host[w])) for w in range(n) if bytes(got[w]) != bytes(host[w])]
    assert not bad, bad[:5]


def _same(batch, a, b, what, tasks=False):
    bad = engine.compare(batch, a, b, last_decision=False)
    if tasks:
        bad += engine.compare_tasks(batch, a, b)
    assert not bad, what + ": " + "\n".join(bad[:10])


def _same_untouched(a, b, what):
    """records no step wrote: raw bytes"""
    for w in range(a.n_wfs):
        if a.result[w].code == abi.NOT_RUN or b.result[w].code == abi.NOT_RUN:
            for x, y in ((a.result, b.result), (a.exec, b.exec), (a.repl, b.repl)):
                assert bytes(x[w]) == bytes(y[w]), (what, w)


@pytest.mark.gpu
def test_replicate_rounds_equal_reference_gpu(engine_gpu):
    """cdr_xdc_replicate_async == the reference round on 65 workflows mixing every kind (Fixture),
    then a second round on the device-resident states the first left; then the same round
    again on a stream without new device memory."""
    fx, (r_state, r_per) = _mixed_fixture()
    rep = xdc.DeviceReplicator(engine_gpu, fx.base, fx.rounds, cluster=fx.cluster, state_plan=fx.state_plan)
    try:
        state, per = rep.run()
        for k, ((dg, rg, ag), (dr, rr, ar)) in enumerate(zip(per, r_per)):
            bad = [(w, fx.kind[w], ref.diff(dg[w], dr[w])) for w in range(fx.n) if bytes(dg[w]) != bytes(dr[w])]
            assert not bad, (k, bad[:5])
            _same(fx.reset, rg, rr, f"round {k} reset", tasks=True)
            _same(fx.apply, ag, ar, f"round {k} apply")
            _same_untouched(rg, rr, f"round {k} reset")
            _same_untouched(ag, ar, f"round {k} apply")
        _same(fx.base, state, r_state, "final state")
        for w in range(fx.n):  # the whole state, failed and untouched records included
            assert bytes(state.result[w]) == bytes(r_state.result[w]), (w, fx.kind[w])
            if r_state.result[w].code == abi.OK:
                assert bytes(state.exec[w]) == bytes(r_state.exec[w]) and bytes(state.repl[w]) == bytes(r_state.repl[w])
        # warm: the same rounds again, on a stream, allocate nothing
        hip = engine._hip()
        st = C.c_void_p()
        assert hip.hipStreamCreate(C.byref(st)) == 0
        try:
            f0, f1, t = C.c_size_t(), C.c_size_t(), C.c_size_t()
            rep.round(1, st)  # the stream's first launches: the runtime sets up its queue
            assert hip.hipStreamSynchronize(st) == 0
            assert hip.hipMemGetInfo(C.byref(f0), C.byref(t)) == 0
            rep.round(1, st)
            assert hip.hipStreamSynchronize(st) == 0
            assert hip.hipMemGetInfo(C.byref(f1), C.byref(t)) == 0
            assert f1.value >= f0.value - (2 << 20)
        finally:
            hip.hipStreamDestroy(st)
        again = rep.download_round(1)[0]  # round 1 again on the states it left: what it applied is a duplicate now
        dup = {("APPLY", "APPLY"): ("DROP", "DUPLICATE")}
        assert _names(again, fx.n) == [dup.get(x, x) for x in _names(r_per[1][0], fx.n)]
    finally:
        rep.close()


@pytest.mark.gpu
def test_replicate_rejects_unplanned_batches_gpu(engine_gpu):
    """An apply batch with fast or wave slices, or a carry of its own: CDR_API_EINVAL, nothing launched."""
    fx, _ = _mixed_fixture()
    rep = xdc.DeviceReplicator(engine_gpu, fx.base, fx.rounds[:1], cluster=fx.cluster, state_plan=fx.state_plan)
    try:
        r = rep.rounds[0][0]
        for field, value in (("n_fast_slices", 1), ("n_wave_slices", 1), ("carry", 8)):
            bad = abi.CdrXdcRound.from_buffer_copy(r)
            setattr(bad.apply, field, value)
            rc = abi.lib().cdr_xdc_replicate_async(engine_gpu.ctx, fx.n, C.byref(bad), C.c_void_p(rep.state_caps_d),
                                                   C.byref(rep.state), C.byref(fx.cluster), None)
            assert rc == -1, field
    finally:
        rep.close()
