"""Hand-built histories for what every SUCCESSFUL event of stateBuilder.applyEvents leaves
behind: the counterpart of tests/fault_cases.py, which pins the failure returns.

Each case is one small workflow with explicit call boundaries and, for each builder kind
(local, 2DC, NDC), the COMPLETE persisted state the replay must leave, in the shape of
engine.export_state: `result`, every non-pad field of `exec`, `repl`, and the `act`, `timer`,
`child`, `cancel`, `signal`, `vh`, `rp` and `sa` rows (handles as strings, floats as
float.hex).  `repl` is stated for every builder: a local or NDC builder has no replication
state (mutableStateBuilder.go:137-231) and its record is all zero, `present` included.

Every value is written by hand from the reference's Go, cited in each case's docstring by
file and line with the abbreviations of tests/fault_cases.py (`sb` =
service/history/stateBuilder.go, `msb` = service/history/mutableStateBuilder.go, `dtm` =
service/history/mutableStateDecisionTaskManager.go, `vh` =
common/persistence/versionHistory.go, `wei` = common/persistence/workflowExecutionInfo.go,
`meta` = common/cluster/metadata.go) and `tb` = service/history/timerBuilder.go.  The CPU
restatement (oracle/) is pinned BY this table (tests/test_effect_sites.py); it is NEVER
used to fill it.  head_exec() below holds the state the common head leaves, hand-written
too, so that a case states only what its own events change; the row templates (act_row,
timer_row, ...) spell out every field of a row, their defaults being the values of this
module's event helpers (asched, tstart, cinit, ...).

What is this project's contract and not the reference's:
  * the UUID-derived ids (create_request_*, cancel_request_*, signal_request_*, branch_id_*):
    cdr_uuid of include/cdr/schema.h:209-230, restated below (mix64, uuid) — the library is
    never called for them;
  * the new run's request id and key: HistoryBuilder gives the new-run entry the request id
    "new-run-request-id" and the key 0x100000 + its parent's position (cadence_amd/history.py);
  * timeSource.Now() is the batch's injected now_ns (BATCH_NOW), event timestamps are
    NOW + eventId and task ids 1000 + eventId (fault_cases.ev);
  * the sticky / client fields of ExecutionInfo are not part of the output record
    (schema.h:419-428), so ClearStickyness (msb:1398-1420) has nothing to show.

The common head (fault_cases.head, version 1, ids 1-4) leaves the workflow Running with no
pending decision:

    call 0: WorkflowExecutionStarted(1) DecisionTaskScheduled(2)
    call 1: DecisionTaskStarted(3)
    call 2: DecisionTaskCompleted(4) <the case's events ...>

The second output of applyEvents — the transfer and timer task lists (sb:613-804, tb) — is
pinned the same way: `Spec.xfer` and `Spec.ttask` are the COMPLETE lists in emission order,
each entry a complete cdr_task record (every non-pad field of abi.CdrTask, the four handles as
strings) spelt with the task templates below (decision_task, activity_task, ..., timer_task's
kin), written by hand from the Go and cited in the case's docstring; head_tasks() holds what
the common head emits.  Each record also carries `by`, the id of the event whose handler
appended it: it is not compared with the output, it gives the hand-known split of a list at a
carry-in cut.  tests/test_task_sites.py pins the oracle and every task-emitting kernel route
to these lists.  The task lists do not depend on the builder kind: stateBuilder's tasks carry
no version (below) and nothing else of a task reads the replication state.

What is this project's contract and not the reference's, for the tasks:
  * `version` is 0 on every stateBuilder task: the Go leaves Version to the caller
    (schema.h:564-566; sb:613-804 never sets it);
  * a failed entry reports no tasks (schema.h: both n_tasks zero);
  * ties are broken deterministically where Go's order comes from a map walk (tb:236-245,
    252-310: the sequence number of a user timer follows the map order, activity candidates
    have none): activity candidates by (time, ScheduleID, kind order: scheduleToClose, then
    startToClose / scheduleToStart, then heartbeat), user timers by (expiry, StartedID).
"""
from __future__ import annotations

from dataclasses import dataclass, field

from cadence_amd import abi
from tests.fault_cases import (ALL, APPLIED, BUILDER_NAMES, D2, IS_NEWRUN, L, N, NOW, at_close, at_started,  # noqa: F401
                               build_batch, can, dt_completed, dt_sched, dt_started, ev, head, marker, started)

S = 10 ** 9                      # one second
DAY = 24 * 3600 * S
BATCH_NOW = 1_700_000_000_000_000_000   # HistoryBuilder.build()'s now_ns: the injected timeSource.Now()
SEED = 1                         # HistoryBuilder.build()'s uuid_seed
EMPTY_ID, EMPTY_V = -23, -24     # common/constants.go:28-41
CREATED, RUNNING, COMPLETED = 0, 1, 2            # dataInterfaces.go:87-94
F0 = float.hex(0.0)
XI_CANCEL, XI_RETRY, XI_EXPIRATION, XI_BRANCH, XI_MEMO, XI_SA, XI_RP, XI_STARTED, XI_VH_BRANCH = \
    0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80, 0x100
AI_CANCEL, AI_RETRY, AI_STARTED = 0x1, 0x2, 0x4
TTS_STC, TTS_S2S, TTS_S2C, TTS_HB = 1, 2, 4, 8   # tb:36-47
RP_ALL = 0x1 | 0x2 | 0x4 | 0x8 | 0x20            # checksum, run id, first-decision id, created, resettable present
RP_EXPIRING, RP_RESETTABLE = 0x10, 0x40

# ------------------------------------------------------------------ cdr_uuid (schema.h:209-230)
_M = (1 << 64) - 1
UUID_BRANCH, UUID_CHILD, UUID_CANCEL, UUID_SIGNAL = 1, 2, 3, 4


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M
    return x ^ (x >> 31)


def uuid(key, site, event_id, seed=SEED):
    a = mix64(seed ^ mix64(key))
    lo = mix64(a ^ (site << 56) ^ (event_id & _M))
    return lo, mix64(lo ^ 0xD6E8FEB86659FD93)


# ------------------------------------------------------------------ events
def asched(eid, aid, version=1, tl="tl", s2s=5, s2c=30, stc=20, hb=0, retry=None):
    a = dict(activityId=aid, taskList={"name": tl}, scheduleToStartTimeoutSeconds=s2s,
             scheduleToCloseTimeoutSeconds=s2c, startToCloseTimeoutSeconds=stc, heartbeatTimeoutSeconds=hb)
    if retry is not None:
        a["retryPolicy"] = retry
    return ev(eid, "ActivityTaskScheduled", version, **a)


def acancel(eid, aid, version=1):
    return ev(eid, "ActivityTaskCancelRequested", version, activityId=aid)


def tstart(eid, tid, fire_s=60, version=1):
    return ev(eid, "TimerStarted", version, timerId=tid, startToFireTimeoutSeconds=fire_s)


def tend(eid, kind, tid, started_id, version=1):
    return ev(eid, "Timer" + kind, version, timerId=tid, startedEventId=started_id)


def cinit(eid, wid="child-wid", domain="target", wtype="child-type", pcp="ABANDON", version=1):
    return ev(eid, "StartChildWorkflowExecutionInitiated", version, domain=domain, workflowId=wid,
              workflowType={"name": wtype}, parentClosePolicy=pcp)


def cstart(eid, init, run="child-run", wid="child-wid", version=1):
    return ev(eid, "ChildWorkflowExecutionStarted", version, initiatedEventId=init,
              workflowExecution={"workflowId": wid, "runId": run})


def ref(eid, etype, init, version=1):
    """An event that names an initiated event and nothing else the replay reads."""
    return ev(eid, etype, version, initiatedEventId=init)


def rce(eid, child_only=False, control=None, version=1, domain="target"):
    a = dict(domain=domain, workflowExecution={"workflowId": "ext-wid", "runId": "ext-run"},
             childWorkflowOnly=child_only)
    if control is not None:
        a["control"] = control
    return ev(eid, "RequestCancelExternalWorkflowExecutionInitiated", version, **a)


def sig(eid, name="sig", input=None, control=None, child_only=False, version=1, domain="target"):
    a = dict(domain=domain, workflowExecution={"workflowId": "ext-wid", "runId": "ext-run"}, signalName=name,
             childWorkflowOnly=child_only)
    if input is not None:
        a["input"] = input
    if control is not None:
        a["control"] = control
    return ev(eid, "SignalExternalWorkflowExecutionInitiated", version, **a)


def upsert(eid, fields, version=1):
    return ev(eid, "UpsertWorkflowSearchAttributes", version, searchAttributes={"indexedFields": fields})


def at(e, timestamp):
    """Event `e` with a timestamp of the case's own (ev's is NOW + eventId): for exact ties."""
    return dict(e, timestamp=timestamp)


def head_with(version=1, **start_attrs):
    """fault_cases.head() with attributes of the case's own on the Started event."""
    return [[started(1, version, **start_attrs), dt_sched(2, version)], [dt_started(3, 2, version)],
            [dt_completed(4, 2, 3, version)]]


# ------------------------------------------------------------------ expected values
class By:
    """A value that differs by builder kind: By(local, 2DC, NDC)."""

    def __init__(self, local, d2, ndc):
        self.v = {L: local, D2: d2, N: ndc}


@dataclass
class Ctx:
    """What an expectation depends on besides the case: the builder kind and the instance's
    position k in its batch (fault_cases.build_batch names workflow k "wf-k-<case>", "run-k",
    "req-k" and HistoryBuilder keys it 0x1000 + k; its new run 0x100000 + k)."""
    builder: int
    k: int
    name: str
    new_run: bool = False
    domain_id: str = "domain-id"

    @property
    def key(self):
        return (0x100000 if self.new_run else 0x1000) + self.k

    @property
    def run_id(self):
        return "next-run" if self.new_run else f"run-{self.k}"


def RUN(c):        # the instance's own run id (msb:1833 RunId: exeInfo.RunID)
    return c.run_id


def _resolve(v, c):
    if isinstance(v, By):
        return v.v[c.builder]
    if callable(v):
        return v(c)
    if isinstance(v, dict):
        return {k: _resolve(x, c) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_resolve(x, c) for x in v]
    return v


def xflags(extra):
    """ExecutionInfo flags: Started, the builder's branch token (msb:313-339) and `extra`."""
    return By(XI_STARTED | XI_BRANCH | extra, XI_STARTED | XI_BRANCH | extra, XI_STARTED | XI_VH_BRANCH | extra)


def head_exec(c: Ctx) -> dict:
    """ExecutionInfo after the common head (events 1-4, version 1), field by field:
    msb:1639-1716 (Started: ids, task list, type, timeouts 100 / 10, InitiatedID EmptyEventID,
    no retry policy, no cron / memo), sb:176 SetHistoryTree (the branch token: on ExecutionInfo
    for local / 2DC, on the version history for NDC — msb:313-339), dtm:229-237 (Running),
    dtm:659-674 (DeleteDecision: every decision field reset, OriginalScheduledTimestamp kept =
    DecisionTaskScheduled(2)'s timestamp), dtm:789-800 (LastProcessedEvent = startedEventId 3),
    sb:155, 603-604 (LastEventTaskID 1004, LastFirstEventID 4, NextEventID 5)."""
    lo, hi = uuid(c.key, UUID_BRANCH, 1)
    return dict(
        domain_id="domain-id", workflow_id=f"wf-{c.k}-{c.name}", run_id=c.run_id,
        create_request_id="new-run-request-id" if c.new_run else f"req-{c.k}",
        parent_domain_id="", parent_workflow_id="", parent_run_id="", task_list="tl", workflow_type="wt",
        cron_schedule="", memo="", nonretriable="", branch_tree_id=c.run_id, workflow_timeout=100,
        decision_timeout_value=10, attempt=0, initiated_id=EMPTY_ID, initial_interval=0, maximum_interval=0,
        backoff_coefficient=F0, maximum_attempts=0, expiration_seconds=0, expiration_time=0,
        branch_id_lo=lo, branch_id_hi=hi, decision_request_id="emptyUuid",
        flags=XI_STARTED | (XI_VH_BRANCH if c.builder == N else XI_BRANCH), completion_event_batch_id=0,
        state=RUNNING, close_status=0, last_first_event_id=4, last_event_task_id=1004, next_event_id=5,
        last_processed_event=3, signal_count=0, decision_timeout=0, decision_version=EMPTY_V,
        decision_schedule_id=EMPTY_ID, decision_started_id=EMPTY_ID, decision_attempt=0, decision_started_ts=0,
        decision_scheduled_ts=0, decision_original_scheduled_ts=NOW + 2, reset_points_len=0, search_attr_len=0)


def no_repl() -> dict:
    """The record of a builder without replication state: untouched, all zero."""
    return dict(current_version=0, start_version=0, last_write_version=0, last_write_event_id=0,
                lri_version=[0] * 8, lri_last_event_id=[0] * 8, lri_mask=0, present=0)


def repl_state(current, start, last_version, last_event_id, lri=None) -> dict:
    """ReplicationState of a 2DC builder (msb:548-581, sb:134-138, 182-184); `lri`:
    {cluster index: (version, last event id)} — LastReplicationInfo."""
    r = dict(current_version=current, start_version=start, last_write_version=last_version,
             last_write_event_id=last_event_id, lri_version=[0] * 8, lri_last_event_id=[0] * 8, lri_mask=0, present=1)
    for cl, (v, e) in (lri or {}).items():
        r["lri_version"][cl], r["lri_last_event_id"][cl] = v, e
        r["lri_mask"] |= 1 << cl
    return r


def act_row(sid, batch, aid, *, status, version=1, started=None, request_id="", expiration=None, cancel=None,
            task_list="tl", s2s=5, s2c=30, stc=20, hb=0, retry=None, attempt=0, heartbeat=None, scheduled_time=None):
    """ActivityInfo of ActivityTaskScheduled(sid) in a call whose first event is `batch`
    (msb:1982-2028), started by event `started` (msb:2083-2098: StartedID, RequestID,
    StartedTime = LastHeartBeatUpdatedTime = its timestamp), cancel requested by event `cancel`
    (msb:2264-2285).  `retry` = (initial, coefficient, maximum interval, maximum attempts,
    non-retriable reasons joined by \\x1f); `expiration` defaults to ScheduledTime +
    scheduleToClose (msb:2011)."""
    r = retry or (0, 0.0, 0, 0, "")
    st = 0 if started is None else NOW + started
    sched = NOW + sid if scheduled_time is None else scheduled_time
    return dict(version=version, schedule_id=sid, scheduled_event_batch_id=batch, scheduled_time=sched,
                started_id=EMPTY_ID if started is None else started, started_time=st,
                last_heartbeat_time=st if heartbeat is None else heartbeat,
                expiration_time=sched + s2c * S if expiration is None else expiration,
                cancel_request_id=EMPTY_ID if cancel is None else cancel, activity_id=aid, request_id=request_id,
                task_list=task_list, nonretriable=r[4], s2s=s2s, s2c=s2c, stc=stc, hb=hb, timer_task_status=status,
                attempt=attempt, initial_interval=r[0], maximum_interval=r[2], maximum_attempts=r[3],
                flags=(AI_CANCEL if cancel is not None else 0) | (AI_RETRY if retry else 0) |
                      (AI_STARTED if started is not None else 0),
                backoff_coefficient=float.hex(r[1]))


def timer_row(tid, started_id, fire_s, task_id, version=1, expiry=None):
    """TimerInfo of TimerStarted(started_id) (msb:2877-2900); task_id 1 once the timer was the
    head of a pick (tb:171-184)."""
    return dict(version=version, started_id=started_id,
                expiry_time=NOW + started_id + fire_s * S if expiry is None else expiry, task_id=task_id,
                timer_id=tid)


def child_row(iid, batch, *, version=1, started=None, run="", wid="child-wid", domain="target", wtype="child-type",
              pcp=0):
    """ChildExecutionInfo of StartChildWorkflowExecutionInitiated(iid) (msb:3256-3280), started
    by event `started` with run id `run` (msb:3312-3325)."""
    return dict(version=version, initiated_id=iid, initiated_event_batch_id=batch,
                started_id=EMPTY_ID if started is None else started,
                create_request_lo=lambda c: uuid(c.key, UUID_CHILD, iid)[0],
                create_request_hi=lambda c: uuid(c.key, UUID_CHILD, iid)[1],
                started_workflow_id=wid, started_run_id=run, domain_name=domain, workflow_type=wtype,
                parent_close_policy=pcp)


def cancel_row(iid, batch, version=1):
    """RequestCancelInfo (msb:2577-2596)."""
    return dict(version=version, initiated_event_batch_id=batch, initiated_id=iid,
                cancel_request_lo=lambda c: uuid(c.key, UUID_CANCEL, iid)[0],
                cancel_request_hi=lambda c: uuid(c.key, UUID_CANCEL, iid)[1])


def signal_row(iid, batch, name="sig", input="", control="", version=1):
    """SignalInfo (msb:2701-2723)."""
    return dict(version=version, initiated_event_batch_id=batch, initiated_id=iid,
                signal_request_lo=lambda c: uuid(c.key, UUID_SIGNAL, iid)[0],
                signal_request_hi=lambda c: uuid(c.key, UUID_SIGNAL, iid)[1],
                signal_name=name, input=input, control=control)


def rp_row(checksum, run, first_decision, created, expiring, flags):
    return dict(binary_checksum=checksum, run_id=run, first_decision_completed_id=first_decision,
                created_time_nano=created, expiring_time_nano=expiring, flags=flags)


# ------------------------------------------------------------------ expected task records
# cdr_task_type (schema.h:536-553: the TransferTaskType* / TaskType* of dataInterfaces.go:121-155)
T_DECISION, T_ACTIVITY, T_CLOSE, T_CANCEL, T_CHILD, T_SIGNAL, T_RECORD_STARTED, T_UPSERT = 0, 1, 2, 3, 4, 5, 6, 8
T_DECISION_TIMEOUT, T_ACTIVITY_TIMEOUT, T_USER_TIMER, T_WF_TIMEOUT, T_DELETE_HISTORY, T_BACKOFF = 16, 17, 18, 19, 20, 22
STC, S2S, S2C, HB = 0, 1, 2, 3           # shared.TimeoutType: StartToClose, ScheduleToStart, ScheduleToClose, Heartbeat
BACKOFF_RETRY, BACKOFF_CRON = 0, 1       # persistence.WorkflowBackoffTimeoutType{Retry,Cron}
CHILD_ONLY = 1                           # CDR_TF_CHILD_ONLY: TargetChildWorkflowOnly
TASK_LISTS = ("xfer", "ttask")


def DOMAIN(c):     # the domainID applyEvents is called with: the instance's own domain id
    return c.domain_id


def T(eid):        # fault_cases.ev's timestamp of event `eid`
    return NOW + eid


def _task(type, by, **kw):
    """A complete cdr_task: every field the type does not set is Go's zero value — 0, or ""
    (handle 0) for the four handles — and `version` is 0 (schema.h:564-566)."""
    r = dict(type=type, timeout_type=0, event_id=0, visibility_ts=0, attempt=0, domain_id="", task_list="",
             target_workflow_id="", target_run_id="", flags=0, version=0, by=by)
    assert set(kw) < set(r)
    r.update(kw)
    return r


def record_started(by=1):
    """sb:174 -> sb:615-617 RecordWorkflowStartedTask{}."""
    return _task(T_RECORD_STARTED, by)


def decision_task(sid, by=None, tl="tl", domain=DOMAIN):
    """sb:196 / 235 / 253 -> sb:619-629 DecisionTask{DomainID, TaskList, ScheduleID}: TaskList =
    ExecutionInfo.TaskList (sb:789-794), not the event's."""
    return _task(T_DECISION, sid if by is None else by, event_id=sid, domain_id=domain, task_list=tl)


def activity_task(sid, tl="tl", domain=DOMAIN):
    """sb:265 -> sb:631-641 ActivityTask{DomainID, TaskList, ScheduleID}: TaskList is again
    ExecutionInfo.TaskList (sb:265, 789-794) — not the activity's own task list."""
    return _task(T_ACTIVITY, sid, event_id=sid, domain_id=domain, task_list=tl)


def child_task(iid, domain_id="id-of-target", wid="child-wid"):
    """sb:370 -> sb:643-653 StartChildExecutionTask{TargetDomainID (the domain cache's id for the
    attribute's domain), TargetWorkflowID, InitiatedID}: no TargetRunID."""
    return _task(T_CHILD, iid, event_id=iid, domain_id=domain_id, target_workflow_id=wid)


def cancel_task(iid, child_only=False, domain_id="id-of-target", wid="ext-wid", run="ext-run"):
    """sb:421 -> sb:655-669 CancelExecutionTask{TargetDomainID, TargetWorkflowID, TargetRunID,
    TargetChildWorkflowOnly, InitiatedID}."""
    return _task(T_CANCEL, iid, event_id=iid, domain_id=domain_id, target_workflow_id=wid, target_run_id=run,
                 flags=CHILD_ONLY if child_only else 0)


def signal_task(iid, child_only=False, domain_id="id-of-target", wid="ext-wid", run="ext-run"):
    """sb:452 -> sb:671-685 SignalExecutionTask, the same five fields."""
    return _task(T_SIGNAL, iid, event_id=iid, domain_id=domain_id, target_workflow_id=wid, target_run_id=run,
                 flags=CHILD_ONLY if child_only else 0)


def upsert_task(by):
    """sb:535 -> sb:687-689 UpsertWorkflowSearchAttributesTask{}."""
    return _task(T_UPSERT, by)


def close_task(by):
    """sb:780 -> sb:691-693 CloseExecutionTask{}."""
    return _task(T_CLOSE, by)


def timer_task(type, by, visibility, timeout_type=0, event_id=0, attempt=0):
    """A timer task: VisibilityTimestamp and, by type, TimeoutType, EventID, Attempt."""
    return _task(type, by, visibility_ts=visibility, timeout_type=timeout_type, event_id=event_id, attempt=attempt)


def wf_timeout(visibility, by=1):
    """sb:173 -> sb:731-756 WorkflowTimeoutTask at the Started event's time + WorkflowTimeout
    (+ the first decision's backoff, sb:743)."""
    return timer_task(T_WF_TIMEOUT, by, visibility)


def backoff_timer(visibility, timeout_type, by=1):
    """sb:742-752 WorkflowBackoffTimerTask at the Started event's time + the backoff; Cron for a
    cron initiator, Retry otherwise."""
    return timer_task(T_BACKOFF, by, visibility, timeout_type)


def decision_timeout(sid, by, timeout_s=10):
    """sb:210 -> tb:130-136, 322-331 DecisionTimeoutTask: the DecisionTaskStarted event's time +
    the decision's timeout, StartToClose, EventID = the ScheduleID, ScheduleAttempt = the decision's
    attempt — which dtm:224 has just forced to 0 (stateBuilder passes a nil decision, sb:204)."""
    return timer_task(T_DECISION_TIMEOUT, by, T(by) + timeout_s * S, STC, sid, 0)


def activity_timeout(sid, timeout_type, visibility, by, attempt=0):
    """sb:267-317 -> tb:211-230, 391-408 ActivityTimeoutTask of the earliest candidate."""
    return timer_task(T_ACTIVITY_TIMEOUT, by, visibility, timeout_type, sid, attempt)


def user_timer(started_id, visibility, by=None):
    """sb:330-348 -> tb:171-184, 391-398 UserTimerTask{VisibilityTimestamp: the expiry, EventID:
    the timer's StartedID}."""
    return timer_task(T_USER_TIMER, started_id if by is None else by, visibility, 0, started_id)


def delete_history(by, days=1):
    """sb:785 -> sb:758-773, tb:314-319 DeleteHistoryEventTask at the close event's time + the
    domain's retention."""
    return timer_task(T_DELETE_HISTORY, by, T(by) + days * DAY)


def head_tasks(c: Ctx, tl="tl", wf_timeout_s=100) -> dict:
    """What the common head (events 1-4) emits: sb:173-174 WorkflowTimeout at event 1's time +
    WorkflowTimeout 100 s (no backoff: sb:742) and RecordWorkflowStarted; sb:196 DecisionTask of
    DecisionTaskScheduled(2) on ExecutionInfo.TaskList; sb:210 DecisionTimeout from
    DecisionTaskStarted(3): event 3's time + the 10 s of the DecisionTaskScheduled event (dtm:157,
    243 — not ExecutionInfo.DecisionTimeoutValue), attempt 0.  DecisionTaskCompleted(4): nothing."""
    return dict(xfer=[record_started(1), decision_task(2, tl=tl)],
                ttask=[wf_timeout(T(1) + wf_timeout_s * S), decision_timeout(2, by=3)])


def closes(by, days=1):
    """appendTasksForFinishedExecutions (sb:775-787) as Spec keywords: for a case that emits
    nothing else of its own."""
    return dict(xfer=[close_task(by)], ttask=[delete_history(by, days)])


HEAD_ONLY = dict(xfer=[], ttask=[])      # a case whose own events append no task


# ------------------------------------------------------------------ the table
TABLES = ("act", "timer", "child", "cancel", "signal", "vh", "rp", "sa")
COUNT = {"act": "n_activity", "timer": "n_timer", "child": "n_child", "cancel": "n_cancel", "signal": "n_signal",
         "vh": "n_vh", "rp": "n_reset_points", "sa": "n_search_attr"}


@dataclass
class Spec:
    """One entry's expected state as the difference from head_exec(): `end` = (first event of
    the last call, last event) -> LastFirstEventID, NextEventID = last + 1, LastEventTaskID =
    1000 + last (sb:155, 603-604); `exec` overrides; the table rows; `vh` = the NDC builder's
    items [(event id, version)] (default: one item, the last event at `version`, vh:203-236);
    `repl` = the 2DC builder's ReplicationState (default: every version `version`, last write
    at the last event, no LastReplicationInfo: cluster 0 is the current one, msb:561-581)."""
    end: tuple
    exec: dict = field(default_factory=dict)
    act: list = field(default_factory=list)
    timer: list = field(default_factory=list)
    child: list = field(default_factory=list)
    cancel: list = field(default_factory=list)
    signal: list = field(default_factory=list)
    rp: list = field(default_factory=list)
    sa: list = field(default_factory=list)     # [(key, value)] in the order of the keys' first use
    vh: list | None = None
    repl: dict | None = None
    version: int = 1
    flags: int = 0                             # cdr_wf_result.flags
    # the task lists: what the entry's events append after head_tasks(**head) — `head` None: the
    # history has no common head (or it is a carry-in suffix), the lists are stated whole
    xfer: list | None = None
    ttask: list | None = None
    head: dict | None = field(default_factory=dict)

    def tasks(self, c: Ctx) -> dict:
        """{"xfer": [...], "ttask": [...]}: the complete expected lists, `by` included."""
        h = head_tasks(c, **self.head) if self.head is not None else dict(xfer=[], ttask=[])
        return {k: _resolve(h[k] + list(getattr(self, k)), c) for k in TASK_LISTS}

    def state(self, c: Ctx) -> dict:
        first, last = self.end
        x = head_exec(c)
        x.update(last_first_event_id=first, next_event_id=last + 1, last_event_task_id=1000 + last)
        x.update(_resolve(self.exec, c))
        d = {"exec": x}
        d["repl"] = _resolve(self.repl if self.repl is not None else
                             repl_state(self.version, self.version, self.version, last), c) \
            if c.builder == D2 else no_repl()
        for t in ("act", "timer", "child", "cancel", "signal", "rp"):
            d[t] = _resolve(getattr(self, t), c)
        d["sa"] = [dict(key=k, value=v) for k, v in self.sa]
        items = self.vh if self.vh is not None else [(last, self.version)]
        d["vh"] = [dict(event_id=e, version=v) for e, v in items] if c.builder == N else []
        r = dict(code=0, flags=self.flags | (IS_NEWRUN if c.new_run else 0), fail_event_id=0, fail_index=0, status="OK")
        r.update({COUNT[t]: len(d[t]) for t in TABLES})
        d["result"] = r
        return d


@dataclass
class Case:
    name: str
    doc: str
    calls: list
    spec: Spec
    new_run: list | None = None
    new_run_call: int = 0
    new_run_spec: Spec | None = None
    domain_id: str = "domain-id"
    retention_days: int = 1
    expected_next_event_id: int = 0
    sites: tuple = ()

    # (what fault_cases.build_batch and test_fault_sites' helpers read of a case)
    @property
    def expect(self):
        return {b: ("OK", 0, 0, self.spec.flags) for b in ALL}

    @property
    def new_run_expect(self):
        return {b: ("OK", 0, 0, IS_NEWRUN) for b in ALL}

    def fails(self, b):
        return False

    def n_events(self):
        return sum(len(c) for c in self.calls)

    def event_types(self):
        return {e["eventType"] for c in self.calls for e in c} | {e["eventType"] for e in self.new_run or []}

    def state(self, builder, k):
        return self.spec.state(self.ctx(builder, k))

    def ctx(self, builder, k, new_run=False):
        return Ctx(builder, k, self.name, new_run=new_run, domain_id=self.domain_id)

    def new_run_state(self, builder, k):
        """The continue-as-new run's entry: an NDC builder behind an NDC parent, otherwise a
        2DC builder (sb:542-556; build_batch: new_run_ndc = the parent is NDC)."""
        return self.new_run_spec.state(self.ctx(N if builder == N else D2, k, new_run=True))

    def tasks(self, builder, k):
        return self.spec.tasks(self.ctx(builder, k))

    def new_run_tasks(self, builder, k):
        return self.new_run_spec.tasks(self.ctx(N if builder == N else D2, k, new_run=True))


CASES: list = []


def case(name, calls, spec, **kw):
    def deco(fn):
        assert fn.__doc__ and name not in {c.name for c in CASES}
        CASES.append(Case(name=name, doc=fn.__doc__, calls=calls, spec=spec, **kw))
        return fn
    return deco


def by_name(name) -> Case:
    return next(c for c in CASES if c.name == name)


def instances(cases=None):
    return [(c, b) for c in (cases or CASES) for b in ALL]


# ---- 1. activities
@case("act_no_retry", head(more=[asched(5, "a")]),
      Spec(end=(4, 5), act=[act_row(5, 4, "a", status=TTS_S2S)],
           xfer=[activity_task(5)], ttask=[activity_timeout(5, S2S, T(5) + 5 * S, by=5)]))
def _():
    """msb:1982-2028 without a retry policy: every retry field zero, HasRetryPolicy false,
    ExpirationTime = ScheduledTime + scheduleToClose 30 s (msb:2011), CancelRequestID
    EmptyEventID, ScheduledEventBatchID = the call's first event 4.  sb:267 -> tb:211-230: the
    earliest of scheduleToClose (+30 s) and scheduleToStart (+5 s) is scheduleToStart, not yet
    created: TimerTaskStatus |= 2 (tb:36-47).  Tasks: sb:265 ActivityTask(5), sb:267 the
    ActivityTimeout of that pick: ScheduleToStart at event 5's time + 5 s, Attempt 0 (tb:297-306,
    400-405)."""


_RETRY = dict(initialIntervalInSeconds=2, backoffCoefficient=1.5, maximumIntervalInSeconds=9, maximumAttempts=4,
              expirationIntervalInSeconds=10, nonRetriableErrorReasons=["bad", "worse"])


@case("act_retry_expiration_below",
      head(more=[asched(5, "a", tl="atl", s2s=7, s2c=25, stc=11, hb=3, retry=_RETRY)]),
      Spec(end=(4, 5), act=[act_row(5, 4, "a", status=TTS_S2S, task_list="atl", s2s=7, s2c=25, stc=11, hb=3,
                                    retry=(2, 1.5, 9, 4, "bad\x1fworse"), expiration=NOW + 5 + 25 * S)],
           xfer=[activity_task(5)], ttask=[activity_timeout(5, S2S, T(5) + 7 * S, by=5)]))
def _():
    """msb:2012-2021 with a retry policy whose expiration interval 10 s is below
    scheduleToClose 25 s: `10 > 25` is false, ExpirationTime stays ScheduledTime + 25 s; the
    five retry fields are copied (msb:2013-2017).  Timer: scheduleToStart (+7 s) first (tb:297-306).
    Tasks: the ActivityTask goes to the workflow's task list "tl" (sb:265, 789-794), not to the
    activity's "atl"; the ActivityTimeout is ScheduleToStart at + 7 s."""


@case("act_retry_expiration_equal",
      head(more=[asched(5, "a", s2s=40, s2c=30, retry=dict(initialIntervalInSeconds=1, backoffCoefficient=2.0,
                                                           expirationIntervalInSeconds=30))]),
      Spec(end=(4, 5), act=[act_row(5, 4, "a", status=TTS_S2C, s2s=40, s2c=30, retry=(1, 2.0, 0, 0, ""),
                                    expiration=NOW + 5 + 30 * S)],
           xfer=[activity_task(5)], ttask=[activity_timeout(5, S2C, T(5) + 30 * S, by=5)]))
def _():
    """msb:2018 `expiration > scheduleToClose` with both 30 s: not larger, ExpirationTime =
    ScheduledTime + 30 s.  No non-retriable reasons, no maximum interval / attempts: zero.
    Timer: scheduleToStart is 40 s here, so scheduleToClose (+30 s) is the head: status |= 4
    (tb:254-267).  Tasks: sb:265, and sb:267 an ActivityTimeout of type ScheduleToClose at + 30 s
    (ExpirationTime equals it: tb:255 `Before` is false)."""


@case("act_retry_expiration_above",
      head() + [[asched(5, "a", retry=dict(initialIntervalInSeconds=6, backoffCoefficient=3.25,
                                           maximumIntervalInSeconds=100, maximumAttempts=0,
                                           expirationIntervalInSeconds=45, nonRetriableErrorReasons=["only"]))]],
      Spec(end=(5, 5), act=[act_row(5, 5, "a", status=TTS_S2S, retry=(6, 3.25, 100, 0, "only"),
                                    expiration=NOW + 5 + 45 * S)],
           xfer=[activity_task(5)], ttask=[activity_timeout(5, S2S, T(5) + 5 * S, by=5)]))
def _():
    """msb:2018-2020: the retry expiration 45 s is larger than scheduleToClose 30 s and
    replaces it: ExpirationTime = ScheduledTime + 45 s.  The activity is scheduled in a call
    of its own: ScheduledEventBatchID 5 (sb:260).  The later ExpirationTime does not move the
    scheduleToClose timer (tb:254-258: only an earlier one does); scheduleToStart +5 s leads.
    Tasks: sb:265 ActivityTask(5), sb:267 ActivityTimeout ScheduleToStart at + 5 s."""


@case("act_cancel_before_start", head(more=[asched(5, "a"), acancel(6, "a")]),
      Spec(end=(4, 6), act=[act_row(5, 4, "a", status=TTS_S2S, cancel=6)],
           xfer=[activity_task(5)], ttask=[activity_timeout(5, S2S, T(5) + 5 * S, by=5)]))
def _():
    """msb:2264-2285 on an activity that has not started: Version = the event's, CancelRequested,
    CancelRequestID = the event's id 6; nothing else moves, no timer pick (sb:307-310).  Tasks:
    those of the schedule (sb:265, 267); ActivityTaskCancelRequested appends none."""


@case("act_cancel_after_start", head(more=[asched(5, "a")]) + [[at_started(6, 5)], [acancel(7, "a")]],
      Spec(end=(7, 7), act=[act_row(5, 4, "a", status=TTS_S2S | TTS_STC, started=6, request_id="a6", cancel=7)],
           xfer=[activity_task(5)],
           ttask=[activity_timeout(5, S2S, T(5) + 5 * S, by=5), activity_timeout(5, STC, T(6) + 20 * S, by=6)]))
def _():
    """msb:2083-2098 then msb:2264-2285: StartedID 6, RequestID, StartedTime =
    LastHeartBeatUpdatedTime = event 6's timestamp; CancelRequestID 7.  Timer after the start
    (sb:276): scheduleToClose (5 + 30 s) against startToClose (6 + 20 s): startToClose, status
    2 | 1 (tb:269-279).  Tasks: sb:276 appends that pick's ActivityTimeout — StartToClose at
    event 6's time + 20 s, EventID the ScheduleID 5 — behind the schedule's ScheduleToStart one;
    the cancel request (sb:307-310) appends nothing."""


@case("act_started_heartbeat", head(more=[asched(5, "a", hb=3)]) + [[at_started(6, 5, 11)]],
      Spec(end=(6, 6), vh=[(5, 1), (6, 11)], repl=repl_state(11, 1, 11, 6),
           act=[act_row(5, 4, "a", status=TTS_S2S | TTS_HB, version=11, started=6, request_id="a6", hb=3)],
           xfer=[activity_task(5)],
           ttask=[activity_timeout(5, S2S, T(5) + 5 * S, by=5), activity_timeout(5, HB, T(6) + 3 * S, by=6)]))
def _():
    """tb:280-295: with a heartbeat timeout the started activity has a third timer, last
    heartbeat (= StartedTime, msb:2095) + 3 s, the earliest: status 2 | 8.  The Started event is
    of version 11: msb:2091 moves the row's Version from the schedule's 1.  Tasks: sb:276 an
    ActivityTimeout of type Heartbeat at event 6's time + 3 s (before scheduleToClose 5 + 30 s
    and startToClose 6 + 20 s); its version stays 0 like every task's."""


for _k in ("Completed", "Failed", "TimedOut", "Canceled"):
    @case(f"act_close_{_k.lower()}",
          head(more=[asched(5, "a"), asched(6, "b")]) + [[at_started(7, 5)], [at_close(8, 5, _k)]],
          Spec(end=(8, 8), act=[act_row(6, 4, "b", status=TTS_S2S)],
               xfer=[activity_task(5), activity_task(6)],
               ttask=[activity_timeout(5, S2S, T(5) + 5 * S, by=5), activity_timeout(6, S2S, T(6) + 5 * S, by=7)]))
    def _():
        """sb:280-305 / 312-319 -> DeleteActivity (msb:1247-1269): the started activity 5 leaves,
        6 stays.  6's timer status: at its own schedule the head is 5's scheduleToStart, already
        created (tb:384-389: nothing); when 5 starts, 5's timers are +30 s / +20 s and 6's
        scheduleToStart (6 + 5 s) leads: status 2 (sb:276); after the close it is the created head.
        Tasks: two ActivityTasks (sb:265); ActivityTimeouts: 5's ScheduleToStart at its schedule
        (sb:267), none at 6's schedule (the list is unchanged), 6's ScheduleToStart appended by
        ActivityTaskStarted(7) — an event of the other activity (sb:276) —, none by the close,
        whose pick (sb:285 / 294 / 303 / 317) finds the created head."""


for _k, _site in (("Completed", 285), ("Failed", 294), ("TimedOut", 303), ("Canceled", 317)):
    @case(f"act_close_{_k.lower()}_picks",
          head(more=[asched(5, "a"), asched(6, "b", s2s=40, s2c=35)]) + [[at_started(7, 5)], [at_close(8, 5, _k)]],
          Spec(end=(8, 8), act=[act_row(6, 4, "b", status=TTS_S2C, s2s=40, s2c=35)],
               xfer=[activity_task(5), activity_task(6)],
               ttask=[activity_timeout(5, S2S, T(5) + 5 * S, by=5), activity_timeout(5, STC, T(7) + 20 * S, by=7),
                      activity_timeout(6, S2C, T(6) + 35 * S, by=8)]),
          sites=(f"sb:{_site}",))
    def _():
        """The pick of an activity close that does append (sb:285 Completed, 294 Failed, 303
        TimedOut, 317 Canceled).  Activity 6 has scheduleToStart 40 s, scheduleToClose 35 s.  At
        5's schedule: its ScheduleToStart (5 + 5 s); at 6's: the head is still that one, created
        (tb:384-389: nothing).  ActivityTaskStarted(7) of 5: candidates 5 + 30 s, 7 + 20 s (5's),
        6 + 35 s, 6 + 40 s (6's): 5's StartToClose (sb:276).  The close deletes 5 (msb:1247-1269)
        and picks among 6's two: ScheduleToClose at 6 + 35 s, not created: appended by event 8,
        status 4 (tb:254-267)."""


@case("act_schedule_to_close_head_expiration_later",
      head(more=[asched(5, "a", s2s=50, s2c=30, retry=dict(initialIntervalInSeconds=1, backoffCoefficient=2.0,
                                                           expirationIntervalInSeconds=45))]),
      Spec(end=(4, 5), act=[act_row(5, 4, "a", status=TTS_S2C, s2s=50, s2c=30, retry=(1, 2.0, 0, 0, ""),
                            expiration=NOW + 5 + 45 * S)],
           xfer=[activity_task(5)], ttask=[activity_timeout(5, S2C, T(5) + 30 * S, by=5)]))
def _():
    """tb:254-258 with an ExpirationTime later than the scheduleToClose expiry (retry expiration
    45 s > 30 s, msb:2018-2020): `Before` is false, the ScheduleToClose candidate stays at
    ScheduledTime + 30 s.  scheduleToStart is 50 s, so that candidate is the head: sb:267 an
    ActivityTimeout of type ScheduleToClose whose visibility is NOT the ExpirationTime; status 4.
    (The earlier-ExpirationTime branch needs a loaded row: CARRY_CASES.)"""


@case("act_exact_ties",
      head(more=[asched(5, "a", s2s=30, s2c=30), at(asched(6, "b", s2s=30, s2c=40), NOW + 5)]),
      Spec(end=(4, 6), act=[act_row(5, 4, "a", status=TTS_S2C, s2s=30, s2c=30),
                            act_row(6, 4, "b", status=0, s2s=30, s2c=40, scheduled_time=NOW + 5)],
           xfer=[activity_task(5), activity_task(6)], ttask=[activity_timeout(5, S2C, T(5) + 30 * S, by=5)]))
def _():
    """Exact ties in the activity pick, where Go's order comes from its map walk and an unstable
    sort (tb:252, 310) and this project's contract is (time, ScheduleID, kind order).  Two kinds
    of one activity: 5's ScheduleToClose and ScheduleToStart both expire at 5 + 30 s; the
    ScheduleToClose candidate (tb:259-267, made first) leads: sb:267 appends it, status 4.  Two
    activities: ActivityTaskScheduled(6) carries event 5's timestamp, so 6's ScheduleToStart
    expires at that same instant; the lower ScheduleID 5 leads, its head is created (tb:384-389):
    nothing is appended for 6 and its status stays 0."""


# ---- 2. user timers
@case("timer_started", head(more=[tstart(5, "t", 60)]),
      Spec(end=(4, 5), timer=[timer_row("t", 5, 60, 1)], xfer=[], ttask=[user_timer(5, T(5) + 60 * S)]))
def _():
    """msb:2877-2900: Version, TimerID, StartedID 5, ExpiryTime = timestamp + 60 s; sb:330 ->
    tb:171-184: the only timer is the head, TaskID = TimerTaskStatusCreated (1).  Tasks: sb:330
    UserTimerTask at the expiry, EventID = StartedID 5 (tb:391-398)."""


@case("timer_fired_repick",
      head(more=[tstart(5, "f1", 30), tstart(6, "f2", 60), tstart(7, "f3", 90)]) + [[tend(8, "Fired", "f1", 5)]],
      Spec(end=(8, 8), timer=[timer_row("f2", 6, 60, 1), timer_row("f3", 7, 90, 0)],
           xfer=[], ttask=[user_timer(5, T(5) + 30 * S), user_timer(6, T(6) + 60 * S, by=8)]))
def _():
    """msb:2930-2939 -> DeleteUserTimer, then sb:339 refreshUserTimerTask: f1 (the head so far,
    the only one with TaskID 1) is gone, f2 (6 + 60 s) is the new head and gets TaskID 1
    (tb:175-181); f3 was never a head: TaskID 0.  Tasks: sb:330 for f1 only — f2 and f3 start
    behind the created head (tb:370-375: nothing) —, then sb:339: TimerFired(8) appends f2's
    UserTimerTask (EventID 6)."""


@case("timer_canceled_repick",
      head(more=[tstart(5, "c1", 90), tstart(6, "c2", 20), tstart(7, "c3", 40)]) + [[tend(8, "Canceled", "c2", 6)]],
      Spec(end=(8, 8), timer=[timer_row("c1", 5, 90, 1), timer_row("c3", 7, 40, 1)],
           xfer=[], ttask=[user_timer(5, T(5) + 90 * S), user_timer(6, T(6) + 20 * S),
                           user_timer(7, T(7) + 40 * S, by=8)]))
def _():
    """msb:2982-2991, sb:348: c1 was the head when it started (TaskID 1), c2 (6 + 20 s) took
    over (TaskID 1), c3 (7 + 40 s) came behind c2 (TaskID 0).  Cancelling c2 makes c3 the head:
    TaskID 1; c1 keeps its stale 1 (nothing ever clears it).  Tasks: sb:330 twice — c2 starts
    later, expires earlier and takes the head: a second UserTimerTask —, none for c3, then sb:348:
    TimerCanceled(8) appends c3's (EventID 7)."""


@case("timer_repick_created_head_then_none",
      head(more=[tstart(5, "k1", 30), tstart(6, "k2", 20)]) + [[tend(7, "Canceled", "k2", 6)],
                                                               [tend(8, "Fired", "k1", 5)]],
      Spec(end=(8, 8), xfer=[], ttask=[user_timer(5, T(5) + 30 * S), user_timer(6, T(6) + 20 * S)]))
def _():
    """tb:370-375 in a re-pick: k1 (5 + 30 s) and then k2 (6 + 20 s) were heads (sb:330 twice).
    TimerCanceled(7) removes k2 (msb:2982-2991); the new head k1 was created already: sb:348's
    `timerTask != nil` is false, the list is unchanged.  TimerFired(8) removes the last timer
    (msb:2930-2939): tb:370 `len(tb.userTimers) > 0` is false, no task; the timer table is empty."""


@case("timer_expiry_tie",
      head(more=[tstart(5, "e1", 60), at(tstart(6, "e2", 60), NOW + 5)]) + [[tend(7, "Fired", "e1", 5)]],
      Spec(end=(7, 7), timer=[timer_row("e2", 6, 60, 1, expiry=NOW + 5 + 60 * S)],
           xfer=[], ttask=[user_timer(5, T(5) + 60 * S), user_timer(6, T(5) + 60 * S, by=7)]))
def _():
    """An exact expiry tie: TimerStarted(6) carries event 5's timestamp, both timers expire at
    NOW + 5 + 60 s.  Go orders equal expiries by a sequence number that follows its map walk
    (tb:236-245, 410-418); this project's contract is (expiry, StartedID): e1 stays the head,
    created: sb:330 appends nothing for e2, its TaskID stays 0.  TimerFired(7) removes e1 and
    sb:339 appends e2's UserTimerTask, EventID 6, at the same visibility; TaskID 1."""


# ---- 3. the events without a mutable-state action
@case("noop_marker", head() + [[marker(5)]], Spec(end=(5, 5), **HEAD_ONLY))
def _():
    """sb:470-471 MarkerRecorded: only sb:155 (LastEventTaskID), sb:603-604 and the version
    prelude (sb:134-154: last write / version-history item at event 5) move."""


@case("noop_cancel_timer_failed", head(more=[ev(5, "CancelTimerFailed", timerId="zz")]),
      Spec(end=(4, 5), **HEAD_ONLY))
def _():
    """sb:352-353 CancelTimerFailed: no mutable state action; counters as for noop_marker, the
    event joining call 2 (LastFirstEventID stays 4)."""


@case("noop_request_cancel_activity_failed",
      head() + [[ev(5, "RequestCancelActivityTaskFailed", activityId="zz")], [marker(6)]],
      Spec(end=(6, 6), **HEAD_ONLY))
def _():
    """sb:321-322 RequestCancelActivityTaskFailed (an activity id nobody scheduled: it is not
    looked up), then a marker in a call of its own: counters only."""


# ---- 4. children
@case("child_initiated", head(more=[cinit(5, pcp="TERMINATE")]),
      Spec(end=(4, 5), child=[child_row(5, 4, pcp=2)], xfer=[child_task(5)], ttask=[]))
def _():
    """msb:3256-3280: Version, InitiatedID 5, InitiatedEventBatchID 4, StartedID EmptyEventID,
    StartedWorkflowID = the attribute's workflowId, DomainName, WorkflowTypeName,
    ParentClosePolicy TERMINATE (2); CreateRequestID = sb:357 uuid.New() -> cdr_uuid site 2.
    Tasks: sb:370 StartChildExecutionTask: TargetDomainID = the domain cache's id for "target"
    (sb:365), TargetWorkflowID "child-wid", InitiatedID 5, no TargetRunID (sb:643-653)."""


@case("child_started",
      head(more=[cinit(5, wid="cw2", domain="other", wtype="ct2", pcp="REQUEST_CANCEL")]) + [[cstart(6, 5, "cr2", "cw2")]],
      Spec(end=(6, 6), child=[child_row(5, 4, started=6, run="cr2", wid="cw2", domain="other", wtype="ct2", pcp=1)],
           xfer=[child_task(5, "id-of-other", "cw2")], ttask=[]))
def _():
    """msb:3312-3325: StartedID 6 and StartedRunID from the event's execution; the Version is
    not touched; everything of msb:3256-3280 stays.  Tasks: sb:370 with the id of domain "other"
    and workflow id "cw2"; ChildWorkflowExecutionStarted (sb:378-381) appends nothing and the
    task's TargetRunID stays empty."""


for _t, _started in (("StartChildWorkflowExecutionFailed", False), ("ChildWorkflowExecutionCompleted", True),
                     ("ChildWorkflowExecutionFailed", True), ("ChildWorkflowExecutionCanceled", True),
                     ("ChildWorkflowExecutionTimedOut", True), ("ChildWorkflowExecutionTerminated", True)):
    _calls = head(more=[cinit(5), cinit(6, wid="cw-b")]) + ([[cstart(7, 5)], [ref(8, _t, 5)]] if _started
                                                            else [[ref(7, _t, 5)]])
    _last = 8 if _started else 7

    @case("child_removed_" + _t.replace("ChildWorkflowExecution", "").replace("StartFailed", "start_failed").lower(),
          _calls, Spec(end=(_last, _last), child=[child_row(6, 4, wid="cw-b")],
                       xfer=[child_task(5), child_task(6, wid="cw-b")], ttask=[]))
    def _():
        """sb:373-406 -> DeletePendingChildExecution (msb:1138-1144): child 5 (started first,
        except for StartChildWorkflowExecutionFailed) leaves, child 6 stays as initiated.  Tasks:
        sb:370 twice; the child's start and close events append nothing."""


# ---- 5. request-cancel and signal of external workflows
@case("cancel_initiated", head(more=[rce(5)]),
      Spec(end=(4, 5), cancel=[cancel_row(5, 4)], xfer=[cancel_task(5)], ttask=[]))
def _():
    """msb:2577-2596: Version, InitiatedEventBatchID 4, InitiatedID 5; CancelRequestID = sb:410
    uuid.New() -> cdr_uuid site 3.  childWorkflowOnly unset, no control.  Tasks: sb:421
    CancelExecutionTask: the id of domain "target", "ext-wid", "ext-run", TargetChildWorkflowOnly
    false, InitiatedID 5 (sb:655-669)."""


@case("cancel_initiated_child_only",
      head() + [[dt_sched(5)], [dt_started(6, 5)], [dt_completed(7, 5, 6), rce(8, child_only=True, control="ctl")]],
      Spec(end=(7, 8), cancel=[cancel_row(8, 7)],
           exec=dict(last_processed_event=6, decision_original_scheduled_ts=NOW + 5),
           xfer=[decision_task(5), cancel_task(8, child_only=True)], ttask=[decision_timeout(5, by=6)]))
def _():
    """msb:2577-2596 behind a second decision: InitiatedEventBatchID 7.  childWorkflowOnly and
    control go to the transfer task only (sb:421-427), the row has neither.  The second
    decision: dtm:659-674 keeps DecisionTaskScheduled(5)'s timestamp, LastProcessedEvent 6.
    Tasks: the second decision's DecisionTask(5) (sb:196) and DecisionTimeout from event 6
    (sb:210), then sb:421 with TargetChildWorkflowOnly true (the control is not on the task)."""


_TWO_CANCELS = head(more=[rce(5), rce(6, child_only=True, control="ctl")])


@case("cancel_failed", _TWO_CANCELS + [[ref(7, "RequestCancelExternalWorkflowExecutionFailed", 5)]],
      Spec(end=(7, 7), cancel=[cancel_row(6, 4)], xfer=[cancel_task(5), cancel_task(6, child_only=True)], ttask=[]))
def _():
    """sb:429-432 -> DeletePendingRequestCancel (msb:1147-1153): 5 leaves, 6 stays.  Tasks: sb:421
    twice, TargetChildWorkflowOnly false then true; the failure event appends nothing."""


@case("cancel_delivered", _TWO_CANCELS + [[ref(7, "ExternalWorkflowExecutionCancelRequested", 6)]],
      Spec(end=(7, 7), cancel=[cancel_row(5, 4)], xfer=[cancel_task(5), cancel_task(6, child_only=True)], ttask=[]))
def _():
    """sb:434-437 -> DeletePendingRequestCancel (msb:1147-1153): 6 leaves, 5 stays.  Tasks: sb:421
    twice, as for cancel_failed."""


@case("signal_initiated", head(more=[sig(5, "sig", input="in-1")]),
      Spec(end=(4, 5), signal=[signal_row(5, 4, "sig", "in-1", "")], xfer=[signal_task(5)], ttask=[]))
def _():
    """msb:2701-2723: Version, InitiatedEventBatchID 4, InitiatedID 5, SignalName, Input; no
    control: nil.  SignalRequestID = sb:441 uuid.New() -> cdr_uuid site 4.  Tasks: sb:452
    SignalExecutionTask: the id of domain "target", "ext-wid", "ext-run", TargetChildWorkflowOnly
    false, InitiatedID 5 (sb:671-685)."""


@case("signal_initiated_child_only_control",
      head(more=[sig(5, "sig2", input=b"\x01\x02", control=b"ctl", child_only=True)]),
      Spec(end=(4, 5), signal=[signal_row(5, 4, "sig2", "b64:0102", "b64:63746c")],
           xfer=[signal_task(5, child_only=True)], ttask=[]))
def _():
    """msb:2716-2717 with binary input and control (HistoryBuilder interns bytes as "b64:" +
    hex); childWorkflowOnly goes to the transfer task only (sb:452-458): its flag is set there."""


_TWO_SIGNALS = head(more=[sig(5, "sig", input="in-1"), sig(6, "sig2", control="c6", child_only=True)])


@case("signal_failed", _TWO_SIGNALS + [[ref(7, "SignalExternalWorkflowExecutionFailed", 5)]],
      Spec(end=(7, 7), signal=[signal_row(6, 4, "sig2", "", "c6")],
           xfer=[signal_task(5), signal_task(6, child_only=True)], ttask=[]))
def _():
    """sb:460-463 -> DeletePendingSignal (msb:1156-1162): 5 leaves, 6 (no input, a control) stays.
    Tasks: sb:452 twice, TargetChildWorkflowOnly false then true."""


@case("signal_delivered", _TWO_SIGNALS + [[ref(7, "ExternalWorkflowExecutionSignaled", 6)]],
      Spec(end=(7, 7), signal=[signal_row(5, 4, "sig", "in-1", "")],
           xfer=[signal_task(5), signal_task(6, child_only=True)], ttask=[]))
def _():
    """sb:465-468 -> DeletePendingSignal (msb:1156-1162): 6 leaves, 5 stays.  Tasks: sb:452 twice."""


@case("ext_own_domain",
      head(more=[cinit(5, domain="home"), rce(6, domain="home"), sig(7, domain="other")]),
      Spec(end=(4, 7), exec=dict(domain_id="id-of-home"), child=[child_row(5, 4, domain="home")],
           cancel=[cancel_row(6, 4)], signal=[signal_row(7, 4)],
           xfer=[child_task(5, "id-of-home"), cancel_task(6, domain_id="id-of-home"),
                 signal_task(7, domain_id="id-of-other")], ttask=[]),
      domain_id="id-of-home")
def _():
    """A child and a request-cancel in the workflow's own domain: the event names the domain
    "home", whose id in the domain cache is this workflow's DomainID (msb:1648), so sb:365 / 417
    resolve the target to the same id the DecisionTask carries (sb:196); the signal goes to
    another domain (sb:448).  Rows: msb:3256-3280 (DomainName is the name, "home"), 2577-2596,
    2701-2723."""


# ---- 6. the workflow itself
@case("wf_signaled_twice", head(more=[ev(5, "WorkflowExecutionSignaled"), ev(6, "WorkflowExecutionSignaled")]),
      Spec(end=(4, 6), exec=dict(signal_count=2), **HEAD_ONLY))
def _():
    """msb:3082-3089: SignalCount++ per event."""


@case("wf_cancel_requested", head() + [[ev(5, "WorkflowExecutionCancelRequested")]],
      Spec(end=(5, 5), exec=dict(flags=xflags(XI_CANCEL)), **HEAD_ONLY))
def _():
    """msb:2504-2510: CancelRequested = true; the workflow keeps running."""


def _closed(status, batch, **more):
    return dict(state=COMPLETED, close_status=status, completion_event_batch_id=batch, **more)


@case("close_completed", head(more=[ev(5, "WorkflowExecutionCompleted")]),
      Spec(end=(4, 5), exec=_closed(1, 4), **closes(5)))
def _():
    """msb:2379-2394: Completed / Completed (wei:83-91), CompletionEventBatchID = the call's
    first event 4 — not the close event's own id 5.  Tasks: sb:488 -> sb:780 CloseExecutionTask,
    sb:785 DeleteHistoryEventTask at event 5's time + the domain's retention of 1 day (sb:763-772)."""


@case("close_failed", head() + [[ev(5, "WorkflowExecutionFailed")]], Spec(end=(5, 5), exec=_closed(2, 5), **closes(5)))
def _():
    """msb:2419-2434: Completed / Failed; the close is alone in its call: batch id 5.  Tasks:
    sb:498 -> sb:780, 785 as for close_completed."""


@case("close_failed_retention_zero", head() + [[ev(5, "WorkflowExecutionFailed")]],
      Spec(end=(5, 5), exec=_closed(2, 5), **closes(5, days=0)), retention_days=0)
def _():
    """msb:2419-2434 in a domain with a retention of 0 days: sb:772 adds a zero duration, the
    DeleteHistoryEventTask (sb:785) is visible at the close event's own time (tb:314-319)."""


@case("close_terminated_retention_three", head(more=[ev(5, "WorkflowExecutionTerminated")]),
      Spec(end=(4, 5), exec=_closed(4, 4), **closes(5, days=3)), retention_days=3)
def _():
    """msb:3047-3062 from Running: Completed / Terminated (4), batch id 4.  Retention 3 days:
    sb:528 -> sb:780, 785 with the DeleteHistoryEventTask at event 5's time + 72 h (sb:772)."""


@case("close_timed_out", head() + [[marker(5), ev(6, "WorkflowExecutionTimedOut")]],
      Spec(end=(5, 6), exec=_closed(6, 5), **closes(6)))
def _():
    """msb:2456-2471: Completed / TimedOut (6); batch id 5, the marker before it.  Tasks: sb:508
    -> sb:780, 785 from event 6, the close — not from the call's first event."""


@case("close_canceled",
      head() + [[ev(5, "WorkflowExecutionCancelRequested")], [dt_sched(6)], [dt_started(7, 6)],
                [dt_completed(8, 6, 7), ev(9, "WorkflowExecutionCanceled")]],
      Spec(end=(8, 9), exec=_closed(3, 8, last_processed_event=7, decision_original_scheduled_ts=NOW + 6,
                                    flags=xflags(XI_CANCEL)),
           xfer=[decision_task(6), close_task(9)], ttask=[decision_timeout(6, by=7), delete_history(9)]))
def _():
    """msb:2504-2510 then, a decision later, msb:2535-2549: Completed / Canceled (3), batch id
    8; CancelRequested stays set.  Tasks: the second decision's (sb:196, 210), then sb:518 ->
    sb:780 CloseExecution — the last of the transfer list — and sb:785 DeleteHistoryEvent — the
    last of the timer list — from event 9."""


@case("close_terminated_while_created", [[started(1), dt_sched(2)], [ev(3, "WorkflowExecutionTerminated")]],
      Spec(end=(3, 3), exec=_closed(4, 3, last_processed_event=EMPTY_ID, decision_version=1, decision_schedule_id=2,
                                    decision_timeout=10, decision_scheduled_ts=NOW + 2),
           head=None, xfer=[record_started(1), decision_task(2), close_task(3)],
           ttask=[wf_timeout(T(1) + 100 * S), delete_history(3)]))
def _():
    """msb:3047-3062 from Created (wei:65-71 accepts Terminated): Completed / Terminated (4),
    batch id 3.  The decision scheduled by event 2 is still pending (dtm:143-167: version 1,
    ScheduleID 2, timeout 10, attempt 0, both scheduled timestamps = event 2's) and
    LastProcessedEvent is still EmptyEventID (msb:1662).  Tasks: sb:173-174, sb:196, no
    DecisionTimeout (the decision never started: sb:210 not reached), sb:528 -> sb:780, 785."""


# ---- 7. search attributes, reset points, parent, cron / memo / retry
@case("sa_start_and_upserts",
      head_with(searchAttributes={"indexedFields": {"sk1": "v1", "sk2": "v2"}})[:2] +
      [[dt_completed(4, 2, 3), upsert(5, {"sk2": "v2b", "sk3": "v3"}), upsert(6, {"sk1": "v1c"})]],
      Spec(end=(4, 6), sa=[("sk1", "v1c"), ("sk2", "v2b"), ("sk3", "v3")],
           exec=dict(search_attr_len=3, flags=xflags(XI_SA)),
           xfer=[upsert_task(5), upsert_task(6)], ttask=[]))
def _():
    """msb:1710-1712 (two attributes on start) and msb:2746-2768 twice: the first upsert
    overwrites sk2 and adds sk3, the second overwrites sk1 (mergeMapOfByteArray: current[k] = v).
    Tasks: sb:535 once per upsert: two UpsertWorkflowSearchAttributesTasks, no field set
    (sb:687-689); the attributes on the Started event append none."""


@case("sa_upsert_from_nil", head(more=[upsert(5, {"u1": "x"})]),
      Spec(end=(4, 5), sa=[("u1", "x")],
           exec=dict(search_attr_len=1, flags=xflags(XI_SA)), xfer=[upsert_task(5)], ttask=[]))
def _():
    """msb:2761-2763: no search attributes on start, the upsert makes the map.  Tasks: sb:535."""


_RP_IN = {"points": [
    {"binaryChecksum": "cks-a", "runId": "prev-run", "firstDecisionCompletedId": 4, "createdTimeNano": 111,
     "resettable": True},
    {"binaryChecksum": "cks-b", "runId": "older-run", "firstDecisionCompletedId": 9, "createdTimeNano": 222,
     "expiringTimeNano": 333, "resettable": False}]}


@case("reset_points_on_start", head_with(prevAutoResetPoints=_RP_IN, continuedExecutionRunId="prev-run"),
      Spec(end=(4, 4), rp=[rp_row("cks-a", "prev-run", 4, 111, NOW + 1 + DAY, RP_ALL | RP_RESETTABLE | RP_EXPIRING),
                           rp_row("cks-b", "older-run", 9, 222, 333, RP_ALL | RP_EXPIRING)],
           exec=dict(reset_points_len=2, flags=xflags(XI_RP)), **HEAD_ONLY))
def _():
    """msb:1700-1705 -> msb:3184-3205: the point of the continued run "prev-run" gets
    ExpiringTimeNano = the Started event's timestamp + retention (1 day); the other point is
    copied as it is (expiring 333, resettable false)."""


@case("reset_points_from_checksums",
      [[started(1), dt_sched(2)], [dt_started(3, 2)],
       [ev(4, "DecisionTaskCompleted", scheduledEventId=2, startedEventId=3, binaryChecksum="cks-new"), sig(5)],
       [dt_sched(6), dt_started(7, 6)],
       [ev(8, "DecisionTaskCompleted", scheduledEventId=6, startedEventId=7, binaryChecksum="cks-2")],
       [dt_sched(9), dt_started(10, 9)],
       [ev(11, "DecisionTaskCompleted", scheduledEventId=9, startedEventId=10, binaryChecksum="cks-new")]],
      Spec(end=(11, 11), signal=[signal_row(5, 4)],
           rp=[rp_row("cks-new", RUN, 4, BATCH_NOW, 0, RP_ALL | RP_RESETTABLE), rp_row("cks-2", RUN, 8, BATCH_NOW, 0, RP_ALL)],
           exec=dict(reset_points_len=2, last_processed_event=10, decision_original_scheduled_ts=NOW + 9,
                     flags=xflags(XI_RP)),
           xfer=[signal_task(5), decision_task(6), decision_task(9)],
           ttask=[decision_timeout(6, by=7), decision_timeout(9, by=10)]))
def _():
    """dtm:789-800 -> msb:1798-1842: a new binary checksum appends a point (RunId = the
    workflow's, FirstDecisionCompletedId = the event's id, CreatedTimeNano = timeSource.Now(),
    resettable by CheckResettable msb:1845-1862).  The first is resettable; the second is added
    while a signal is pending: not resettable; the third decision repeats "cks-new": no point
    (msb:1814-1819).  Tasks: sb:452 for the signal, then sb:196 and sb:210 for each of the two
    further decisions, interleaved in event order across the calls."""


_PARENT = dict(parentWorkflowDomain="pdom", parentWorkflowExecution={"workflowId": "pwid", "runId": "prun"},
               parentInitiatedEventId=17)


def _without(d, key):
    return {k: v for k, v in d.items() if k != key}


@case("parent_all", head_with(**_PARENT),
      Spec(end=(4, 4), exec=dict(parent_domain_id="id-of-pdom", parent_workflow_id="pwid", parent_run_id="prun",
                                 initiated_id=17), **HEAD_ONLY))
def _():
    """sb:160-167 (the domain cache's id for the parent domain), msb:1673-1684: all three parts."""


@case("parent_no_domain", head_with(**_without(_PARENT, "parentWorkflowDomain")),
      Spec(end=(4, 4), exec=dict(parent_workflow_id="pwid", parent_run_id="prun", initiated_id=17), **HEAD_ONLY))
def _():
    """msb:1673-1675: parentDomainID nil, ParentDomainID stays ""."""


@case("parent_no_execution", head_with(**_without(_PARENT, "parentWorkflowExecution")),
      Spec(end=(4, 4), exec=dict(parent_domain_id="id-of-pdom", initiated_id=17), **HEAD_ONLY))
def _():
    """msb:1676-1679: no ParentWorkflowExecution, both ids stay ""."""


@case("parent_no_initiated", head_with(**_without(_PARENT, "parentInitiatedEventId")),
      Spec(end=(4, 4), exec=dict(parent_domain_id="id-of-pdom", parent_workflow_id="pwid", parent_run_id="prun"),
           **HEAD_ONLY))
def _():
    """msb:1680-1684: ParentInitiatedEventId nil -> InitiatedID = EmptyEventID."""


@case("wf_cron_memo",
      head_with(cronSchedule="*/5 * * * *", memo={"fields": {"m": "1"}}, taskList={"name": "other-tl"},
                workflowType={"name": "other-wt"}, executionStartToCloseTimeoutSeconds=250,
                taskStartToCloseTimeoutSeconds=7),
      Spec(end=(4, 4), exec=dict(cron_schedule="*/5 * * * *", memo="[('m', '1')]", task_list="other-tl",
                                 workflow_type="other-wt", workflow_timeout=250, decision_timeout_value=7,
                                 flags=xflags(XI_MEMO)),
           head=dict(tl="other-tl", wf_timeout_s=250), **HEAD_ONLY))
def _():
    """msb:1651-1654, 1671, 1707-1709: task list, type, both timeouts, CronSchedule and Memo
    (HistoryBuilder interns a memo as repr(sorted(fields.items()))).  Tasks: sb:173
    WorkflowTimeout at + 250 s — a cron schedule without a first-decision backoff gives no
    backoff timer (sb:742) —; sb:196 DecisionTask on ExecutionInfo.TaskList "other-tl" although
    DecisionTaskScheduled(2) names "tl" (sb:789-794); sb:210 DecisionTimeout at + 10 s, the
    DecisionTaskScheduled event's timeout (dtm:157), not DecisionTimeoutValue 7."""


@case("started_backoff_cron",
      head_with(firstDecisionTaskBackoffSeconds=60, initiator="CronSchedule", cronSchedule="* * * * *"),
      Spec(end=(4, 4), exec=dict(cron_schedule="* * * * *"), head=None,
           xfer=[record_started(1), decision_task(2)],
           ttask=[backoff_timer(T(1) + 60 * S, BACKOFF_CRON), wf_timeout(T(1) + 160 * S), decision_timeout(2, by=3)]))
def _():
    """sb:740-752: a first-decision backoff of 60 s on a run a cron schedule initiated: the
    WorkflowBackoffTimerTask at event 1's time + 60 s with WorkflowBackoffTimeoutTypeCron comes
    first, then the WorkflowTimeoutTask, pushed out by the backoff: + 100 s + 60 s (sb:743, 754).
    Neither the backoff nor the initiator is persisted (msb:1639-1716 reads neither)."""


@case("started_backoff_retry",
      head_with(firstDecisionTaskBackoffSeconds=30, initiator="RetryPolicy", attempt=1),
      Spec(end=(4, 4), exec=dict(attempt=1), head=None,
           xfer=[record_started(1), decision_task(2)],
           ttask=[backoff_timer(T(1) + 30 * S, BACKOFF_RETRY), wf_timeout(T(1) + 130 * S), decision_timeout(2, by=3)]))
def _():
    """sb:744-747 with another initiator (RetryPolicy): WorkflowBackoffTimeoutTypeRetry, at + 30 s;
    the WorkflowTimeoutTask at + 130 s behind it.  Attempt 1 is the event's (msb:1686)."""


@case("wf_retry_expiration_attempt",
      head_with(retryPolicy=dict(initialIntervalInSeconds=3, backoffCoefficient=2.5, maximumIntervalInSeconds=60,
                                 maximumAttempts=5, expirationIntervalInSeconds=600, nonRetriableErrorReasons=["x"]),
                expirationTimestamp=NOW + 600 * S, attempt=2),
      Spec(end=(4, 4), exec=dict(attempt=2, initial_interval=3, maximum_interval=60, backoff_coefficient=float.hex(2.5),
                                 maximum_attempts=5, expiration_seconds=600, expiration_time=NOW + 600 * S,
                                 nonretriable="x",
                                 flags=xflags(XI_RETRY | XI_EXPIRATION)), **HEAD_ONLY))
def _():
    """msb:1686-1698: Attempt, ExpirationTime (from expirationTimestamp) and the six retry
    policy fields."""


@case("wf_other_domain_and_retention",
      head_with(prevAutoResetPoints={"points": [{"binaryChecksum": "cks-r", "runId": "prev-3"}]},
                continuedExecutionRunId="prev-3"),
      Spec(end=(4, 4), rp=[rp_row("cks-r", "prev-3", 0, 0, NOW + 1 + 3 * DAY, 0x1 | 0x2 | RP_EXPIRING)],
           exec=dict(domain_id="other-domain-id", reset_points_len=1,
                     flags=xflags(XI_RP)), **HEAD_ONLY),
      domain_id="other-domain-id", retention_days=3)
def _():
    """msb:1648 (DomainID = the domain entry's) and msb:3195 with a retention of 3 days; the
    point carries a checksum and a run id only: the other fields stay unset.  Tasks: the head's,
    the DecisionTask with this workflow's DomainID "other-domain-id" (sb:196)."""


# ---- 8. decisions
@case("decision_scheduled_with_attempt", [[started(1), dt_sched(2, attempt=3)]],
      Spec(end=(1, 2), exec=dict(state=CREATED, last_processed_event=EMPTY_ID, decision_version=1,
                                 decision_schedule_id=2, decision_timeout=10, decision_attempt=3,
                                 decision_scheduled_ts=NOW + 2),
           head=None, xfer=[record_started(1), decision_task(2)], ttask=[wf_timeout(T(1) + 100 * S)]))
def _():
    """dtm:143-167: Version, ScheduleID 2, StartedID EmptyEventID, RequestID emptyUUID, timeout
    10, Attempt from the event (3), both scheduled timestamps = the event's (sb:189-191).  The
    workflow is still Created (msb:1656-1661), LastProcessedEvent EmptyEventID (msb:1662).
    Tasks: sb:173-174 and sb:196; a DecisionTask carries no attempt (sb:619-629)."""


@case("decision_started", [[started(1), dt_sched(2, attempt=3)], [dt_started(3, 2)]],
      Spec(end=(3, 3), exec=dict(last_processed_event=EMPTY_ID, decision_version=1, decision_schedule_id=2,
                                 decision_started_id=3, decision_request_id="r3", decision_timeout=10,
                                 decision_started_ts=NOW + 3, decision_scheduled_ts=NOW + 2),
           head=None, xfer=[record_started(1), decision_task(2)],
           ttask=[wf_timeout(T(1) + 100 * S), decision_timeout(2, by=3)]))
def _():
    """dtm:200-253: Running (dtm:228-235), StartedID 3, RequestID, StartedTimestamp = the
    event's, the scheduled timestamps kept — and Attempt forced to 0 although the schedule
    said 3 (dtm:224).  Tasks: sb:210 passes that decision's Attempt on: the DecisionTimeoutTask's
    ScheduleAttempt is 0, not 3 (tb:322-331)."""


@case("decision_timed_out_schedule_to_start",
      [[started(1), dt_sched(2)],
       [ev(3, "DecisionTaskTimedOut", scheduledEventId=2, startedEventId=0, timeoutType="SCHEDULE_TO_START")]],
      Spec(end=(3, 3), exec=dict(state=CREATED, last_processed_event=EMPTY_ID, decision_original_scheduled_ts=0),
           head=None, xfer=[record_started(1), decision_task(2)], ttask=[wf_timeout(T(1) + 100 * S)]))
def _():
    """dtm:269-279 with TimeoutTypeScheduleToStart: FailDecision(false) (dtm:635-656): every
    decision field reset, Attempt 0, ScheduledTimestamp 0, OriginalScheduledTimestamp 0; with
    DecisionAttempt 0 no transient decision follows (dtm:170-172).  Tasks: sb:234 `decision !=
    nil` is false: no second DecisionTask; only sb:173-174 and sb:196."""


def _transient(schedule_id, attempt, version=1):
    return dict(last_processed_event=EMPTY_ID, decision_version=By(EMPTY_V, version, version),
                decision_schedule_id=schedule_id, decision_timeout=10, decision_attempt=attempt,
                decision_scheduled_ts=BATCH_NOW, decision_original_scheduled_ts=0)


@case("decision_timed_out_start_to_close",
      [[started(1), dt_sched(2)], [dt_started(3, 2)],
       [ev(4, "DecisionTaskTimedOut", scheduledEventId=2, startedEventId=3, timeoutType="START_TO_CLOSE")]],
      Spec(end=(4, 4), exec=_transient(4, 1), head=None,
           xfer=[record_started(1), decision_task(2), decision_task(4)],
           ttask=[wf_timeout(T(1) + 100 * S), decision_timeout(2, by=3)]))
def _():
    """dtm:269-279 -> FailDecision(true): Attempt 0 + 1, ScheduledTimestamp = Now; then sb:229 ->
    dtm:169-198 the transient decision: Version = GetCurrentVersion() (msb:491-502: EmptyVersion
    for a local builder, the event's version otherwise), ScheduleID = NextEventID — still 4, set
    by the previous call (sb:604) —, timeout = DecisionTimeoutValue 10, Attempt 1,
    ScheduledTimestamp = Now, OriginalScheduledTimestamp 0 (not set in dtm:184-194).  Tasks:
    sb:235 a DecisionTask whose ScheduleID is the transient decision's 4; no DecisionTimeout for
    it, it has not started."""


@case("transient_decision_started",
      [[started(1, taskStartToCloseTimeoutSeconds=7), dt_sched(2)], [dt_started(3, 2)],
       [ev(4, "DecisionTaskTimedOut", scheduledEventId=2, startedEventId=3, timeoutType="START_TO_CLOSE")],
       [dt_started(5, 4)]],
      Spec(end=(5, 5), exec=dict(decision_timeout_value=7, last_processed_event=EMPTY_ID, decision_version=1,
                                 decision_schedule_id=4, decision_started_id=5, decision_request_id="r5",
                                 decision_timeout=7, decision_attempt=0, decision_started_ts=NOW + 5,
                                 decision_scheduled_ts=BATCH_NOW, decision_original_scheduled_ts=0),
           head=None, xfer=[record_started(1), decision_task(2), decision_task(4)],
           ttask=[wf_timeout(T(1) + 100 * S), decision_timeout(2, by=3), decision_timeout(4, by=5, timeout_s=7)]))
def _():
    """The transient decision (dtm:169-198: ScheduleID 4, timeout = DecisionTimeoutValue 7, Attempt
    1, ScheduledTimestamp Now) starts: DecisionTaskStarted(5) names ScheduleID 4 and dtm:212 finds
    it.  dtm:224 forces Attempt to 0, dtm:238-249: Version the event's, StartedID 5, RequestID,
    DecisionTimeout 7 and ScheduledTimestamp kept, OriginalScheduledTimestamp 0.  Tasks: sb:235
    DecisionTask(4); then sb:210 the DecisionTimeoutTask of the retried decision: EventID 4, event
    5's time + 7 s — the first decision's was + 10 s, its DecisionTaskScheduled event's — and
    ScheduleAttempt 0: on this path the attempt never reaches the task (sb:204 passes nil,
    dtm:224; tb:322-331)."""


@case("decision_failed",
      [[started(1), dt_sched(2)], [dt_started(3, 2)],
       [ev(4, "DecisionTaskFailed", 11, scheduledEventId=2, startedEventId=3)]],
      Spec(end=(4, 4), exec=_transient(4, 1, 11), vh=[(3, 1), (4, 11)], repl=repl_state(11, 1, 11, 4),
           head=None, xfer=[record_started(1), decision_task(2), decision_task(4)],
           ttask=[wf_timeout(T(1) + 100 * S), decision_timeout(2, by=3)]))
def _():
    """dtm:264-267 FailDecision(true), then the transient decision as for a start-to-close
    timeout (sb:241-257, dtm:169-198).  The failing event is the first of version 11: the
    prelude has already moved the current version (sb:137, 140 -> msb:473-475, before the
    version-history item is added), so the transient decision's Version is 11, not 1.  Tasks:
    sb:253 DecisionTask with the transient ScheduleID 4; the task's version is 0 all the same."""


@case("started_twice_while_created",
      [[started(1, memo={"fields": {"keep": "1"}},
                prevAutoResetPoints={"points": [{"binaryChecksum": "cks-gone", "runId": "r0"}]}), dt_sched(2, attempt=3)],
       [started(3, 11, taskList={"name": "tl2"}, workflowType={"name": "wt2"}, executionStartToCloseTimeoutSeconds=50,
                taskStartToCloseTimeoutSeconds=5, parentInitiatedEventId=9)]],
      Spec(end=(3, 3), vh=[(2, 1), (3, 11)], repl=repl_state(11, 11, 11, 3),
           exec=dict(task_list="tl2", workflow_type="wt2", workflow_timeout=50, decision_timeout_value=5, initiated_id=9,
                     state=CREATED, last_processed_event=EMPTY_ID, decision_attempt=3, decision_scheduled_ts=NOW + 2,
                     memo="[('keep', '1')]", flags=xflags(XI_MEMO),
                     branch_id_lo=lambda c: uuid(c.key, UUID_BRANCH, 3)[0],
                     branch_id_hi=lambda c: uuid(c.key, UUID_BRANCH, 3)[1]),
           head=None, xfer=[record_started(1), decision_task(2), record_started(3)],
           ttask=[wf_timeout(T(1) + 100 * S), wf_timeout(T(3) + 50 * S, by=3)]))
def _():
    """A second Started while the workflow is still Created (wei:58-63 accepts it) shows what
    msb:1639-1716 resets of a pending decision: exactly DecisionVersion, DecisionScheduleID,
    DecisionStartedID, DecisionRequestID and DecisionTimeout (msb:1665-1669) — DecisionAttempt 3
    and the two scheduled timestamps of DecisionTaskScheduled(2) survive.  The attributes are the
    second event's, but the first event's Memo stays — msb:1707-1709 writes it only when the event
    has one — while its reset point goes: msb:1700-1705 assigns AutoResetPoints always, here nil
    (msb:3191-3193).  sb:176 makes a new branch token (cdr_uuid at event 3) and sb:182-184 sets
    StartVersion to the second event's version 11.  Tasks: sb:173-174 run for each Started event:
    a second RecordWorkflowStarted and a second WorkflowTimeout, at event 3's time + the new 50 s;
    the DecisionTask(2) between them went to the task list of that moment, "tl" (sb:196)."""


@case("marker_on_a_fresh_builder", [[marker(1, 11)]],
      Spec(end=(1, 1), vh=[(1, 11)], repl=repl_state(11, 1, 11, 1),
           exec=dict(domain_id="", workflow_id="", run_id="", create_request_id="", task_list="", workflow_type="",
                     branch_tree_id="", workflow_timeout=0, decision_timeout_value=0, initiated_id=0, branch_id_lo=0,
                     branch_id_hi=0, flags=0, state=CREATED, last_processed_event=EMPTY_ID,
                     decision_original_scheduled_ts=0), head=None, xfer=[], ttask=[]))
def _():
    """A history without a Started event shows what the constructors leave (msb:137-231):
    DecisionVersion EmptyVersion, DecisionScheduleID / StartedID EmptyEventID, DecisionRequestID
    emptyUUID, State Created, LastProcessedEvent EmptyEventID, everything else Go's zero value
    (InitiatedID 0, not EmptyEventID: msb:1680-1684 never ran; no branch token: sb:176 never
    ran).  2DC: StartVersion stays the constructor's — the domain's failover version 1
    (msb:211-213) — while the marker's version 11 moves the rest (sb:137-138)."""


@case("decision_failed_then_timed_out",
      [[started(1, 11), dt_sched(2, 11)], [dt_started(3, 2, 11)],
       [ev(4, "DecisionTaskFailed", 11, scheduledEventId=2, startedEventId=3)],
       [ev(5, "DecisionTaskTimedOut", 11, scheduledEventId=4, startedEventId=0, timeoutType="SCHEDULE_TO_CLOSE")]],
      Spec(end=(5, 5), version=11, exec=_transient(5, 2, 11), head=None,
           xfer=[record_started(1), decision_task(2), decision_task(4), decision_task(5)],
           ttask=[wf_timeout(T(1) + 100 * S), decision_timeout(2, by=3)]))
def _():
    """The transient decision of event 4 (attempt 1) times out: FailDecision(true) makes the
    attempt 2 (dtm:651-654) and the next transient decision sits at NextEventID 5 (dtm:186).
    All events carry version 11 (cluster 0's, meta:187-203): DecisionVersion 11 for 2DC / NDC.
    Tasks: sb:253 DecisionTask(4), then sb:235 DecisionTask(5): each transient ScheduleID is the
    NextEventID the previous call left (sb:604)."""


@case("decision_failed_beside_a_timer",
      [[started(1, 11), dt_sched(2, 11)], [dt_started(3, 2, 11)], [dt_completed(4, 2, 3, 11), tstart(5, "dft", 60, 11)],
       [dt_sched(6, 11), dt_started(7, 6, 11)],
       [ev(8, "DecisionTaskFailed", 11, scheduledEventId=6, startedEventId=7)]],
      Spec(end=(8, 8), version=11, timer=[timer_row("dft", 5, 60, 1, version=11)],
           exec=dict(_transient(8, 1, 11), last_processed_event=3), head=None,
           xfer=[record_started(1), decision_task(2), decision_task(6), decision_task(8)],
           ttask=[wf_timeout(T(1) + 100 * S), decision_timeout(2, by=3), user_timer(5, T(5) + 60 * S),
                  decision_timeout(6, by=7)]))
def _():
    """The transient decision (dtm:169-198) of a history that also starts a user timer — which
    keeps it off the fast-path kernel for every builder: the second decision (6, 7) fails, the
    transient one sits at NextEventID 8 (sb:604 of the previous call) with attempt 1, version 11
    for 2DC / NDC; LastProcessedEvent is the first decision's 3 (dtm:789-800), the failed one
    never completed.  Tasks: sb:330 UserTimer(5) between the two DecisionTimeouts (sb:210 from
    events 3 and 7); sb:196 DecisionTask(6), sb:253 DecisionTask(8)."""


# ---- 9. versions
@case("xdc_second_cluster", head() + [[marker(5, 2), tstart(6, "x2", 60, 2)]],
      Spec(end=(5, 6), timer=[timer_row("x2", 6, 60, 1, version=2)], vh=[(4, 1), (6, 2)],
           repl=repl_state(2, 1, 2, 6, lri={1: (2, 6)}), xfer=[], ttask=[user_timer(6, T(6) + 60 * S)]))
def _():
    """sb:134-138 with a call of version 2 — cluster 1's (2 % 10, meta:187-203), not the current
    one: CurrentVersion 2 (msb:548-556), LastWriteVersion 2 / LastWriteEventID 6 and
    LastReplicationInfo[cluster 1] = (2, 6) (msb:561-581); StartVersion stays the Started event's 1
    (sb:182-184).  NDC: a second item (vh:229-231).  The timer carries version 2.  Tasks: sb:330
    UserTimer(6); the task's version is 0 whatever the event's (schema.h:564-566)."""


@case("xdc_third_then_second_cluster", head(3) + [[marker(5, 12)]],
      Spec(end=(5, 5), vh=[(4, 3), (5, 12)], repl=repl_state(12, 3, 12, 5, lri={2: (3, 4), 1: (12, 5)}), **HEAD_ONLY))
def _():
    """The head at version 3 (cluster 2's): StartVersion 3, LastReplicationInfo[2] follows each
    call's last event up to (3, 4); then one event of version 12 (cluster 1's): a second entry
    (12, 5), the first kept (msb:570-580)."""


@case("versions_rise_in_and_between_calls",
      head(more=[marker(5, 11), asched(6, "a", 11)]) + [[cinit(7, version=21), rce(8, version=21),
                                                         sig(9, version=21), tstart(10, "vt", 60, 21)]],
      Spec(end=(7, 10), act=[act_row(6, 4, "a", status=TTS_S2S, version=11)],
           timer=[timer_row("vt", 10, 60, 1, version=21)], child=[child_row(7, 7, version=21)],
           cancel=[cancel_row(8, 7, version=21)], signal=[signal_row(9, 7, version=21)],
           vh=[(4, 1), (6, 11), (10, 21)], repl=repl_state(21, 1, 21, 10),
           xfer=[activity_task(6), child_task(7), cancel_task(8), signal_task(9)],
           ttask=[activity_timeout(6, S2S, T(6) + 5 * S, by=6), user_timer(10, T(10) + 60 * S)]))
def _():
    """Versions 1, 11, 21 are all cluster 0's, the current one: no LastReplicationInfo
    (msb:570).  Each row takes its event's version (msb:1993, 2586, 2711, 2889, 3265) and the
    batch id of its call (7).  NDC: the version rises inside call 2 (events 5-6) and again at
    call 3: three items (vh:229-235).  Tasks: sb:265, 267 (event 6), sb:370, 421, 452, 330 (events
    7-10), every one with version 0."""


# ---- 10. continue-as-new
@case("continue_as_new", head(more=[can(5)]),
      Spec(end=(4, 5), exec=_closed(5, 4), flags=APPLIED, **closes(5)),
      new_run=[started(1, 11, cronSchedule="@daily", attempt=1), dt_sched(2, 11)], new_run_call=2,
      new_run_spec=Spec(end=(1, 2), version=11,
                        exec=dict(state=CREATED, last_processed_event=EMPTY_ID, cron_schedule="@daily", attempt=1,
                                  decision_version=11, decision_schedule_id=2, decision_timeout=10,
                                  decision_scheduled_ts=NOW + 2),
                        head=None, xfer=[record_started(1), decision_task(2)], ttask=[wf_timeout(T(1) + 100 * S)]))
def _():
    """sb:537-595.  The parent: msb:3207-3224 Completed / ContinuedAsNew (5), batch id 4; its
    result says the new run's history was applied.  The new run (sb:542-571): a fresh builder —
    NDC behind an NDC parent, 2DC otherwise —, the parent's domain and workflow id, the run id of
    the event's newExecutionRunId, its own request id and branch; Started(1) and
    DecisionTaskScheduled(2) of version 11 in one call leave it Created with decision 2 pending,
    ReplicationState all 11 (sb:137-138, 182-184) or one version-history item (2, 11).  Tasks:
    the parent's list ends with sb:592 -> sb:780 CloseExecution and sb:785 DeleteHistoryEvent from
    event 5; the new run's own lists (sb:576-577, its state builder's) are its Started tasks
    (sb:173-174: WorkflowTimeout at its event 1's time + 100 s, no backoff although it has a cron
    schedule: sb:742) and its first DecisionTask(2) (sb:196), in the parent's domain."""


# ---- 11. every table at once
_DENSE = [[started(1, searchAttributes={"indexedFields": {"dk": "dv"}},
                   prevAutoResetPoints={"points": [{"binaryChecksum": "cks-d", "runId": "gone-run",
                                                    "firstDecisionCompletedId": 4, "createdTimeNano": 5,
                                                    "resettable": True}]},
                   continuedExecutionRunId="prev-d"), dt_sched(2)],
          [dt_started(3, 2)],
          [dt_completed(4, 2, 3), asched(5, "da"), tstart(6, "dt", 60), cinit(7), rce(8),
           sig(9, "dsig", input="din", control="dctl"), upsert(10, {"dk2": "dv2"})],
          [at_started(11, 5), ev(12, "WorkflowExecutionSignaled")]]


@case("dense_all_tables", _DENSE,
      Spec(end=(11, 12), act=[act_row(5, 4, "da", status=TTS_S2S | TTS_STC, started=11, request_id="a11")],
           timer=[timer_row("dt", 6, 60, 1)], child=[child_row(7, 4)], cancel=[cancel_row(8, 4)],
           signal=[signal_row(9, 4, "dsig", "din", "dctl")], sa=[("dk", "dv"), ("dk2", "dv2")],
           rp=[rp_row("cks-d", "gone-run", 4, 5, 0, RP_ALL | RP_RESETTABLE)],
           exec=dict(signal_count=1, reset_points_len=1, search_attr_len=2,
                     flags=xflags(XI_SA | XI_RP)),
           xfer=[activity_task(5), child_task(7), cancel_task(8), signal_task(9), upsert_task(10)],
           ttask=[activity_timeout(5, S2S, T(5) + 5 * S, by=5), user_timer(6, T(6) + 60 * S),
                  activity_timeout(5, STC, T(11) + 20 * S, by=11)]),
      sites=("dense",))
def _():
    """Every table populated by 12 events: msb:1700-1712 (a reset point of another run: no
    expiry added; a search attribute), msb:1982-2028 + 2083-2098 (activity 5 started by 11:
    timers 5 + 30 s / 11 + 20 s, startToClose leads, status 2 | 1), msb:2877-2900, 3256-3280,
    2577-2596, 2701-2723, 2746-2768, 3082-3089.  Tasks: sb:265, 370, 421, 452, 535 on the transfer
    list; sb:267 (ScheduleToStart 5 + 5 s), sb:330, and sb:276 (StartToClose 11 + 20 s) in the
    next call on the timer list."""


# Fields of the output records that no replay from an empty state ever varies
CONSTANT: dict = {}


# ------------------------------------------------------------------ carry-in onto hand-made rows
@dataclass
class CarryCase:
    """A loaded state with rows set by hand, then one more event.  `prefix` is replayed to get
    a loaded state; `patch` = (table, row index, {field: value}) is then written into that row;
    `suffix` is the one call replayed onto it; `spec` the complete expected state."""
    name: str
    doc: str
    prefix: list
    patch: tuple
    suffix: list
    spec: Spec

    def state(self, builder, k):
        return self.spec.state(Ctx(builder, k, self.name))

    def tasks(self, builder, k):
        """The lists of the suffix call alone (the spec's `head` is None)."""
        return self.spec.tasks(Ctx(builder, k, self.name))


CARRY_CASES = [
    CarryCase(
        "carry_activity_row",
        """A loaded ActivityInfo (msb:272-295 Load) of a started, heartbeating, retried activity:
        Attempt 3, TimerTaskStatus 1 | 2 | 8, LastHeartBeatUpdatedTime 7 s after StartedTime.  Then
        ActivityTaskCancelRequested (msb:2264-2285) writes Version, CancelRequested and
        CancelRequestID and nothing else: every loaded field comes back as it went in.""",
        prefix=head(more=[asched(5, "a", hb=3, retry=_RETRY)]) + [[at_started(6, 5)]],
        patch=("act", 0, dict(attempt=3, timer_task_status=TTS_STC | TTS_S2S | TTS_HB,
                              last_heartbeat_time=NOW + 6 + 7 * S)),
        suffix=[acancel(7, "a", 11)],
        spec=Spec(end=(7, 7), vh=[(6, 1), (7, 11)], repl=repl_state(11, 1, 11, 7),
                  act=[act_row(5, 4, "a", status=TTS_STC | TTS_S2S | TTS_HB, version=11, started=6, request_id="a6",
                               cancel=7, hb=3, retry=(2, 1.5, 9, 4, "bad\x1fworse"), attempt=3,
                               heartbeat=NOW + 6 + 7 * S)],
                  head=None, xfer=[], ttask=[])),
    CarryCase(
        "carry_child_row",
        """A loaded ChildExecutionInfo that is already started: run "cr-1", and a StartedID set by
        hand to 60, which no event of the history carries.  The one further event initiates another
        child (msb:3256-3280) and leaves the loaded row alone: every field of it, the started ones
        included, comes back as it went in (msb:272-295 Load), next to the new row of version 11 and
        batch 7.  Tasks: the suffix's sb:370 StartChildExecutionTask for the new child only.""",
        prefix=head(more=[cinit(5, wid="cw", domain="other", wtype="ct", pcp="TERMINATE")]) + [[cstart(6, 5, "cr-1", "cw")]],
        patch=("child", 0, dict(started_id=60)),
        suffix=[cinit(7, wid="cw-new", version=11)],
        spec=Spec(end=(7, 7), vh=[(6, 1), (7, 11)], repl=repl_state(11, 1, 11, 7),
                  child=[child_row(5, 4, started=60, run="cr-1", wid="cw", domain="other", wtype="ct", pcp=2),
                         child_row(7, 7, wid="cw-new", version=11)],
                  head=None, xfer=[child_task(7, wid="cw-new")], ttask=[])),
    CarryCase(
        "carry_status_bit_cleared",
        """A loaded ActivityInfo whose TimerTaskStatus was cleared by hand and whose Attempt is 3.
        The suffix schedules a second activity (scheduleToStart 50 s, scheduleToClose 60 s); its pick
        (sb:267 -> tb:211-230) loads both rows: the head is 5's ScheduleToStart at 5 + 5 s, and with
        the bit cleared it counts as not created (tb:305, 384-389): an ActivityTimeoutTask for the
        LOADED activity, Attempt 3 taken from the row (tb:302, 404), and the bit is set again.  The
        unpatched state (bit 2 set by the prefix) would emit nothing.  sb:265: ActivityTask(6).""",
        prefix=head(more=[asched(5, "a")]),
        patch=("act", 0, dict(timer_task_status=0, attempt=3)),
        suffix=[asched(6, "b", s2s=50, s2c=60)],
        spec=Spec(end=(6, 6), act=[act_row(5, 4, "a", status=TTS_S2S, attempt=3),
                                   act_row(6, 6, "b", status=0, s2s=50, s2c=60)],
                  head=None, xfer=[activity_task(6)],
                  ttask=[activity_timeout(5, S2S, T(5) + 5 * S, by=6, attempt=3)])),
    CarryCase(
        "carry_status_bit_set",
        """A loaded ActivityInfo with the StartToClose bit set by hand.  ActivityTaskStarted(6)
        (msb:2083-2098) then picks (sb:276): ScheduleToClose 5 + 30 s against StartToClose 6 + 20 s;
        the head is StartToClose and the row says it is created (tb:278, 384-389): nothing is
        appended.  The unpatched state (bit 2 only) would emit the StartToClose ActivityTimeout.""",
        prefix=head(more=[asched(5, "a")]),
        patch=("act", 0, dict(timer_task_status=TTS_S2S | TTS_STC)),
        suffix=[at_started(6, 5)],
        spec=Spec(end=(6, 6), act=[act_row(5, 4, "a", status=TTS_S2S | TTS_STC, started=6, request_id="a6")],
                  head=None, xfer=[], ttask=[])),
    CarryCase(
        "carry_expiration_before_schedule_to_close",
        """A loaded ActivityInfo whose ExpirationTime was set by hand to ScheduledTime + 12 s, earlier
        than the scheduleToClose expiry 5 + 30 s — as a retried activity's is (msb:2011-2020 alone
        never makes it earlier).  ActivityTaskStarted(6) picks (sb:276): tb:254-258 takes the
        ScheduleToClose candidate's time from ExpirationTime, 5 + 12 s, ahead of StartToClose
        6 + 20 s: an ActivityTimeoutTask of type ScheduleToClose whose visibility is the
        ExpirationTime; status 2 | 4.""",
        prefix=head(more=[asched(5, "a")]),
        patch=("act", 0, dict(expiration_time=NOW + 5 + 12 * S)),
        suffix=[at_started(6, 5)],
        spec=Spec(end=(6, 6), act=[act_row(5, 4, "a", status=TTS_S2S | TTS_S2C, started=6, request_id="a6",
                                           expiration=NOW + 5 + 12 * S)],
                  head=None, xfer=[], ttask=[activity_timeout(5, S2C, T(5) + 12 * S, by=6)])),
    CarryCase(
        "carry_timer_task_id_cleared",
        """A loaded TimerInfo whose TaskID was cleared by hand.  TimerStarted(6) of a later timer
        (6 + 90 s) picks (sb:330 -> tb:171-184): the head is the LOADED timer (5 + 60 s), not created
        by its row (tb:242, 370-375): a UserTimerTask with EventID 5 appended by event 6, and TaskID
        1 again; the new timer's TaskID stays 0.  Unpatched, nothing would be appended.""",
        prefix=head(more=[tstart(5, "t", 60)]),
        patch=("timer", 0, dict(task_id=0)),
        suffix=[tstart(6, "u", 90)],
        spec=Spec(end=(6, 6), timer=[timer_row("t", 5, 60, 1), timer_row("u", 6, 90, 0)],
                  head=None, xfer=[], ttask=[user_timer(5, T(5) + 60 * S, by=6)])),
]


# ------------------------------------------------------------------ the comparer
def diff(want, got, path=""):
    """Every difference between an expected state and an exported one, as 'path: want != got'."""
    if isinstance(want, dict) and isinstance(got, dict):
        out = []
        for k in sorted(set(want) | set(got)):
            if k not in want or k not in got:
                out.append(f"{path}.{k}: {'missing in expected' if k not in want else 'missing in got'}")
            else:
                out += diff(want[k], got[k], f"{path}.{k}")
        return out
    if isinstance(want, list) and isinstance(got, list):
        if len(want) != len(got):
            return [f"{path}: {len(want)} rows expected, {len(got)} got"]
        return [d for j, (a, b) in enumerate(zip(want, got)) for d in diff(a, b, f"{path}[{j}]")]
    return [] if type(want) is type(got) and want == got else [f"{path}: {want!r} != {got!r}"]


def exported(batch, out, w, repl=True):
    """engine.export_state plus the replication record of every builder (`repl`=False: of the
    2DC builder only, as engine.compare reads it — the kernels leave other builders' records
    untouched)."""
    from cadence_amd import engine
    d = engine.export_state(batch, out, w)
    if d["result"]["code"] == abi.OK and "repl" not in d and repl:
        d["repl"] = engine._rec(out.repl[w], batch.strings or None)
    return d


# The filler of the lane-placement batch: not in the table.  It opens what dense_all_tables
# opens — one activity, one timer, one child, one request-cancel, one signal: the lane planner's
# entity counts and slot footprint — in as many events (12), and closes the first three again.
SPARSE_TWIN = Case(
    name="sparse_twin",
    doc="""msb:1247-1269 (the activity, never started, completes), msb:2930-2939 (the timer fires) and
    sb:373-376 -> msb:1138-1144 (the child fails to start) empty three tables again; the
    request-cancel (msb:2577-2596) and the signal (msb:2701-2723) of call 2 stay pending.  Tasks:
    sb:265, 370, 421, 452 and sb:267 (ScheduleToStart 5 + 5 s), sb:330; the three closing events
    append nothing — sb:285 and sb:339 pick from empty tables (tb:370, 384) — and there is no
    Upsert task and no StartToClose timeout: the two records the dense entry has beyond these.""",
    calls=head(more=[asched(5, "qa"), tstart(6, "qt", 60), cinit(7), rce(8), sig(9)]) +
    [[at_close(10, 5), tend(11, "Fired", "qt", 6), ref(12, "StartChildWorkflowExecutionFailed", 7)]],
    spec=Spec(end=(10, 12), cancel=[cancel_row(8, 4)], signal=[signal_row(9, 4)],
              xfer=[activity_task(5), child_task(7), cancel_task(8), signal_task(9)],
              ttask=[activity_timeout(5, S2S, T(5) + 5 * S, by=5), user_timer(6, T(6) + 60 * S)]))


# ------------------------------------------------------------------ the task table's coverage
# Every append site of stateBuilder.applyEvents: site -> (the event type(s) whose handler holds it,
# the task type it appends, the cases that reach it).  tests/test_task_sites.py checks that each
# named case expects such a record, appended by such an event.
_CLOSES = ("WorkflowExecutionCompleted", "WorkflowExecutionFailed", "WorkflowExecutionTimedOut",
           "WorkflowExecutionCanceled", "WorkflowExecutionTerminated", "WorkflowExecutionContinuedAsNew")
_CLOSE_CASES = ("close_completed", "close_failed", "close_timed_out", "close_canceled",
                "close_terminated_while_created", "close_terminated_retention_three", "close_failed_retention_zero",
                "continue_as_new")
TASK_SITES = {
    "sb:173": (("WorkflowExecutionStarted",), (T_WF_TIMEOUT, T_BACKOFF),
               ("noop_marker", "started_backoff_cron", "started_backoff_retry", "started_twice_while_created")),
    "sb:174": (("WorkflowExecutionStarted",), (T_RECORD_STARTED,), ("noop_marker", "started_twice_while_created")),
    "sb:196": (("DecisionTaskScheduled",), (T_DECISION,), ("noop_marker", "cancel_initiated_child_only", "wf_cron_memo")),
    "sb:210": (("DecisionTaskStarted",), (T_DECISION_TIMEOUT,), ("noop_marker", "transient_decision_started")),
    "sb:235": (("DecisionTaskTimedOut",), (T_DECISION,),
               ("decision_timed_out_start_to_close", "decision_failed_then_timed_out", "transient_decision_started")),
    "sb:253": (("DecisionTaskFailed",), (T_DECISION,), ("decision_failed", "decision_failed_beside_a_timer")),
    "sb:265": (("ActivityTaskScheduled",), (T_ACTIVITY,), ("act_no_retry", "act_retry_expiration_below")),
    "sb:267": (("ActivityTaskScheduled",), (T_ACTIVITY_TIMEOUT,), ("act_no_retry", "act_retry_expiration_equal")),
    "sb:276": (("ActivityTaskStarted",), (T_ACTIVITY_TIMEOUT,), ("act_cancel_after_start", "act_started_heartbeat")),
    "sb:285": (("ActivityTaskCompleted",), (T_ACTIVITY_TIMEOUT,), ("act_close_completed_picks",)),
    "sb:294": (("ActivityTaskFailed",), (T_ACTIVITY_TIMEOUT,), ("act_close_failed_picks",)),
    "sb:303": (("ActivityTaskTimedOut",), (T_ACTIVITY_TIMEOUT,), ("act_close_timedout_picks",)),
    "sb:317": (("ActivityTaskCanceled",), (T_ACTIVITY_TIMEOUT,), ("act_close_canceled_picks",)),
    "sb:330": (("TimerStarted",), (T_USER_TIMER,), ("timer_started", "timer_canceled_repick")),
    "sb:339": (("TimerFired",), (T_USER_TIMER,), ("timer_fired_repick", "timer_expiry_tie")),
    "sb:348": (("TimerCanceled",), (T_USER_TIMER,), ("timer_canceled_repick",)),
    "sb:370": (("StartChildWorkflowExecutionInitiated",), (T_CHILD,), ("child_initiated", "ext_own_domain")),
    "sb:421": (("RequestCancelExternalWorkflowExecutionInitiated",), (T_CANCEL,),
               ("cancel_initiated", "cancel_initiated_child_only")),
    "sb:452": (("SignalExternalWorkflowExecutionInitiated",), (T_SIGNAL,),
               ("signal_initiated", "signal_initiated_child_only_control")),
    "sb:535": (("UpsertWorkflowSearchAttributes",), (T_UPSERT,), ("sa_start_and_upserts", "sa_upsert_from_nil")),
    "sb:576-577": (("WorkflowExecutionContinuedAsNew",), (), ("continue_as_new",)),   # the new run's own lists
    "sb:780": (_CLOSES, (T_CLOSE,), _CLOSE_CASES),
    "sb:785": (_CLOSES, (T_DELETE_HISTORY,), _CLOSE_CASES),
}

# Fields of cdr_task that no stateBuilder task ever varies
TASK_CONSTANT = {"CdrTask.version": "sb:613-804 builds every task without a Version; it is the caller's to set "
                                    "(schema.h:564-566): 0"}


# ------------------------------------------------------------------ the task comparer
def without_by(rows):
    return [{f: v for f, v in r.items() if f != "by"} for r in rows]


def task_diff(want, got):
    """Every difference between expected lists ({"xfer": [...], "ttask": [...]}, `by` ignored)
    and exported ones, as 'list[j].field: want != got' — counts and order included."""
    return diff({k: without_by(want[k]) for k in TASK_LISTS}, got)


def split_by(want, first_suffix_event):
    """The hand-known split of expected lists at a carry-in cut: (the records appended by
    events before `first_suffix_event`, those appended at or after it)."""
    pre = {k: [r for r in want[k] if r["by"] < first_suffix_event] for k in TASK_LISTS}
    suf = {k: [r for r in want[k] if r["by"] >= first_suffix_event] for k in TASK_LISTS}
    return pre, suf


def exported_tasks(batch, out, w):
    """The task lists of entry w as engine._rec renders them (the four handles as strings)."""
    from cadence_amd import engine
    return {k: [engine._rec(r, batch.strings or None) for r in out.task_rows(w, k)] for k in TASK_LISTS}
