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


def rce(eid, child_only=False, control=None, version=1):
    a = dict(domain="target", workflowExecution={"workflowId": "ext-wid", "runId": "ext-run"},
             childWorkflowOnly=child_only)
    if control is not None:
        a["control"] = control
    return ev(eid, "RequestCancelExternalWorkflowExecutionInitiated", version, **a)


def sig(eid, name="sig", input=None, control=None, child_only=False, version=1):
    a = dict(domain="target", workflowExecution={"workflowId": "ext-wid", "runId": "ext-run"}, signalName=name,
             childWorkflowOnly=child_only)
    if input is not None:
        a["input"] = input
    if control is not None:
        a["control"] = control
    return ev(eid, "SignalExternalWorkflowExecutionInitiated", version, **a)


def upsert(eid, fields, version=1):
    return ev(eid, "UpsertWorkflowSearchAttributes", version, searchAttributes={"indexedFields": fields})


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
            task_list="tl", s2s=5, s2c=30, stc=20, hb=0, retry=None, attempt=0, heartbeat=None):
    """ActivityInfo of ActivityTaskScheduled(sid) in a call whose first event is `batch`
    (msb:1982-2028), started by event `started` (msb:2083-2098: StartedID, RequestID,
    StartedTime = LastHeartBeatUpdatedTime = its timestamp), cancel requested by event `cancel`
    (msb:2264-2285).  `retry` = (initial, coefficient, maximum interval, maximum attempts,
    non-retriable reasons joined by \\x1f); `expiration` defaults to ScheduledTime +
    scheduleToClose (msb:2011)."""
    r = retry or (0, 0.0, 0, 0, "")
    st = 0 if started is None else NOW + started
    return dict(version=version, schedule_id=sid, scheduled_event_batch_id=batch, scheduled_time=NOW + sid,
                started_id=EMPTY_ID if started is None else started, started_time=st,
                last_heartbeat_time=st if heartbeat is None else heartbeat,
                expiration_time=NOW + sid + s2c * S if expiration is None else expiration,
                cancel_request_id=EMPTY_ID if cancel is None else cancel, activity_id=aid, request_id=request_id,
                task_list=task_list, nonretriable=r[4], s2s=s2s, s2c=s2c, stc=stc, hb=hb, timer_task_status=status,
                attempt=attempt, initial_interval=r[0], maximum_interval=r[2], maximum_attempts=r[3],
                flags=(AI_CANCEL if cancel is not None else 0) | (AI_RETRY if retry else 0) |
                      (AI_STARTED if started is not None else 0),
                backoff_coefficient=float.hex(r[1]))


def timer_row(tid, started_id, fire_s, task_id, version=1):
    """TimerInfo of TimerStarted(started_id) (msb:2877-2900); task_id 1 once the timer was the
    head of a pick (tb:171-184)."""
    return dict(version=version, started_id=started_id, expiry_time=NOW + started_id + fire_s * S, task_id=task_id,
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
        return self.spec.state(Ctx(builder, k, self.name))

    def new_run_state(self, builder, k):
        """The continue-as-new run's entry: an NDC builder behind an NDC parent, otherwise a
        2DC builder (sb:542-556; build_batch: new_run_ndc = the parent is NDC)."""
        return self.new_run_spec.state(Ctx(N if builder == N else D2, k, self.name, new_run=True))


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
@case("act_no_retry", head(more=[asched(5, "a")]), Spec(end=(4, 5), act=[act_row(5, 4, "a", status=TTS_S2S)]))
def _():
    """msb:1982-2028 without a retry policy: every retry field zero, HasRetryPolicy false,
    ExpirationTime = ScheduledTime + scheduleToClose 30 s (msb:2011), CancelRequestID
    EmptyEventID, ScheduledEventBatchID = the call's first event 4.  sb:267 -> tb:211-230: the
    earliest of scheduleToClose (+30 s) and scheduleToStart (+5 s) is scheduleToStart, not yet
    created: TimerTaskStatus |= 2 (tb:36-47)."""


_RETRY = dict(initialIntervalInSeconds=2, backoffCoefficient=1.5, maximumIntervalInSeconds=9, maximumAttempts=4,
              expirationIntervalInSeconds=10, nonRetriableErrorReasons=["bad", "worse"])


@case("act_retry_expiration_below",
      head(more=[asched(5, "a", tl="atl", s2s=7, s2c=25, stc=11, hb=3, retry=_RETRY)]),
      Spec(end=(4, 5), act=[act_row(5, 4, "a", status=TTS_S2S, task_list="atl", s2s=7, s2c=25, stc=11, hb=3,
                                    retry=(2, 1.5, 9, 4, "bad\x1fworse"), expiration=NOW + 5 + 25 * S)]))
def _():
    """msb:2012-2021 with a retry policy whose expiration interval 10 s is below
    scheduleToClose 25 s: `10 > 25` is false, ExpirationTime stays ScheduledTime + 25 s; the
    five retry fields are copied (msb:2013-2017).  Timer: scheduleToStart (+7 s) first (tb:297-306)."""


@case("act_retry_expiration_equal",
      head(more=[asched(5, "a", s2s=40, s2c=30, retry=dict(initialIntervalInSeconds=1, backoffCoefficient=2.0,
                                                           expirationIntervalInSeconds=30))]),
      Spec(end=(4, 5), act=[act_row(5, 4, "a", status=TTS_S2C, s2s=40, s2c=30, retry=(1, 2.0, 0, 0, ""),
                                    expiration=NOW + 5 + 30 * S)]))
def _():
    """msb:2018 `expiration > scheduleToClose` with both 30 s: not larger, ExpirationTime =
    ScheduledTime + 30 s.  No non-retriable reasons, no maximum interval / attempts: zero.
    Timer: scheduleToStart is 40 s here, so scheduleToClose (+30 s) is the head: status |= 4
    (tb:254-267)."""


@case("act_retry_expiration_above",
      head() + [[asched(5, "a", retry=dict(initialIntervalInSeconds=6, backoffCoefficient=3.25,
                                           maximumIntervalInSeconds=100, maximumAttempts=0,
                                           expirationIntervalInSeconds=45, nonRetriableErrorReasons=["only"]))]],
      Spec(end=(5, 5), act=[act_row(5, 5, "a", status=TTS_S2S, retry=(6, 3.25, 100, 0, "only"),
                                    expiration=NOW + 5 + 45 * S)]))
def _():
    """msb:2018-2020: the retry expiration 45 s is larger than scheduleToClose 30 s and
    replaces it: ExpirationTime = ScheduledTime + 45 s.  The activity is scheduled in a call
    of its own: ScheduledEventBatchID 5 (sb:260).  The later ExpirationTime does not move the
    scheduleToClose timer (tb:254-258: only an earlier one does); scheduleToStart +5 s leads."""


@case("act_cancel_before_start", head(more=[asched(5, "a"), acancel(6, "a")]),
      Spec(end=(4, 6), act=[act_row(5, 4, "a", status=TTS_S2S, cancel=6)]))
def _():
    """msb:2264-2285 on an activity that has not started: Version = the event's, CancelRequested,
    CancelRequestID = the event's id 6; nothing else moves, no timer pick (sb:307-310)."""


@case("act_cancel_after_start", head(more=[asched(5, "a")]) + [[at_started(6, 5)], [acancel(7, "a")]],
      Spec(end=(7, 7), act=[act_row(5, 4, "a", status=TTS_S2S | TTS_STC, started=6, request_id="a6", cancel=7)]))
def _():
    """msb:2083-2098 then msb:2264-2285: StartedID 6, RequestID, StartedTime =
    LastHeartBeatUpdatedTime = event 6's timestamp; CancelRequestID 7.  Timer after the start
    (sb:276): scheduleToClose (5 + 30 s) against startToClose (6 + 20 s): startToClose, status
    2 | 1 (tb:269-279)."""


@case("act_started_heartbeat", head(more=[asched(5, "a", hb=3)]) + [[at_started(6, 5, 11)]],
      Spec(end=(6, 6), vh=[(5, 1), (6, 11)], repl=repl_state(11, 1, 11, 6),
           act=[act_row(5, 4, "a", status=TTS_S2S | TTS_HB, version=11, started=6, request_id="a6", hb=3)]))
def _():
    """tb:280-295: with a heartbeat timeout the started activity has a third timer, last
    heartbeat (= StartedTime, msb:2095) + 3 s, the earliest: status 2 | 8.  The Started event is
    of version 11: msb:2091 moves the row's Version from the schedule's 1."""


for _k in ("Completed", "Failed", "TimedOut", "Canceled"):
    @case(f"act_close_{_k.lower()}",
          head(more=[asched(5, "a"), asched(6, "b")]) + [[at_started(7, 5)], [at_close(8, 5, _k)]],
          Spec(end=(8, 8), act=[act_row(6, 4, "b", status=TTS_S2S)]))
    def _():
        """sb:280-305 / 312-319 -> DeleteActivity (msb:1247-1269): the started activity 5 leaves,
        6 stays.  6's timer status: at its own schedule the head is 5's scheduleToStart, already
        created (tb:384-389: nothing); when 5 starts, 5's timers are +30 s / +20 s and 6's
        scheduleToStart (6 + 5 s) leads: status 2 (sb:276); after the close it is the created head."""


# ---- 2. user timers
@case("timer_started", head(more=[tstart(5, "t", 60)]), Spec(end=(4, 5), timer=[timer_row("t", 5, 60, 1)]))
def _():
    """msb:2877-2900: Version, TimerID, StartedID 5, ExpiryTime = timestamp + 60 s; sb:330 ->
    tb:171-184: the only timer is the head, TaskID = TimerTaskStatusCreated (1)."""


@case("timer_fired_repick",
      head(more=[tstart(5, "f1", 30), tstart(6, "f2", 60), tstart(7, "f3", 90)]) + [[tend(8, "Fired", "f1", 5)]],
      Spec(end=(8, 8), timer=[timer_row("f2", 6, 60, 1), timer_row("f3", 7, 90, 0)]))
def _():
    """msb:2930-2939 -> DeleteUserTimer, then sb:339 refreshUserTimerTask: f1 (the head so far,
    the only one with TaskID 1) is gone, f2 (6 + 60 s) is the new head and gets TaskID 1
    (tb:175-181); f3 was never a head: TaskID 0."""


@case("timer_canceled_repick",
      head(more=[tstart(5, "c1", 90), tstart(6, "c2", 20), tstart(7, "c3", 40)]) + [[tend(8, "Canceled", "c2", 6)]],
      Spec(end=(8, 8), timer=[timer_row("c1", 5, 90, 1), timer_row("c3", 7, 40, 1)]))
def _():
    """msb:2982-2991, sb:348: c1 was the head when it started (TaskID 1), c2 (6 + 20 s) took
    over (TaskID 1), c3 (7 + 40 s) came behind c2 (TaskID 0).  Cancelling c2 makes c3 the head:
    TaskID 1; c1 keeps its stale 1 (nothing ever clears it)."""


# ---- 3. the events without a mutable-state action
@case("noop_marker", head() + [[marker(5)]], Spec(end=(5, 5)))
def _():
    """sb:470-471 MarkerRecorded: only sb:155 (LastEventTaskID), sb:603-604 and the version
    prelude (sb:134-154: last write / version-history item at event 5) move."""


@case("noop_cancel_timer_failed", head(more=[ev(5, "CancelTimerFailed", timerId="zz")]), Spec(end=(4, 5)))
def _():
    """sb:352-353 CancelTimerFailed: no mutable state action; counters as for noop_marker, the
    event joining call 2 (LastFirstEventID stays 4)."""


@case("noop_request_cancel_activity_failed",
      head() + [[ev(5, "RequestCancelActivityTaskFailed", activityId="zz")], [marker(6)]], Spec(end=(6, 6)))
def _():
    """sb:321-322 RequestCancelActivityTaskFailed (an activity id nobody scheduled: it is not
    looked up), then a marker in a call of its own: counters only."""


# ---- 4. children
@case("child_initiated", head(more=[cinit(5, pcp="TERMINATE")]), Spec(end=(4, 5), child=[child_row(5, 4, pcp=2)]))
def _():
    """msb:3256-3280: Version, InitiatedID 5, InitiatedEventBatchID 4, StartedID EmptyEventID,
    StartedWorkflowID = the attribute's workflowId, DomainName, WorkflowTypeName,
    ParentClosePolicy TERMINATE (2); CreateRequestID = sb:357 uuid.New() -> cdr_uuid site 2."""


@case("child_started",
      head(more=[cinit(5, wid="cw2", domain="other", wtype="ct2", pcp="REQUEST_CANCEL")]) + [[cstart(6, 5, "cr2", "cw2")]],
      Spec(end=(6, 6), child=[child_row(5, 4, started=6, run="cr2", wid="cw2", domain="other", wtype="ct2", pcp=1)]))
def _():
    """msb:3312-3325: StartedID 6 and StartedRunID from the event's execution; the Version is
    not touched; everything of msb:3256-3280 stays."""


for _t, _started in (("StartChildWorkflowExecutionFailed", False), ("ChildWorkflowExecutionCompleted", True),
                     ("ChildWorkflowExecutionFailed", True), ("ChildWorkflowExecutionCanceled", True),
                     ("ChildWorkflowExecutionTimedOut", True), ("ChildWorkflowExecutionTerminated", True)):
    _calls = head(more=[cinit(5), cinit(6, wid="cw-b")]) + ([[cstart(7, 5)], [ref(8, _t, 5)]] if _started
                                                            else [[ref(7, _t, 5)]])
    _last = 8 if _started else 7

    @case("child_removed_" + _t.replace("ChildWorkflowExecution", "").replace("StartFailed", "start_failed").lower(),
          _calls, Spec(end=(_last, _last), child=[child_row(6, 4, wid="cw-b")]))
    def _():
        """sb:373-406 -> DeletePendingChildExecution (msb:1138-1144): child 5 (started first,
        except for StartChildWorkflowExecutionFailed) leaves, child 6 stays as initiated."""


# ---- 5. request-cancel and signal of external workflows
@case("cancel_initiated", head(more=[rce(5)]), Spec(end=(4, 5), cancel=[cancel_row(5, 4)]))
def _():
    """msb:2577-2596: Version, InitiatedEventBatchID 4, InitiatedID 5; CancelRequestID = sb:410
    uuid.New() -> cdr_uuid site 3.  childWorkflowOnly unset, no control."""


@case("cancel_initiated_child_only",
      head() + [[dt_sched(5)], [dt_started(6, 5)], [dt_completed(7, 5, 6), rce(8, child_only=True, control="ctl")]],
      Spec(end=(7, 8), cancel=[cancel_row(8, 7)],
           exec=dict(last_processed_event=6, decision_original_scheduled_ts=NOW + 5)))
def _():
    """msb:2577-2596 behind a second decision: InitiatedEventBatchID 7.  childWorkflowOnly and
    control go to the transfer task only (sb:421-427), the row has neither.  The second
    decision: dtm:659-674 keeps DecisionTaskScheduled(5)'s timestamp, LastProcessedEvent 6."""


_TWO_CANCELS = head(more=[rce(5), rce(6, child_only=True, control="ctl")])


@case("cancel_failed", _TWO_CANCELS + [[ref(7, "RequestCancelExternalWorkflowExecutionFailed", 5)]],
      Spec(end=(7, 7), cancel=[cancel_row(6, 4)]))
def _():
    """sb:429-432 -> DeletePendingRequestCancel (msb:1147-1153): 5 leaves, 6 stays."""


@case("cancel_delivered", _TWO_CANCELS + [[ref(7, "ExternalWorkflowExecutionCancelRequested", 6)]],
      Spec(end=(7, 7), cancel=[cancel_row(5, 4)]))
def _():
    """sb:434-437 -> DeletePendingRequestCancel (msb:1147-1153): 6 leaves, 5 stays."""


@case("signal_initiated", head(more=[sig(5, "sig", input="in-1")]),
      Spec(end=(4, 5), signal=[signal_row(5, 4, "sig", "in-1", "")]))
def _():
    """msb:2701-2723: Version, InitiatedEventBatchID 4, InitiatedID 5, SignalName, Input; no
    control: nil.  SignalRequestID = sb:441 uuid.New() -> cdr_uuid site 4."""


@case("signal_initiated_child_only_control",
      head(more=[sig(5, "sig2", input=b"\x01\x02", control=b"ctl", child_only=True)]),
      Spec(end=(4, 5), signal=[signal_row(5, 4, "sig2", "b64:0102", "b64:63746c")]))
def _():
    """msb:2716-2717 with binary input and control (HistoryBuilder interns bytes as "b64:" +
    hex); childWorkflowOnly goes to the transfer task only (sb:452-458)."""


_TWO_SIGNALS = head(more=[sig(5, "sig", input="in-1"), sig(6, "sig2", control="c6", child_only=True)])


@case("signal_failed", _TWO_SIGNALS + [[ref(7, "SignalExternalWorkflowExecutionFailed", 5)]],
      Spec(end=(7, 7), signal=[signal_row(6, 4, "sig2", "", "c6")]))
def _():
    """sb:460-463 -> DeletePendingSignal (msb:1156-1162): 5 leaves, 6 (no input, a control) stays."""


@case("signal_delivered", _TWO_SIGNALS + [[ref(7, "ExternalWorkflowExecutionSignaled", 6)]],
      Spec(end=(7, 7), signal=[signal_row(5, 4, "sig", "in-1", "")]))
def _():
    """sb:465-468 -> DeletePendingSignal (msb:1156-1162): 6 leaves, 5 stays."""


# ---- 6. the workflow itself
@case("wf_signaled_twice", head(more=[ev(5, "WorkflowExecutionSignaled"), ev(6, "WorkflowExecutionSignaled")]),
      Spec(end=(4, 6), exec=dict(signal_count=2)))
def _():
    """msb:3082-3089: SignalCount++ per event."""


@case("wf_cancel_requested", head() + [[ev(5, "WorkflowExecutionCancelRequested")]],
      Spec(end=(5, 5), exec=dict(flags=xflags(XI_CANCEL))))
def _():
    """msb:2504-2510: CancelRequested = true; the workflow keeps running."""


def _closed(status, batch, **more):
    return dict(state=COMPLETED, close_status=status, completion_event_batch_id=batch, **more)


@case("close_completed", head(more=[ev(5, "WorkflowExecutionCompleted")]), Spec(end=(4, 5), exec=_closed(1, 4)))
def _():
    """msb:2379-2394: Completed / Completed (wei:83-91), CompletionEventBatchID = the call's
    first event 4 — not the close event's own id 5."""


@case("close_failed", head() + [[ev(5, "WorkflowExecutionFailed")]], Spec(end=(5, 5), exec=_closed(2, 5)))
def _():
    """msb:2419-2434: Completed / Failed; the close is alone in its call: batch id 5."""


@case("close_timed_out", head() + [[marker(5), ev(6, "WorkflowExecutionTimedOut")]],
      Spec(end=(5, 6), exec=_closed(6, 5)))
def _():
    """msb:2456-2471: Completed / TimedOut (6); batch id 5, the marker before it."""


@case("close_canceled",
      head() + [[ev(5, "WorkflowExecutionCancelRequested")], [dt_sched(6)], [dt_started(7, 6)],
                [dt_completed(8, 6, 7), ev(9, "WorkflowExecutionCanceled")]],
      Spec(end=(8, 9), exec=_closed(3, 8, last_processed_event=7, decision_original_scheduled_ts=NOW + 6,
                                    flags=xflags(XI_CANCEL))))
def _():
    """msb:2504-2510 then, a decision later, msb:2535-2549: Completed / Canceled (3), batch id
    8; CancelRequested stays set."""


@case("close_terminated_while_created", [[started(1), dt_sched(2)], [ev(3, "WorkflowExecutionTerminated")]],
      Spec(end=(3, 3), exec=_closed(4, 3, last_processed_event=EMPTY_ID, decision_version=1, decision_schedule_id=2,
                                    decision_timeout=10, decision_scheduled_ts=NOW + 2)))
def _():
    """msb:3047-3062 from Created (wei:65-71 accepts Terminated): Completed / Terminated (4),
    batch id 3.  The decision scheduled by event 2 is still pending (dtm:143-167: version 1,
    ScheduleID 2, timeout 10, attempt 0, both scheduled timestamps = event 2's) and
    LastProcessedEvent is still EmptyEventID (msb:1662)."""


# ---- 7. search attributes, reset points, parent, cron / memo / retry
@case("sa_start_and_upserts",
      head_with(searchAttributes={"indexedFields": {"sk1": "v1", "sk2": "v2"}})[:2] +
      [[dt_completed(4, 2, 3), upsert(5, {"sk2": "v2b", "sk3": "v3"}), upsert(6, {"sk1": "v1c"})]],
      Spec(end=(4, 6), sa=[("sk1", "v1c"), ("sk2", "v2b"), ("sk3", "v3")],
           exec=dict(search_attr_len=3, flags=xflags(XI_SA))))
def _():
    """msb:1710-1712 (two attributes on start) and msb:2746-2768 twice: the first upsert
    overwrites sk2 and adds sk3, the second overwrites sk1 (mergeMapOfByteArray: current[k] = v)."""


@case("sa_upsert_from_nil", head(more=[upsert(5, {"u1": "x"})]),
      Spec(end=(4, 5), sa=[("u1", "x")],
           exec=dict(search_attr_len=1, flags=xflags(XI_SA))))
def _():
    """msb:2761-2763: no search attributes on start, the upsert makes the map."""


_RP_IN = {"points": [
    {"binaryChecksum": "cks-a", "runId": "prev-run", "firstDecisionCompletedId": 4, "createdTimeNano": 111,
     "resettable": True},
    {"binaryChecksum": "cks-b", "runId": "older-run", "firstDecisionCompletedId": 9, "createdTimeNano": 222,
     "expiringTimeNano": 333, "resettable": False}]}


@case("reset_points_on_start", head_with(prevAutoResetPoints=_RP_IN, continuedExecutionRunId="prev-run"),
      Spec(end=(4, 4), rp=[rp_row("cks-a", "prev-run", 4, 111, NOW + 1 + DAY, RP_ALL | RP_RESETTABLE | RP_EXPIRING),
                           rp_row("cks-b", "older-run", 9, 222, 333, RP_ALL | RP_EXPIRING)],
           exec=dict(reset_points_len=2, flags=xflags(XI_RP))))
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
                     flags=xflags(XI_RP))))
def _():
    """dtm:789-800 -> msb:1798-1842: a new binary checksum appends a point (RunId = the
    workflow's, FirstDecisionCompletedId = the event's id, CreatedTimeNano = timeSource.Now(),
    resettable by CheckResettable msb:1845-1862).  The first is resettable; the second is added
    while a signal is pending: not resettable; the third decision repeats "cks-new": no point
    (msb:1814-1819)."""


_PARENT = dict(parentWorkflowDomain="pdom", parentWorkflowExecution={"workflowId": "pwid", "runId": "prun"},
               parentInitiatedEventId=17)


def _without(d, key):
    return {k: v for k, v in d.items() if k != key}


@case("parent_all", head_with(**_PARENT),
      Spec(end=(4, 4), exec=dict(parent_domain_id="id-of-pdom", parent_workflow_id="pwid", parent_run_id="prun",
                                 initiated_id=17)))
def _():
    """sb:160-167 (the domain cache's id for the parent domain), msb:1673-1684: all three parts."""


@case("parent_no_domain", head_with(**_without(_PARENT, "parentWorkflowDomain")),
      Spec(end=(4, 4), exec=dict(parent_workflow_id="pwid", parent_run_id="prun", initiated_id=17)))
def _():
    """msb:1673-1675: parentDomainID nil, ParentDomainID stays ""."""


@case("parent_no_execution", head_with(**_without(_PARENT, "parentWorkflowExecution")),
      Spec(end=(4, 4), exec=dict(parent_domain_id="id-of-pdom", initiated_id=17)))
def _():
    """msb:1676-1679: no ParentWorkflowExecution, both ids stay ""."""


@case("parent_no_initiated", head_with(**_without(_PARENT, "parentInitiatedEventId")),
      Spec(end=(4, 4), exec=dict(parent_domain_id="id-of-pdom", parent_workflow_id="pwid", parent_run_id="prun")))
def _():
    """msb:1680-1684: ParentInitiatedEventId nil -> InitiatedID = EmptyEventID."""


@case("wf_cron_memo",
      head_with(cronSchedule="*/5 * * * *", memo={"fields": {"m": "1"}}, taskList={"name": "other-tl"},
                workflowType={"name": "other-wt"}, executionStartToCloseTimeoutSeconds=250,
                taskStartToCloseTimeoutSeconds=7),
      Spec(end=(4, 4), exec=dict(cron_schedule="*/5 * * * *", memo="[('m', '1')]", task_list="other-tl",
                                 workflow_type="other-wt", workflow_timeout=250, decision_timeout_value=7,
                                 flags=xflags(XI_MEMO))))
def _():
    """msb:1651-1654, 1671, 1707-1709: task list, type, both timeouts, CronSchedule and Memo
    (HistoryBuilder interns a memo as repr(sorted(fields.items())))."""


@case("wf_retry_expiration_attempt",
      head_with(retryPolicy=dict(initialIntervalInSeconds=3, backoffCoefficient=2.5, maximumIntervalInSeconds=60,
                                 maximumAttempts=5, expirationIntervalInSeconds=600, nonRetriableErrorReasons=["x"]),
                expirationTimestamp=NOW + 600 * S, attempt=2),
      Spec(end=(4, 4), exec=dict(attempt=2, initial_interval=3, maximum_interval=60, backoff_coefficient=float.hex(2.5),
                                 maximum_attempts=5, expiration_seconds=600, expiration_time=NOW + 600 * S,
                                 nonretriable="x",
                                 flags=xflags(XI_RETRY | XI_EXPIRATION))))
def _():
    """msb:1686-1698: Attempt, ExpirationTime (from expirationTimestamp) and the six retry
    policy fields."""


@case("wf_other_domain_and_retention",
      head_with(prevAutoResetPoints={"points": [{"binaryChecksum": "cks-r", "runId": "prev-3"}]},
                continuedExecutionRunId="prev-3"),
      Spec(end=(4, 4), rp=[rp_row("cks-r", "prev-3", 0, 0, NOW + 1 + 3 * DAY, 0x1 | 0x2 | RP_EXPIRING)],
           exec=dict(domain_id="other-domain-id", reset_points_len=1,
                     flags=xflags(XI_RP))),
      domain_id="other-domain-id", retention_days=3)
def _():
    """msb:1648 (DomainID = the domain entry's) and msb:3195 with a retention of 3 days; the
    point carries a checksum and a run id only: the other fields stay unset."""


# ---- 8. decisions
@case("decision_scheduled_with_attempt", [[started(1), dt_sched(2, attempt=3)]],
      Spec(end=(1, 2), exec=dict(state=CREATED, last_processed_event=EMPTY_ID, decision_version=1,
                                 decision_schedule_id=2, decision_timeout=10, decision_attempt=3,
                                 decision_scheduled_ts=NOW + 2)))
def _():
    """dtm:143-167: Version, ScheduleID 2, StartedID EmptyEventID, RequestID emptyUUID, timeout
    10, Attempt from the event (3), both scheduled timestamps = the event's (sb:189-191).  The
    workflow is still Created (msb:1656-1661), LastProcessedEvent EmptyEventID (msb:1662)."""


@case("decision_started", [[started(1), dt_sched(2, attempt=3)], [dt_started(3, 2)]],
      Spec(end=(3, 3), exec=dict(last_processed_event=EMPTY_ID, decision_version=1, decision_schedule_id=2,
                                 decision_started_id=3, decision_request_id="r3", decision_timeout=10,
                                 decision_started_ts=NOW + 3, decision_scheduled_ts=NOW + 2)))
def _():
    """dtm:200-253: Running (dtm:228-235), StartedID 3, RequestID, StartedTimestamp = the
    event's, the scheduled timestamps kept — and Attempt forced to 0 although the schedule
    said 3 (dtm:224)."""


@case("decision_timed_out_schedule_to_start",
      [[started(1), dt_sched(2)],
       [ev(3, "DecisionTaskTimedOut", scheduledEventId=2, startedEventId=0, timeoutType="SCHEDULE_TO_START")]],
      Spec(end=(3, 3), exec=dict(state=CREATED, last_processed_event=EMPTY_ID, decision_original_scheduled_ts=0)))
def _():
    """dtm:269-279 with TimeoutTypeScheduleToStart: FailDecision(false) (dtm:635-656): every
    decision field reset, Attempt 0, ScheduledTimestamp 0, OriginalScheduledTimestamp 0; with
    DecisionAttempt 0 no transient decision follows (dtm:170-172)."""


def _transient(schedule_id, attempt, version=1):
    return dict(last_processed_event=EMPTY_ID, decision_version=By(EMPTY_V, version, version),
                decision_schedule_id=schedule_id, decision_timeout=10, decision_attempt=attempt,
                decision_scheduled_ts=BATCH_NOW, decision_original_scheduled_ts=0)


@case("decision_timed_out_start_to_close",
      [[started(1), dt_sched(2)], [dt_started(3, 2)],
       [ev(4, "DecisionTaskTimedOut", scheduledEventId=2, startedEventId=3, timeoutType="START_TO_CLOSE")]],
      Spec(end=(4, 4), exec=_transient(4, 1)))
def _():
    """dtm:269-279 -> FailDecision(true): Attempt 0 + 1, ScheduledTimestamp = Now; then sb:229 ->
    dtm:169-198 the transient decision: Version = GetCurrentVersion() (msb:491-502: EmptyVersion
    for a local builder, the event's version otherwise), ScheduleID = NextEventID — still 4, set
    by the previous call (sb:604) —, timeout = DecisionTimeoutValue 10, Attempt 1,
    ScheduledTimestamp = Now, OriginalScheduledTimestamp 0 (not set in dtm:184-194)."""


@case("decision_failed",
      [[started(1), dt_sched(2)], [dt_started(3, 2)],
       [ev(4, "DecisionTaskFailed", 11, scheduledEventId=2, startedEventId=3)]],
      Spec(end=(4, 4), exec=_transient(4, 1, 11), vh=[(3, 1), (4, 11)], repl=repl_state(11, 1, 11, 4)))
def _():
    """dtm:264-267 FailDecision(true), then the transient decision as for a start-to-close
    timeout (sb:241-257, dtm:169-198).  The failing event is the first of version 11: the
    prelude has already moved the current version (sb:137, 140 -> msb:473-475, before the
    version-history item is added), so the transient decision's Version is 11, not 1."""


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
                     branch_id_hi=lambda c: uuid(c.key, UUID_BRANCH, 3)[1])))
def _():
    """A second Started while the workflow is still Created (wei:58-63 accepts it) shows what
    msb:1639-1716 resets of a pending decision: exactly DecisionVersion, DecisionScheduleID,
    DecisionStartedID, DecisionRequestID and DecisionTimeout (msb:1665-1669) — DecisionAttempt 3
    and the two scheduled timestamps of DecisionTaskScheduled(2) survive.  The attributes are the
    second event's, but the first event's Memo stays — msb:1707-1709 writes it only when the event
    has one — while its reset point goes: msb:1700-1705 assigns AutoResetPoints always, here nil
    (msb:3191-3193).  sb:176 makes a new branch token (cdr_uuid at event 3) and sb:182-184 sets
    StartVersion to the second event's version 11."""


@case("marker_on_a_fresh_builder", [[marker(1, 11)]],
      Spec(end=(1, 1), vh=[(1, 11)], repl=repl_state(11, 1, 11, 1),
           exec=dict(domain_id="", workflow_id="", run_id="", create_request_id="", task_list="", workflow_type="",
                     branch_tree_id="", workflow_timeout=0, decision_timeout_value=0, initiated_id=0, branch_id_lo=0,
                     branch_id_hi=0, flags=0, state=CREATED, last_processed_event=EMPTY_ID,
                     decision_original_scheduled_ts=0)))
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
      Spec(end=(5, 5), version=11, exec=_transient(5, 2, 11)))
def _():
    """The transient decision of event 4 (attempt 1) times out: FailDecision(true) makes the
    attempt 2 (dtm:651-654) and the next transient decision sits at NextEventID 5 (dtm:186).
    All events carry version 11 (cluster 0's, meta:187-203): DecisionVersion 11 for 2DC / NDC."""


@case("decision_failed_beside_a_timer",
      [[started(1, 11), dt_sched(2, 11)], [dt_started(3, 2, 11)], [dt_completed(4, 2, 3, 11), tstart(5, "dft", 60, 11)],
       [dt_sched(6, 11), dt_started(7, 6, 11)],
       [ev(8, "DecisionTaskFailed", 11, scheduledEventId=6, startedEventId=7)]],
      Spec(end=(8, 8), version=11, timer=[timer_row("dft", 5, 60, 1, version=11)],
           exec=dict(_transient(8, 1, 11), last_processed_event=3)))
def _():
    """The transient decision (dtm:169-198) of a history that also starts a user timer — which
    keeps it off the fast-path kernel for every builder: the second decision (6, 7) fails, the
    transient one sits at NextEventID 8 (sb:604 of the previous call) with attempt 1, version 11
    for 2DC / NDC; LastProcessedEvent is the first decision's 3 (dtm:789-800), the failed one
    never completed."""


# ---- 9. versions
@case("xdc_second_cluster", head() + [[marker(5, 2), tstart(6, "x2", 60, 2)]],
      Spec(end=(5, 6), timer=[timer_row("x2", 6, 60, 1, version=2)], vh=[(4, 1), (6, 2)],
           repl=repl_state(2, 1, 2, 6, lri={1: (2, 6)})))
def _():
    """sb:134-138 with a call of version 2 — cluster 1's (2 % 10, meta:187-203), not the current
    one: CurrentVersion 2 (msb:548-556), LastWriteVersion 2 / LastWriteEventID 6 and
    LastReplicationInfo[cluster 1] = (2, 6) (msb:561-581); StartVersion stays the Started event's 1
    (sb:182-184).  NDC: a second item (vh:229-231).  The timer carries version 2."""


@case("xdc_third_then_second_cluster", head(3) + [[marker(5, 12)]],
      Spec(end=(5, 5), vh=[(4, 3), (5, 12)], repl=repl_state(12, 3, 12, 5, lri={2: (3, 4), 1: (12, 5)})))
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
           vh=[(4, 1), (6, 11), (10, 21)], repl=repl_state(21, 1, 21, 10)))
def _():
    """Versions 1, 11, 21 are all cluster 0's, the current one: no LastReplicationInfo
    (msb:570).  Each row takes its event's version (msb:1993, 2586, 2711, 2889, 3265) and the
    batch id of its call (7).  NDC: the version rises inside call 2 (events 5-6) and again at
    call 3: three items (vh:229-235)."""


# ---- 10. continue-as-new
@case("continue_as_new", head(more=[can(5)]),
      Spec(end=(4, 5), exec=_closed(5, 4), flags=APPLIED),
      new_run=[started(1, 11, cronSchedule="@daily", attempt=1), dt_sched(2, 11)], new_run_call=2,
      new_run_spec=Spec(end=(1, 2), version=11,
                        exec=dict(state=CREATED, last_processed_event=EMPTY_ID, cron_schedule="@daily", attempt=1,
                                  decision_version=11, decision_schedule_id=2, decision_timeout=10,
                                  decision_scheduled_ts=NOW + 2)))
def _():
    """sb:537-595.  The parent: msb:3207-3224 Completed / ContinuedAsNew (5), batch id 4; its
    result says the new run's history was applied.  The new run (sb:542-571): a fresh builder —
    NDC behind an NDC parent, 2DC otherwise —, the parent's domain and workflow id, the run id of
    the event's newExecutionRunId, its own request id and branch; Started(1) and
    DecisionTaskScheduled(2) of version 11 in one call leave it Created with decision 2 pending,
    ReplicationState all 11 (sb:137-138, 182-184) or one version-history item (2, 11)."""


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
                     flags=xflags(XI_SA | XI_RP))),
      sites=("dense",))
def _():
    """Every table populated by 12 events: msb:1700-1712 (a reset point of another run: no
    expiry added; a search attribute), msb:1982-2028 + 2083-2098 (activity 5 started by 11:
    timers 5 + 30 s / 11 + 20 s, startToClose leads, status 2 | 1), msb:2877-2900, 3256-3280,
    2577-2596, 2701-2723, 2746-2768, 3082-3089."""


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
                               heartbeat=NOW + 6 + 7 * S)])),
    CarryCase(
        "carry_child_row",
        """A loaded ChildExecutionInfo that is already started: run "cr-1", and a StartedID set by
        hand to 60, which no event of the history carries.  The one further event initiates another
        child (msb:3256-3280) and leaves the loaded row alone: every field of it, the started ones
        included, comes back as it went in (msb:272-295 Load), next to the new row of version 11 and
        batch 7.""",
        prefix=head(more=[cinit(5, wid="cw", domain="other", wtype="ct", pcp="TERMINATE")]) + [[cstart(6, 5, "cr-1", "cw")]],
        patch=("child", 0, dict(started_id=60)),
        suffix=[cinit(7, wid="cw-new", version=11)],
        spec=Spec(end=(7, 7), vh=[(6, 1), (7, 11)], repl=repl_state(11, 1, 11, 7),
                  child=[child_row(5, 4, started=60, run="cr-1", wid="cw", domain="other", wtype="ct", pcp=2),
                         child_row(7, 7, wid="cw-new", version=11)])),
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
    request-cancel (msb:2577-2596) and the signal (msb:2701-2723) of call 2 stay pending.""",
    calls=head(more=[asched(5, "qa"), tstart(6, "qt", 60), cinit(7), rce(8), sig(9)]) +
    [[at_close(10, 5), tend(11, "Fired", "qt", 6), ref(12, "StartChildWorkflowExecutionFailed", 7)]],
    spec=Spec(end=(10, 12), cancel=[cancel_row(8, 4)], signal=[signal_row(9, 4)]))
