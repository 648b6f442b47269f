"""TEST INFRASTRUCTURE: the standby task processors restated in plain Python over
engine.Outputs rows — the reference cdr_standby_tasks_async is checked against (the role
tests/sync_ref.py plays for SyncActivity).

Per request, in arrival order: timerQueueStandbyProcessorImpl.process
(service/history/timerQueueStandbyProcessor.go:173-626) or
transferQueueStandbyProcessorImpl.process (transferQueueStandbyProcessor.go:137-660) with the
loads and verifyTaskVersion of xdcUtil.go:70-169.  The activity timer pick is sync_ref's.
"""
from cadence_amd import abi
from tests import sync_ref

SEC = 1_000_000_000
_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1
_i64 = sync_ref._i64
rbytes = sync_ref.rbytes
last_write_version = sync_ref.last_write_version


def unix(ns):
    """time.Time.Unix(): whole seconds, floored (Python's // floors)."""
    return ns // SEC


def time_sub(now, t):
    """time.Time.Sub: the difference, saturating."""
    return max(_I64_MIN, min(_I64_MAX, now - t))


def start_version(state, w):
    """GetStartVersion (mutableStateBuilder.go:504-524); None where it fails."""
    r, cp = state.result[w], state.plan.caps[w]
    if state.repl[w].present:
        return state.repl[w].start_version
    if (state.exec[w].flags & abi.XI_VH_BRANCH) or r.n_vh:
        if min(r.n_vh, cp.vh_cap) == 0:
            return None
        return state.tables["vh"][cp.vh_off].version
    return abi.EMPTY_VERSION


def _rows(state, w, table, count):
    cp = state.plan.caps[w]
    off = getattr(cp, table + "_off")
    n = min(getattr(state.result[w], count), getattr(cp, table + "_cap"))
    return off, [state.tables[table][off + j] for j in range(n)]  # references into the table


def _result(q, action, reason, code=abi.OK, nxt=0, lwv=0):
    return abi.CdrStandbyResult(action=action, reason=reason, code=code, next_event_id=nxt, last_write_version=lwv,
                                act_row=abi.SB_NO_ROW, task_row=abi.SB_NO_ROW, tag=q.tag)


def _stateless(t):
    """The types process() answers before it loads a state: (action, reason) or None."""
    if t.type == abi.TT_ACTIVITY_RETRY_TIMER:
        return abi.SB_DONE, abi.SBR_RETRY_TIMER
    if t.type == abi.TT_RESET_WORKFLOW:
        return abi.SB_DONE, abi.SBR_RESET_WORKFLOW
    if t.type == abi.TT_DECISION_TIMEOUT and t.timeout_type == abi.TIMEOUT_SCHEDULE_TO_START:
        return abi.SB_DONE, abi.SBR_DECISION_S2S
    if t.type == abi.TT_DELETE_HISTORY:
        return abi.SB_HOST, abi.SBR_DELETE_HISTORY
    if abi.TT_UPSERT_SA < t.type < abi.TT_DECISION_TIMEOUT:
        return abi.SB_E_TASK_TYPE, abi.SBR_UNKNOWN_TRANSFER
    if t.type > abi.TT_WORKFLOW_BACKOFF:
        return abi.SB_E_TASK_TYPE, abi.SBR_UNKNOWN_TIMER
    return None


def verify_one(state, q, now, delay):
    """One request against `state` (act rows updated in place); returns its cdr_standby_result."""
    w, t = q.wf, q.task
    if w >= state.n_wfs or (w >= 0 and state.result[w].code != abi.OK):
        return _result(q, abi.SB_E_STATE, abi.SBR_BAD_STATE)
    early = _stateless(t)
    if early:
        return _result(q, *early)
    if w < 0:
        return _result(q, abi.SB_DONE, abi.SBR_NO_WORKFLOW)
    x = state.exec[w]
    _, lwv = last_write_version(state, w)
    nxt, lw = x.next_event_id, abi.EMPTY_VERSION if lwv is None else lwv

    def res(action, reason, code=abi.OK):
        return _result(q, action, reason, code, nxt, lw)
    dec_retry = (t.type in (abi.TT_DECISION_TIMEOUT, abi.TT_DECISION) and x.decision_schedule_id == t.event_id
                 and x.decision_attempt > 0)
    if t.event_id >= nxt and not dec_retry:
        return res(abi.SB_DONE, abi.SBR_STALE_EVENT_ID)
    running = x.state in (abi.STATE_CREATED, abi.STATE_RUNNING)
    if not running and x.state not in (abi.STATE_COMPLETED, abi.STATE_ZOMBIE):
        return res(abi.SB_E_STATE, abi.SBR_E_WF_STATE, abi.P_UNKNOWN_WF_STATE)
    if not running and t.type != abi.TT_CLOSE_EXECUTION:
        return res(abi.SB_DONE, abi.SBR_NOT_RUNNING)
    discard = time_sub(now, t.visibility_ts) > _i64(3 * delay)
    pending = abi.SB_RETRY if not discard else (
        abi.SB_DISCARDED if q.flags & abi.SBT_LAST_ATTEMPT else abi.SB_FETCH)
    push = time_sub(now, t.visibility_ts) > delay

    def verified(version):
        return not (q.flags & abi.SBT_GLOBAL_DOMAIN) or version == t.version

    def lookup(table, count, key, gone, bad_version):
        _, rows = _rows(state, w, table, count)
        hit = [r for r in rows if getattr(r, key) == t.event_id]
        if not hit:
            return None, res(abi.SB_DONE, gone)
        if not verified(hit[0].version):
            return None, res(abi.SB_DONE, bad_version)
        return hit[0], None

    if t.type == abi.TT_USER_TIMER:
        _, rows = _rows(state, w, "timer", "n_timer")
        if rows and unix(min(r.expiry_time for r in rows)) <= unix(t.visibility_ts):
            return res(pending, abi.SBR_USER_TIMER_PENDING)
        return res(abi.SB_DONE, abi.SBR_USER_TIMER_NONE)
    if t.type == abi.TT_ACTIVITY_TIMEOUT:
        off, rows = _rows(state, w, "act", "n_activity")
        cands = [c for a in rows for c in sync_ref.candidates(a)]
        if cands and unix(min(cands)[0]) <= unix(t.visibility_ts):
            return res(pending, abi.SBR_ACT_TIMER_PENDING)
        if lwv is None:
            return res(abi.SB_E_STATE, abi.SBR_E_LAST_WRITE_VERSION, abi.E_VH_EMPTY)
        r = res(abi.SB_UPDATED, abi.SBR_ACT_TIMER_UPDATED)
        hit = [j for j, a in enumerate(rows) if a.schedule_id == t.event_id]
        if t.timeout_type == abi.TIMEOUT_HEARTBEAT and hit:
            rows[hit[0]].timer_task_status &= ~abi.TTS_HEARTBEAT
            r.flags |= abi.SB_STATE_UPDATED
            r.act_row = off + hit[0]
        head = sync_ref.pick(rows)
        if head is not None:
            k, ts, ty = head
            r.flags |= abi.SB_HAS_TIMER_TASK
            r.task_row = off + k
            r.timer_task = abi.CdrTask(type=abi.TT_ACTIVITY_TIMEOUT, timeout_type=ty, event_id=rows[k].schedule_id,
                                       visibility_ts=ts, attempt=rows[k].attempt)
        return r if r.flags else res(abi.SB_DONE, abi.SBR_ACT_TIMER_NO_UPDATE)
    if t.type == abi.TT_DECISION_TIMEOUT:
        if x.decision_schedule_id != t.event_id:
            return res(abi.SB_DONE, abi.SBR_DECISION_GONE)
        if not verified(x.decision_version):
            return res(abi.SB_DONE, abi.SBR_DECISION_VERSION)
        return res(pending, abi.SBR_DECISION_PENDING)
    if t.type == abi.TT_WORKFLOW_BACKOFF:
        if x.decision_schedule_id != abi.EMPTY_EVENT_ID or x.last_processed_event != abi.EMPTY_EVENT_ID:
            return res(abi.SB_DONE, abi.SBR_BACKOFF_DECIDED)
        return res(pending, abi.SBR_BACKOFF_PENDING)
    if t.type in (abi.TT_WORKFLOW_TIMEOUT, abi.TT_RECORD_STARTED):
        sv = start_version(state, w)
        timeout = t.type == abi.TT_WORKFLOW_TIMEOUT
        if sv is None:
            return res(abi.SB_E_STATE, abi.SBR_E_START_VERSION, abi.E_VH_EMPTY)
        if not verified(sv):
            return res(abi.SB_DONE, abi.SBR_WF_TIMEOUT_VERSION if timeout else abi.SBR_STARTED_VERSION)
        if timeout:
            return res(pending, abi.SBR_WF_TIMEOUT_PENDING)
        return res(abi.SB_RECORD_STARTED, abi.SBR_STARTED_RECORD)
    if t.type == abi.TT_ACTIVITY:
        a, out = lookup("act", "n_activity", "schedule_id", abi.SBR_XACT_GONE, abi.SBR_XACT_VERSION)
        if out:
            return out
        if a.started_id != abi.EMPTY_EVENT_ID:
            return res(abi.SB_DONE, abi.SBR_XACT_STARTED)
        r = res(abi.SB_PUSH_ACTIVITY if push else abi.SB_RETRY, abi.SBR_XACT_PENDING)
        if push:
            r.push_timeout_s, r.task_list = min(a.s2s, abi.MAX_TASK_TIMEOUT), t.task_list
        return r
    if t.type == abi.TT_DECISION:
        if x.decision_schedule_id != t.event_id:
            return res(abi.SB_DONE, abi.SBR_XDEC_GONE)
        if not verified(x.decision_version):
            return res(abi.SB_DONE, abi.SBR_XDEC_VERSION)
        if x.decision_started_id != abi.EMPTY_EVENT_ID:
            return res(abi.SB_DONE, abi.SBR_XDEC_STARTED)
        r = res(abi.SB_PUSH_DECISION if push else abi.SB_RETRY, abi.SBR_XDEC_PENDING)
        if push:
            r.push_timeout_s, r.task_list = min(x.workflow_timeout, abi.MAX_TASK_TIMEOUT), t.task_list
        return r
    if t.type == abi.TT_CLOSE_EXECUTION:
        if running:
            return res(abi.SB_DONE, abi.SBR_CLOSE_RUNNING)
        if lwv is None:
            return res(abi.SB_E_STATE, abi.SBR_E_LAST_WRITE_VERSION, abi.E_VH_EMPTY)
        if not verified(lwv):
            return res(abi.SB_DONE, abi.SBR_CLOSE_VERSION)
        return res(abi.SB_RECORD_CLOSED, abi.SBR_CLOSE_RECORD)
    if t.type == abi.TT_CANCEL_EXECUTION:
        _, out = lookup("cancel", "n_cancel", "initiated_id", abi.SBR_CANCEL_GONE, abi.SBR_CANCEL_VERSION)
        return out or res(pending, abi.SBR_CANCEL_PENDING)
    if t.type == abi.TT_SIGNAL_EXECUTION:
        _, out = lookup("signal", "n_signal", "initiated_id", abi.SBR_SIGNAL_GONE, abi.SBR_SIGNAL_VERSION)
        return out or res(pending, abi.SBR_SIGNAL_PENDING)
    if t.type == abi.TT_START_CHILD:
        c, out = lookup("child", "n_child", "initiated_id", abi.SBR_CHILD_GONE, abi.SBR_CHILD_VERSION)
        if out:
            return out
        if c.started_id != abi.EMPTY_EVENT_ID:
            return res(abi.SB_DONE, abi.SBR_CHILD_STARTED)
        return res(pending, abi.SBR_CHILD_PENDING)
    assert t.type == abi.TT_UPSERT_SA, t.type
    return res(abi.SB_UPSERT, abi.SBR_UPSERT_RECORD)


def verify(state, reqs, now, delay):
    """Every request of `reqs` in order; `state`'s act table is updated in place."""
    return [verify_one(state, q, now, delay) for q in reqs]


copy_state = sync_ref.copy_state
