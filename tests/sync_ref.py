"""TEST INFRASTRUCTURE: historyReplicator.SyncActivity restated in plain Python over
engine.Outputs rows — the reference cdr_sync_activity_async is checked against (the role
tests/mutation_ref.py plays for the mutation).

Per request, in arrival order (service/history/historyReplicator.go:198-294): the exits, then
resetActivityTimerTaskStatus, ReplicateActivityInfo on the row (mutableStateBuilder.go:
1200-1231) and GetActivityTimerTaskIfNeeded over the workflow's rows (timerBuilder.go:211-230,
249-312, 384-408) with the project's tie rule: time, scheduleID, ScheduleToClose <
StartToClose / ScheduleToStart < Heartbeat.
"""
import ctypes as C

from cadence_amd import abi

SEC = 1_000_000_000


def last_write_version(state, w):
    """(builder kind, GetLastWriteVersion, mutableStateBuilder.go:526-545) of record w, the
    kind read from the records as schema.h cdr_sync_result says: 2DC when repl.present is set,
    else NDC when exec.flags has CDR_XI_VH_BRANCH or there are version-history items, else
    local.  None where the reference's call fails (NDC without items)."""
    r, cp = state.result[w], state.plan.caps[w]
    if state.repl[w].present:
        return abi.BUILDER_2DC, state.repl[w].last_write_version
    if (state.exec[w].flags & abi.XI_VH_BRANCH) or r.n_vh:
        n = min(r.n_vh, cp.vh_cap)
        if n == 0:
            return abi.BUILDER_NDC, None
        return abi.BUILDER_NDC, state.tables["vh"][cp.vh_off + n - 1].version
    return abi.BUILDER_LOCAL, abi.EMPTY_VERSION


_BIT = {abi.TIMEOUT_START_TO_CLOSE: abi.TTS_START_TO_CLOSE, abi.TIMEOUT_SCHEDULE_TO_START: abi.TTS_SCHEDULE_TO_START,
        abi.TIMEOUT_SCHEDULE_TO_CLOSE: abi.TTS_SCHEDULE_TO_CLOSE, abi.TIMEOUT_HEARTBEAT: abi.TTS_HEARTBEAT}


def _i64(x):
    """Wrap to int64 as Go's arithmetic does."""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def _go_mod(a, b):
    """Go's (and C's) %: the sign of the dividend."""
    m = abs(a) % abs(b)
    return -m if a < 0 else m


def candidates(a):
    """loadActivityTimers' timers of one row: (time, scheduleID, order, timeout type)."""
    if a.schedule_id == abi.EMPTY_EVENT_ID:
        return []
    s2c = _i64(a.scheduled_time + a.s2c * SEC)
    if a.expiration_time < s2c:
        s2c = a.expiration_time
    out = [(s2c, a.schedule_id, 0, abi.TIMEOUT_SCHEDULE_TO_CLOSE)]
    if a.started_id != abi.EMPTY_EVENT_ID:
        st = a.started_time if a.flags & abi.AI_STARTED_TIME_SET else 0
        out.append((_i64(st + a.stc * SEC), a.schedule_id, 1, abi.TIMEOUT_START_TO_CLOSE))
        if a.hb > 0:
            lhb = a.last_heartbeat_time if a.flags & abi.AI_STARTED_TIME_SET else 0
            out.append((_i64(max(lhb, st) + a.hb * SEC), a.schedule_id, 2, abi.TIMEOUT_HEARTBEAT))
    else:
        out.append((_i64(a.scheduled_time + a.s2s * SEC), a.schedule_id, 1, abi.TIMEOUT_SCHEDULE_TO_START))
    return out


def pick(rows):
    """GetActivityTimerTaskIfNeeded over `rows` (modified in place): None when there is no
    timer or the head's task exists already, else (row index, time, timeout type) of the new
    task, whose bit is set on its row."""
    cands = [(c, j) for j, a in enumerate(rows) for c in candidates(a)]
    if not cands:
        return None
    (t, _, _, ty), j = min(cands)
    if rows[j].timer_task_status & _BIT[ty]:
        return None
    rows[j].timer_task_status |= _BIT[ty]
    return j, t, ty


def _result(q, action, code=abi.OK, nxt=0, lwv=0):
    r = abi.CdrSyncResult(action=action, code=code, next_event_id=nxt, last_write_version=lwv,
                          act_row=abi.SYNC_NO_ROW, task_row=abi.SYNC_NO_ROW, tag=q.tag)
    return r


def sync_one(state, q, increment):
    """One request against `state` (act rows updated in place); returns its cdr_sync_result."""
    w = q.wf
    if w < 0:
        return _result(q, abi.SYNC_SKIP_NO_WORKFLOW)
    if w >= state.n_wfs or state.result[w].code != abi.OK:
        return _result(q, abi.SYNC_E_STATE)
    x = state.exec[w]
    kind, lwv = last_write_version(state, w)
    nxt = x.next_event_id
    lw = abi.EMPTY_VERSION if lwv is None else lwv
    if x.state in (abi.STATE_COMPLETED, abi.STATE_ZOMBIE):
        return _result(q, abi.SYNC_SKIP_NOT_RUNNING, nxt=nxt, lwv=lw)
    if x.state not in (abi.STATE_CREATED, abi.STATE_RUNNING):
        return _result(q, abi.SYNC_SKIP_NOT_RUNNING, abi.P_UNKNOWN_WF_STATE, nxt, lw)
    if q.scheduled_id >= nxt:
        if lwv is None:
            return _result(q, abi.SYNC_SKIP_STALE_VERSION, abi.E_VH_EMPTY, nxt, lw)
        if q.version < lwv:
            return _result(q, abi.SYNC_SKIP_STALE_VERSION, nxt=nxt, lwv=lw)
        return _result(q, abi.SYNC_RETRY_2DC if kind == abi.BUILDER_2DC else abi.SYNC_RETRY_NDC, nxt=nxt, lwv=lw)
    off = state.plan.caps[w].act_off
    n = min(state.result[w].n_activity, state.plan.caps[w].act_cap)
    rows = [state.tables["act"][off + j] for j in range(n)]  # references into the table
    hit = [j for j, a in enumerate(rows) if a.schedule_id == q.scheduled_id]
    if not hit:
        return _result(q, abi.SYNC_SKIP_NO_ACTIVITY, nxt=nxt, lwv=lw)
    j = hit[0]
    a = rows[j]
    if a.version > q.version:
        return _result(q, abi.SYNC_SKIP_LOCAL_VERSION_LARGER, nxt=nxt, lwv=lw)
    if a.version == q.version:
        if a.attempt > q.attempt:
            return _result(q, abi.SYNC_SKIP_LOCAL_ATTEMPT_LARGER, nxt=nxt, lwv=lw)
        hb_set = a.flags & (abi.AI_STARTED_TIME_SET | abi.AI_HEARTBEAT_TIME_SET)
        if a.attempt == q.attempt and hb_set and a.last_heartbeat_time > q.last_heartbeat_time:
            return _result(q, abi.SYNC_SKIP_HEARTBEAT_OLDER, nxt=nxt, lwv=lw)
    reset = _go_mod(_i64(q.version - a.version), increment) != 0 or a.attempt < q.attempt
    started = q.started_id != abi.EMPTY_EVENT_ID
    a.version = q.version
    a.scheduled_time = q.scheduled_time
    a.started_id = q.started_id
    a.last_heartbeat_time = q.last_heartbeat_time
    a.started_time = q.started_time if started else 0
    a.attempt = q.attempt
    a.flags = (a.flags & ~abi.AI_STARTED_TIME_SET) | abi.AI_HEARTBEAT_TIME_SET | (
        abi.AI_STARTED_TIME_SET if started else 0)
    if reset:
        a.timer_task_status = 0
    r = _result(q, abi.SYNC_APPLIED, nxt=nxt, lwv=lw)
    r.flags = abi.SYNC_RESET_TIMER_STATUS if reset else 0
    r.event_time = max(q.scheduled_time, q.started_time, q.last_heartbeat_time)
    r.act_row = off + j
    head = pick(rows)
    if head is not None:
        k, t, ty = head
        r.flags |= abi.SYNC_HAS_TIMER_TASK
        r.task_row = off + k
        r.timer_task = abi.CdrTask(type=abi.TT_ACTIVITY_TIMEOUT, timeout_type=ty, event_id=rows[k].schedule_id,
                                   visibility_ts=t, attempt=rows[k].attempt)
    return r


def sync(state, reqs, increment=10):
    """Every request of `reqs` in order; `state`'s act table is updated in place."""
    return [sync_one(state, q, increment) for q in reqs]


def copy_state(state):
    """A copy of an Outputs that shares nothing the sync path writes (the act table)."""
    import copy
    st = copy.copy(state)
    st.tables = dict(state.tables)
    act = type(state.tables["act"])()
    C.memmove(act, state.tables["act"], C.sizeof(act))
    st.tables["act"] = act
    return st


def rbytes(x) -> bytes:
    return bytes(memoryview(x).cast("B"))
