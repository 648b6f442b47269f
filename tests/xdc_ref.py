"""TEST INFRASTRUCTURE: a plain-Python restatement of the 2DC replicator's admission decision
(historyReplicator.ApplyEvents, service/history/historyReplicator.go:339-763; H below) and of
one replication round, written from the reference independently of csrc/xdc_admit.h.

The round composes ``oracle.replay`` on the same reset and apply batches the device replays: the
reset prefix with its page calls on a fresh builder, the apply batch with carry onto the state.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle
from cadence_amd import abi, engine

A = {n: i for i, n in enumerate(abi.XDC_ACTIONS)}
R = {n: i for i, n in enumerate(abi.XDC_REASONS)}


class _Exit(Exception):
    pass


def _running(state):
    """IsWorkflowExecutionRunning (mutableStateBuilder.go:1422-1434); None where it panics"""
    if state in (abi.STATE_CREATED, abi.STATE_RUNNING):
        return True
    if state in (abi.STATE_COMPLETED, abi.STATE_ZOMBIE):
        return False
    return None


def _go_mod(a, b):
    """Go's (and C's) remainder: the sign of the dividend"""
    m = abs(a) % b
    return -m if a < 0 else m


def _cluster_of(m, v):
    """ClusterNameForFailoverVersion (common/cluster/metadata.go:187-203); None where it panics"""
    if v == abi.EMPTY_VERSION:
        return m.current_cluster
    init = _go_mod(v, m.failover_version_increment)
    for i in range(m.n_clusters):
        if m.initial_version[i] == init:
            return i
    return None


def _dec(**kw):
    d = dict(code=0, action=0, reason=0, via=0, reset_event_id=0, hint_next_event_id=0, hint_run=0, reapply_to=0,
             terminate_current_first=0, flags=0, cas_prev_is_self=0, cas_prev_state=0, cas_prev_last_write_version=0)
    d.update(kw)
    return d


def apply_other(d, t, state, next_event_id):
    """ApplyOtherEvents H:655-694 + ApplyReplicationTask H:704-707; d keeps its other fields"""
    d = dict(d)
    if t.first_event_id < next_event_id:  # H:664-671
        d.update(action=A["DROP"], reason=R["DUPLICATE"])
        return d
    run = _running(state)
    if run is None:
        d.update(action=A["DROP"], reason=R["E_WF_STATE"], code=36)
        return d
    if t.first_event_id > next_event_id:
        if not run:  # H:672-677
            d.update(action=A["DROP"], reason=R["CLOSED_AHEAD"])
        else:  # H:679-685
            d.update(action=A["RETRY"], reason=R["BUFFER"], hint_run=0, hint_next_event_id=next_event_id)
        return d
    if not run:  # H:704-707
        d.update(action=A["DROP"], reason=R["CLOSED"])
        return d
    d.update(action=A["APPLY"], reason=R["APPLY"])
    return d


def _reset(t, x_state, lwv, reason, reset_event_id):
    """resetMutableState H:1142-1189 with conflictResolutionTerminateCurrentRunningIfNotSelf H:925-999"""
    run = _running(x_state)
    if run is None:
        return _dec(reason=R["E_WF_STATE"], code=36)
    if run:  # H:938-947
        return _dec(action=A["RESET_APPLY"], reason=reason, via=abi.XDV_RESET, reset_event_id=reset_event_id,
                    cas_prev_is_self=1, cas_prev_last_write_version=lwv, cas_prev_state=x_state)
    if not t.flags & abi.XDC_CUR_PRESENT:  # H:953-960
        return _dec(reason=R["E_NO_CURRENT"], code=abi.E_BAD_INPUT)
    if t.version <= t.cur_last_write_version:  # H:972-975, 1170-1172
        return _dec(action=A["DROP"], reason=R["RESET_ABANDONED"], via=abi.XDV_RESET)
    self_ = 1 if t.flags & abi.XDC_CUR_IS_SELF else 0
    if t.cur_close_status != abi.CLOSE_NONE:  # H:977-982
        return _dec(action=A["RESET_APPLY"], reason=reason, via=abi.XDV_RESET, reset_event_id=reset_event_id,
                    cas_prev_is_self=self_, cas_prev_last_write_version=t.cur_last_write_version,
                    cas_prev_state=t.cur_state)
    return _dec(action=A["RESET_APPLY"], reason=reason, via=abi.XDV_RESET, reset_event_id=reset_event_id,  # H:984-998
                cas_prev_is_self=self_, cas_prev_last_write_version=t.cur_last_write_version,
                cas_prev_state=abi.STATE_COMPLETED, terminate_current_first=1,
                flags=abi.XDD_CAS_VERSION_FROM_TERMINATE)


def _checkpoint(t, rs):
    """getLatestCheckpoint H:1115-1140 in the order schema.h fixes: remote then local, ascending
    cluster index, a later entry wins only on a strictly greater version"""
    cv, ce = abi.EMPTY_VERSION, abi.EMPTY_EVENT_ID
    for mask, vers, ids in ((t.ri_mask, t.ri_version, t.ri_last_event_id),
                            (rs.lri_mask, rs.lri_version, rs.lri_last_event_id)):
        for i in range(abi.MAX_CLUSTERS):
            if mask >> i & 1 and (cv == abi.EMPTY_VERSION or vers[i] > cv):
                cv, ce = vers[i], ids[i]
    return cv, ce


def admit_one(t, r, x, rs, m) -> dict:
    """The decision for task t against the records (result r, exec x, repl rs), cluster metadata m."""
    if t.n_events == 0:  # H:377-381
        return _dec(action=A["DROP"], reason=R["EMPTY_TASK"])
    no_state = bool(t.flags & abi.XDC_NO_STATE)
    if not no_state and (r.code != abi.OK or not rs.present):
        return _dec(reason=R["E_STATE"], code=abi.E_BAD_INPUT)
    if t.first_event_type == abi.EV["WorkflowExecutionStarted"]:  # H:398-410
        if not no_state:
            return _dec(action=A["DROP"], reason=R["DUPLICATE_START"])
        return _dec(action=A["APPLY_FRESH"], reason=R["START"])
    if no_state:  # ApplyOtherEventsMissingMutableState H:451-519
        if not t.flags & abi.XDC_CUR_PRESENT:
            return _dec(action=A["RETRY"], reason=R["MISSING_NO_CURRENT"], hint_next_event_id=abi.FIRST_EVENT_ID)
        cur_running = bool(t.flags & abi.XDC_CUR_RUNNING)
        is_reset = bool(t.flags & abi.XDC_RESET_WORKFLOW)
        if t.cur_last_write_version > t.last_event_version:
            return _dec(action=A["REAPPLY"], reason=R["MISSING_STALE"], reapply_to=1)
        if t.cur_last_write_version < t.last_event_version:
            term = 1 if cur_running else 0
            if is_reset:
                return _dec(action=A["APPLY_RESET_EVENT"], reason=R["MISSING_NEWER_RESET"], terminate_current_first=term)
            return _dec(action=A["RETRY"], reason=R["MISSING_NEWER"], terminate_current_first=term,
                        hint_next_event_id=abi.FIRST_EVENT_ID)
        if cur_running:
            if t.last_event_task_id < t.cur_last_event_task_id:
                return _dec(action=A["DROP"], reason=R["MISSING_SAME_OLDER_TASK"])
            return _dec(action=A["RETRY"], reason=R["MISSING_SAME_RUNNING"], hint_run=1,
                        hint_next_event_id=t.cur_next_event_id)
        if is_reset:
            return _dec(action=A["APPLY_RESET_EVENT"], reason=R["MISSING_SAME_RESET"])
        return _dec(action=A["RETRY"], reason=R["MISSING_SAME_CLOSED"], hint_next_event_id=abi.FIRST_EVENT_ID)
    # ApplyOtherEventsVersionChecking H:521-653
    lwv = rs.last_write_version
    if lwv > t.version:
        run = _running(x.state)
        if run is None:
            return _dec(reason=R["E_WF_STATE"], code=36)
        if run:
            return _dec(action=A["REAPPLY"], reason=R["STALE_RUNNING"])
        if t.flags & abi.XDC_CUR_IS_SELF:
            return _dec(action=A["REAPPLY"], reason=R["STALE_SELF"])
        return _dec(action=A["REAPPLY"], reason=R["STALE_OTHER"], reapply_to=1)
    if lwv == t.version:
        return apply_other(_dec(via=abi.XDV_SAME_VERSION), t, x.state, x.next_event_id)
    prev = _cluster_of(m, lwv)
    if prev is None:
        return _dec(reason=R["E_CLUSTER"], code=abi.P_UNKNOWN_CLUSTER)
    if prev != m.current_cluster:
        if _go_mod(t.version - lwv, m.failover_version_increment) != 0:
            return _dec(reason=R["E_MORE_THAN_2DC"], code=abi.E_XDC_MORE_THAN_2DC)
        return apply_other(_dec(via=abi.XDV_SAME_CLUSTER), t, x.state, x.next_event_id)
    ri_ok = bool(t.ri_mask >> prev & 1)
    if not ri_ok or lwv > t.ri_version[prev]:
        cv, ce = _checkpoint(t, rs)
        if cv == abi.EMPTY_VERSION:
            return _dec(reason=R["E_MISSING_REPL_INFO"], code=abi.E_XDC_MISSING_REPL_INFO)
        return _reset(t, x.state, lwv, R["RESET_REJECTED"], ce)
    if lwv < t.ri_version[prev]:
        return _dec(reason=R["E_REMOTE_HIGHER_VERSION"], code=abi.E_XDC_REMOTE_HIGHER_VERSION)
    if t.ri_last_event_id[prev] > rs.last_write_event_id:
        return _dec(reason=R["E_CORRUPTED_REPL_INFO"], code=abi.E_XDC_CORRUPTED_REPL_INFO)
    if t.flags & abi.XDC_HAS_BUFFERED:  # flushEventsBuffer H:1211-1218
        run = _running(x.state)
        if run is None:
            return _dec(reason=R["E_WF_STATE"], code=36)
        if run:
            return _dec(action=A["FLUSH_BUFFER"], reason=R["FLUSH_BUFFER"])
    if t.ri_last_event_id[prev] < rs.last_write_event_id:
        return _reset(t, x.state, lwv, R["RESET_CONFLICT"], t.ri_last_event_id[prev])
    return apply_other(_dec(via=abi.XDV_EVENT_ID_MATCH), t, x.state, x.next_event_id)


def to_struct(d: dict) -> abi.CdrXdcDecision:
    s = abi.CdrXdcDecision()
    for k, v in d.items():
        setattr(s, k, v)
    return s


def admit(tasks, n, state: engine.Outputs, cluster):
    dec = (abi.CdrXdcDecision * max(1, n))()
    for w in range(n):
        dec[w] = to_struct(admit_one(tasks[w], state.result[w], state.exec[w], state.repl[w], cluster))
    return dec


def diff(a, b):
    """Fields in which two cdr_xdc_decision records differ"""
    return [f for f, _ in abi.CdrXdcDecision._fields_ if getattr(a, f) != getattr(b, f)]


# ----------------------------------------------------------------------------- the round
_OFF = {t: t + "_off" for t in engine.TABLES}
_CAP = {t: t + "_cap" for t in engine.TABLES}


def copy_state(src: engine.Outputs, dst: engine.Outputs, w: int):
    """Entry w of dst := entry w of src, rows at dst's capacities; a table that does not fit is
    left and the entry's code becomes CDR_E_BAD_INPUT (the round's state copy)."""
    r = src.result[w]
    C.memmove(C.byref(dst.exec[w]), C.byref(src.exec[w]), C.sizeof(abi.CdrExecInfo))
    C.memmove(C.byref(dst.repl[w]), C.byref(src.repl[w]), C.sizeof(abi.CdrReplState))
    C.memmove(C.byref(dst.result[w]), C.byref(r), C.sizeof(abi.CdrWfResult))
    if r.code != abi.OK:
        return
    ok = True
    for t in engine.TABLES:
        n = getattr(r, engine.TABLE_COUNT[t])
        sc, dc = src.plan.caps[w], dst.plan.caps[w]
        if n > getattr(dc, _CAP[t]):
            ok = False
            continue
        so, do = getattr(sc, _OFF[t]), getattr(dc, _OFF[t])
        sz = C.sizeof(engine.TABLE_TYPES[t])
        if n:
            C.memmove(C.addressof(dst.tables[t]) + do * sz, C.addressof(src.tables[t]) + so * sz, n * sz)
    if not ok:
        dst.result[w].code = abi.E_BAD_INPUT


def _not_run(out: engine.Outputs, w: int):
    out.result[w] = abi.CdrWfResult(code=abi.NOT_RUN)


def _take(full: engine.Outputs, out: engine.Outputs, w: int, tasks: bool):
    """Entry w of a whole-batch oracle replay into the masked output (same plan)"""
    copy_state(full, out, w)
    if full.result[w].code != abi.OK:  # a failed entry: the replay still wrote its records
        pass
    if tasks:
        c = full.plan.caps[w]
        for kind, off, idx in (("xfer", c.xfer_off, 0), ("ttask", c.ttask_off, 1)):
            k = full.tasks["n"][2 * w + idx]
            out.tasks["n"][2 * w + idx] = k
            for j in range(k):
                out.tasks[kind][off + j] = full.tasks[kind][off + j]


def round_(state: engine.Outputs, tasks, reset: engine.Batch, reset_plan, apply: engine.Batch, apply_plan, cluster,
           reset_tasks: bool = True):
    """One replication round on the host: `state` (Outputs laid out by the state plan) is updated
    in place; returns (decisions, reset Outputs, apply Outputs) as cdr_xdc_replicate_async leaves
    them in buffers that were zero before the call."""
    n = state.n_wfs
    dec = admit(tasks, n, state, cluster)
    reset_out = engine.Outputs(reset, reset_plan, tasks=reset_tasks)
    apply_out = engine.Outputs(apply, apply_plan)
    for w in range(n):
        _not_run(apply_out, w)
    # 2. conflictResolver.reset
    full = oracle.replay(reset, reset_plan, tasks=reset_tasks)
    do_apply = np.zeros(n, bool)
    for w in range(n):
        d = dec[w]
        if d.code != abi.OK:
            _not_run(reset_out, w)
            continue
        if d.action in (A["APPLY"], A["APPLY_FRESH"]):
            do_apply[w] = True
        if d.action != A["RESET_APPLY"]:
            _not_run(reset_out, w)
            continue
        _take(full, reset_out, w, reset_tasks)
        rr = reset_out.result[w]
        if rr.code != abi.OK:
            state.result[w] = rr
            d.action, d.reason, d.code = A["DROP"], R["E_RESET_REPLAY"], rr.code
            continue
        if reset_out.exec[w].next_event_id != d.reset_event_id + 1:
            state.result[w] = abi.CdrWfResult(code=abi.E_BAD_INPUT)
            d.action, d.reason, d.code = A["DROP"], R["E_RESET_PREFIX"], abi.E_BAD_INPUT
            continue
        x, old = reset_out.exec[w], state.exec[w]  # conflictResolver.go:141-142
        x.branch_tree_id, x.branch_id_lo, x.branch_id_hi = old.branch_tree_id, old.branch_id_lo, old.branch_id_hi
        x.flags = (x.flags & ~abi.XI_HAS_BRANCH) | (old.flags & abi.XI_HAS_BRANCH)
        copy_state(reset_out, state, w)
        if state.result[w].code != abi.OK:
            d.action, d.reason, d.code = A["DROP"], R["E_RESET_REPLAY"], state.result[w].code
            continue
        d.flags |= abi.XDD_RESET_RAN
        nd = apply_other({f: getattr(d, f) for f, _ in abi.CdrXdcDecision._fields_}, tasks[w], x.state, x.next_event_id)
        dec[w] = to_struct(nd)
        if nd["code"] == abi.OK and nd["action"] == A["APPLY"]:
            do_apply[w] = True
    # 3. ApplyReplicationTask: carry-in replay onto the loaded / reset state
    src = np.full(n, -1, np.int32)
    for w in range(n):
        if do_apply[w] and dec[w].action != A["APPLY_FRESH"]:
            src[w] = w
    ap = engine.Batch(events=apply.events, wfs=apply.wfs, kvs=apply.kvs, rps=apply.rps, cluster=apply.cluster,
                      now_ns=apply.now_ns, uuid_seed=apply.uuid_seed, empty_uuid=apply.empty_uuid,
                      strings=apply.strings, carry=engine.Carry(src=src, state=state))
    full = oracle.replay(ap, apply_plan)
    for w in range(n):
        if not do_apply[w]:
            continue
        _take(full, apply_out, w, False)
        if apply_out.result[w].code != abi.OK:
            state.result[w] = apply_out.result[w]
        else:
            copy_state(apply_out, state, w)
    return dec, reset_out, apply_out
