"""2DC replication over batches of workflows — historyReplicator.ApplyEvents
(service/history/historyReplicator.go:339-763), the replication path while EnableNDC is off,
for one replication task per workflow per round.

``admit_host`` / ``admit`` take the admission decision alone (``cdr_xdc_admit_host`` on host
records, ``cdr_xdc_admit_async`` on the device): drop, apply, apply on a fresh builder, reset to
the last common checkpoint and apply, or hand the task back to the caller (reapply, retry,
flush the buffer, apply a reset event).  ``DeviceReplicator`` drives whole rounds behind
``cdr_xdc_replicate_async``: admit, conflictResolver.reset of the workflows that need it
(conflictResolver.go:66-184, the replay kernels with the other workflows masked), the event-id
check against the reset state, the apply replay onto the loaded or reset states, and the
adoption of the applied states — on the device, with no host round trip and no allocation.

This module is plumbing: records, planning, packing and device buffers.  The CPU restatement
lives with the tests (tests/xdc_ref.py).
"""
from __future__ import annotations

import ctypes as C

from . import abi, engine, ndc

PAGE_SIZE = 1000  # defaultHistoryPageSize (conflictResolver.go:94-133 reads the prefix in pages)


def new_tasks(n: int):
    return (abi.CdrXdcTask * max(1, n))()


def new_decisions(n: int, fill: int = 0):
    dec = (abi.CdrXdcDecision * max(1, n))()
    if fill:
        C.memset(dec, fill, C.sizeof(dec))
    return dec


def fill_task(t, *, version, first_event_id=1, next_event_id=None, n_events=1, first_event_type=None,
              last_event_version=None, last_event_task_id=0, flags=0, replication_info=None, cur=None):
    """One cdr_xdc_task.  replication_info: {cluster index: (version, last_event_id)};
    cur: the current run's summary as a dict (last_write_version, last_event_task_id,
    next_event_id, state, close_status, is_self, running) — sets CDR_XDC_CUR_*."""
    t.version = version
    t.first_event_id = first_event_id
    t.next_event_id = first_event_id + n_events if next_event_id is None else next_event_id
    t.n_events = n_events
    t.first_event_type = abi.EV["DecisionTaskScheduled"] if first_event_type is None else first_event_type
    t.last_event_version = version if last_event_version is None else last_event_version
    t.last_event_task_id = last_event_task_id
    t.ri_mask = 0
    for c, (v, e) in (replication_info or {}).items():
        t.ri_mask |= 1 << c
        t.ri_version[c], t.ri_last_event_id[c] = v, e
    if cur is not None:
        flags |= abi.XDC_CUR_PRESENT
        flags |= abi.XDC_CUR_IS_SELF if cur.get("is_self") else 0
        flags |= abi.XDC_CUR_RUNNING if cur.get("running") else 0
        t.cur_last_write_version = cur.get("last_write_version", 0)
        t.cur_last_event_task_id = cur.get("last_event_task_id", 0)
        t.cur_next_event_id = cur.get("next_event_id", 0)
        t.cur_state = cur.get("state", abi.STATE_RUNNING if cur.get("running") else abi.STATE_COMPLETED)
        t.cur_close_status = cur.get("close_status", abi.CLOSE_NONE if cur.get("running") else abi.CLOSE_COMPLETED)
    t.flags = flags
    return t


def task_from_entry(t, batch: engine.Batch, w: int, **kw):
    """The request fields of a task whose events are entry w of `batch`."""
    d = batch.wfs[w]
    first, last = batch.events[d.ev_off], batch.events[d.ev_off + d.ev_len - 1]
    return fill_task(t, version=kw.pop("version", last.version), first_event_id=first.event_id,
                     next_event_id=last.event_id + 1, n_events=d.ev_len, first_event_type=first.type,
                     last_event_version=last.version, last_event_task_id=last.task_id, **kw)


def _stream(stream):
    return stream if isinstance(stream, C.c_void_p) else C.c_void_p(stream)


def _check_cluster(cluster):
    return cluster if cluster is not None else engine.default_cluster()


def admit_host(tasks, n: int, state: engine.Outputs, cluster=None):
    """cdr_xdc_admit_host: decisions of tasks[0..n) against the host records of `state`."""
    dec = new_decisions(n)
    rc = abi.lib().cdr_xdc_admit_host(C.addressof(tasks), n, C.addressof(state.plan.caps), C.byref(state.cstruct()),
                                      C.byref(_check_cluster(cluster)), C.addressof(dec))
    if rc:
        raise RuntimeError(f"cdr_xdc_admit_host rc={rc}")
    return dec


def admit(eng: engine.Engine, tasks, n: int, state: engine.Outputs, cluster=None, fill: int = 0):
    """cdr_xdc_admit_async (k_xdc_admit): the same decisions on the device; the decision buffer
    is pre-filled with `fill`."""
    dev = ndc._Dev()
    try:
        o = abi.CdrOut()
        o.result, o.exec, o.repl = dev.up(state.result), dev.up(state.exec), dev.up(state.repl)
        dec = new_decisions(n, fill)
        pd = dev.up(dec)
        rc = abi.lib().cdr_xdc_admit_async(eng.ctx, C.c_void_p(dev.up(tasks)), n, None, C.byref(o),
                                           C.byref(_check_cluster(cluster)), C.c_void_p(pd), None)
        if rc:
            raise RuntimeError(f"cdr_xdc_admit_async rc={rc}")
        dev.down(dec, pd)
        return dec
    finally:
        dev.close()


def paged(batch: engine.Batch, page: int = PAGE_SIZE) -> engine.Batch:
    """`batch` with its applyEvents calls re-cut as conflictResolver.reset makes them: one call
    per page of `page` events from the entry's first (conflictResolver.go:94-133).  The events
    are copied; the entries must not be continue-as-new links."""
    ev = (abi.CdrEvent * max(1, len(batch.events)))()
    if len(batch.events):
        C.memmove(ev, batch.events, C.sizeof(abi.CdrEvent) * len(batch.events))
    for w in range(batch.n_wfs):
        d = batch.wfs[w]
        for k in range(d.ev_len):
            e = ev[d.ev_off + k]
            e.flags = (e.flags & ~abi.EVF_BATCH_FIRST) | (abi.EVF_BATCH_FIRST if k % page == 0 else 0)
    ev = (abi.CdrEvent * len(batch.events)).from_buffer(ev) if len(batch.events) else (abi.CdrEvent * 0)()
    return engine.Batch(events=ev, wfs=batch.wfs, kvs=batch.kvs, rps=batch.rps, cluster=batch.cluster,
                        now_ns=batch.now_ns, uuid_seed=batch.uuid_seed, empty_uuid=batch.empty_uuid,
                        strings=batch.strings)


def state_caps_for(base: engine.Batch, rounds, live_sum: bool = False) -> engine.Plan:
    """Per-workflow capacities of the state buffer a replication run keeps: room for the largest
    state any round can leave — the base's rows, or a reset prefix's, plus every apply batch's new
    rows (ndc.state_caps_for's bound, with every round's reset batch counted).  rounds:
    [(reset batch, apply batch, tasks)]."""
    parts = [(b, None, None) for r, a, _ in rounds for b in (r, a)]
    return ndc.state_caps_for(base, parts[0][0], parts[1:], live_sum) if parts else engine.plan(base)


def plan_apply(apply: engine.Batch, bound_caps) -> engine.Plan:
    """cdr_plan_ndc_apply: an apply batch's capacities for loaded states within bound_caps."""
    caps = (abi.CdrWfCaps * max(1, apply.n_wfs))()
    tot = abi.CdrTotals()
    rc = abi.lib().cdr_plan_ndc_apply(C.byref(apply.cstruct()), bound_caps, caps, C.byref(tot))
    if rc:
        raise RuntimeError(f"cdr_plan_ndc_apply rc={rc}")
    return engine.Plan(caps=caps, totals=tot)


class DeviceReplicator:
    """The device-resident 2DC replication run over a batch of workflows: the base histories
    replayed into the state buffer (or a state uploaded as it is), then one
    cdr_xdc_replicate_async call per round, with every buffer allocated up front.
    rounds: [(reset batch, apply batch, tasks)], entry w of each = workflow w."""

    def __init__(self, eng: engine.Engine, base: engine.Batch, rounds, cluster=None, state_plan=None,
                 reset_tasks: bool = True):
        n = base.n_wfs
        self.eng, self.n, self.dev = eng, n, ndc._Dev()
        dev = self.dev
        self.cluster = _check_cluster(cluster)
        self.state_plan = state_plan or state_caps_for(base, rounds)
        live_bound = state_caps_for(base, rounds, live_sum=True).caps
        self.base_db = ndc.upload_batch(dev, base, self.state_plan.caps, cls=True)
        self.state = ndc.alloc_out(dev, n, self.state_plan.totals)
        self.state_caps_d = dev.up(self.state_plan.caps)
        self.reset_tasks = reset_tasks
        self.rounds = []
        for reset, apply, tasks in rounds:
            rp = engine.plan(reset)
            ap = plan_apply(apply, live_bound)
            r = abi.CdrXdcRound()
            r.tasks = dev.up(tasks)
            # task lists need a plan without wave slices (cdr_replay_sliced_async)
            r.reset = ndc.upload_batch(dev, reset, rp.caps, 0 if reset_tasks else abi.PLAN_WAVE | abi.PLAN_PAR)
            r.reset_out = ndc.alloc_out(dev, n, rp.totals, tasks=reset_tasks)
            r.apply = ndc.upload_batch(dev, apply, ap.caps, 0)
            r.apply_out = ndc.alloc_out(dev, n, ap.totals)
            r.dec = dev.alloc(max(1, n) * C.sizeof(abi.CdrXdcDecision))
            self.rounds.append((r, rp, ap))

    def base_replay(self, stream=None):
        rc = abi.lib().cdr_replay_sliced_async(self.eng.ctx, C.byref(self.base_db), C.byref(self.state),
                                               _stream(stream))
        if rc:
            raise RuntimeError(f"cdr_replay_sliced_async rc={rc}")

    def upload_state(self, state: engine.Outputs):
        """The state buffer := host records laid out by the replicator's state plan."""
        hip = self.dev.hip
        for name, src in [("result", state.result), ("exec", state.exec), ("repl", state.repl)] + [
                (t, state.tables[t]) for t in engine.TABLES]:
            if hip.hipMemcpy(C.c_void_p(getattr(self.state, name)), C.c_void_p(C.addressof(src)),
                             C.c_size_t(C.sizeof(src)), 1) != 0:
                raise RuntimeError("hipMemcpy H2D failed")

    def round(self, k: int, stream=None):
        rc = abi.lib().cdr_xdc_replicate_async(self.eng.ctx, self.n, C.byref(self.rounds[k][0]),
                                               C.c_void_p(self.state_caps_d), C.byref(self.state),
                                               C.byref(self.cluster), _stream(stream))
        if rc:
            raise RuntimeError(f"cdr_xdc_replicate_async rc={rc}")

    def download_round(self, k: int):
        """(decisions, reset Outputs, apply Outputs) of round k."""
        r, rp, ap = self.rounds[k]
        dec = new_decisions(self.n)
        self.dev.down(dec, r.dec)
        return (dec, ndc.download_out(self.dev, r.reset_out, self.n, rp, tasks=self.reset_tasks),
                ndc.download_out(self.dev, r.apply_out, self.n, ap))

    def download_state(self) -> engine.Outputs:
        return ndc.download_out(self.dev, self.state, self.n, self.state_plan)

    def run(self, base_replay: bool = True):
        """Base replay + every round; returns (state Outputs, [(decisions, reset Outputs, apply
        Outputs) per round])."""
        if base_replay:
            self.base_replay()
        per_round = []
        for k in range(len(self.rounds)):
            self.round(k)
            per_round.append(self.download_round(k))
        return self.download_state(), per_round

    def close(self):
        self.dev.close()
