"""SyncActivity requests for loaded states (cdr_sync_activity_async, include/cdr/cdr.h).

``Requests`` holds h.SyncActivityRequest records in the ABI's form, ``plan`` groups them by
state through ``cdr_plan_sync`` and ``synth_requests`` derives a deterministic mix of
requests from a state's own rows — every exit of historyReplicator.SyncActivity
(service/history/historyReplicator.go:160-295) and both kinds of applied request.
``Engine.sync_activity`` (engine.py) applies them on the device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi

SEC = 1_000_000_000


class Requests:
    """A ctypes array of cdr_sync_activity in arrival order."""

    def __init__(self, reqs=()):
        reqs = list(reqs)
        self.n = len(reqs)
        self.arr = (abi.CdrSyncActivity * max(1, self.n))()
        for i, r in enumerate(reqs):
            self.arr[i] = r

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if not 0 <= i < self.n:
            raise IndexError(i)
        return self.arr[i]

    def __iter__(self):
        return (self.arr[i] for i in range(self.n))

    def gathered(self, order) -> C.Array:
        """The requests in `order` (plan()'s grouped sequence), as a new array."""
        out = (abi.CdrSyncActivity * max(1, self.n))()
        for i, k in enumerate(order):
            out[i] = self.arr[int(k)]
        return out


def request(wf, scheduled_id, version, attempt=0, scheduled_time=0, started_id=abi.EMPTY_EVENT_ID, started_time=0,
            last_heartbeat_time=0, tag=0) -> abi.CdrSyncActivity:
    return abi.CdrSyncActivity(version=version, scheduled_id=scheduled_id, scheduled_time=scheduled_time,
                               started_id=started_id, started_time=started_time,
                               last_heartbeat_time=last_heartbeat_time, attempt=attempt, wf=wf, tag=tag)


def plan(reqs: Requests, n_states: int):
    """(order, req_off) of cdr_plan_sync: order[i] = index of the i-th request of the grouped
    sequence; state s owns [req_off[s], req_off[s + 1]); the requests that address no state
    (wf < 0 or wf >= n_states) are the trailing group [req_off[n_states], req_off[n_states + 1])."""
    order = np.zeros(max(1, len(reqs)), np.uint32)
    req_off = np.zeros(n_states + 2, np.uint32)
    rc = abi.lib().cdr_plan_sync(C.addressof(reqs.arr), len(reqs), n_states, order.ctypes.data, req_off.ctypes.data)
    if rc:
        raise RuntimeError(f"cdr_plan_sync rc={rc}")
    return order[:len(reqs)], req_off


def last_write_version(state, w: int):
    """(builder kind, GetLastWriteVersion) of loaded record w as the sync path reads it
    (schema.h cdr_sync_result): None where the reference's call fails (NDC, no items)."""
    r = state.result[w]
    if state.repl[w].present:
        return abi.BUILDER_2DC, state.repl[w].last_write_version
    if (state.exec[w].flags & abi.XI_VH_BRANCH) or r.n_vh:
        n = min(r.n_vh, state.plan.caps[w].vh_cap)
        if n == 0:
            return abi.BUILDER_NDC, None
        return abi.BUILDER_NDC, state.tables["vh"][state.plan.caps[w].vh_off + n - 1].version
    return abi.BUILDER_LOCAL, abi.EMPTY_VERSION


def synth_requests(state, seed: int, per_wf: int, increment: int = 10) -> Requests:
    """`per_wf` requests for every record of `state` (an engine.Outputs), derived from the
    record's own rows as they are now, in a random interleaving of the workflows that keeps
    each workflow's requests in generation order.  The mix: schedule ids of pending
    activities, of finished ones (below next_event_id, not pending) and at or past
    next_event_id with versions below and above the last write version; versions lower,
    equal, larger from the same cluster (+ increment) and from another cluster (+ 1); attempts
    of -1, 0 and +1; heartbeats older, equal and newer; started and unstarted activities; and
    a few requests for a workflow that is not found (wf = -1)."""
    rng = np.random.default_rng(seed)
    per = []
    for w in range(state.n_wfs):
        ok = state.result[w].code == abi.OK
        rows = state.rows(w, "act") if ok else []
        nxt = state.exec[w].next_event_id if ok else 10
        _, lwv = last_write_version(state, w) if ok else (0, 0)
        lwv = 0 if lwv is None else lwv
        pending = {a.schedule_id for a in rows}
        mine = []
        for k in range(per_wf):
            tag = (w << 16) | k
            u = rng.random()
            if u < 0.02:
                mine.append(request(-1, int(rng.integers(1, 100)), 1, tag=tag))
                continue
            if u < 0.14:  # scheduleID >= nextEventID
                ver = lwv + int(rng.choice([-1, -increment, 0, increment, 1]))
                mine.append(request(w, nxt + int(rng.integers(0, 4)), ver, tag=tag))
                continue
            if u < 0.24 or not rows:  # below nextEventID, not pending
                free = [i for i in range(1, min(int(nxt), 64)) if i not in pending]
                sid = int(rng.choice(free)) if free else 0
                mine.append(request(w, sid, lwv, tag=tag))
                continue
            a = rows[int(rng.integers(0, len(rows)))]
            ver = a.version + int(rng.choice([-increment, 0, increment, 1], p=[0.08, 0.62, 0.12, 0.18]))
            att = a.attempt + int(rng.choice([-1, 0, 1], p=[0.12, 0.63, 0.25]))
            hb_set = a.flags & (abi.AI_STARTED_TIME_SET | abi.AI_HEARTBEAT_TIME_SET)
            hb0 = a.last_heartbeat_time if hb_set else a.scheduled_time
            hb = hb0 + int(rng.choice([-1, 0, 1, 30], p=[0.15, 0.2, 0.4, 0.25])) * SEC
            if rng.random() < 0.45:  # the retry case: scheduled again, not started
                started_id, started_time = abi.EMPTY_EVENT_ID, 0
            elif a.started_id != abi.EMPTY_EVENT_ID:
                started_id = a.started_id
                started_time = a.started_time if a.flags & abi.AI_STARTED_TIME_SET else a.scheduled_time
            else:
                started_id, started_time = a.schedule_id + 1, a.scheduled_time + SEC
            sched_time = a.scheduled_time + int(rng.choice([0, 0, 2])) * SEC
            mine.append(request(w, a.schedule_id, ver, att, sched_time, started_id, started_time, hb, tag))
        per.append(mine)
    # interleave the workflows, each one's requests in order
    slots = np.repeat(np.arange(state.n_wfs), per_wf)
    rng.shuffle(slots)
    nxt_i = [0] * state.n_wfs
    out = []
    for w in slots:
        out.append(per[w][nxt_i[w]])
        nxt_i[w] += 1
    return Requests(out)
