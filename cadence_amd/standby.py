"""Standby task verification requests for loaded states (cdr_standby_tasks_async,
include/cdr/cdr.h).

``Requests`` holds cdr_standby_task records in arrival order, ``request`` / ``from_task`` build
one, ``plan`` groups them by state through ``cdr_plan_standby`` and ``tasks_to_requests`` turns
the transfer and timer tasks an ``engine.Outputs`` holds into requests — what the standby
processors (service/history/timerQueueStandbyProcessor.go, transferQueueStandbyProcessor.go)
receive.  ``Engine.standby_tasks`` (engine.py) verifies them on the device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi

SEC = 1_000_000_000


class Requests:
    """A ctypes array of cdr_standby_task in arrival order."""

    def __init__(self, reqs=()):
        reqs = list(reqs)
        self.n = len(reqs)
        self.arr = (abi.CdrStandbyTask * max(1, self.n))()
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
        out = (abi.CdrStandbyTask * max(1, self.n))()
        for i, k in enumerate(order):
            out[i] = self.arr[int(k)]
        return out


def request(wf, type, event_id=0, visibility_ts=0, timeout_type=0, version=0, attempt=0, task_list=0, flags=0,
            tag=0) -> abi.CdrStandbyTask:
    """One request from the task fields the verification reads."""
    q = abi.CdrStandbyTask(wf=wf, flags=flags, tag=tag)
    q.task = abi.CdrTask(type=type, timeout_type=timeout_type, event_id=event_id, visibility_ts=visibility_ts,
                         attempt=attempt, task_list=task_list, version=version)
    return q


def from_task(wf, task, flags=0, tag=0, version=None) -> abi.CdrStandbyTask:
    """One request from an emitted cdr_task (copied whole); `version` overrides the task's
    (stateBuilder's tasks leave it to the caller, schema.h cdr_task)."""
    q = abi.CdrStandbyTask(wf=wf, flags=flags, tag=tag)
    q.task = abi.CdrTask.from_buffer_copy(task)
    if version is not None:
        q.task.version = version
    return q


def plan(reqs: Requests, n_states: int):
    """(order, req_off) of cdr_plan_standby, as sync.plan: state s owns [req_off[s],
    req_off[s + 1]), the requests that address no state the trailing group."""
    order = np.zeros(max(1, len(reqs)), np.uint32)
    req_off = np.zeros(n_states + 2, np.uint32)
    rc = abi.lib().cdr_plan_standby(C.addressof(reqs.arr), len(reqs), n_states, order.ctypes.data,
                                    req_off.ctypes.data)
    if rc:
        raise RuntimeError(f"cdr_plan_standby rc={rc}")
    return order[:len(reqs)], req_off


def tasks_to_requests(outputs, flags=0, version=None, per_wf=None, wf_of=None, xfer_visibility=None) -> Requests:
    """The transfer and timer tasks `outputs` (an engine.Outputs replayed with tasks=True, or a
    rebuild's) holds for its OK entries, as requests in emission order: entry w's transfer tasks,
    then its timer tasks, addressed to state wf_of(w) (default: w itself).  `flags`: CDR_SBT_*
    for every request; `version`: None keeps each task's own, a callable gives
    version(w, task), a number is used for all; `per_wf`: at most that many tasks per entry;
    `xfer_visibility`: the visibility_ts of the transfer tasks (the replay leaves it 0; persistence
    stamps them when they are written).
    The tag is w << 16 | the task's ordinal within the entry."""
    out = []
    for w in range(outputs.n_wfs):
        if outputs.result[w].code != abi.OK:
            continue
        tasks = outputs.task_rows(w, "xfer") + outputs.task_rows(w, "ttask")
        if per_wf is not None:
            tasks = tasks[:per_wf]
        for k, t in enumerate(tasks):
            v = version(w, t) if callable(version) else version
            q = from_task(w if wf_of is None else wf_of(w), t, flags, (w << 16) | k, v)
            if xfer_visibility is not None and t.type < abi.TT_DECISION_TIMEOUT:
                q.task.visibility_ts = xfer_visibility
            out.append(q)
    return Requests(out)
