"""k_replay_fast at four waves per SIMD (replay_fast.inc): what the smaller register and LDS
footprint moved.  The entry's output offsets, run id and capacities are read from its descriptors
in the rare steps that store a VersionHistory item or a reset point; the failed event's id is read
back from its row after the loop; the last VersionHistory item is (prev_id, prev_ver); the
activity slot has ten planes, so the TASKS pool's base moved.

Every case is two fast slices, 64 + 1 workflows of at most 40 events (the second slice's row and
output offsets are not zero), through cdr_replay_sliced_async against the CPU restatement, every
record byte for byte (engine.compare)."""
import ctypes as C
import functools

import numpy as np
import pytest

from cadence_amd import abi, engine
from cadence_amd.history import HistoryBuilder
from .test_fast_uniform_gpu import UHist, host_type_flags
from .test_operand_hints_gpu import check, run_sliced

gpu = pytest.mark.gpu
FAST_CK = 8  # replay_fast.inc: reset-point checksums cached in LDS
GONE = "a domain the cache does not know"
N = 65


def build(hists):
    hb = HistoryBuilder()
    hb.domains_missing = {GONE}
    for i, h in enumerate(hists):
        hb.workflow(workflow_id=f"w{i}", run_id=f"r{i}", request_id=f"q{i}", retention_days=1 + i % 3).calls = h.calls
    return hb.build()


class Case:
    """The batch, its plan (with `short`: {entry: (capacity field, value)} replaced in the planner's
    capacities, offsets and totals kept) and the oracle's outputs under that plan.  The oracle checks
    a state slice's capacity at the end and reports no location; the contract's (schema.h
    CDR_E_BAD_INPUT) is the first event whose rows did not fit — here always Started, index 0."""

    def __init__(self, hists, short=None):
        import oracle
        self.batch = build(hists)
        pl = engine.plan(self.batch)
        if short:
            caps = (abi.CdrWfCaps * self.batch.n_wfs)()
            C.memmove(caps, pl.caps, C.sizeof(caps))
            tot = abi.CdrTotals()
            C.memmove(C.byref(tot), C.byref(pl.totals), C.sizeof(tot))
            for w, (f, v) in short.items():
                assert v < getattr(caps[w], f)
                setattr(caps[w], f, v)
            pl = engine.Plan(caps=caps, totals=tot)
        self.pl = pl
        self.ref = oracle.replay(self.batch, self.pl, tasks=True)
        for w in short or ():
            r = self.ref.result[w]
            assert (r.code, r.fail_event_id, r.fail_index) == (abi.E_BAD_INPUT, 0, 0)
            r.fail_event_id = hists[w].calls[0][0]["eventId"]

    def codes(self):
        return [abi.STATUS[self.ref.result[w].code] for w in range(self.batch.n_wfs)]


def started_attrs(h):
    return h.calls[0][0]["workflowExecutionStartedEventAttributes"]


def reset_points(lane, n):
    return {"points": [{"binaryChecksum": f"old{lane}-{j}", "runId": f"prev-{lane}", "firstDecisionCompletedId": 4,
                        "createdTimeNano": 10 ** 18, "resettable": True} for j in range(n)]}


# ---------------------------------------------------------------- 1. rare stores at lane-dependent rows
def rare(lane, uniform):
    """Twelve decisions.  The lane's j-th binary checksum is new until the lane has lane % 12 + 1
    of them (up to 12 > FAST_CK: the lookup past the cache), then repeats its newest; the last
    decision repeats an old one (ck0, or ck9 past the cache).  Two version bumps open new
    VersionHistory items: on every lane in the same rows (`uniform`) or in rows of the lane's own."""
    h = UHist(lane=lane, base=3 * lane)
    nck = lane % 12 + 1
    bumps = (3, 7) if uniform else (1 + lane % 4, 6 + lane % 5)
    if lane % 3 == 0:  # reset points rolled over by Started, in front of the decisions'
        started_attrs(h)["prevAutoResetPoints"] = reset_points(lane, 1 + lane % 2)
    for j in range(11):
        if j in bumps:
            h.ver += 10 + lane
        h.done_decision(checksum=f"ck{min(j, nck - 1)}")
    h.done_decision(checksum="ck9" if lane % 2 else "ck0")
    assert h.n == 37
    return h


@functools.lru_cache(maxsize=None)
def rare_case(uniform):
    return Case([rare(i, uniform) for i in range(N)])


def slice0_rows(c):
    nf, ns, tf, lane_wf = host_type_flags(c)
    assert (nf, ns) == (2, 2)
    assert (lane_wf[:64] >= 0).all() and (lane_wf[64:] >= 0).sum() == 1
    return tf[:len(tf) // 2]  # (both slices are as long as their longest history: the same)


def test_rare_store_premises():
    for uniform in (True, False):
        c = rare_case(uniform)
        assert set(c.codes()) == {"OK"}
        tf = slice0_rows(c)
        assert (tf[1:] == tf[1:, :1]).all() == uniform
        n_rp = [c.ref.result[w].n_reset_points for w in range(N)]
        assert max(n_rp) > FAST_CK and len(set(n_rp)) >= 8
        assert {c.ref.result[w].n_vh for w in range(N)} == {3}
        assert c.pl.caps[64].vh_off > 0 and c.pl.caps[64].rp_off > 0


def run_and_check(eng, c, tasks, skip=None):
    masked = set(np.nonzero(skip)[0].tolist()) if skip is not None else set()
    got = run_sliced(eng, c.batch, c.pl, tasks=tasks, skip=skip, want_fast=(2, 2))
    check(c, got, skip=masked)
    if tasks:
        bad = [m for m in engine.compare_tasks(c.batch, got, c.ref) if int(m.split()[1].rstrip(":")) not in masked]
        assert not bad, "\n".join(bad[:8])
        for w in range(c.batch.n_wfs):
            if w not in masked and c.ref.result[w].code == abi.OK:
                assert tuple(got.tasks["n"][2 * w:2 * w + 2]) == tuple(c.ref.tasks["n"][2 * w:2 * w + 2]), w
    for w in masked:  # a masked entry's records are untouched
        assert bytes(got.result[w]) == bytes(C.sizeof(abi.CdrWfResult))
        assert bytes(got.exec[w]) == bytes(C.sizeof(abi.CdrExecInfo))
    return got


@gpu
@pytest.mark.parametrize("tasks", [False, True], ids=["states", "tasks"])
@pytest.mark.parametrize("uniform", [True, False], ids=["uniform-rows", "per-lane-rows"])
def test_rare_stores_at_lane_dependent_rows(engine_gpu, uniform, tasks):
    """New reset points and VersionHistory items land in each entry's own slices (offsets read
    from the descriptors at the store).  TASKS: 65 x 24 task records against a pool of 320."""
    c = rare_case(uniform)
    if tasks:
        assert int(sum(c.ref.tasks["n"][:128])) > 1000
    run_and_check(engine_gpu, c, tasks)


# ---------------------------------------------------------------- 2. failures
# what fails where: (status, fail_index); fail_event_id is the event's id (the lane's own base + index + 1)
ROW1 = ("E_DECISION_NOT_FOUND", 1)
MID_START = ("P_ACTIVITY_STARTED_NIL", 15)
MID_CLOSE = ("E_ACTIVITY_NOT_FOUND", 16)
LAST = ("E_ACTIVITY_NOT_FOUND", 30)
DOMAIN = ("E_DOMAIN_NOT_FOUND", 0)
RP_CAP = ("E_BAD_INPUT", 0)
SA_CAP = ("E_BAD_INPUT", 0)
FAILS = {1: ROW1, 2: MID_START, 3: MID_CLOSE, 4: LAST, 5: DOMAIN, 6: RP_CAP, 7: SA_CAP}
EMPTY_EVENT_ID = -23


def failing(lane, uniform):
    """One shape for every lane (uniform rows: what fails is an operand's value) — a decision
    started at row 1, two activities with eight signals between Scheduled and Started (operand
    distances 9 and 10: no hint, the key is loaded) closing at rows 16 and 30 — and the lane's
    failure, lane % 8 of FAILS (0: none).  Not `uniform`: lane % 3 signals after row 2, so the
    rows differ from lane to lane from row 3 on — the uniform loop is left before its first
    step — and every later failure is that many rows further on."""
    what = lane % 8
    h = UHist(lane=lane, base=5 * lane)
    a = started_attrs(h)
    a["searchAttributes"] = {"indexedFields": {f"Custom{j}Field": f"v{lane}-{j}" for j in range(2 + lane % 2)}}
    a["prevAutoResetPoints"] = reset_points(lane, 3)
    if what == 5:
        a["parentWorkflowDomain"] = GONE
        a["parentWorkflowExecution"] = {"workflowId": "pw", "runId": "pr"}
        a["parentInitiatedEventId"] = 7
    # row 1: a DecisionTaskStarted with no decision scheduled names the empty event id, or fails
    st = h.add("DecisionTaskStarted", scheduledEventId=h.id + 4 if what == 1 else EMPTY_EVENT_ID, requestId="rq")
    h.add("DecisionTaskCompleted", scheduledEventId=st - 1, startedEventId=st, binaryChecksum="ck")
    extra = 0 if uniform else lane % 3
    for _ in range(extra):
        h.add("WorkflowExecutionSignaled")
    for j, bad_start, bad_close in ((0, what == 2, what == 3), (1, False, what == 4)):
        h.done_decision(checksum=f"ck{j}")
        s = h.add("ActivityTaskScheduled", same_call=True, activityId=f"L{lane}-a{j}", taskList={"name": "atl"},
                  scheduleToStartTimeoutSeconds=5, scheduleToCloseTimeoutSeconds=50, startToCloseTimeoutSeconds=20,
                  heartbeatTimeoutSeconds=0)
        for _ in range(8):
            h.add("WorkflowExecutionSignaled")
        st = h.add("ActivityTaskStarted", scheduledEventId=s - 2 if bad_start else s, requestId="arq")
        h.add("ActivityTaskCompleted", same_call=True, scheduledEventId=s - 2 if bad_close else s, startedEventId=st)
    assert h.n == 31 + extra
    return h


@functools.lru_cache(maxsize=None)
def failing_case(uniform):
    short = {}
    for w in range(N):
        if w % 8 == 6:
            short[w] = ("rp_cap", 2)
        if w % 8 == 7:
            short[w] = ("sa_cap", 1)
    return Case([failing(i, uniform) for i in range(N)], short)


def expected(c, w, uniform):
    """(status, fail_event_id, fail_index) of entry w by hand."""
    what = w % 8
    if what == 0:
        return ("OK", 0, 0)
    status, idx = FAILS[what]
    if what in (2, 3, 4) and not uniform:
        idx += w % 3
    return (status, 5 * w + idx + 1, idx)


def test_failing_premises():
    for uniform in (True, False):
        c = failing_case(uniform)
        tf = slice0_rows(c)
        assert (tf[1:] == tf[1:, :1]).all() == uniform
        for w in range(N):
            r = c.ref.result[w]
            assert (abi.STATUS[r.code], r.fail_event_id, r.fail_index) == expected(c, w, uniform), w


@gpu
@pytest.mark.parametrize("tasks", [False, True], ids=["states", "tasks"])
@pytest.mark.parametrize("uniform", [True, False], ids=["uniform-loop", "per-lane-loop"])
def test_failures_at_lane_dependent_rows(engine_gpu, uniform, tasks):
    """Lanes fail at row 1, in mid-history, at the last row and in the Started block (parent domain
    missing, reset points and search attributes past their capacity), each with its code, event id
    and index, the counts zero — and the rows after the failure change nothing: every failing
    lane's history goes on with events that are valid or would fail again with another code."""
    c = failing_case(uniform)
    got = run_and_check(engine_gpu, c, tasks)
    for w in range(N):
        r = got.result[w]
        assert (abi.STATUS[r.code], r.fail_event_id, r.fail_index) == expected(c, w, uniform), w
        if r.code != abi.OK:
            assert (r.n_activity, r.n_timer, r.n_child, r.n_cancel, r.n_signal) == (0, 0, 0, 0, 0), w
            assert (r.n_vh, r.n_reset_points, r.n_search_attr) == (0, 0, 0), w
            if tasks:
                assert tuple(got.tasks["n"][2 * w:2 * w + 2]) == (0, 0), w


# ---------------------------------------------------------------- 3. missing and masked lanes
def skip_mask():
    skip = np.zeros(N, np.uint8)
    skip[[0, 1, 6, 17, 37, 63]] = 1  # lane 0, failing lanes (1, 6, 17), the first slice's last lane
    return skip


@gpu
@pytest.mark.parametrize("tasks", [False, True], ids=["states", "tasks"])
@pytest.mark.parametrize("which", ["rare-uniform", "rare-per-lane", "fail-uniform", "fail-per-lane"])
def test_masked_entries(engine_gpu, which, tasks):
    """The wave's transposes rank lanes by the exec mask: with entries masked out (and the second
    slice's 63 missing lanes) every other record is still whole and in its place."""
    kind, loop = which.split("-", 1)
    c = (rare_case if kind == "rare" else failing_case)(loop == "uniform")
    run_and_check(engine_gpu, c, tasks, skip=skip_mask())


@gpu
@pytest.mark.parametrize("which", ["rare", "fail"])
def test_only_the_second_slice(engine_gpu, which):
    """Every entry of the first slice masked: its wave ends at once, the one-lane slice stands alone."""
    c = (rare_case if which == "rare" else failing_case)(False)
    skip = np.ones(N, np.uint8)
    skip[64] = 0
    run_and_check(engine_gpu, c, True, skip=skip)
