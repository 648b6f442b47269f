"""Under-sized and exactly-full output capacities on every kernel route (schema.h CDR_E_BAD_INPUT,
cdr.h cdr_replay_sliced_async).

An entry whose grow-only state slices (vh / rp / sa) or task slices (xfer / ttask) cannot hold
what its history produces ends CDR_E_BAD_INPUT with zero counts, writes nothing outside its
slices and leaves the rest of the batch alone; a slice that is exactly full is fine.

Victims come from the oracle's output under the planner's capacities: OK entries without a new
run or a parent whose final count of the kind is >= 2, shrunk to count - 1 (the edge), plus a
second set shrunk to 0.  Two layouts: *short* keeps the planner's offsets and totals, so the rows
a victim lost are a dead zone inside its own allocation (an unguarded kernel overruns into it and
nowhere else); *tight* packs every slice of the five kinds to the oracle's final count and
allocates 64 rows more than the totals.  Every device output buffer is filled with 0xA5 first.

The failure location of a task slice is (last event id, ev_len).  That of a state slice is the
first event whose row does not fit: `_state_walk` below finds it from the events alone (and is
itself checked against the oracle's final counts in test_fixtures_cover); every route, the general
kernel included, must report that event, so all routes agree with the general one.
"""
import ctypes as C

import numpy as np
import pytest

from cadence_amd import abi, engine, ndc

STATE = ("vh", "rp", "sa")
TASK = ("xfer", "ttask")
KINDS = STATE + TASK
CAP = {k: k + "_cap" for k in KINDS}
OFF = {k: k + "_off" for k in KINDS}
E_BAD_INPUT, E_REFRESH_CAPACITY = 13, 16
CANARY = 0xA5
TAIL = 64
REG_FLAGS = abi.SLICE_REG | abi.SLICE_REG2 | abi.SLICE_REG0

# route -> how it is reached: the synthetic cases (config, workflows), the plan mode, class blocks,
# task lists, the register-table / fast path switches, the slices that belong to the route and
# the kinds it supports
ROUTES = {
    "general": dict(cases=((0, 256), (3, 300)), mode=0, cls=False, tasks=True, reg=False, fast=False,
                    mask=None, kinds=KINDS),
    "fast": dict(cases=((1, 300), (2, 300), ("hand", 128)), mode=0, cls=False, tasks=True, reg=True, fast=True,
                 mask=abi.SLICE_FAST, kinds=KINDS),
    "reg": dict(cases=((3, 300), (5, 300)), mode=0, cls=False, tasks=True, reg=True, fast=True,
                mask=REG_FLAGS, kinds=KINDS),
    "cls": dict(cases=((3, 300), (4, 150), (5, 300)), mode=0, cls=True, tasks=True, reg=True, fast=True,
                mask=REG_FLAGS, kinds=KINDS),
    # (a wave slice holds one history, in lane 0; 295 workflows: the batch's last entry is on one)
    "wave": dict(cases=((5, 295),), mode=abi.PLAN_WAVE, cls=False, tasks=False, reg=True, fast=True,
                 mask=abi.SLICE_WAVE, kinds=STATE, edge=1),
}
_cache = {}


# ------------------------------------------------------------------ plans
def _copy_plan(pl, n):
    caps = (abi.CdrWfCaps * max(1, n))()
    C.memmove(caps, pl.caps, C.sizeof(caps))
    tot = abi.CdrTotals()
    C.memmove(C.byref(tot), C.byref(pl.totals), C.sizeof(tot))
    return engine.Plan(caps=caps, totals=tot)


def short_plan(pl, n, victims):
    """The planner's offsets and totals; each victim's capacity replaced (never an offset or a
    total: the rows [off + new_cap, off + planner_cap) stay the victim's own, a dead zone)."""
    p = _copy_plan(pl, n)
    for w, kind, cap in victims:
        assert cap < getattr(pl.caps[w], CAP[kind])
        setattr(p.caps[w], CAP[kind], cap)
    return p


def tight_plan(pl, n, ref):
    """Every capacity of the five kinds set to the oracle's final count, offsets re-packed."""
    p = _copy_plan(pl, n)
    for w in range(n):
        for kind in KINDS:
            setattr(p.caps[w], CAP[kind], _count(ref, w, kind))
    p.totals = ndc.offsets_from_caps(p.caps, n)
    return p


def _count(out, w, kind):
    if kind in TASK:
        return int(out.tasks["n"][2 * w + (1 if kind == "ttask" else 0)])
    return int(getattr(out.result[w], engine.TABLE_COUNT[kind]))


def _slices(batch, caps, mode):
    """(lane_wf[n_slices, 64], slice_flags[n_slices]) of the batch's slice plan (host planner)."""
    L = abi.lib()
    ns, rows, nw = C.c_uint32(), C.c_uint64(), C.c_uint32()
    L.cdr_plan_slices_ex(batch.wfs, caps, batch.n_wfs, mode, None, None, None, None, C.byref(ns), C.byref(rows),
                         C.byref(nw))
    lane = np.zeros(max(1, ns.value) * 64, np.int32)
    flags = np.zeros(max(1, ns.value), np.uint32)
    L.cdr_plan_slices_ex(batch.wfs, caps, batch.n_wfs, mode, lane.ctypes.data, None, None, flags.ctypes.data,
                         C.byref(ns), C.byref(rows), C.byref(nw))
    words, nf = C.c_uint64(), C.c_uint32()
    L.cdr_plan_scratch(caps, lane.ctypes.data, ns.value, None, None, None, flags.ctypes.data, C.byref(words),
                       C.byref(nf))
    return lane.reshape(-1, 64)[:ns.value], flags[:ns.value]


# ------------------------------------------------------------------ the events alone
def _state_walk(batch, w, kind, cap=None):
    """Entry w's rows of a state kind from its events: (final count, causes, failure) where
    causes is the set of event kinds that added rows ("started" / "event": a version run's first
    event, a new binary checksum, an upserted new key) and failure, for a capacity `cap`, the
    (event id, index) of the first event whose row does not fit (None: everything fits)."""
    d = batch.wfs[w]
    EV = abi.EV
    n, causes, fail = 0, set(), None
    keys, last_ver = set(), None

    def add(k, e, cause, rows=1):
        nonlocal n, fail
        n += rows
        causes.add(cause)
        if cap is not None and fail is None and n > cap:
            fail = (int(e.event_id), k)

    for k in range(d.ev_len):
        e = batch.events[d.ev_off + k]
        if kind == "vh":
            if d.builder == abi.BUILDER_NDC and (last_ver is None or e.version > last_ver):
                add(k, e, "started" if k == 0 else "event")
                last_ver = e.version
        elif e.type == EV["WorkflowExecutionStarted"]:
            a = e.a.started
            if kind == "rp" and a.flags & abi.SF_HAS_RESET_POINTS:
                keys = {batch.rps[a.reset_points_off + q].binary_checksum
                        if batch.rps[a.reset_points_off + q].flags & abi.RP_HAS_CHECKSUM else 0
                        for q in range(a.reset_points_len)}
                n = 0
                if a.reset_points_len:
                    add(k, e, "started", a.reset_points_len)
            if kind == "sa" and a.flags & abi.SF_HAS_SEARCH_ATTR:
                keys = {batch.kvs[a.search_attr_off + q].key for q in range(a.search_attr_len)}
                n = 0
                if a.search_attr_len:
                    add(k, e, "started", a.search_attr_len)
        elif kind == "rp" and e.type == EV["DecisionTaskCompleted"]:
            cks = e.a.dt.binary_checksum
            if cks != 0 and cks not in keys:
                keys.add(cks)
                add(k, e, "event")
        elif kind == "sa" and e.type == EV["UpsertWorkflowSearchAttributes"]:
            for q in range(e.a.upsert.search_attr_len):
                key = batch.kvs[e.a.upsert.search_attr_off + q].key
                if key not in keys:
                    keys.add(key)
                    add(k, e, "event")
    return n, causes, fail


def _end_of_history(batch, w):
    d = batch.wfs[w]
    return int(batch.events[d.ev_off + d.ev_len - 1].event_id), int(d.ev_len)


# ------------------------------------------------------------------ fixtures
NS = 10 ** 9
T0 = 1_600_000_000 * NS


def _hand_fast(n):
    """Hand-written fast-path histories (NDC builder, decisions only) whose version changes from
    one decision to the next: version histories of 2 or 3 items, which the synthetic fast-path
    configs (one version each) lack; with search attributes and rolled-over reset points on
    Started and a new binary checksum per decision."""
    from cadence_amd.history import HistoryBuilder
    hb = HistoryBuilder()
    for i in range(n):
        w = hb.workflow(workflow_id=f"wf-{i}", run_id=f"run-{i}", request_id=f"req-{i}", retention_days=1 + i % 3)
        st = {"workflowType": {"name": "wt"}, "taskList": {"name": "tl"}, "executionStartToCloseTimeoutSeconds": 100,
              "taskStartToCloseTimeoutSeconds": 10}
        if i % 2 == 0:
            st["searchAttributes"] = {"indexedFields": {f"k{j}": f"v{i}-{j}" for j in range(2 + i % 3)}}
        if i % 3 == 0:
            st["prevAutoResetPoints"] = {"points": [
                {"binaryChecksum": f"old-{j}", "runId": f"prev-{i}", "firstDecisionCompletedId": 4,
                 "createdTimeNano": T0, "resettable": True} for j in range(1 + i % 2)]}
        ev = [dict(eventId=1, version=1, timestamp=T0 + NS, eventType="WorkflowExecutionStarted",
                   workflowExecutionStartedEventAttributes=st)]
        calls, eid = [], 2
        for r in range(2 + i % 2):
            v = 1 + 10 * r
            ev.append(dict(eventId=eid, version=v, timestamp=T0 + eid * NS, eventType="DecisionTaskScheduled",
                           decisionTaskScheduledEventAttributes={"taskList": {"name": "tl"},
                                                                 "startToCloseTimeoutSeconds": 10, "attempt": 0}))
            calls.append(ev)
            calls.append([dict(eventId=eid + 1, version=v, timestamp=T0 + (eid + 1) * NS,
                               eventType="DecisionTaskStarted",
                               decisionTaskStartedEventAttributes={"scheduledEventId": eid, "requestId": f"r{r}"})])
            ev = [dict(eventId=eid + 2, version=v, timestamp=T0 + (eid + 2) * NS, eventType="DecisionTaskCompleted",
                       decisionTaskCompletedEventAttributes={"scheduledEventId": eid, "startedEventId": eid + 1,
                                                             "binaryChecksum": f"bin-{r}"})]
            eid += 3
        calls.append(ev)
        w.calls = calls
    return hb.build()


def _case(cfg, n, carry=False):
    """(batch, planner plan, oracle outputs with task lists under the planner's capacities);
    cfg "hand": the hand-written fast-path histories."""
    key = ("case", cfg, n, carry)
    if key not in _cache:
        import oracle
        if cfg == "hand":
            b = _hand_fast(n)
        elif carry:  # as test_tasks.test_gpu_tasks_carry builds its batch (the prefix's states: the oracle's)
            b0 = engine.synth_batch(cfg, n, seed=61)
            pre, cut = engine.split_batch(b0, 2)
            b = engine.suffix_batch(b0, cut, pre, oracle.replay(pre))
        else:
            b = engine.synth_batch(cfg, n, seed=0x5EED0700 + cfg)
        pl = engine.plan(b)
        _cache[key] = (b, pl, oracle.replay(b, pl, tasks=True))
    return _cache[key]


def _eligible(batch, ref, w, kind, least=2):
    d = batch.wfs[w]
    return ref.result[w].code == abi.OK and d.newrun < 0 and d.parent < 0 and _count(ref, w, kind) >= least


def _route_entries(batch, pl, mode, mask):
    """{entry: lane} of the entries on the route's slices."""
    lane, flags = _slices(batch, pl.caps, mode)
    pos = {}
    for s in range(len(flags)):
        if mask is None or flags[s] & mask:
            for l in range(64):
                if lane[s, l] >= 0:
                    pos[int(lane[s, l])] = l
    return pos


def _victims(batch, pl, ref, mode, mask, kinds, only=None, edge=3):
    """[(entry, kind, new_cap)]: the last entry of the batch, then per kind `edge` entries at
    count - 1 — one in lane 0, one in lane 63 and one in a middle lane of the route's slices
    where the kind has eligible entries there, any lane otherwise — and one more at 0; an entry
    is the victim of one kind only.  `only`: restrict to these entries."""
    pos = _route_entries(batch, pl, mode, mask)
    if only is not None:
        pos = {w: l for w, l in pos.items() if w in only}
    used, out = set(), []
    last = batch.n_wfs - 1
    if last in pos:
        for kind in [k for k in TASK if k in kinds] or kinds:
            if _eligible(batch, ref, last, kind):
                out.append((last, kind, _count(ref, last, kind) - 1))
                used.add(last)
                break
    for kind in kinds:
        # (a kind with no eligible entry in lane 0 or 63 takes another lane: three edge victims)
        for want in (lambda l: l == 0, lambda l: l == 63, lambda l: 0 < l < 63, lambda l: True, lambda l: True):
            if len([v for v in out if v[1] == kind and v[0] != last]) >= edge:
                break
            w = next((w for w in sorted(pos) if w not in used and want(pos[w]) and _eligible(batch, ref, w, kind)), None)
            if w is not None:
                out.append((w, kind, _count(ref, w, kind) - 1))
                used.add(w)
        # shrunk to 0: an entry whose Started event already brings rows of the kind, if there is one
        # (a single row where no entry of the route has two)
        at_started = (lambda w: kind in STATE and _state_walk(batch, w, kind, 0)[2][1] == 0)
        for least, pref in ((2, at_started), (2, lambda w: True), (1, lambda w: True)):
            w = next((w for w in sorted(pos) if w not in used and _eligible(batch, ref, w, kind, least) and pref(w)),
                     None)
            if w is not None:
                out.append((w, kind, 0))
                used.add(w)
                break
    return out


def _route_cases(route):
    """[(case key, batch, plan, ref, victims)] of a route."""
    r = ROUTES[route]
    out = []
    for cfg, n in r["cases"]:
        b, pl, ref = _case(cfg, n)
        out.append(((cfg, n), b, pl, ref, _victims(b, pl, ref, r["mode"], r["mask"], r["kinds"],
                                                   edge=r.get("edge", 3))))
    return out


def _carry_case():
    b, pl, ref = _case(3, 300, carry=True)
    loaded = {w for w in range(b.n_wfs) if b.carry.src[w] >= 0}
    return b, pl, ref, _victims(b, pl, ref, 0, REG_FLAGS, TASK, only=loaded)


def _expected(batch, ref_short, victims):
    """The oracle's outputs under the shrunk plan with the contract's location for the state
    victims (the oracle checks at the end and reports none for them)."""
    for w, kind, cap in victims:
        r = ref_short.result[w]
        assert r.code == E_BAD_INPUT
        if kind in STATE:
            fail = _state_walk(batch, w, kind, cap)[2]
            assert fail is not None
            r.fail_event_id, r.fail_index = fail
    return ref_short


# ------------------------------------------------------------------ CPU: the oracle
def _check_victims(batch, out, victims, tasks=True, location=True):
    for w, kind, cap in victims:
        r = out.result[w]
        assert r.code == E_BAD_INPUT, (w, kind, cap, r.code)
        assert [getattr(r, f) for f in engine.TABLE_COUNT.values()] == [0] * 8, (w, kind)
        if tasks:
            assert out.tasks["n"][2 * w] == 0 and out.tasks["n"][2 * w + 1] == 0, (w, kind)
        if location:
            want = _end_of_history(batch, w) if kind in TASK else _state_walk(batch, w, kind, cap)[2]
            assert (r.fail_event_id, r.fail_index) == want, (w, kind, cap, r.fail_event_id, r.fail_index, want)


def _others_equal(batch, got, ref, victims, last_decision=True):
    """Every entry but the victims equal (results, states, task lists) in `got` and `ref`
    (last_decision=False: the device outputs of _run_sliced carry no lastDecision records)."""
    skip = {w for w, _, _ in victims}
    assert all(got.result[w].code != abi.OK for w in skip)
    keep = [(w, bytes(ref.result[w])) for w in skip]
    for w in skip:  # failed in `got`: with its record on both sides engine.compare looks at no state of theirs
        C.memmove(C.byref(ref.result[w]), C.byref(got.result[w]), C.sizeof(abi.CdrWfResult))
    try:
        bad = engine.compare(batch, got, ref, last_decision=last_decision) + \
            (engine.compare_tasks(batch, got, ref) if got.tasks else [])
    finally:
        for w, r in keep:
            C.memmove(C.byref(ref.result[w]), r, len(r))
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_short_caps(kind):
    """The oracle under a shrunk plan: CDR_E_BAD_INPUT with zero counts for exactly the victims
    (task victims at the end of the history), every other entry as under the planner's plan."""
    import oracle
    for cfg, n in ((0, 256), (5, 300)):
        b, pl, ref = _case(cfg, n)
        vic = [v for v in _victims(b, pl, ref, 0, None, (kind,))]
        assert len(vic) >= 4 and {c for _, _, c in vic} >= {0}
        got = oracle.replay(b, short_plan(pl, b.n_wfs, vic), tasks=True)
        _check_victims(b, got, vic, location=kind in TASK)
        bad = [w for w in range(b.n_wfs) if got.result[w].code == E_BAD_INPUT and ref.result[w].code != E_BAD_INPUT]
        assert sorted(bad) == sorted(w for w, _, _ in vic)
        _others_equal(b, got, ref, vic)


def test_oracle_tight_caps():
    """Every slice of the five kinds exactly full: every entry as under the planner's plan."""
    import oracle
    for cfg, n in ((0, 256), (3, 300), (4, 150), (5, 300)):
        b, pl, ref = _case(cfg, n)
        tp = tight_plan(pl, b.n_wfs, ref)
        assert tp.totals.vh + tp.totals.rp + tp.totals.sa < pl.totals.vh + pl.totals.rp + pl.totals.sa or \
            tp.totals.xfer + tp.totals.ttask < pl.totals.xfer + pl.totals.ttask
        got = oracle.replay(b, tp, tasks=True)
        for w in range(b.n_wfs):
            assert bytes(got.result[w]) == bytes(ref.result[w]), w
        # same rows at the re-packed offsets: compare through each plan's own offsets
        for w in range(b.n_wfs):
            if ref.result[w].code != abi.OK:
                continue
            for t in engine.TABLES:
                assert [bytes(r) for r in got.rows(w, t)] == [bytes(r) for r in ref.rows(w, t)], (w, t)
            for t in TASK:
                assert [bytes(r) for r in got.task_rows(w, t)] == [bytes(r) for r in ref.task_rows(w, t)], (w, t)


def test_fixtures_cover():
    """The chosen batches give every route what its tests need (the oracle alone): per route and
    kind at least 4 eligible entries on the route's slices; victims in lane 0, lane 63, a middle
    lane and the batch's last entry; search-attribute victims that fail at a Started event and at
    an UpsertWorkflowSearchAttributes adding a new key; reset-point victims that fail at Started's
    rolled-over points and at a new binary checksum; version-history victims of >= 2 items.  The
    event walk that gives the state victims' failure locations reproduces the oracle's counts."""
    for route, r in ROUTES.items():
        elig = {k: 0 for k in r["kinds"]}
        lanes, last, causes, vh_items, reg_variants = set(), False, {k: set() for k in STATE}, [], 0
        for (cfg, n), b, pl, ref, vic in _route_cases(route):
            pos = _route_entries(b, pl, r["mode"], r["mask"])
            if route == "fast":
                assert engine.fast_slices(b, pl) == (len(_slices(b, pl.caps, 0)[1]),) * 2
            if route == "reg":
                reg_variants |= int(np.bitwise_or.reduce(_slices(b, pl.caps, 0)[1])) & REG_FLAGS
            for k in r["kinds"]:
                elig[k] += sum(_eligible(b, ref, w, k) for w in pos)
            for w, kind, cap in vic:
                assert w in pos
                lanes.add(0 if pos[w] == 0 else 63 if pos[w] == 63 else 1)
                last |= w == b.n_wfs - 1
                if kind in STATE:
                    cnt, _, fail = _state_walk(b, w, kind, cap)
                    assert cnt == _count(ref, w, kind), (route, cfg, w, kind, cnt)
                    assert fail is not None
                    k = fail[1]
                    causes[kind].add("started" if b.events[b.wfs[w].ev_off + k].type ==
                                     abi.EV["WorkflowExecutionStarted"] else "event")
                    if kind == "vh" and cap > 0:
                        vh_items.append(cnt)
            assert len({w for w, _, _ in vic}) == len(vic)
        assert all(v >= 4 for v in elig.values()), (route, elig)
        assert lanes == ({0} if route == "wave" else {0, 1, 63}) and last, (route, lanes, last)
        # (UpsertWorkflowSearchAttributes is no fast-path event type: there Started alone brings keys)
        assert causes["sa"] == ({"started"} if route == "fast" else {"started", "event"}), (route, causes)
        assert causes["rp"] == {"started", "event"}, (route, causes)
        assert vh_items and min(vh_items) >= 2, (route, vh_items)
        if route == "reg":
            assert reg_variants == REG_FLAGS
    b, pl, ref, vic = _carry_case()
    assert {k for _, k, _ in vic} == set(TASK) and len(vic) >= 6


# ------------------------------------------------------------------ GPU
def _upload_carry(dev, cy):
    """The batch's loaded states (cdr_carry) as a device-resident record."""
    st = cy.state
    hc = cy.cstruct()
    dc = abi.CdrCarry(n_src=hc.n_src, totals=hc.totals)
    dc.src = dev.up(cy.src)
    dc.caps = dev.up(st.plan.caps)
    dc.state.result, dc.state.exec, dc.state.repl = dev.up(st.result), dev.up(st.exec), dev.up(st.repl)
    for t in engine.TABLES:
        setattr(dc.state, t, dev.up(st.tables[t]))
    if cy.in_memory is not None:
        dc.in_memory = dev.up(cy.in_memory)
    return dev.up(dc)


def _run_sliced(eng, batch, pl, mode=0, cls=False, tasks=True, reg=True, fast=True, tail=0, task_rows=None,
                refresh=None):
    """`batch` with capacities `pl` through cdr_replay_sliced_async into device buffers of this
    test's own — `tail` rows longer than the totals, every byte 0xA5 before the launch — and back.
    `refresh`: (now_ns, flags) — replay without task lists, then cdr_refresh_tasks_async."""
    L = abi.lib()
    dev = ndc._Dev()
    n = batch.n_wfs
    try:
        db = ndc.upload_batch(dev, batch, pl.caps, mode, cls)
        if batch.carry is not None:
            db.carry = _upload_carry(dev, batch.carry)
        if task_rows is not None:
            db.task_rows = task_rows
        big = abi.CdrTotals()
        for f, _ in abi.CdrTotals._fields_:
            setattr(big, f, getattr(pl.totals, f) + tail)
        want_tasks = tasks or refresh is not None
        o = ndc.alloc_out(dev, n, big, want_tasks)
        sizes = [(o.result, max(1, n) * C.sizeof(abi.CdrWfResult)), (o.exec, max(1, n) * C.sizeof(abi.CdrExecInfo)),
                 (o.repl, max(1, n) * C.sizeof(abi.CdrReplState))]
        sizes += [(getattr(o, t), max(1, getattr(big, t)) * C.sizeof(engine.TABLE_TYPES[t])) for t in engine.TABLES]
        if want_tasks:
            sizes += [(o.transfer, max(1, big.xfer) * C.sizeof(abi.CdrTask)),
                      (o.timer_tasks, max(1, big.ttask) * C.sizeof(abi.CdrTask)), (o.n_tasks, 2 * max(1, n) * 4)]
        for p, nb in sizes:
            assert dev.hip.hipMemset(C.c_void_p(p), CANARY, C.c_size_t(nb)) == 0
        old_reg = L.cdr_set_reg_path(eng.ctx, 1 if reg else 0)
        old_fast = eng.set_fast_path(fast)
        try:
            if refresh is None:
                assert L.cdr_replay_sliced_async(eng.ctx, C.byref(db), C.byref(o), None) == 0
            else:  # the replay alone (no task lists), then the refresher into the task slices
                ro = abi.CdrOut()
                C.memmove(C.byref(ro), C.byref(o), C.sizeof(ro))
                ro.transfer = ro.timer_tasks = ro.n_tasks = None
                assert L.cdr_replay_sliced_async(eng.ctx, C.byref(db), C.byref(ro), None) == 0
                assert L.cdr_refresh_tasks_async(eng.ctx, C.byref(db), C.byref(o), refresh[0], refresh[1], None) == 0
            return ndc.download_out(dev, o, n, engine.Plan(caps=pl.caps, totals=big), want_tasks)  # (synchronises)
        finally:
            eng.set_fast_path(old_fast)
            L.cdr_set_reg_path(eng.ctx, old_reg)
    finally:
        dev.close()


def _table(out, kind):
    return out.tasks[kind] if kind in TASK else out.tables[kind]


def _canary(out, kind, lo, hi):
    """Rows [lo, hi) of a table still hold the fill, byte for byte."""
    t = _table(out, kind)
    sz = C.sizeof(t._type_)
    raw = np.frombuffer(t, dtype=np.uint8)[lo * sz:hi * sz]
    return len(raw) == (hi - lo) * sz and bool((raw == CANARY).all())


def _check_short(eng, batch, pl, vic, **route):
    import oracle
    sp = short_plan(pl, batch.n_wfs, vic)
    tasks = route.get("tasks", True)
    want = _expected(batch, oracle.replay(batch, sp, tasks=tasks), vic)
    got = _run_sliced(eng, batch, sp, **route)
    _check_victims(batch, got, vic, tasks=tasks)
    _others_equal(batch, got, want, vic, last_decision=False)
    for w, kind, cap in vic:  # what the victim lost of its slice: untouched
        off = getattr(pl.caps[w], OFF[kind])
        assert _canary(got, kind, off + cap, off + getattr(pl.caps[w], CAP[kind])), (w, kind, cap)


def _route_args(route):
    r = ROUTES[route]
    return dict(mode=r["mode"], cls=r["cls"], tasks=r["tasks"], reg=r["reg"], fast=r["fast"])


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES) + ["carry"])
def test_gpu_short_caps(engine_gpu, route):
    """Short layout: every victim CDR_E_BAD_INPUT with zero counts at the contract's location,
    every other entry equal to the oracle, the rows the victims lost still 0xA5."""
    if route == "carry":  # loaded entries on the register-table kernels' carry-in instantiations
        b, pl, _, vic = _carry_case()
        _check_short(engine_gpu, b, pl, vic, mode=0, cls=False, tasks=True)
        return
    for _, b, pl, _, vic in _route_cases(route):
        if vic:
            _check_short(engine_gpu, b, pl, vic, **_route_args(route))


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_gpu_tight_caps(engine_gpu, route):
    """Tight layout: every slice of the five kinds exactly full.  Every entry as the oracle's, the
    64 rows after every table's total still 0xA5."""
    import oracle
    args = _route_args(route)
    for _, b, pl, ref, _ in _route_cases(route):
        tp = tight_plan(pl, b.n_wfs, ref)
        want = oracle.replay(b, tp, tasks=args["tasks"])
        got = _run_sliced(engine_gpu, b, tp, tail=TAIL, **args)
        bad = engine.compare(b, got, want, last_decision=False) + \
            (engine.compare_tasks(b, got, want) if args["tasks"] else [])
        assert not bad, "\n".join(bad[:10])
        for w in range(b.n_wfs):
            assert got.result[w].code == ref.result[w].code, w
        for kind in engine.TABLES + (TASK if args["tasks"] else ()):
            total = getattr(tp.totals, kind)
            assert _canary(got, kind, total, total + TAIL), kind


@pytest.mark.gpu
def test_gpu_short_caps_host_route(engine_gpu):
    """The same victims through cdr_replay_batch (host buffers, the Go caller's path)."""
    import oracle
    for cfg, n in ((3, 300), (5, 300)):
        b, pl, ref = _case(cfg, n)
        vic = _victims(b, pl, ref, 0, None, KINDS)
        sp = short_plan(pl, b.n_wfs, vic)
        got = engine_gpu.replay(b, sp, tasks=True)
        _check_victims(b, got, vic, location=False)
        _others_equal(b, got, oracle.replay(b, sp, tasks=True), vic)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["total", "zero", "half"])
def test_gpu_task_staging_rows(engine_gpu, rows):
    """The class kernels' task staging sized by cdr_dev_batch.task_rows: the true total, 0 (the
    last entry's offsets + capacities read back) and half the total (entries staged past it are
    handed on to k_replay_reg<TASKS>): results and task lists equal the oracle's either way."""
    for cfg, n in ((3, 300), (5, 300)):
        b, pl, ref = _case(cfg, n)
        total = pl.totals.xfer + pl.totals.ttask
        got = _run_sliced(engine_gpu, b, pl, mode=0, cls=True, tasks=True,
                          task_rows={"total": total, "zero": 0, "half": total // 2}[rows])
        bad = engine.compare(b, got, ref, last_decision=False) + engine.compare_tasks(b, got, ref)
        assert not bad, "\n".join(bad[:10])
        assert all(got.result[w].code == abi.OK for w in range(b.n_wfs))


@pytest.mark.gpu
def test_gpu_refresh_capacity(engine_gpu):
    """cdr_refresh_tasks_async with task slices one below what the refresher emits:
    CDR_E_REFRESH_CAPACITY on the GPU and in the oracle, no tasks, the victims' pending rows
    (timer_task_status, task_id) as the oracle leaves them, the lost rows still 0xA5."""
    import oracle
    b, pl, _ = _case(3, 300)
    full = oracle.rebuild(b, pl)
    vic = [(w, kind, _count(full, w, kind) - 1) for w, kind in
           ((5, "xfer"), (64, "ttask"), (127, "xfer"), (b.n_wfs - 1, "ttask"))]
    assert all(_eligible(b, full, w, kind) for w, kind, _ in vic)
    sp = short_plan(pl, b.n_wfs, vic)
    want = oracle.rebuild(b, sp)
    got = _run_sliced(engine_gpu, b, sp, mode=0, cls=True, tasks=False,
                      refresh=(b.now_ns, abi.REFRESH_ADVANCED_VISIBILITY))
    for w, kind, cap in vic:
        assert want.result[w].code == E_REFRESH_CAPACITY and got.result[w].code == E_REFRESH_CAPACITY, (w, kind)
        assert bytes(got.result[w]) == bytes(want.result[w]), w
        assert got.tasks["n"][2 * w] == 0 and got.tasks["n"][2 * w + 1] == 0
        assert [r.timer_task_status for r in got.rows(w, "act")] == [r.timer_task_status for r in want.rows(w, "act")]
        assert [r.task_id for r in got.rows(w, "timer")] == [r.task_id for r in want.rows(w, "timer")]
        off = getattr(pl.caps[w], OFF[kind])
        assert _canary(got, kind, off + cap, off + getattr(pl.caps[w], CAP[kind])), (w, kind)
    codes = [w for w in range(b.n_wfs) if want.result[w].code == E_REFRESH_CAPACITY]
    assert sorted(codes) == sorted(w for w, _, _ in vic)
    _others_equal(b, got, want, vic, last_decision=False)
