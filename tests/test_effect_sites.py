"""What every successful event of stateBuilder.applyEvents leaves behind, hand-derived
(tests/effect_cases.py), on the CPU restatement and on every kernel route.

CPU: each instance (case x builder) through oracle.replay must leave exactly the complete
state written by hand from the reference's Go; meta-tests hold the table to its coverage —
every event type in an OK case, every field of every output record with two expected values,
the handler branches by name — and prove that the comparer sees every field.  The carry-in
property is checked at every call boundary of every instance, and two loaded states with
hand-set rows pin the per-field loads of the carry prologue.

GPU: the table's batch bit-exact against the oracle on every route of
tests/test_fault_sites.ROUTES (with the task lists where the route emits them), every instance
against its hand-written state, after asserting from the slice plan that the route takes the
instances it claims; the fast-path kernel's claim, the class kernel alone, the carry-in cuts on
both carry kernels and the placement of a dense entry at the edges of its slices.
"""
import ctypes as C
import re

import numpy as np
import pytest

import oracle
from cadence_amd import abi, engine
from tests import effect_cases as EC
from tests import fault_cases as FC
from tests.test_capacity import _slices
from tests.test_fault_sites import (DEFAULT_MODE, REG_CAPS, REG_SLICES, ROUTES, WAVE_ALL, _assert_equal,
                                    _assert_split_equal, _entry_slices, _force_reg, _Knobs, _label, _split)
from tests.test_fault_sites import _refused as _fs_refused

_cache = {}
RECORDS = {"exec": abi.CdrExecInfo, "repl": abi.CdrReplState, "act": abi.CdrActivityInfo, "timer": abi.CdrTimerInfo,
           "child": abi.CdrChildInfo, "cancel": abi.CdrCancelInfo, "signal": abi.CdrSignalInfo, "vh": abi.CdrVHItem,
           "rp": abi.CdrResetPoint, "sa": abi.CdrKV}


def _fields(rec):
    return [f for f, _ in rec._fields_ if not f.startswith("_pad")]


def _table():
    """(batch, entries, plan, oracle outputs with task lists) of the whole table: one batch."""
    if "t" not in _cache:
        b, entries = EC.build_batch(EC.instances())
        pl = engine.plan(b)
        _cache["t"] = (b, entries, pl, oracle.replay(b, pl, tasks=True))
    return _cache["t"]


def _want(entries):
    """{entry index: the hand-written state} of a build_batch(); entry k of `entries` is
    workflow k of the batch."""
    want = {}
    for k, (c, bld, w, nr) in enumerate(entries):
        want[w] = c.state(bld, k)
        if nr is not None:
            want[nr] = c.new_run_state(bld, k)
    return want


def _assert_hand_states(b, entries, out, what, repl=True):
    want = _want(entries)
    names = {w: _label(c, bld) for c, bld, w, nr in entries}
    names.update({nr: _label(c, bld) + " new run" for c, bld, w, nr in entries if nr is not None})
    bad = []
    for w, st in want.items():
        if not repl and b.wfs[w].builder != abi.BUILDER_2DC:
            st = {k: v for k, v in st.items() if k != "repl"}
        bad += [f"{names[w]} {d}" for d in EC.diff(st, EC.exported(b, out, w, repl))]
    assert not bad, what + ":\n" + "\n".join(bad[:20])
    return len(want)


# ====================================================================== CPU: the table itself
def test_table_shape():
    """At most 40 events per history and 256 entries per batch; every case cites the Go; more
    than 150 instances; every expected record states exactly the record's non-pad fields."""
    names = [c.name for c in EC.CASES]
    assert len(names) == len(set(names))
    for c in EC.CASES + EC.CARRY_CASES:
        assert re.search(r"\b(sb|msb|dtm|vh|wei|meta|tb):\d+", c.doc), c.name
    for c in EC.CASES:
        assert c.n_events() <= 40 and len(c.new_run or []) <= 40, c.name
    b, entries, pl, ref = _table()
    assert b.n_wfs <= 256 and len(entries) > 150
    assert len(EC.CONSTANT) <= 3 and all(re.search(r"\b(sb|msb|dtm|tb):\d+", why) for why in EC.CONSTANT.values())
    for w, st in _want(entries).items():
        assert set(st) == {"result"} | set(RECORDS)
        for t, rec in RECORDS.items():
            for row in ([st[t]] if isinstance(st[t], dict) else st[t]):
                assert sorted(row) == sorted(_fields(rec)), (w, t)


def test_every_event_type_has_an_ok_case():
    seen = set().union(*(c.event_types() for c in EC.CASES))
    assert seen == set(abi.EVENT_TYPES) and len(seen) == 42


NOOP = {"noop_marker": "MarkerRecorded", "noop_cancel_timer_failed": "CancelTimerFailed",
        "noop_request_cancel_activity_failed": "RequestCancelActivityTaskFailed"}
COUNTERS = {".exec.next_event_id", ".exec.last_first_event_id", ".exec.last_event_task_id", ".vh[0].event_id",
            ".repl.last_write_event_id"}


def test_noop_events_move_only_the_counters():
    """The expected state of a no-op case differs from the plain head's in the counters alone."""
    for name, etype in NOOP.items():
        c = EC.by_name(name)
        assert etype in c.event_types()
        for bld in FC.ALL:
            plain = EC.Spec(end=(4, 4)).state(EC.Ctx(bld, 0, name))
            moved = {d.split(":")[0] for d in EC.diff(plain, c.state(bld, 0))}
            assert moved and moved <= COUNTERS, (name, moved)
            assert ".exec.next_event_id" in moved and ".exec.last_event_task_id" in moved


def _all_expected():
    """Every expected state of the table, the new runs' and the hand-made carry-in instances'."""
    b, entries, pl, ref = _table()
    states = list(_want(entries).values())
    states += [c.state(bld, 0) for c in EC.CARRY_CASES for bld in FC.ALL]
    return states


def test_every_field_takes_two_expected_values():
    """No field of any output record passes by being constant: outside CONSTANT each takes at
    least two distinct hand-written values somewhere in the table."""
    seen = {(t, f): set() for t, rec in RECORDS.items() for f in _fields(rec)}
    for st in _all_expected():
        for t in RECORDS:
            for row in ([st[t]] if isinstance(st[t], dict) else st[t]):
                for f, v in row.items():
                    seen[(t, f)].add(repr(v))
    flat = sorted(f"{RECORDS[t].__name__}.{f}" for (t, f), vals in seen.items() if len(vals) < 2)
    assert flat == sorted(EC.CONSTANT), flat


# the handler branches the table has to hold, by case name
BRANCHES = ["act_retry_expiration_below", "act_retry_expiration_equal", "act_retry_expiration_above", "act_no_retry",
            "act_cancel_before_start", "act_cancel_after_start", "act_close_completed", "act_close_failed",
            "act_close_timedout", "act_close_canceled", "timer_fired_repick", "timer_canceled_repick",
            "child_initiated", "child_started", "child_removed_start_failed", "child_removed_completed",
            "child_removed_failed", "child_removed_canceled", "child_removed_timedout", "child_removed_terminated",
            "cancel_initiated", "cancel_initiated_child_only", "cancel_failed", "cancel_delivered",
            "signal_initiated", "signal_initiated_child_only_control", "signal_failed", "signal_delivered",
            "wf_signaled_twice", "wf_cancel_requested", "close_completed", "close_failed", "close_timed_out",
            "close_canceled", "close_terminated_while_created", "sa_start_and_upserts", "reset_points_on_start",
            "parent_all", "parent_no_domain", "parent_no_execution", "parent_no_initiated", "wf_cron_memo",
            "wf_retry_expiration_attempt", "decision_timed_out_schedule_to_start",
            "decision_timed_out_start_to_close", "decision_failed", "xdc_second_cluster",
            "versions_rise_in_and_between_calls", "continue_as_new", "dense_all_tables"]


def test_required_branches_are_in_the_table():
    have = {c.name for c in EC.CASES}
    assert not [n for n in BRANCHES if n not in have]
    # the closes: state, close status, and the batch id is the call's first event
    for name, status in (("close_completed", 1), ("close_failed", 2), ("close_canceled", 3),
                         ("close_terminated_while_created", 4), ("continue_as_new", 5), ("close_timed_out", 6)):
        c = EC.by_name(name)
        x = c.state(FC.N, 0)["exec"]
        assert (x["state"], x["close_status"]) == (2, status)
        assert x["completion_event_batch_id"] == c.calls[-1][0]["eventId"] == x["last_first_event_id"]
    # the timer re-picks leave a timer the pick reached (task_id 1) that was not the first head
    for name in ("timer_fired_repick", "timer_canceled_repick"):
        rows = EC.by_name(name).state(FC.L, 0)["timer"]
        assert len(rows) == 2 and any(r["task_id"] == 1 and r["started_id"] > 5 for r in rows)
    x = EC.by_name("xdc_second_cluster").state(FC.D2, 0)
    assert x["repl"]["lri_mask"] == 0b10 and len(EC.by_name("xdc_second_cluster").state(FC.N, 0)["vh"]) == 2
    assert EC.by_name("decision_failed").state(FC.N, 0)["exec"]["decision_attempt"] == 1


def test_uuid_restatement():
    """mix64 / uuid of the table module against schema.h's cdr_uuid, through the branch id the
    oracle writes (site 1) — and a fixed point of mix64 written down once (splitmix64 of 0)."""
    assert EC.mix64(0) == 0xE220A8397B1DCDAF
    b, entries, pl, ref = _table()
    for k, (c, bld, w, nr) in enumerate(entries[:6]):
        lo, hi = EC.uuid(b.wfs[w].wf_key, EC.UUID_BRANCH, 1)
        assert b.wfs[w].wf_key == 0x1000 + k and (ref.exec[w].branch_id_lo, ref.exec[w].branch_id_hi) == (lo, hi)


# ====================================================================== CPU: the oracle against the table
def test_oracle_gives_the_hand_written_states():
    b, entries, pl, ref = _table()
    assert all(ref.result[w].code == abi.OK for w in range(b.n_wfs))
    n = _assert_hand_states(b, entries, ref, "oracle")
    assert n > 150


def _mutated(rec, f, strings):
    """A changed value of field `f` of ctypes record `rec` (a handle: another valid handle)."""
    v = getattr(rec, f)
    if hasattr(v, "__len__"):
        v[0] ^= 1
        return None
    if isinstance(v, float):
        return v + 1.0
    if f in engine._HANDLE_FIELDS:
        return (v + 1) % len(strings)
    return v ^ 1


def test_comparer_sees_every_field():
    """Change one field of one record of an oracle output (the dense case, which populates every
    table; the 2DC instance for the replication state): the comparison against the hand-written
    state must report it.  The record is restored afterwards."""
    b, entries, pl, ref = _table()
    n = 0
    for c, bld, w, nr in entries:
        if c.name != "dense_all_tables":
            continue
        want = _want(entries)[w]
        assert not EC.diff(want, EC.exported(b, ref, w))
        for t, rec in RECORDS.items():
            if t == "repl" and bld != FC.D2:
                continue
            if t == "vh" and bld != FC.N:
                continue
            target = {"exec": ref.exec, "repl": ref.repl}[t][w] if t in ("exec", "repl") else ref.rows(w, t)[0]
            saved = bytes(memoryview(target).cast("B"))
            for f in _fields(rec):
                new = _mutated(target, f, b.strings)
                if new is not None:
                    setattr(target, f, new)
                try:
                    bad = EC.diff(want, EC.exported(b, ref, w))
                finally:
                    C.memmove(C.addressof(target), saved, len(saved))
                # (the path of the field itself: `version` is not answered by a report on `lri_version`;
                # an array field reports its element, `.lri_version[0]`)
                assert bad and any(re.sub(r"\[\d+\]$", "", d.split(":")[0]).endswith("." + f) for d in bad), (t, f)
                n += 1
            assert not EC.diff(want, EC.exported(b, ref, w)), t
    assert n == sum(len(_fields(r)) for r in RECORDS.values()) + \
        2 * sum(len(_fields(r)) for t, r in RECORDS.items() if t not in ("repl", "vh"))


# ---------------------------------------------------------------- carry-in at every call boundary
def _cut_rounds(b, entries):
    """cut arrays, one per call ordinal j >= 1: every top-level entry with more than j calls is
    cut before its call j (a continue-as-new entry: up to its continue-as-new call, which the
    prefix never reaches — engine.split_batch's rule); 0 = not cut in this round."""
    calls = {w: engine._calls(b, w) for c, bld, w, nr in entries}
    rounds = []
    for j in range(1, max(len(v) for v in calls.values())):
        cut = np.zeros(b.n_wfs, np.int64)
        for c, bld, w, nr in entries:
            if j < len(calls[w]) and (nr is None or j <= c.new_run_call):
                cut[w] = calls[w][j]
        rounds.append(cut)
    return rounds


# Carried entries the planner keeps off the register-table carry kernel (they go to the general kernel)
CARRY_NOT_REG = {"started_twice_while_created": "a loaded entry whose suffix is a second Started event gets "
                                                "CDR_CAP_LOADED alone, no register-table flag (two of its builders)"}


def _assert_carry_plan(sb, names):
    """From the host planner: every carried entry is planned as loaded (CDR_CAP_LOADED) and sits
    in a register-table slice — the carry kernel's — but for CARRY_NOT_REG.  `names`: {entry: case name}."""
    p2 = engine.plan(sb)
    kind, _ = _entry_slices(sb, p2, DEFAULT_MODE)
    carried = [w for w in range(sb.n_wfs) if sb.carry.src[w] >= 0]
    assert carried and all(p2.caps[w].flags & abi.CAP_LOADED for w in carried)
    off = [w for w in carried if not kind[w] & REG_SLICES]
    assert len(off) <= 2 and all(names[w] in CARRY_NOT_REG for w in off), [names[w] for w in off]
    assert all(bool(p2.caps[w].flags & REG_CAPS) == bool(kind[w] & REG_SLICES) for w in carried)


def _assert_suffix_equal(b, full, sb, suf, cut):
    """test_fault_sites._assert_split_equal, its rule — an index into the entry's own events
    shifts by the cut — applied to lastDecision.event_index as well (its failing cases never end
    in a decision event; these cases do)."""
    for w in range(b.n_wfs):
        ld = suf.last_decision[w]
        if sb.carry.src[w] >= 0 and ld.source != 0:
            ld.event_index += int(cut[w])
    _assert_split_equal(b, full, sb, suf, cut)


def test_oracle_carry_in_at_every_call_boundary():
    """Prefix, then the suffix onto the loaded state (mutableStateBuilder.Load + applyEvents):
    the hand-written state again.  mutableStateBuilder.Load changes nothing an OK entry shows
    (test_fault_sites._assert_split_equal's rule: only a failed entry's fail_index shifts)."""
    b, entries, pl, full = _table()
    rounds = _cut_rounds(b, entries)
    assert len(rounds) >= 5
    n_carried = 0
    for j, cut in enumerate(rounds):
        pre, pre_out, sb = _split(b, cut, oracle.replay)
        assert all((sb.carry.src[w] >= 0) == (cut[w] > 0) for w in range(b.n_wfs))
        n_carried += int((sb.carry.src >= 0).sum())
        _assert_carry_plan(sb, {w: c.name for c, bld, w, nr in entries})
        suf = oracle.replay(sb)
        _assert_suffix_equal(b, full, sb, suf, cut)
        _assert_hand_states(sb, entries, suf, f"cut before call {j + 1}")
    assert n_carried > 300


# ---------------------------------------------------------------- carry-in onto hand-set rows
def _carry_batches(replay):
    """(suffix batch, entries) of EC.CARRY_CASES for every builder: the prefix replayed by
    `replay`, the case's patch written into the loaded row, the one-call suffix on top."""
    class _Shim:  # what build_batch reads of a case
        def __init__(self, cc):
            self.name, self.calls, self.new_run, self.expected_next_event_id = cc.name, cc.prefix + [cc.suffix], None, 0
            self.case = cc
    items = [(_Shim(cc), bld) for cc in EC.CARRY_CASES for bld in FC.ALL]
    b, entries = EC.build_batch(items)
    cut = np.array([engine._calls(b, w)[-1] for w in range(b.n_wfs)], np.int64)
    pre, _ = engine.cut_batches(b, cut)
    pre_out = replay(pre)
    for s, bld, w, nr in entries:
        table, row, patch = s.case.patch
        rec = pre_out.rows(w, table)[row]
        for f, v in patch.items():
            setattr(rec, f, v)
    sb = engine.suffix_batch(b, cut, pre, pre_out)
    assert (sb.carry.src >= 0).all()
    return sb, entries


def _assert_carry_states(sb, entries, out, what, repl=True):
    """`repl`=False: the replication record of the 2DC instances only (the kernels leave the
    other builders' records untouched)."""
    bad = []
    for k, (s, bld, w, nr) in enumerate(entries):
        st = s.case.state(bld, k)
        if not repl and bld != FC.D2:
            del st["repl"]
        bad += [f"{_label(s, bld)} {d}" for d in EC.diff(st, EC.exported(sb, out, w, repl))]
    assert not bad, what + ":\n" + "\n".join(bad[:20])


def test_oracle_carry_in_onto_hand_set_rows():
    sb, entries = _carry_batches(oracle.replay)
    _assert_carry_plan(sb, {w: s.name for s, bld, w, nr in entries})
    _assert_carry_states(sb, entries, oracle.replay(sb), "oracle")


# ====================================================================== routes: what the planner gives to whom
# Cases whose local / NDC instances the planner keeps off the fast-path kernel, with the reason
TWO_LIVE = ["act_close_completed", "act_close_failed", "act_close_timedout", "act_close_canceled",
            "act_close_completed_picks", "act_close_failed_picks", "act_close_timedout_picks",
            "act_close_canceled_picks", "act_exact_ties"]
NOT_FAST_TYPES = ["timer_started", "timer_fired_repick", "timer_canceled_repick", "timer_repick_created_head_then_none",
                  "timer_expiry_tie", "ext_own_domain", "child_initiated", "child_started",
                  "child_removed_start_failed", "child_removed_completed", "child_removed_failed",
                  "child_removed_canceled", "child_removed_timedout", "child_removed_terminated", "cancel_initiated",
                  "cancel_initiated_child_only", "cancel_failed", "cancel_delivered", "signal_initiated",
                  "signal_initiated_child_only_control", "signal_failed", "signal_delivered", "sa_start_and_upserts",
                  "sa_upsert_from_nil", "reset_points_from_checksums", "decision_failed_beside_a_timer",
                  "xdc_second_cluster", "versions_rise_in_and_between_calls", "continue_as_new", "dense_all_tables"]
UNREACHABLE = {
    "fast": [
        (NOT_FAST_TYPES, FC.ALL, "an event type outside CDR_FAST_TYPES: timers, children, external cancels and "
                                 "signals, search-attribute upserts, continue-as-new (host.cpp caps_one)"),
        (TWO_LIVE, FC.ALL, "two live activities"),
        (["marker_on_a_fresh_builder", "started_twice_while_created"], FC.ALL,
         "a first event that is not Started, or a second Started (host.cpp caps_one)"),
        ("*", (FC.D2,), "the fast-path kernel keeps no replication state: 2DC entries never get CDR_CAP_FAST"),
    ],
    "reg": [("fast", (FC.L, FC.N), "CDR_CAP_FAST entries take no other kernel's flag; the same cases' 2DC instances "
                                   "run on the register-table kernels")],
    "wave": [("fast", (FC.L, FC.N), "CDR_CAP_FAST entries never get CDR_CAP_WAVE; the same cases' 2DC instances run "
                                    "on the wave kernel")],
    "par": [("*", FC.ALL, "PAR slices take histories longer than CDR_LONG_MIN (1024) events only")],
}
# Event types the fast-path kernel replays in OK instances of the table (CDR_FAST_TYPES holds no others
# but the four activity closes, whose cases here keep two activities live)
FAST_EVENT_TYPES = 19


def _refused(route, c, bld):
    """test_fault_sites._refused on this module's UNREACHABLE."""
    fast_capable = not _fs_refused("fast", c, bld, False, UNREACHABLE)
    return _fs_refused(route, c, bld, fast_capable, UNREACHABLE)


def _taken(route):
    """(entries the route's kernel takes per the slice plan, entries UNREACHABLE refuses it)."""
    b, entries, pl, ref = _table()
    mode = WAVE_ALL if route == "wave" else DEFAULT_MODE if route == "par" else 0
    kind, _ = _entry_slices(b, pl, mode)
    mask = {"fast": abi.SLICE_FAST, "reg": REG_SLICES, "wave": abi.SLICE_WAVE, "par": abi.SLICE_PAR}[route]
    taken = {w for c, bld, w, nr in entries if kind.get(w, 0) & mask}
    refused = {w for c, bld, w, nr in entries if _refused(route, c, bld)}
    return taken, refused


@pytest.mark.parametrize("route", ["fast", "reg", "wave", "par"])
def test_unreachable_pairs(route):
    """The planner gives a route exactly the instances UNREACHABLE does not list, from the host
    planner alone: a planner change that drops — or adds — coverage fails here."""
    b, entries, pl, ref = _table()
    taken, refused = _taken(route)
    for c, bld, w, nr in entries:
        assert (w in taken) != (w in refused), (route, _label(c, bld), w in taken)
        if route == "fast":
            assert bool(pl.caps[w].flags & abi.CAP_FAST) == (w in taken), _label(c, bld)
        if route == "reg":
            assert bool(pl.caps[w].flags & REG_CAPS) == (w in taken), _label(c, bld)
    assert (len(taken) == 0) == (route == "par")
    assert all(len(reason) > 10 for rows in UNREACHABLE.values() for _, _, reason in rows)


def test_fast_path_event_types():
    """At least ten distinct event types run on the fast-path kernel in OK instances."""
    b, entries, pl, ref = _table()
    types = set().union(*(c.event_types() for c, bld, w, nr in entries if pl.caps[w].flags & abi.CAP_FAST))
    assert len(types) == FAST_EVENT_TYPES >= 10, sorted(types)


# routes that emit task lists (api: a replay with task lists plans lane slices only, so the wave
# route has none and "par" would be "default" again)
TASK_ROUTES = ("default", "reg0", "reg", "reg2", "general")


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_gpu_route(engine_gpu, route):
    """The table's batch on one route: the route's claim on the plan first; then bit-exact
    against the oracle (with the task lists where the route emits them) and, every instance,
    against its hand-written state."""
    r = dict(ROUTES[route])
    force = r.pop("force", "none")
    b, entries, pl, ref = _table()
    p = pl if force == "none" else _force_reg(pl, b.n_wfs, force)
    kind, _ = _entry_slices(b, p, r.get("mode", DEFAULT_MODE))
    reg_taken, _ = _taken("reg")
    if route in ("reg0", "reg", "reg2"):
        want = {"reg0": abi.SLICE_REG0, "reg": abi.SLICE_REG, "reg2": abi.SLICE_REG2}[route]
        assert len(reg_taken) > 100 and all(kind[w] == want for w in reg_taken), route
    elif route == "wave":
        on = [w for c, bld, w, nr in entries if pl.caps[w].flags & abi.CAP_WAVE]
        assert len(on) > 100 and all(kind[w] == abi.SLICE_WAVE for w in on)
    elif route == "general":
        assert not any(k & (abi.SLICE_WAVE | abi.SLICE_PAR) for k in kind.values())
    elif route == "par":
        assert not any(k & abi.SLICE_PAR for k in kind.values())  # UNREACHABLE["par"]
    else:  # default routing: fast-path and register-table slices (no history here is long or divergent enough
        # for a wave slice of its own; the wave route forces them)
        assert {abi.SLICE_FAST, abi.SLICE_REG0} <= set(kind.values())
    with _Knobs(engine_gpu, **r):
        got = engine_gpu.replay(b, p)
        got_t = engine_gpu.replay(b, p, tasks=True) if route in TASK_ROUTES else None
    _assert_equal(b, got, ref, route)
    _assert_hand_states(b, entries, got, route, repl=False)
    if got_t is not None:
        _assert_equal(b, got_t, ref, route + ", tasks", tasks=True)
        _assert_hand_states(b, entries, got_t, route + ", tasks", repl=False)


@pytest.mark.gpu
def test_gpu_fast_route_claim(engine_gpu):
    """Instances whose caps carry CDR_CAP_FAST sit in CDR_SLICE_FAST slices and give the same,
    hand-written, state with the fast path on and off."""
    b, entries, pl, ref = _table()
    nf, ns = engine.fast_slices(b, pl)
    assert nf > 0
    kind, _ = _entry_slices(b, pl, DEFAULT_MODE)
    on = [w for c, bld, w, nr in entries if pl.caps[w].flags & abi.CAP_FAST]
    assert len(on) > 50 and all(kind[w] == abi.SLICE_FAST for w in on)
    types = set().union(*(c.event_types() for c, bld, w, nr in entries if w in set(on)))
    assert len(types) == FAST_EVENT_TYPES >= 10
    for fast in (True, False):
        with _Knobs(engine_gpu, fast=fast):
            got = engine_gpu.replay(b, pl)
        _assert_equal(b, got, ref, f"fast path {fast}")
        _assert_hand_states(b, entries, got, f"fast path {fast}", repl=False)


@pytest.mark.gpu
def test_gpu_class_kernel_alone(engine_gpu):
    """k_replay_cls without the k_replay_reg pass behind it: every instance it keeps (no
    CLS_RETRY) has the hand-written state, and it keeps at least half of the register-table
    instances."""
    b, entries, pl, ref = _table()
    with _Knobs(engine_gpu, cls=abi.CLS_ALONE):
        got = engine_gpu.replay(b, pl)
    retried = {w for w in range(b.n_wfs) if got.result[w].code == abi.CLS_RETRY}
    assert all(pl.caps[w].flags & REG_CAPS for w in retried)
    # (a handed-on entry's continue-as-new run is left CDR_NOT_APPLIED by k_finalize)
    skip = retried | {w for w in range(b.n_wfs) if b.wfs[w].parent in retried}
    kept = [e for e in entries if e[2] not in skip]
    reg_taken, _ = _taken("reg")
    print(f"class kernel alone: keeps {len(reg_taken - retried)} of {len(reg_taken)} register-table instances")
    want = _want(entries)
    bad = []
    for w in range(b.n_wfs):
        if w in skip:
            continue
        st = want[w] if b.wfs[w].builder == abi.BUILDER_2DC else {k: v for k, v in want[w].items() if k != "repl"}
        bad += [f"wf {w} {d}" for d in EC.diff(st, EC.exported(b, got, w, repl=False))]
    assert not bad, "\n".join(bad[:20])
    bad = [x for x in engine.compare(b, got, ref, limit=10 ** 9) if int(re.match(r"wf (\d+):", x).group(1)) not in skip]
    assert not bad, "\n".join(bad[:10])
    assert kept and 2 * len(reg_taken - retried) >= len(reg_taken)


@pytest.mark.gpu
def test_gpu_carry_in_at_every_call_boundary(engine_gpu):
    """The cuts of test_oracle_carry_in_at_every_call_boundary on the GPU's own loaded prefix:
    the register-table carry kernel (default route) and the general kernel's carry prologue
    (reg=False), bit-exact against the oracle on the same carry-in batch and equal to the
    hand-written state."""
    b, entries, pl, ref = _table()
    full = engine_gpu.replay(b)
    for j, cut in enumerate(_cut_rounds(b, entries)):
        pre, pre_out, sb = _split(b, cut, engine_gpu.replay)
        _assert_equal(pre, pre_out, oracle.replay(pre), "prefix")
        assert all((sb.carry.src[w] >= 0) == (cut[w] > 0) for w in range(b.n_wfs))
        _assert_carry_plan(sb, {w: c.name for c, bld, w, nr in entries})
        sref = oracle.replay(sb)
        for reg in (True, False):
            with _Knobs(engine_gpu, reg=reg):
                got = engine_gpu.replay(sb)
            what = f"cut before call {j + 1}, " + ("register-table carry kernel" if reg else "general kernel")
            _assert_equal(sb, got, sref, what)
            _assert_hand_states(sb, entries, got, what, repl=False)
            _assert_suffix_equal(b, full, sb, got, cut)


@pytest.mark.gpu
def test_gpu_carry_in_onto_hand_set_rows(engine_gpu):
    """EC.CARRY_CASES on the GPU's own prefix, both carry kernels."""
    sb, entries = _carry_batches(engine_gpu.replay)
    _assert_carry_plan(sb, {w: s.name for s, bld, w, nr in entries})
    sref = oracle.replay(sb)
    _assert_carry_states(sb, entries, sref, "oracle on the GPU's prefix")
    for reg in (True, False):
        with _Knobs(engine_gpu, reg=reg):
            got = engine_gpu.replay(sb)
        _assert_equal(sb, got, sref, f"reg={reg}")
        _assert_carry_states(sb, entries, got, f"reg={reg}", repl=False)


# ---------------------------------------------------------------- lane placement
DENSE_AT = (0, 63, 64)


def _lane_batch():
    """128 register-table entries: the densest case at entries 0, 63 and 64 (one per builder
    kind), EC.SPARSE_TWIN everywhere else.  The lane planner orders a kernel group by length
    class, entity counts, slot footprint and length, all descending, and keeps the entry order
    among equals (host.cpp, the LaneKey sort).  Beside the plain head the dense entries would
    always lead their slice — lanes 0, 1, 2 —, so the filler is the twin that ties with them in
    every key and leaves other, sparser, rows: the entry order then is the lane order."""
    dense = EC.by_name("dense_all_tables")
    items = [(dense, FC.ALL[DENSE_AT.index(k)]) if k in DENSE_AT else (EC.SPARSE_TWIN, FC.ALL[k % 3])
             for k in range(128)]
    return EC.build_batch(items)


def _assert_lane_placement(b, pl):
    """From the slice plan: two full register-table slices, entry k at slice k // 64, lane k % 64 —
    the dense entries at slice 0 lane 0, slice 0 lane 63 and slice 1 lane 0."""
    lane_wf, flags = _slices(b, pl.caps, DEFAULT_MODE)
    assert lane_wf.shape == (2, 64) and list(flags) == [abi.SLICE_REG0, abi.SLICE_REG0]
    assert [int(w) for w in lane_wf.ravel()] == list(range(128))
    assert (int(lane_wf[0, 0]), int(lane_wf[0, 63]), int(lane_wf[1, 0])) == DENSE_AT


def test_lane_batch_puts_the_dense_entries_at_the_slice_edges():
    b, entries = _lane_batch()
    pl = engine.plan(b)
    _assert_lane_placement(b, pl)
    _assert_hand_states(b, entries, oracle.replay(b, pl), "oracle")


@pytest.mark.gpu
def test_gpu_lane_placement(engine_gpu):
    """The dense state at the first lane of a slice, at its last lane and at the first lane of
    the next slice, on the default route: it lands at those entries, and every neighbour has
    the sparse twin's state, field for field, and none of the dense rows."""
    b, entries = _lane_batch()
    pl = engine.plan(b)
    _assert_lane_placement(b, pl)
    got = engine_gpu.replay(b, pl)
    _assert_equal(b, got, oracle.replay(b, pl), "default route")
    _assert_hand_states(b, entries, got, "default route", repl=False)
    for w in range(128):
        r = got.result[w]
        assert (r.n_activity, r.n_timer, r.n_child, r.n_search_attr) == ((1, 1, 1, 2) if w in DENSE_AT else (0, 0, 0, 0)), w
