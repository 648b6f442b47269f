"""Every failure return of stateBuilder.applyEvents, hand-built (tests/fault_cases.py), on
the CPU restatement and on every kernel route.

CPU: each case through oracle.replay must leave exactly the result record derived by hand
from the reference's Go; the codes reached are the codes the table claims, and every
CDR_E_* / CDR_P_* that oracle/replay_ref.cpp's applyEvents and AddOrUpdateItem return is
reached or listed unreachable with a reason.  The carry-in property (cut before the failing
call, replay the prefix, then the suffix onto the loaded state) is checked on the oracle too.

GPU: the same batches bit-exact against the oracle on each route — default routing, the
fast-path kernel, the register-table kernels without the class kernel (each variant), the
class kernel alone, the wave kernel and the general kernel — after asserting from the slice
plan that the route takes the cases it claims.  What the planner never gives to a route is in
UNREACHABLE with the reason, and the test asserts that the planner indeed refuses it.
"""
import ctypes as C
import re

import numpy as np
import pytest

import oracle
from cadence_amd import abi, engine
from tests import fault_cases as FC
from tests.test_capacity import _canary, _run_sliced, _slices
from tests.test_carry import _force_small_tables

REG_CAPS = abi.CAP_REG | abi.CAP_REG2 | abi.CAP_REG0
REG_SLICES = abi.SLICE_REG | abi.SLICE_REG2 | abi.SLICE_REG0
DEFAULT_MODE = abi.PLAN_WAVE | abi.PLAN_PAR
WAVE_ALL = abi.PLAN_WAVE | abi.PLAN_WAVE_ALL
_cache = {}


def _batches():
    """[(batch, entries, plan, oracle outputs with task lists)] of the table."""
    if "b" not in _cache:
        out = []
        for items in FC.batches():
            b, entries = FC.build_batch(items)
            pl = engine.plan(b)
            out.append((b, entries, pl, oracle.replay(b, pl, tasks=True)))
        _cache["b"] = out
    return _cache["b"]


def _long():
    if "long" not in _cache:
        c = FC.by_name("long_prefix_then_failure")
        b, entries = FC.build_batch([(c, bld) for bld in FC.ALL] + [(FC.by_name("clean_head"), FC.N)])
        pl = engine.plan(b)
        _cache["long"] = (b, entries, pl, oracle.replay(b, pl, tasks=True))
    return _cache["long"]


def _record(out, w):
    r = out.result[w]
    return (r.code, r.fail_event_id, r.fail_index, r.flags)


def _label(c, bld):
    return f"{c.name}[{FC.BUILDER_NAMES[bld]}]"


# ====================================================================== CPU
def test_table_shape():
    """At most about 40 events per history (one long case apart); every case cites the Go."""
    names = [c.name for c in FC.CASES]
    assert len(names) == len(set(names))
    for c in FC.CASES:
        assert re.search(r"\b(sb|msb|dtm|vh|wei|meta|go):?\d*", c.doc) or "head alone" in c.doc, c.name
        if "long" not in c.sites:
            assert c.n_events() <= 40 and len(c.new_run or []) <= 40, c.name
    assert sum(1 for c in FC.CASES if "long" in c.sites) == 1
    assert all(len(items) <= 256 for items in FC.batches())


def test_oracle_gives_the_hand_derived_records():
    """Each instance: exactly (code, fail_event_id, fail_index, flags) of the table — OK for
    the legal neighbours — and a failed entry reports no state rows and no tasks."""
    n = 0
    for b, entries, pl, ref in _batches() + [_long()]:
        want = FC.expected_records(entries)
        for c, bld, w, nr in entries:
            for idx in (w, nr):
                if idx is None:
                    continue
                assert _record(ref, idx) == want[idx], (_label(c, bld), "new run" if idx == nr else "")
                if want[idx][0] != abi.OK:
                    assert all(getattr(ref.result[idx], f) == 0 for f in engine.TABLE_COUNT.values()), _label(c, bld)
                    assert ref.tasks["n"][2 * idx] == 0 and ref.tasks["n"][2 * idx + 1] == 0, _label(c, bld)
                n += 1
    assert n > 300


def _apply_events_codes():
    """The CDR_E_* / CDR_P_* names in the bodies of AddOrUpdateItem, DeleteActivity and
    applyEvents of oracle/replay_ref.cpp, plus the rebuild check of replay_one."""
    import os
    src = open(os.path.join(os.path.dirname(oracle.__file__), "replay_ref.cpp")).read()

    def body(start, end):
        i = src.index(start)
        return src[i:src.index(end, i)]
    text = body("int32_t AddOrUpdateItem(", "struct ActivityInfo")
    text += body("int32_t DeleteActivity(", "// timerBuilder.GetActivityTimerTaskIfNeeded")
    text += body("GoErr applyEvents(", "}  // namespace")
    text += body("void replay_one(", "delete newRun;")
    return {m[4:] for m in re.findall(r"CDR_[EP]_[A-Z_]+", text)}


def test_every_apply_events_status_is_reached():
    claimed = set().union(*(c.codes for c in FC.CASES)) - {"OK", "NOT_APPLIED"}
    reached = set()
    for b, entries, pl, ref in _batches() + [_long()]:
        reached |= {abi.STATUS[ref.result[w].code] for w in range(b.n_wfs)}
    reached -= {"OK", "NOT_APPLIED"}
    assert reached == claimed
    in_source = _apply_events_codes()
    assert len(in_source) >= 16
    # E_BAD_INPUT is a capacity verdict of write_state (tests/test_capacity.py), not of applyEvents
    assert in_source - FC.NOT_APPLY_EVENTS == reached, (sorted(in_source - reached), sorted(reached - in_source))
    for site, (code, reason) in FC.UNREACHABLE_SITES.items():
        assert code in reached and len(reason) > 40, site  # the code itself is reached at its other sites


def test_unreachable_transition_is_unreachable():
    """UNREACHABLE_SITES["transition_decision_started"]: Created -> Running / None is accepted."""
    assert oracle.lib().cdro_state_transition(abi.STATE_CREATED, abi.CLOSE_NONE, abi.STATE_RUNNING, abi.CLOSE_NONE) == 1


# ---------------------------------------------------------------- carry-in cuts
# Instances with no call boundary before the failing event: nothing to cut (the issue's
# exemption for the Started-event domain failure, and its relatives at index 0 / in call 0)
NO_PREFIX = {
    "history_empty": "no events",
    "unknown_type_first_event": "fails at index 0",
    "vh_negative_event_id_first": "fails at index 0",
    "decision_first_event": "fails at index 0",
    "domain_missing_started": "the failing event is the Started event",
    "unknown_cluster_first_call": "fails at index 0",
    "unknown_cluster_by_last_event": "fails at index 0",
}
# ... and the NextEventID check, which is a verdict on a whole history: its prefix fails it too
# ... and the failures a Load heals: mutableStateBuilder.Load rebuilds ByActivityID from the pending
# infos (mutableStateBuilder.go:286-288), so the entry a duplicate's close deleted is back after the
# cut and the suffix replays clean — in the reference as here (test_load_heals_duplicate_activity_id)
LOAD_HEALS = ("activity_id_not_found", "activity_id_not_found_other_order", "missing_activity_info_duplicate")
NO_CUT = {"rebuild_next_event_id": "expected_next_event_id applies to the prefix as well",
          **{n: "Load rebuilds ByActivityID" for n in LOAD_HEALS}}


def _cuts(b, entries):
    """cut[w]: the last call boundary at or before entry w's failing event (a failure inside
    the new run: before the parent's continue-as-new call); 0 = not cut."""
    cut = np.zeros(b.n_wfs, np.int64)
    for c, bld, w, nr in entries:
        code, _, idx, flags = c.expect[bld]
        if code == "OK" or c.name.split("+")[0] in NO_CUT:
            continue
        calls = engine._calls(b, w)
        if flags & FC.IN_NEWRUN:
            cut[w] = calls[c.new_run_call]
        else:
            cut[w] = max([k for k in calls if k <= idx], default=0)
        if nr is not None and cut[w] > calls[c.new_run_call]:
            cut[w] = calls[c.new_run_call]  # (split_batch's rule: the prefix never reaches the new-run call)
    return cut


def _assert_split_equal(batch, full, suf_batch, suf, cut):
    """tests/test_carry.py's check of the same name, aware of failures inside a new run: a
    failed entry fails the same way on the loaded state, its fail_index shifted by the cut —
    unless the index is the new run's own (CDR_RF_IN_NEWRUN), which no cut of the parent moves."""
    for w in range(batch.n_wfs):
        a, b = suf.result[w], full.result[w]
        if b.code != abi.OK:
            assert (a.code, a.fail_event_id, a.flags) == (b.code, b.fail_event_id, b.flags), w
            shift = cut[w] if suf_batch.carry.src[w] >= 0 and not b.flags & FC.IN_NEWRUN else 0
            assert a.fail_index + shift == b.fail_index, w
            a.fail_index = b.fail_index  # compared above
    bad = engine.compare(batch, suf, full)
    assert not bad, "\n".join(bad[:10])


def _split(b, cut, replay):
    pre, _ = engine.cut_batches(b, cut)
    pre_out = replay(pre)
    return pre, pre_out, engine.suffix_batch(b, cut, pre, pre_out)


def test_load_heals_duplicate_activity_id():
    """LOAD_HEALS: cut after the first close of a duplicated activityId, the suffix on the loaded
    state is OK where the whole history fails."""
    items = [(FC.by_name(n), bld) for n in LOAD_HEALS for bld in FC.ALL]
    b, entries = FC.build_batch(items)
    cut = np.array([engine._calls(b, w)[-1] for w in range(b.n_wfs)], np.int64)
    pre, pre_out, sb = _split(b, cut, oracle.replay)
    assert (sb.carry.src >= 0).all()
    full, suf = oracle.replay(b), oracle.replay(sb)
    assert all(full.result[w].code != abi.OK and suf.result[w].code == abi.OK for w in range(b.n_wfs))


def test_no_prefix_list_is_exact():
    got = set()
    for b, entries, pl, ref in _batches():
        cut = _cuts(b, entries)
        got |= {c.name.split("+")[0] for c, bld, w, nr in entries if c.fails(bld) and cut[w] == 0} - set(NO_CUT)
    assert got == set(NO_PREFIX)


def test_oracle_carry_in_fails_the_same_way():
    """Cut at the last call boundary before the failing event: the suffix replayed onto the
    loaded prefix fails with the same code and event id, fail_index shifted by the cut."""
    for b, entries, pl, full in _batches() + [_long()]:
        cut = _cuts(b, entries)
        pre, pre_out, sb = _split(b, cut, oracle.replay)
        for c, bld, w, nr in entries:  # every prefix is clean, so every cut entry is carried
            assert (sb.carry.src[w] >= 0) == (cut[w] > 0), _label(c, bld)
        assert (sb.carry.src >= 0).sum() > 20 or b.n_wfs < 10
        _assert_split_equal(b, oracle.replay(b), sb, oracle.replay(sb), cut)


# ====================================================================== GPU routes
def _entry_slices(b, pl, mode):
    """(slice flags of the slice each entry sits in, its lane) under plan mode `mode`."""
    lane_wf, flags = _slices(b, pl.caps, mode)
    kind, lane = {}, {}
    for s in range(lane_wf.shape[0]):
        for l in range(64):
            w = int(lane_wf[s, l])
            if w >= 0:
                kind[w], lane[w] = int(flags[s]), l
    return kind, lane


def _copy_plan(pl, n):
    caps = (abi.CdrWfCaps * max(1, n))()
    C.memmove(caps, pl.caps, C.sizeof(caps))
    tot = abi.CdrTotals()
    C.memmove(C.byref(tot), C.byref(pl.totals), C.sizeof(tot))
    return engine.Plan(caps=caps, totals=tot)


def _force_reg(pl, n, variant):
    """Every register-table entry on one variant: its own (None), the 6-activity tables
    (CAP_REG without CAP_REG0) or the 12-activity tables (CAP_REG2 alone) — larger tables
    than the planner chose, never smaller."""
    p = _copy_plan(pl, n)
    for w in range(n):
        f = p.caps[w].flags
        if not f & REG_CAPS or variant is None:
            continue
        f &= ~REG_CAPS
        p.caps[w].flags = f | (abi.CAP_REG if variant == abi.CAP_REG else abi.CAP_REG2)
    return p


# What the planner never gives to a route, by case (base name; "+timer" twins included where
# they exist) and builder, with the reason.  test_unreachable_pairs asserts every line.
NOT_FAST_TYPES = ["history_empty", "newrun_history_empty", "newrun_history_empty_entry", "unknown_type_42",
                  "unknown_type_43", "unknown_type_63", "unknown_type_64", "unknown_type_99", "unknown_type_254",
                  "unknown_type_255", "unknown_type_256", "unknown_type_261", "unknown_type_2147483653",
                  "unknown_type_first_event", "started_twice_running", "started_twice_created",
                  "started_after_close", "can_after_close", "can_while_created", "decision_first_event",
                  "domain_missing_child", "domain_missing_cancel", "domain_missing_signal", "domain_known_all",
                  "child_started_nil", "two_failures_first_wins", "two_failures_one_call", "newrun_fails",
                  "newrun_fails_first_event", "newrun_fails_prelude", "newrun_not_reached", "timer_started_twice",
                  "timer_fired_unknown", "child_close_unknown", "signal_cancel_close_unknown"]
TWO_LIVE = ["activity_id_not_found", "activity_id_not_found_other_order", "activity_id_duplicate_one_close",
            "missing_activity_info_duplicate"]
IDS_NOT_INCREASING = ["vh_event_id_equal", "vh_event_id_lower", "vh_event_id_equal_higher_version",
                      "vh_event_id_zero", "vh_negative_event_id", "vh_negative_event_id_first", "prelude_wins"]
UNREACHABLE = {
    "fast": [
        (NOT_FAST_TYPES, FC.ALL, "no events, an event type outside CDR_FAST_TYPES, a second Started or a first "
                                 "event that is not Started (host.cpp caps_one)"),
        (TWO_LIVE, FC.ALL, "two live activities"),
        ("*", (FC.D2,), "the fast-path kernel keeps no replication state: 2DC entries never get CDR_CAP_FAST"),
        ("+timer", FC.ALL, "the twins end in a TimerStarted, outside CDR_FAST_TYPES"),
    ],
    "reg": [
        (IDS_NOT_INCREASING, FC.ALL, "the register-table envelope needs strictly increasing event ids below 2^31"),
        (["history_empty"], FC.ALL, "no events"),
        ("fast", (FC.L, FC.N), "CDR_CAP_FAST entries take no other kernel's flag; their +timer twins stand in"),
    ],
    "wave": [
        ("fast", (FC.L, FC.N), "CDR_CAP_FAST entries never get CDR_CAP_WAVE; their +timer twins stand in"),
    ],
    "par": [("*", FC.ALL, "PAR slices take histories longer than CDR_LONG_MIN (1024) events only")],
}


def _base(c):
    return c.name.split("+")[0]


def _refused(route, c, bld, fast_capable, table=None):
    """`table`: another module's UNREACHABLE in this one's form (tests/test_effect_sites.py)."""
    for names, builders, _ in (UNREACHABLE if table is None else table)[route]:
        if bld not in builders:
            continue
        if names == "*" or (names == "+timer" and "tail" in c.sites) or \
                (names == "fast" and fast_capable and "tail" not in c.sites) or \
                (isinstance(names, list) and _base(c) in names):
            return True
    return False


def _route_sets(route):
    """For every batch: (entries the route's kernel takes per the slice plan, entries
    UNREACHABLE says it never takes) as sets of entry indices."""
    out = []
    for b, entries, pl, ref in _batches():
        mode = WAVE_ALL if route == "wave" else DEFAULT_MODE if route == "par" else 0
        kind, _ = _entry_slices(b, pl, mode)
        mask = {"fast": abi.SLICE_FAST, "reg": REG_SLICES, "wave": abi.SLICE_WAVE, "par": abi.SLICE_PAR}[route]
        # (the fast-capable base instances: by the plan's own flag, which the fast list must explain)
        fastcap = {w for c, bld, w, nr in entries if "tail" not in c.sites and
                   not _refused("fast", c, bld, False)}
        taken = {w for c, bld, w, nr in entries if kind.get(w, 0) & mask}
        refused = {w for c, bld, w, nr in entries if _refused(route, c, bld, w in fastcap)}
        out.append((b, entries, pl, taken, refused))
    return out


@pytest.mark.parametrize("route", ["fast", "reg", "wave", "par"])
def test_unreachable_pairs(route):
    """The planner gives a route exactly the instances UNREACHABLE does not list (so a planner
    change that drops — or adds — coverage fails here); checked from the host planner alone."""
    n_taken = 0
    for b, entries, pl, taken, refused in _route_sets(route):
        top = {w for c, bld, w, nr in entries}
        for c, bld, w, nr in entries:
            assert (w in taken) != (w in refused), (route, _label(c, bld), w in taken)
            if route == "fast":
                assert bool(pl.caps[w].flags & abi.CAP_FAST) == (w in taken), _label(c, bld)
            if route == "reg":
                assert bool(pl.caps[w].flags & REG_CAPS) == (w in taken), _label(c, bld)
        assert taken | refused == top
        n_taken += len(taken)
    assert (n_taken == 0) == (route == "par")


def test_route_coverage_of_codes():
    """Which failure codes each specialised route meets, from the table and the plan alone."""
    fast, reg, wave = set(), set(), set()
    for route, acc in (("fast", fast), ("reg", reg), ("wave", wave)):
        for b, entries, pl, taken, refused in _route_sets(route):
            acc |= {c.expect[bld][0] for c, bld, w, nr in entries if w in taken}
    every = {"E_NEWRUN_HISTORY_EMPTY", "E_UNKNOWN_EVENT_TYPE", "E_INVALID_STATE_TRANSITION", "E_VH_LOWER_VERSION",
             "E_DECISION_NOT_FOUND", "E_ACTIVITY_NOT_FOUND", "E_ACTIVITY_ID_NOT_FOUND", "E_MISSING_ACTIVITY_INFO",
             "E_DOMAIN_NOT_FOUND", "P_ACTIVITY_STARTED_NIL", "P_CHILD_STARTED_NIL", "P_VH_ITEM_INVALID",
             "P_UNKNOWN_CLUSTER", "OK"}
    # (E_VH_LOWER_EVENT_ID on the register-table kernels: inside a new run only — UNREACHABLE["reg"])
    assert reg == every | {"E_VH_LOWER_EVENT_ID", "E_REBUILD_NEXT_EVENT_ID"}
    assert wave == every | {"E_VH_LOWER_EVENT_ID", "E_REBUILD_NEXT_EVENT_ID", "E_HISTORY_EMPTY"}
    assert fast == {"OK", "E_INVALID_STATE_TRANSITION", "E_VH_LOWER_VERSION", "E_VH_LOWER_EVENT_ID",
                    "E_DECISION_NOT_FOUND", "E_ACTIVITY_NOT_FOUND", "E_MISSING_ACTIVITY_INFO", "E_DOMAIN_NOT_FOUND",
                    "P_ACTIVITY_STARTED_NIL", "P_VH_ITEM_INVALID", "E_REBUILD_NEXT_EVENT_ID"}


class _Knobs:
    """Engine switches of one route, restored on exit."""

    def __init__(self, eng, cls=None, mode=None, reg=None, fast=None):
        self.eng, self.want, self.old = eng, dict(cls=cls, mode=mode, reg=reg, fast=fast), {}

    def __enter__(self):
        e, w = self.eng, self.want
        if w["cls"] is not None:
            self.old["cls"] = e.set_cls(w["cls"])
        if w["mode"] is not None:
            self.old["mode"] = e.set_plan_mode(w["mode"])
        if w["reg"] is not None:
            self.old["reg"] = abi.lib().cdr_set_reg_path(e.ctx, 1 if w["reg"] else 0)
        if w["fast"] is not None:
            self.old["fast"] = e.set_fast_path(w["fast"])
        return self

    def __exit__(self, *a):
        e, o = self.eng, self.old
        if "fast" in o:
            e.set_fast_path(o["fast"])
        if "reg" in o:
            abi.lib().cdr_set_reg_path(e.ctx, o["reg"])
        if "mode" in o:
            e.set_plan_mode(o["mode"])
        if "cls" in o:
            e.set_cls(o["cls"])


ROUTES = {
    "default": dict(),
    "par": dict(mode=DEFAULT_MODE),
    "reg0": dict(cls=False, force=None),
    "reg": dict(cls=False, force=abi.CAP_REG),
    "reg2": dict(cls=False, force=abi.CAP_REG2),
    "wave": dict(mode=WAVE_ALL),
    "general": dict(cls=False, mode=0, reg=False, fast=False),
}


def _assert_equal(b, got, ref, what, tasks=False):
    bad = engine.compare(b, got, ref) + (engine.compare_tasks(b, got, ref) if tasks else [])
    assert not bad, what + ":\n" + "\n".join(bad[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_gpu_route(engine_gpu, route):
    """The table's batches (and the long history) on one route, bit-exact against the oracle;
    the route's claim on the plan first."""
    r = dict(ROUTES[route])
    force = r.pop("force", "none")
    for b, entries, pl, ref in _batches() + [_long()]:
        p = pl if force == "none" else _force_reg(pl, b.n_wfs, force)
        mode = r.get("mode", DEFAULT_MODE)
        kind, _ = _entry_slices(b, p, mode)
        if route in ("reg0", "reg", "reg2"):
            want = {"reg0": abi.SLICE_REG0, "reg": abi.SLICE_REG, "reg2": abi.SLICE_REG2}[route]
            on = [w for c, bld, w, nr in entries if pl.caps[w].flags & REG_CAPS]
            assert on and all(kind[w] == want for w in on), route
        elif route == "wave":
            on = [w for c, bld, w, nr in entries if pl.caps[w].flags & abi.CAP_WAVE]
            assert on and all(kind[w] == abi.SLICE_WAVE for w in on)
        elif route == "general":
            assert not any(k & (abi.SLICE_WAVE | abi.SLICE_PAR) for k in kind.values())
        elif route == "par":
            assert not any(k & abi.SLICE_PAR for k in kind.values())  # UNREACHABLE["par"]
        else:  # default routing: fast, register-table (class kernel first) and wave slices all occur
            assert b.n_wfs < 10 or {abi.SLICE_FAST, abi.SLICE_REG0, abi.SLICE_WAVE} <= set(kind.values())
        with _Knobs(engine_gpu, **r):
            got = engine_gpu.replay(b, p)
        _assert_equal(b, got, ref, route)
        want = FC.expected_records(entries)  # ... and the hand-derived record itself
        for w, t in want.items():
            assert _record(got, w) == t, (route, w)


@pytest.mark.gpu
def test_gpu_fast_route_claim(engine_gpu):
    """The fast-path kernel replays the fast-shaped instances (engine.fast_slices > 0 and their
    slices are CDR_SLICE_FAST), failures at lanes the planner chose; with the fast path off the
    same slices go through the general kernel."""
    n_failing = 0
    for b, entries, pl, ref in _batches():
        nf, ns = engine.fast_slices(b, pl)
        assert nf > 0
        kind, _ = _entry_slices(b, pl, DEFAULT_MODE)
        on = [(c, bld, w) for c, bld, w, nr in entries if pl.caps[w].flags & abi.CAP_FAST]
        assert all(kind[w] == abi.SLICE_FAST for _, _, w in on)
        n_failing += sum(1 for c, bld, w in on if c.fails(bld))
        _assert_equal(b, engine_gpu.replay(b, pl), ref, "fast path on")
        with _Knobs(engine_gpu, fast=False):
            _assert_equal(b, engine_gpu.replay(b, pl), ref, "fast path off")
    assert n_failing >= 30


@pytest.mark.gpu
def test_gpu_class_kernel_alone(engine_gpu):
    """k_replay_cls without the k_replay_reg pass behind it: every failing register-table
    entry comes back CLS_RETRY (never a wrong OK, never a code of its own), and every entry
    the class kernel kept equals the oracle."""
    n_retry = 0
    for b, entries, pl, ref in _batches():
        with _Knobs(engine_gpu, cls=abi.CLS_ALONE):
            got = engine_gpu.replay(b, pl)
        retried = {w for w in range(b.n_wfs) if got.result[w].code == abi.CLS_RETRY}
        for c, bld, w, nr in entries:
            if pl.caps[w].flags & REG_CAPS and ref.result[w].code != abi.OK:
                # (a failure inside the new run is the new run's lane's — which may be another
                # kernel's — joined by k_finalize: the parent shows it, or the hand-on code)
                own = not ref.result[w].flags & FC.IN_NEWRUN
                assert got.result[w].code in ((abi.CLS_RETRY,) if own else (abi.CLS_RETRY, ref.result[w].code)), \
                    (_label(c, bld), got.result[w].code)
            if w in retried:
                assert pl.caps[w].flags & REG_CAPS, _label(c, bld)
        n_retry += len(retried)
        # a handed-on entry's continue-as-new run is left CDR_NOT_APPLIED by k_finalize
        skip = retried | {w for w in range(b.n_wfs) if b.wfs[w].parent in retried}
        bad = [x for x in engine.compare(b, got, ref, limit=10 ** 9)
               if int(re.match(r"wf (\d+):", x).group(1)) not in skip]
        assert not bad, "\n".join(bad[:10])
    assert n_retry >= 60


# ---------------------------------------------------------------- lanes 0, 31, 32, 63 and whole slices
def _lane_batch(builder, tail):
    """64 entries of one shape: activity_not_found_completed at 0, 31, 32 and 63, its clean
    twin (the same events, the close naming the pending activity) elsewhere."""
    bad, good = FC.by_name("activity_not_found_completed"), FC.by_name("clean_activity")
    if tail:
        bad, good = FC.with_timer_tail(bad), FC.with_timer_tail(good)
    return FC.build_batch([(bad if k in (0, 31, 32, 63) else good, builder) for k in range(64)])


LANE_SHAPES = {"fast": (FC.N, False, abi.SLICE_FAST), "fast_local": (FC.L, False, abi.SLICE_FAST),
               "reg_2dc": (FC.D2, False, abi.SLICE_REG0), "reg_ndc": (FC.N, True, abi.SLICE_REG0)}


def test_lane_batches_put_failures_at_the_slice_edges():
    for name, (bld, tail, want) in LANE_SHAPES.items():
        b, entries = _lane_batch(bld, tail)
        pl = engine.plan(b)
        kind, lane = _entry_slices(b, pl, DEFAULT_MODE)
        assert set(kind.values()) == {want}, name
        assert sorted(lane[w] for c, _, w, _ in entries if c.fails(bld)) == [0, 31, 32, 63], name


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(LANE_SHAPES))
def test_gpu_failures_at_slice_edges(engine_gpu, shape):
    bld, tail, _ = LANE_SHAPES[shape]
    b, entries = _lane_batch(bld, tail)
    pl = engine.plan(b)
    ref = oracle.replay(b, pl)
    assert sum(1 for w in range(64) if ref.result[w].code != abi.OK) == 4
    for route in ("default", "general") if shape.startswith("fast") else ("default", "reg0", "reg2", "wave", "general"):
        r = dict(ROUTES[route])
        force = r.pop("force", "none")
        p = pl if force == "none" else _force_reg(pl, b.n_wfs, force)
        with _Knobs(engine_gpu, **r):
            _assert_equal(b, engine_gpu.replay(b, p), ref, f"{shape} on {route}")


def _uniform_batches():
    """One fast slice whose 64 lanes all fail at the same row (the wave-uniform scalar path of
    k_replay_fast), and one whose lanes fail at 64 different rows (6 .. 69; the only histories
    above 40 events besides the long case: 64 distinct rows need them)."""
    same = FC.build_batch([(FC.by_name("fail_mid_call"), FC.N)] * 64)
    rows = FC.build_batch([(FC.fail_at_row(k), FC.N if k % 2 else FC.L) for k in range(64)])
    return {"same_row": same, "different_rows": rows}


def test_uniform_batches_are_one_fast_slice():
    for name, (b, entries) in _uniform_batches().items():
        pl = engine.plan(b)
        assert engine.fast_slices(b, pl) == (1, 1), name
        ref = oracle.replay(b, pl)
        rows = {ref.result[w].fail_index for w in range(64)}
        assert all(ref.result[w].code == FC.CODE["E_ACTIVITY_NOT_FOUND"] for w in range(64))
        assert len(rows) == (1 if name == "same_row" else 64)
        assert FC.expected_records(entries) == {w: _record(ref, w) for w in range(64)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["same_row", "different_rows"])
def test_gpu_whole_slice_fails(engine_gpu, name):
    b, entries = _uniform_batches()[name]
    pl = engine.plan(b)
    ref = oracle.replay(b, pl, tasks=True)
    _assert_equal(b, engine_gpu.replay(b, pl), ref, "fast")
    _assert_equal(b, engine_gpu.replay(b, pl, tasks=True), ref, "fast, tasks", tasks=True)
    with _Knobs(engine_gpu, fast=False):
        _assert_equal(b, engine_gpu.replay(b, pl), ref, "general")


# ---------------------------------------------------------------- what a failed entry leaves
TASK_ROUTES = {  # (lane slices only: task lists come from no wave / PAR slice)
    "fast_and_reg": dict(mode=0, cls=False, reg=True, fast=True),  # fast-path and register-table slices
    "cls": dict(mode=0, cls=True, reg=True, fast=True),
    "general": dict(mode=0, cls=False, reg=False, fast=False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(TASK_ROUTES))
def test_gpu_failed_entry_leaves_no_tasks(engine_gpu, route):
    """tasks=True into device buffers filled with 0xA5: state and task lists of the OK entries
    equal the oracle's; every failed entry's task counts and state counts equal the oracle's
    (zero); and nothing is written past an entry's own rows — the rows [n, cap) of every OK
    entry's task slices, and so whatever lies between a failed entry and its neighbours' lists,
    still hold the fill."""
    n_adjacent = 0
    for b, entries, pl, ref in _batches():
        got = _run_sliced(engine_gpu, b, pl, tasks=True, **TASK_ROUTES[route])
        bad = engine.compare(b, got, ref, last_decision=False) + engine.compare_tasks(b, got, ref)
        assert not bad, "\n".join(bad[:10])
        n_failed = 0
        wrong = [(w, list(got.tasks["n"][2 * w:2 * w + 2]), list(ref.tasks["n"][2 * w:2 * w + 2]))
                 for w in range(b.n_wfs) if list(got.tasks["n"][2 * w:2 * w + 2]) != list(ref.tasks["n"][2 * w:2 * w + 2])]
        assert not wrong, wrong[:10]
        for w in range(b.n_wfs):
            if ref.result[w].code != abi.OK:
                n_failed += 1
                assert got.tasks["n"][2 * w] == 0 and got.tasks["n"][2 * w + 1] == 0, w
                assert all(getattr(got.result[w], f) == 0 for f in engine.TABLE_COUNT.values()), w
                continue
            c = pl.caps[w]
            for kind, off, cap, n in (("xfer", c.xfer_off, c.xfer_cap, got.tasks["n"][2 * w]),
                                      ("ttask", c.ttask_off, c.ttask_cap, got.tasks["n"][2 * w + 1])):
                assert _canary(got, kind, off + n, off + cap), (w, kind)
        assert n_failed > 30
        # entries next to a failed one: their lists are the oracle's (compare_tasks above)
        n_adjacent += sum(1 for w in range(b.n_wfs - 1) if ref.result[w].code != abi.OK and
                          ref.result[w + 1].code == abi.OK and ref.tasks["n"][2 * (w + 1)] > 0)
    assert n_adjacent > 50


# ---------------------------------------------------------------- carry-in
@pytest.mark.gpu
def test_gpu_carry_in_fails_the_same_way(engine_gpu):
    """The failing suffix onto the GPU's own loaded prefix — default route, the forced
    small-table hand-on chain, the general kernel — bit-exact against the oracle on the same
    carry-in batch, and failing as the whole history does (fail_index shifted by the cut)."""
    for b, entries, pl, ref in _batches() + [_long()]:
        cut = _cuts(b, entries)
        pre, pre_out, sb = _split(b, cut, engine_gpu.replay)
        _assert_equal(pre, pre_out, oracle.replay(pre), "prefix")
        assert all((sb.carry.src[w] >= 0) == (cut[w] > 0) for w in range(b.n_wfs))
        sref = oracle.replay(sb)
        full = engine_gpu.replay(b)
        got = engine_gpu.replay(sb)
        _assert_equal(sb, got, sref, "default route")
        _assert_split_equal(b, full, sb, got, cut)
        pl2 = engine.plan(sb)
        assert _force_small_tables(sb, pl2) > 0
        got = engine_gpu.replay(sb, pl2)
        _assert_equal(sb, got, sref, "hand-on chain")
        _assert_split_equal(b, full, sb, got, cut)
        with _Knobs(engine_gpu, reg=False):
            got = engine_gpu.replay(sb)
        _assert_equal(sb, got, sref, "general kernel")
        _assert_split_equal(b, full, sb, got, cut)
    # LOAD_HEALS: the loaded state's ByActivityID is rebuilt from its rows on the GPU too
    b, entries = FC.build_batch([(FC.by_name(n), bld) for n in LOAD_HEALS for bld in FC.ALL])
    cut = np.array([engine._calls(b, w)[-1] for w in range(b.n_wfs)], np.int64)
    pre, pre_out, sb = _split(b, cut, engine_gpu.replay)
    sref = oracle.replay(sb)
    assert all(sref.result[w].code == abi.OK for w in range(b.n_wfs))
    _assert_equal(sb, engine_gpu.replay(sb), sref, "healed by the load")
    with _Knobs(engine_gpu, reg=False):
        _assert_equal(sb, engine_gpu.replay(sb), sref, "healed by the load, general kernel")
