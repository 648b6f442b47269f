"""Every task stateBuilder.applyEvents emits, hand-derived (the `xfer` / `ttask` lists of
tests/effect_cases.py), on the CPU restatement and on every task-emitting kernel route.

CPU: the oracle's transfer and timer task lists of every instance (case x builder, the
continue-as-new runs included) must equal the lists written by hand from the reference's Go —
every field, the counts and the order; meta-tests hold the table to its coverage (every append
site of stateBuilder.go reached, every cdr_task_type present, every field of cdr_task with two
expected values) and prove that the comparer sees every field, a dropped record and a swapped
pair.  At every call boundary the prefix must emit exactly the records whose `by` event lies
before the cut and the suffix, replayed onto the loaded state, exactly the others; loaded rows
patched by hand (CARRY_CASES) pin what the picks read from a row.

GPU: the same lists on every route of tests/test_effect_sites.TASK_ROUTES, on the fast-path
kernel (claimed from the slice plan) and with it off, on the class kernel with and without the
register-table pass behind it, on both carry kernels at every call boundary and on the
hand-patched rows, at the edges of a slice, and into device buffers pre-filled with 0xA5.
A difference names the case, the builder kind, the list and the field.
"""
import ctypes as C
import re

import pytest

import oracle
from cadence_amd import abi, engine
from tests import effect_cases as EC
from tests import fault_cases as FC
from tests.test_capacity import _canary, _run_sliced
from tests.test_effect_sites import (DENSE_AT, TASK_ROUTES, _assert_carry_plan, _assert_carry_states,
                                     _assert_hand_states, _assert_lane_placement, _carry_batches, _cut_rounds,
                                     _lane_batch, _table, _taken)
from tests.test_fault_sites import DEFAULT_MODE, ROUTES, _assert_equal, _entry_slices, _force_reg, _Knobs, _label, _split
from tests.test_fault_sites import TASK_ROUTES as SLICED_TASK_ROUTES

TASK_FIELDS = [f for f, _ in abi.CdrTask._fields_ if not f.startswith("_pad")]
# the append sites of stateBuilder.applyEvents (stateBuilder.go)
SITES = ["sb:173", "sb:174", "sb:196", "sb:210", "sb:235", "sb:253", "sb:265", "sb:267", "sb:276", "sb:285", "sb:294",
         "sb:303", "sb:317", "sb:330", "sb:339", "sb:348", "sb:370", "sb:421", "sb:452", "sb:535", "sb:576-577",
         "sb:780", "sb:785"]


def _replay_tasks(b, pl=None):
    return oracle.replay(b, pl, tasks=True)


def _want_tasks(entries):
    """{entry index: the hand-written lists} of a build_batch(), `by` included."""
    want = {}
    for k, (c, bld, w, nr) in enumerate(entries):
        want[w] = c.tasks(bld, k)
        if nr is not None:
            want[nr] = c.new_run_tasks(bld, k)
    return want


def _names(entries):
    names = {w: _label(c, bld) for c, bld, w, nr in entries}
    names.update({nr: _label(c, bld) + " new run" for c, bld, w, nr in entries if nr is not None})
    return names


def _diff_tasks(b, out, want, names):
    """['<case>[<builder>] .<list>[j].<field>: want != got', ...] over the entries of `want`."""
    return [f"{names[w]} {d}" for w, lists in want.items() for d in EC.task_diff(lists, EC.exported_tasks(b, out, w))]


def _assert_hand_tasks(b, entries, out, what, only=None):
    want = _want_tasks(entries)
    if only is not None:
        want = {w: v for w, v in want.items() if w in only}
    bad = _diff_tasks(b, out, want, _names(entries))
    assert not bad, what + ":\n" + "\n".join(bad[:20])
    return len(want)


def _all_cases():
    return EC.CASES + [EC.SPARSE_TWIN]


def _all_expected_lists():
    """Every expected pair of lists: the table's instances, their new runs, the carry-in
    instances and the lane filler."""
    b, entries, pl, ref = _table()
    lists = list(_want_tasks(entries).values())
    lists += [c.tasks(bld, 0) for c in EC.CARRY_CASES + [EC.SPARSE_TWIN] for bld in FC.ALL]
    return lists


# ====================================================================== CPU: the table itself
def test_task_table_shape():
    """Every case states both lists; every record states exactly the non-pad fields of
    abi.CdrTask plus `by`; `by` names an event of the history and never decreases along a list
    (a list is in emission order); every case with tasks of its own cites sb: or tb: lines; the
    batch stays within 256 entries of at most 40 events."""
    for c in _all_cases():
        specs = [(c.spec, [e for call in c.calls for e in call])]
        if c.new_run_spec is not None:
            specs.append((c.new_run_spec, c.new_run))
        assert c.n_events() <= 40, c.name
        for spec, events in specs:
            assert spec.xfer is not None and spec.ttask is not None, c.name
            ids = {e["eventId"] for e in events}
            lists = spec.tasks(c.ctx(FC.L, 0))
            for kind in EC.TASK_LISTS:
                for r in lists[kind]:
                    assert sorted(r) == sorted(TASK_FIELDS + ["by"]), (c.name, kind)
                    assert r["by"] in ids, (c.name, kind, r["by"])
                    assert (r["type"] >= 16) == (kind == "ttask") and r["type"] in abi.TASK_TYPES, (c.name, kind)
                by = [r["by"] for r in lists[kind]]
                assert by == sorted(by), (c.name, kind)
            if spec.xfer or spec.ttask:
                assert re.search(r"\b(sb|tb):\d+", c.doc), c.name
    for cc in EC.CARRY_CASES:
        assert cc.spec.head is None and cc.spec.xfer is not None and cc.spec.ttask is not None, cc.name
        assert re.search(r"\b(sb|tb):\d+", cc.doc) or not (cc.spec.xfer or cc.spec.ttask), cc.name
        for kind, rows in cc.tasks(FC.L, 0).items():
            assert all(sorted(r) == sorted(TASK_FIELDS + ["by"]) and r["by"] == cc.suffix[0]["eventId"] for r in rows)
    b, entries, pl, ref = _table()
    assert b.n_wfs <= 256
    assert all(re.search(r"\b(sb|tb):\d+", why) for why in EC.TASK_CONSTANT.values())


def test_task_lists_do_not_depend_on_the_builder():
    """stateBuilder's tasks carry no version (schema.h:564-566) and read nothing of the
    replication state or the version histories: the three builder kinds of a case expect the
    same lists."""
    for c in _all_cases():
        lists = [c.tasks(bld, 0) for bld in FC.ALL]
        assert lists[0] == lists[1] == lists[2], c.name
    for cc in EC.CARRY_CASES:
        lists = [cc.tasks(bld, 0) for bld in FC.ALL]
        assert lists[0] == lists[1] == lists[2], cc.name


def test_every_append_site_has_a_case_and_every_task_type_occurs():
    assert sorted(EC.TASK_SITES) == sorted(SITES)
    for site, (etypes, ttypes, names) in EC.TASK_SITES.items():
        assert names, site
        for name in names:
            c = EC.by_name(name)
            etype = {e["eventId"]: e["eventType"] for call in c.calls for e in call}
            if site == "sb:576-577":  # the new run's own lists
                nr = c.new_run_tasks(FC.N, 0)
                assert nr["xfer"] and nr["ttask"] and set(etype.values()) & set(etypes), name
                continue
            lists = c.tasks(FC.L, 0)
            hit = [r for kind in EC.TASK_LISTS for r in lists[kind] if r["type"] in ttypes and etype[r["by"]] in etypes]
            assert hit, (site, name)
    # each close event type reaches appendTasksForFinishedExecutions in some case of sb:780 / 785
    for site in ("sb:780", "sb:785"):
        closing = set()
        for name in EC.TASK_SITES[site][2]:
            c = EC.by_name(name)
            etype = {e["eventId"]: e["eventType"] for call in c.calls for e in call}
            closing |= {etype[r["by"]] for kind in EC.TASK_LISTS for r in c.tasks(FC.L, 0)[kind]
                        if r["type"] in EC.TASK_SITES[site][1]}
        assert closing == set(EC.TASK_SITES[site][0]), site
    seen = {r["type"] for lists in _all_expected_lists() for kind in EC.TASK_LISTS for r in lists[kind]}
    assert seen == set(abi.TASK_TYPES), sorted(set(abi.TASK_TYPES) ^ seen)


def test_every_task_field_takes_two_expected_values():
    """No field of cdr_task passes by being constant: outside TASK_CONSTANT each takes at
    least two distinct hand-written values in the table."""
    seen = {f: set() for f in TASK_FIELDS}
    for lists in _all_expected_lists():
        for kind in EC.TASK_LISTS:
            for r in lists[kind]:
                for f in TASK_FIELDS:
                    seen[f].add(repr(r[f]))
    flat = sorted(f"CdrTask.{f}" for f, vals in seen.items() if len(vals) < 2)
    assert flat == sorted(EC.TASK_CONSTANT), flat


def test_required_task_edges_are_in_the_table():
    """The edges where the state can be right while the task is wrong, by what the hand-written
    lists say."""
    def rows(name, kind, type_):
        return [r for r in EC.by_name(name).tasks(FC.L, 0)[kind] if r["type"] == type_]
    # backoff before timeout, both types, the timeout pushed out
    for name, tt in (("started_backoff_cron", EC.BACKOFF_CRON), ("started_backoff_retry", EC.BACKOFF_RETRY)):
        t = EC.by_name(name).tasks(FC.L, 0)["ttask"]
        assert [r["type"] for r in t[:2]] == [EC.T_BACKOFF, EC.T_WF_TIMEOUT] and t[0]["timeout_type"] == tt
        assert t[1]["visibility_ts"] - t[0]["visibility_ts"] == 100 * EC.S
    # the transient decision's ScheduleID and the started one's timeout
    assert [r["event_id"] for r in rows("transient_decision_started", "xfer", EC.T_DECISION)] == [2, 4]
    assert [(r["event_id"], r["attempt"]) for r in rows("transient_decision_started", "ttask", EC.T_DECISION_TIMEOUT)] == \
        [(2, 0), (4, 0)]
    # every activity timeout type occurs; a heartbeat and a start-to-close winner; a nonzero attempt
    at = [r for lists in _all_expected_lists() for r in lists["ttask"] if r["type"] == EC.T_ACTIVITY_TIMEOUT]
    assert {r["timeout_type"] for r in at} == {EC.STC, EC.S2S, EC.S2C, EC.HB}
    assert {r["attempt"] for r in at} == {0, 3}
    # child-only true and false on both external tasks; an empty TargetRunID on the child task only
    for t in (EC.T_CANCEL, EC.T_SIGNAL):
        flags = {r["flags"] for lists in _all_expected_lists() for r in lists["xfer"] if r["type"] == t}
        assert flags == {0, EC.CHILD_ONLY}
    ext = [r for lists in _all_expected_lists() for r in lists["xfer"] if r["type"] in (EC.T_CHILD, EC.T_CANCEL, EC.T_SIGNAL)]
    assert all((r["target_run_id"] == "") == (r["type"] == EC.T_CHILD) for r in ext)
    own = EC.by_name("ext_own_domain").tasks(FC.L, 0)["xfer"]
    assert own[1]["domain_id"] == own[2]["domain_id"] == "id-of-home"  # the DecisionTask's and the child's
    # two upserts: two tasks; retention 0, 1 and 3 days
    assert len(rows("sa_start_and_upserts", "xfer", EC.T_UPSERT)) == 2
    days = {(r["visibility_ts"] - EC.T(r["by"])) // EC.DAY for lists in _all_expected_lists() for r in lists["ttask"]
            if r["type"] == EC.T_DELETE_HISTORY}
    assert days == {0, 1, 3}
    # a close is the last of both lists
    for name in EC.TASK_SITES["sb:780"][2]:
        lists = EC.by_name(name).tasks(FC.L, 0)
        assert lists["xfer"][-1]["type"] == EC.T_CLOSE and lists["ttask"][-1]["type"] == EC.T_DELETE_HISTORY, name
    # CARRY_CASES: one emits for a loaded row, one emits nothing, one carries the row's attempt
    by_name = {cc.name: cc.tasks(FC.L, 0) for cc in EC.CARRY_CASES}
    assert by_name["carry_status_bit_cleared"]["ttask"][0]["attempt"] == 3
    assert by_name["carry_status_bit_set"] == {"xfer": [], "ttask": []}
    assert by_name["carry_expiration_before_schedule_to_close"]["ttask"][0]["visibility_ts"] == EC.NOW + 5 + 12 * EC.S
    assert by_name["carry_timer_task_id_cleared"]["ttask"][0]["event_id"] == 5


# ====================================================================== CPU: the oracle against the table
def test_oracle_gives_the_hand_written_task_lists():
    b, entries, pl, ref = _table()
    assert all(ref.result[w].code == abi.OK for w in range(b.n_wfs))
    n = _assert_hand_tasks(b, entries, ref, "oracle")
    assert n == b.n_wfs > 150 and any(nr is not None for c, bld, w, nr in entries)


def _mutated(rec, f, strings):
    v = getattr(rec, f)
    if f in engine._HANDLE_FIELDS:
        return (v + 1) % len(strings)
    return v ^ 1


def test_task_comparer_sees_every_field():
    """One record of each list of an oracle output (the dense case's CancelExecution task, which
    sets every handle, and its first ActivityTimeout): changing each field in turn, dropping the
    record and swapping it with its neighbour must each produce a diff that names the list — and,
    for a field, the field.  Everything is restored afterwards."""
    b, entries, pl, ref = _table()
    c, bld, w, nr = next(e for e in entries if e[0].name == "dense_all_tables")
    k = entries.index((c, bld, w, nr))
    want = c.tasks(bld, k)

    def bad():
        return EC.task_diff(want, EC.exported_tasks(b, ref, w))
    assert not bad()
    n = 0
    for kind, j in (("xfer", 4), ("ttask", 2)):
        rowsj = ref.task_rows(w, kind)
        target, other = rowsj[j], rowsj[j + 1]
        assert want[kind][j]["type"] == (EC.T_CANCEL if kind == "xfer" else EC.T_ACTIVITY_TIMEOUT)
        saved, saved_other = bytes(memoryview(target).cast("B")), bytes(memoryview(other).cast("B"))
        for f in TASK_FIELDS:
            setattr(target, f, _mutated(target, f, b.strings))
            try:
                d = bad()
            finally:
                C.memmove(C.addressof(target), saved, len(saved))
            assert d and all(x.startswith(f".{kind}[{j}].{f}:") for x in d), (kind, f, d)
            n += 1
        # swapped with the next record
        C.memmove(C.addressof(target), saved_other, len(saved))
        C.memmove(C.addressof(other), saved, len(saved))
        try:
            d = bad()
        finally:
            C.memmove(C.addressof(target), saved, len(saved))
            C.memmove(C.addressof(other), saved_other, len(saved))
        assert any(x.startswith(f".{kind}[{j}].") for x in d) and any(x.startswith(f".{kind}[{j + 1}].") for x in d)
        # the last record dropped
        slot = 2 * w + (0 if kind == "xfer" else 1)
        ref.tasks["n"][slot] -= 1
        try:
            d = bad()
        finally:
            ref.tasks["n"][slot] += 1
        assert d == [f".{kind}: {len(want[kind])} rows expected, {len(want[kind]) - 1} got"]
        assert not bad()
    assert n == 2 * len(TASK_FIELDS)


def test_removing_or_changing_a_hand_written_record_is_noticed():
    """The other direction: one record dropped from, or one field changed in, the expected lists
    of every instance differs from what the oracle gives."""
    b, entries, pl, ref = _table()
    n = 0
    for w, lists in _want_tasks(entries).items():
        got = EC.exported_tasks(b, ref, w)
        for kind in EC.TASK_LISTS:
            for j, r in enumerate(lists[kind]):
                less = dict(lists, **{kind: lists[kind][:j] + lists[kind][j + 1:]})
                assert EC.task_diff(less, got), (w, kind, j)
                for f in TASK_FIELDS:
                    v = r[f] + "x" if isinstance(r[f], str) else r[f] + 1
                    other = dict(lists, **{kind: lists[kind][:j] + [dict(r, **{f: v})] + lists[kind][j + 1:]})
                    assert EC.task_diff(other, got) == [f".{kind}[{j}].{f}: {v!r} != {r[f]!r}"], (w, kind, j, f)
                n += 1
    assert n > 1000


# ---------------------------------------------------------------- carry-in at every call boundary
def _first_suffix_event(b, w, cut):
    return b.events[b.wfs[w].ev_off + int(cut[w])].event_id


def _assert_task_split(b, entries, cut, pre, pre_out, sb, suf_out, what):
    """The prefix's lists are the records whose `by` lies before the cut, the suffix's the
    others, and the two concatenated are the full hand-written lists.  An entry that is not cut
    replays whole in both; a new run the prefix never reaches is not applied and reports no
    tasks, and the suffix replays it whole."""
    want, names = _want_tasks(entries), _names(entries)
    want_pre, want_suf = {}, {}
    for w, lists in want.items():
        parent = b.wfs[w].parent
        if cut[w] > 0:
            want_pre[w], want_suf[w] = EC.split_by(lists, _first_suffix_event(b, w, cut))
        elif parent >= 0 and cut[parent] > 0:
            assert pre_out.result[w].code != abi.OK, names[w]
            assert pre_out.tasks["n"][2 * w] == 0 and pre_out.tasks["n"][2 * w + 1] == 0, names[w]
            want_suf[w] = lists
        else:
            want_pre[w] = want_suf[w] = lists
    bad = _diff_tasks(pre, pre_out, want_pre, names)
    assert not bad, what + ", prefix:\n" + "\n".join(bad[:20])
    bad = _diff_tasks(sb, suf_out, want_suf, names)
    assert not bad, what + ", suffix:\n" + "\n".join(bad[:20])
    n = 0
    for w in want:
        if cut[w] > 0:
            p, s = EC.exported_tasks(pre, pre_out, w), EC.exported_tasks(sb, suf_out, w)
            both = {kind: p[kind] + s[kind] for kind in EC.TASK_LISTS}
            assert not EC.task_diff(want[w], both), names[w]
            n += 1
    return n


def test_oracle_task_carry_in_at_every_call_boundary():
    b, entries, pl, full = _table()
    n = 0
    for j, cut in enumerate(_cut_rounds(b, entries)):
        pre, pre_out, sb = _split(b, cut, _replay_tasks)
        n += _assert_task_split(b, entries, cut, pre, pre_out, sb, _replay_tasks(sb), f"cut before call {j + 1}")
    assert n > 300


def _assert_carry_tasks(sb, entries, out, what):
    bad = []
    for k, (s, bld, w, nr) in enumerate(entries):
        bad += [f"{_label(s, bld)} {d}" for d in EC.task_diff(s.case.tasks(bld, k), EC.exported_tasks(sb, out, w))]
    assert not bad, what + ":\n" + "\n".join(bad[:20])


def test_oracle_tasks_onto_hand_set_rows():
    """EC.CARRY_CASES: the suffix's lists on rows patched by hand — and the unpatched twin of
    each patch that changes a pick emits something else, so the patch is what the lists show."""
    sb, entries = _carry_batches(oracle.replay)
    _assert_carry_plan(sb, {w: s.name for s, bld, w, nr in entries})
    out = _replay_tasks(sb)
    _assert_carry_states(sb, entries, out, "oracle")
    _assert_carry_tasks(sb, entries, out, "oracle")
    # the unpatched loaded state: the same suffix on the prefix as replayed
    import numpy as np
    b, _ = EC.build_batch([(s, bld) for s, bld, w, nr in entries])
    cut = np.array([engine._calls(b, w)[-1] for w in range(b.n_wfs)], np.int64)
    pre, pre_out, plain_sb = _split(b, cut, oracle.replay)
    plain = _replay_tasks(plain_sb)
    changed = {s.name for k, (s, bld, w, nr) in enumerate(entries)
               if EC.task_diff(s.case.tasks(bld, k), EC.exported_tasks(plain_sb, plain, w))}
    assert changed == {"carry_status_bit_cleared", "carry_status_bit_set", "carry_expiration_before_schedule_to_close",
                       "carry_timer_task_id_cleared"}


# ---------------------------------------------------------------- lane placement
N_DENSE, N_SPARSE = (7, 5), (6, 4)   # (transfer, timer) records of dense_all_tables and of its sparse twin


def _assert_lane_tasks(b, entries, out, what):
    _assert_hand_tasks(b, entries, out, what)
    for w in range(128):
        n = (int(out.tasks["n"][2 * w]), int(out.tasks["n"][2 * w + 1]))
        assert n == (N_DENSE if w in DENSE_AT else N_SPARSE), (what, w, n)
        if w not in DENSE_AT:  # none of the records only the dense entry has
            assert not any(r.type == EC.T_UPSERT for r in out.task_rows(w, "xfer")), (what, w)
            assert not any(r.type == EC.T_ACTIVITY_TIMEOUT and r.timeout_type == EC.STC
                           for r in out.task_rows(w, "ttask")), (what, w)


def test_oracle_tasks_on_the_lane_batch():
    b, entries = _lane_batch()
    pl = engine.plan(b)
    _assert_lane_placement(b, pl)
    _assert_lane_tasks(b, entries, _replay_tasks(b, pl), "oracle")


# ====================================================================== GPU
@pytest.mark.gpu
@pytest.mark.parametrize("route", list(TASK_ROUTES))
def test_gpu_task_route(engine_gpu, route):
    """The table's batch with task lists on one route: the state assertions of
    test_effect_sites.test_gpu_route stay, and the route's lists equal the hand-written ones —
    not only the oracle's."""
    r = dict(ROUTES[route])
    force = r.pop("force", "none")
    b, entries, pl, ref = _table()
    p = pl if force == "none" else _force_reg(pl, b.n_wfs, force)
    with _Knobs(engine_gpu, **r):
        got = engine_gpu.replay(b, p, tasks=True)
    _assert_hand_states(b, entries, got, route + ", tasks", repl=False)
    assert _assert_hand_tasks(b, entries, got, route) == b.n_wfs
    _assert_equal(b, got, ref, route + ", tasks", tasks=True)


@pytest.mark.gpu
def test_gpu_fast_route_claim_with_tasks(engine_gpu):
    """In the task plan (lane slices only) the CDR_CAP_FAST instances sit in CDR_SLICE_FAST
    slices — k_replay_fast<TASKS> emits their lists — and they give the hand-written lists with
    the fast path on and off."""
    b, entries, pl, ref = _table()
    nf, ns = engine.fast_slices(b, pl)
    kind, _ = _entry_slices(b, pl, 0)
    on = {w for c, bld, w, nr in entries if pl.caps[w].flags & abi.CAP_FAST}
    print(f"fast-path instances in the task plan: {len(on)} in {nf} of {ns} slices")
    assert nf > 0 and len(on) > 0, f"{len(on)} fast-path instances"
    assert all(kind[w] == abi.SLICE_FAST for w in on)
    for fast in (True, False):
        with _Knobs(engine_gpu, fast=fast):
            got = engine_gpu.replay(b, pl, tasks=True)
        assert _assert_hand_tasks(b, entries, got, f"fast path {fast}", only=on) == len(on)
        _assert_hand_tasks(b, entries, got, f"fast path {fast}, every instance")


@pytest.mark.gpu
def test_gpu_class_kernel_with_tasks(engine_gpu):
    """k_replay_cls<TASKS> staging + k_tasks_merge: with the register-table pass behind it
    (CLS_BUILD) every instance has the hand-written lists; alone (CLS_ALONE) every instance it
    keeps has them, and it keeps at least half of the register-table instances."""
    b, entries, pl, ref = _table()
    with _Knobs(engine_gpu, cls=abi.CLS_BUILD):
        got = engine_gpu.replay(b, pl, tasks=True)
    _assert_hand_states(b, entries, got, "CLS_BUILD, tasks", repl=False)
    assert _assert_hand_tasks(b, entries, got, "CLS_BUILD") == b.n_wfs
    with _Knobs(engine_gpu, cls=abi.CLS_ALONE):
        alone = engine_gpu.replay(b, pl, tasks=True)
    retried = {w for w in range(b.n_wfs) if alone.result[w].code == abi.CLS_RETRY}
    skip = retried | {w for w in range(b.n_wfs) if b.wfs[w].parent in retried}
    kept = set(range(b.n_wfs)) - skip
    reg_taken, _ = _taken("reg")
    print(f"class kernel alone, tasks: keeps {len(reg_taken - retried)} of {len(reg_taken)} register-table instances")
    assert all(alone.result[w].code == abi.OK for w in kept)
    assert _assert_hand_tasks(b, entries, alone, "CLS_ALONE", only=kept) == len(kept)
    assert all(alone.tasks["n"][2 * w] == 0 and alone.tasks["n"][2 * w + 1] == 0 for w in retried)
    assert kept and 2 * len(reg_taken - retried) >= len(reg_taken)


@pytest.mark.gpu
def test_gpu_task_carry_in_at_every_call_boundary(engine_gpu):
    """The cuts of the CPU test on the GPU's own prefix, with tasks=True: the prefix's lists
    and, on the register-table carry kernel and on the general kernel's carry prologue, the
    suffix's lists equal the `by` split of the hand-written lists."""
    b, entries, pl, ref = _table()
    names = {w: c.name for c, bld, w, nr in entries}
    for j, cut in enumerate(_cut_rounds(b, entries)):
        pre, pre_out, sb = _split(b, cut, lambda x: engine_gpu.replay(x, tasks=True))
        _assert_carry_plan(sb, names)
        for reg in (True, False):
            with _Knobs(engine_gpu, reg=reg):
                got = engine_gpu.replay(sb, tasks=True)
            what = f"cut before call {j + 1}, " + ("register-table carry kernel" if reg else "general kernel")
            _assert_task_split(b, entries, cut, pre, pre_out, sb, got, what)
            _assert_hand_states(sb, entries, got, what, repl=False)


@pytest.mark.gpu
def test_gpu_tasks_onto_hand_set_rows(engine_gpu):
    """EC.CARRY_CASES with tasks on the GPU's own prefix, both carry kernels."""
    sb, entries = _carry_batches(engine_gpu.replay)
    _assert_carry_plan(sb, {w: s.name for s, bld, w, nr in entries})
    for reg in (True, False):
        with _Knobs(engine_gpu, reg=reg):
            got = engine_gpu.replay(sb, tasks=True)
        _assert_carry_states(sb, entries, got, f"reg={reg}", repl=False)
        _assert_carry_tasks(sb, entries, got, f"reg={reg}")


@pytest.mark.gpu
def test_gpu_lane_placement_with_tasks(engine_gpu):
    """The dense entry at slice 0 lane 0, slice 0 lane 63 and slice 1 lane 0 has the dense
    lists; every neighbour has exactly the sparse twin's and none of the dense records; the
    counts of all 128 entries."""
    b, entries = _lane_batch()
    pl = engine.plan(b)
    _assert_lane_placement(b, pl)
    _assert_lane_tasks(b, entries, engine_gpu.replay(b, pl, tasks=True), "default route")


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(SLICED_TASK_ROUTES))
def test_gpu_task_slices_in_prefilled_buffers(engine_gpu, route):
    """tasks=True into device buffers filled with 0xA5 (test_capacity._run_sliced): the lists
    equal the table; nothing is written past an entry's n_tasks within its capacity slice; the
    pad field of every emitted record is zero."""
    b, entries, pl, ref = _table()
    got = _run_sliced(engine_gpu, b, pl, tasks=True, **SLICED_TASK_ROUTES[route])
    assert _assert_hand_tasks(b, entries, got, route) == b.n_wfs
    n = 0
    for w in range(b.n_wfs):
        c = pl.caps[w]
        for kind, off, cap, k in (("xfer", c.xfer_off, c.xfer_cap, 0), ("ttask", c.ttask_off, c.ttask_cap, 1)):
            cnt = int(got.tasks["n"][2 * w + k])
            assert cnt <= cap and _canary(got, kind, off + cnt, off + cap), (w, kind)
            assert all(getattr(r, "_pad") == 0 for r in got.task_rows(w, kind)), (w, kind)
            n += cnt
    assert n > 1000
