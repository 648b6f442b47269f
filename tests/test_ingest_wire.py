"""The device thrift decoder (csrc/ingest.hip, cdr_ingest_decode) on hand-built wire
edges (tests/thrift_cases.py): what a newer server, a storage fault or a foreign
serializer sends and the synthetic encoder never writes.

CPU: the cases through the restatement (oracle/thrift_decode.py) only — the builder's
well-formed blobs decode to the intended records, each family's statuses are the expected
ones, and the expected records are stated independently of the decoder under test: an
unknown field changes nothing, a field of another wire type is an absent field, a
repeated field is its last occurrence (the generated FromWire assigns each occurrence in
turn and replaces a struct-valued field whole).

GPU: each family as one batch of many blobs, device == restatement record for record
(`assert_same_decode` of tests/test_ingest.py; strict, the string table included, for
every well-formed blob; by string where a field is repeated or the bytes are corrupt)."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

from cadence_amd import abi, ingest
from oracle import thrift_decode as TD
from tests import thrift_cases as TC
from tests.test_ingest import _by_string, assert_same_decode, oracle_decode

STAGE = 12288  # CDR_INGEST_STAGE (csrc/ingest.hip): bytes of one wavefront's blobs staged in LDS
SEEDS = [b"", b"emptyUuid", b"pdom", b"pdom-id", b"cdom", b"cdom-id"]
DOMAINS = [(2, 3), (4, 5)]


def batch(blobs, seeds=SEEDS, domain_map=DOMAINS, entry_blob0=None):
    """Blobs as one decode input; by default one entry per blob."""
    off = np.zeros(len(blobs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blobs]) if blobs else []
    e0 = np.arange(len(blobs) + 1, dtype=np.uint32) if entry_blob0 is None else np.array(entry_blob0, np.uint32)
    return ingest.Encoded(np.frombuffer(b"".join(blobs) or b"\0", np.uint8).copy(), off, e0, list(seeds), {},
                          list(domain_map))


def rp_by_string(p, strings):
    return (strings[p.binary_checksum], strings[p.run_id], p.first_decision_completed_id, p.created_time_nano,
            p.expiring_time_nano, p.flags)


def records(ref, by_string=False, drop=()):
    """A decode (the restatement's tuple) as comparable values."""
    ev, kvs, rps, ev_off, st, est, strings = ref
    if not by_string:
        return ([bytes(e) for e in ev], [tuple(k) for k in kvs], [bytes(p) for p in rps], list(map(int, ev_off)),
                list(st), list(est), list(strings))
    evs = [{k: v for k, v in _by_string(e, strings).items() if k not in drop} for e in ev]
    return (evs, [(strings[a], strings[b]) for a, b in kvs], [rp_by_string(p, strings) for p in rps],
            list(map(int, ev_off)), list(st), list(est))


def no_off(d):
    """An event by string without its row offsets (they depend on the blobs before it)."""
    return {k: v for k, v in d.items() if k not in ("search_attr_off", "reset_points_off")}


def union_types(enc, status):
    """Per event of every decoded blob: the event type whose attribute struct is the last
    one the event carries (None: it carries none the record form keeps)."""
    data = enc.blob_bytes.tobytes()
    out = []
    for b, st in enumerate(status):
        if st != TD.DEC_OK:
            continue
        hist = TD.Reader(data, int(enc.blob_off[b]) + 1, int(enc.blob_off[b + 1])).value(TD.T_STRUCT, 0, "history")
        for ev in TD.fget(hist, 10, TD.T_LIST)[0][2]:
            attr = [fid for fid, ft, v, span in ev[1] if ft == TD.T_STRUCT and 40 <= fid <= 450 and fid % 10 == 0]
            out.append(abi.EV[TC.ATTR_TYPE[attr[-1]]] if attr and attr[-1] in TC.ATTR_TYPE else None)
    return out


def by_union(e, strings, etype):
    """`_by_string` of the union member the attribute struct filled, whatever the
    (corrupted) eventType says: a union read as another member would take plain numbers
    for handles, and these depend on the numbering."""
    if etype is None:
        return {"hdr": bytes(e)[:40], "union": bytes(e)[40:]}
    c = type(e).from_buffer_copy(bytes(e))
    c.type = etype
    return _by_string(c, strings) | {"hdr": bytes(e)[:40]}


def check_gpu(eng, enc, ref=None, by_string=False, corrupt=False, **kw):
    """Device decode == restatement; by string the reset-point rows and every row count too
    (assert_same_decode compares events and kv rows there).  `corrupt`: the same by-string
    comparison with each event's union read as the member its attribute struct filled."""
    ref = oracle_decode(enc) if ref is None else ref
    d = ingest.decode(eng, enc, **kw)
    if corrupt:
        ev, kvs, rps, ev_off, st, est, strings = ref
        assert list(d.blob_status) == list(st) and list(d.entry_status) == list(est)
        assert list(d.ev_off) == list(ev_off) and len(d.events) == len(ev)
        ut = union_types(enc, st)
        assert len(ut) == len(ev)
        bad = [i for i in range(len(ev)) if by_union(d.events[i], d.strings, ut[i]) != by_union(ev[i], strings, ut[i])]
        assert not bad, (len(bad), bad[:5], by_union(d.events[bad[0]], d.strings, ut[bad[0]]), by_union(ev[bad[0]], strings, ut[bad[0]]))
        assert [(d.strings[k.key], d.strings[k.value]) for k in d.kvs] == [(strings[a], strings[b]) for a, b in kvs]
    else:
        assert_same_decode(d, ref, by_string=by_string)
    assert (len(d.kvs), len(d.rps)) == (len(ref[1]), len(ref[2]))
    assert [rp_by_string(p, d.strings) for p in d.rps] == [rp_by_string(p, ref[6]) for p in ref[2]]
    return d


def statuses(cases):
    return [c[2] for c in cases]


# ------------------------------------------------------------------ the builder itself
@functools.lru_cache(None)
def families_decoded():
    return oracle_decode(batch([TC.blob(TC.history(TC.family_events()))]))


def test_builder_events_decode_to_the_intended_records():
    ev, kvs, rps, ev_off, st, est, S = families_decoded()
    assert st == [0] and len(ev) == len(TC.FAMILIES) and ev_off == [0, len(ev)]
    assert [e.event_id for e in ev] == list(range(1, len(ev) + 1))
    assert [abi.EVENT_TYPES[e.type] for e in ev][:3] == ["WorkflowExecutionStarted", "DecisionTaskScheduled",
                                                          "DecisionTaskStarted"]
    assert ev[0].flags == abi.EVF_BATCH_FIRST and all(e.flags == 0 for e in ev[1:])
    s = ev[0].a.started
    assert (S[s.workflow_type], S[s.task_list], S[s.parent_workflow_id], S[s.parent_run_id], S[s.continued_run_id],
            S[s.cron_schedule]) == (b"wt", b"tl", b"pw", b"pr", b"crun", b"* * * * *")
    assert (s.parent_domain_id, s.parent_initiated_id, s.exec_timeout_s, s.task_timeout_s, s.attempt, s.expiration_ts,
            s.first_decision_backoff_s) == (3, 3, 3600, 10, 1, 1_700_000_000, 30)
    want = (abi.SF_HAS_PARENT_DOMAIN | abi.SF_HAS_PARENT_EXEC | abi.SF_HAS_PARENT_INITIATED | abi.SF_HAS_INITIATOR |
            abi.SF_CRON_INITIATOR | abi.SF_HAS_RETRY | abi.SF_HAS_MEMO | abi.SF_HAS_SEARCH_ATTR | abi.SF_HAS_RESET_POINTS)
    assert s.flags == want
    assert (s.retry_initial_s, s.backoff_coefficient, s.retry_max_interval_s, s.retry_max_attempts,
            s.retry_expiration_s) == (2, 1.5, 60, 5, 600)
    assert S[s.nonretriable] == TC.value(TC.T_LIST, TC.Lst(TC.T_STRING, [b"bad", b"worse"]))
    assert S[s.memo] == TC.value(TC.T_STRUCT, TC.memo(120).v)
    assert [(S[k], S[v]) for k, v in kvs[s.search_attr_off:s.search_attr_off + s.search_attr_len]] == [
        (b"k1", b"v1"), (b"k2", b"v2")]
    assert [rp_by_string(p, S) for p in rps] == [
        (b"ck0", b"rr0", 4, 10**18, 2 * 10**18, 0x3F | abi.RP_RESETTABLE), (b"ck1", b"rr1", 5, 10**18 + 1, 2 * 10**18 + 1, 0x3F)]
    by = {abi.EVENT_TYPES[e.type]: e for e in ev}
    a = by["ActivityTaskScheduled"].a.at_sched
    assert (S[a.activity_id], S[a.task_list], a.s2c_s, a.s2s_s, a.stc_s, a.hb_s, a.retry_max_attempts, a.nonretriable) == (
        b"act-1", b"atl", 100, 20, 80, 5, 5, 0)
    x = by["StartChildWorkflowExecutionInitiated"].a.ext
    assert (S[x.domain], x.target_domain_id, S[x.workflow_id], S[x.workflow_type], S[x.input], S[x.control],
            x.parent_close_policy, x.flags) == (b"cdom", 5, b"child-wf", b"cwt", b"cin", b"cctl", 1, 0)
    x = by["SignalExternalWorkflowExecutionInitiated"].a.ext
    assert (S[x.domain], S[x.workflow_id], S[x.run_id], S[x.signal_name], S[x.input], S[x.control], x.flags) == (
        b"sdom", b"sw", b"sr", b"sig", b"sin", b"sctl", abi.XF_CHILD_ONLY | abi.XF_DOMAIN_MISSING)
    assert (by["ChildWorkflowExecutionCompleted"].a.ref.initiated_event_id,
            S[by["ChildWorkflowExecutionCompleted"].a.ref.run_id]) == (3, b"child-run")
    assert (S[by["TimerStarted"].a.timer.timer_id], by["TimerStarted"].a.timer.start_to_fire_s) == (b"timer-1", 30)
    assert S[by["DecisionTaskCompleted"].a.dt.binary_checksum] == b"cksum"
    assert S[by["WorkflowExecutionContinuedAsNew"].a.can.new_execution_run_id] == b"new-run"
    u = by["UpsertWorkflowSearchAttributes"].a.upsert
    assert [(S[k], S[v]) for k, v in kvs[u.search_attr_off:u.search_attr_off + u.search_attr_len]] == [
        (b"k1", b"v9"), (b"k3", b"v3")]
    assert not any(bytes(by["WorkflowExecutionCompleted"])[40:])  # an attribute struct the record does not keep
    assert not any(b"not-kept" in x for x in S)


# ------------------------------------------------------------------ (a) forward compatibility
@functools.lru_cache(None)
def forward():
    cases = TC.forward_compat_cases()
    return cases, batch([c[0][1] for c in cases]), batch([c[1] for c in cases])


def test_unknown_fields_change_nothing_oracle():
    """An unknown field of any wire type, anywhere in any struct the decoder walks: status
    OK and the records of the same blob without it (inside Memo, which is kept as its
    bytes: the memo string is the Memo with the field, everything else equal)."""
    cases, enc, plain = forward()
    assert len(cases) > 500 and {c[2] for c in cases} >= {"History", "HistoryEvent", "attr40", "WorkflowType",
                                                           "TaskList", "WorkflowExecution", "RetryPolicy",
                                                           "SearchAttributes", "ResetPoints", "ResetPointInfo", "Memo"}
    got, want = oracle_decode(enc), oracle_decode(plain)
    assert got[4] == statuses([c[0] for c in cases]) == [0] * len(cases)
    memo = [i for i, c in enumerate(cases) if c[2] == "Memo"]
    if not memo:
        assert records(got) == records(want)
        return
    assert records(got, True, drop=("memo",)) == records(want, True, drop=("memo",))
    ev, S = got[0], got[6]
    plain_memo = TC.value(TC.T_STRUCT, TC.memo(120).v)
    for i in range(len(cases)):
        e = ev[got[3][i]]
        if e.type == 0 and e.a.started.flags & abi.SF_HAS_MEMO:
            m = S[e.a.started.memo]
            assert (m != plain_memo and len(m) > len(plain_memo) and m in cases[i][0][1]) if i in memo else m == plain_memo


@pytest.mark.gpu
def test_unknown_fields_gpu(engine_gpu):
    cases, enc, plain = forward()
    check_gpu(engine_gpu, enc)


# ------------------------------------------------------------------ (b) wrong wire type
@functools.lru_cache(None)
def wrong():
    cases = TC.wrong_type_cases()
    return cases, batch([c[0][1] for c in cases]), batch([c[1] for c in cases])


def test_wrong_wire_type_is_an_absent_field_oracle():
    """thriftrw ignores a field whose wire type is not the IDL's (and reads no entries of
    a list / map whose element types are not): the records of the blob without the field."""
    cases, enc, removed = wrong()
    names = {c[0][0] for c in cases}
    assert len(cases) > 300 and {"b/sa-map-i32-string", "b/sa-as-list", "b/rps-list-i64", "b/reasons-as-set",
                                 "b/reasons-empty-list", "b/events-list-i64", "b/events-count-0"} <= names
    assert {"b/eventId-as-i32", "b/eventId-as-string", "b/tasklist-as-string", "b/attr-field-as-i64"} <= names
    assert any(n.startswith("b/TaskList.10-as-") for n in names) and any(n.startswith("b/ResetPointInfo.60-as-") for n in names)
    got, want = oracle_decode(enc), oracle_decode(removed)
    assert got[4] == statuses([c[0] for c in cases])
    assert set(got[4]) == {TD.DEC_OK, TD.DEC_NO_EVENTS}
    assert records(got) == records(want)


@pytest.mark.gpu
def test_wrong_wire_type_gpu(engine_gpu):
    cases, enc, removed = wrong()
    check_gpu(engine_gpu, enc)


# ------------------------------------------------------------------ (c) repeated fields
@functools.lru_cache(None)
def repeated():
    cases = TC.repeated_cases()
    return cases, batch([c[0][1] for c in cases]), batch([c[1] for c in cases])


def test_repeated_field_keeps_its_last_occurrence_oracle():
    """Each occurrence assigns in turn, a struct-valued field is replaced whole: the
    records (events, kv rows, reset points and their counts) of the blob holding only the
    last occurrence.  By string: strings of a replaced occurrence may still take handles."""
    cases, enc, last = repeated()
    got, want = oracle_decode(enc), oracle_decode(last)
    assert got[4] == [0] * len(cases)
    a, b = records(got, True), records(want, True)
    for i, c in enumerate(cases):
        lo, hi = got[3][i], got[3][i + 1]
        assert a[0][lo:hi] == b[0][lo:hi], c[0][0]
    assert a == b


@pytest.mark.gpu
def test_repeated_fields_gpu(engine_gpu):
    cases, enc, last = repeated()
    check_gpu(engine_gpu, enc, by_string=True)


@functools.lru_cache(None)
def repeated_lists():
    """The malformed blobs first, then well-formed ones: 192 blobs (three wavefronts)."""
    cases = TC.repeated_list_cases()
    good = [TC.blob(TC.history([TC.started(1, b"g%d" % i, full=False), TC.upsert(2)])) for i in range(192 - len(cases))]
    return cases, batch([c[0][1] for c in cases] + good), batch([c[1] for c in cases] + good), good


def test_repeated_events_list_keeps_the_last_list_oracle():
    cases, enc, last, good = repeated_lists()
    got, want = oracle_decode(enc), oracle_decode(last)
    assert got[4] == statuses([c[0] for c in cases]) + [0] * len(good)
    assert records(got, True) == records(want, True)


@pytest.mark.gpu
def test_repeated_events_list_gpu(engine_gpu):
    """History field 10 twice.  Before the fill pass bounded its stores to the rows the
    count pass reported (the last list's), an earlier, longer list wrote its events, kv
    rows and reset points over the following blobs' slots, and past the buffers for the
    last blob: the observable symptom is in the well-formed blobs after the malformed
    ones, so their records are checked on their own too.  By string: the intern pass
    still takes the dropped events' strings (it cannot know a list is not the last
    without a further pass), so handles may count strings no record names."""
    cases, enc, last, good = repeated_lists()
    ref = oracle_decode(enc)
    d = check_gpu(engine_gpu, enc, ref, by_string=True)
    alone = oracle_decode(batch(good))
    n = len(alone[0])
    assert [no_off(_by_string(e, d.strings)) for e in list(d.events)[-n:]] == [
        no_off(_by_string(e, alone[6])) for e in alone[0]]
    assert [(d.strings[k.key], d.strings[k.value]) for k in list(d.kvs)[-len(alone[1]):]] == [
        (alone[6][a], alone[6][b]) for a, b in alone[1]]
    assert [rp_by_string(p, d.strings) for p in list(d.rps)[-len(alone[2]):]] == [rp_by_string(p, alone[6]) for p in alone[2]]


# ------------------------------------------------------------------ (d) depth
@functools.lru_cache(None)
def depth():
    cases = TC.depth_cases()
    return cases, batch([c[0][1] for c in cases])


def first_failing(cases, st):
    out = {}
    for (c, place, kind, levels), s in zip(cases, st):
        assert s in (TD.DEC_OK, TD.DEC_DEPTH), (c[0], s)
        if s == TD.DEC_DEPTH:
            out[place, kind] = min(levels, out.get((place, kind), 99))
        else:
            assert out.get((place, kind), 99) > levels, c[0]  # no level passes above a failing one
    return out


def test_depth_limit_oracle():
    """CDR_THRIFT_MAX_DEPTH counts the containers open inside one skipped value, that value
    being level 1 (cdr/ingest.h): 16 levels pass and 17 fail at every place a skip starts,
    however deep the walked structs around it are; inside Memo the Memo struct is level 1."""
    cases, enc = depth()
    st = oracle_decode(enc)[4]
    assert st == statuses([c[0] for c in cases])
    assert first_failing(cases, st) == {(p, k): TD.MAX_DEPTH + 1 for p in TC.DEPTH_PLACES for k in ("struct", "list", "map")}


@pytest.mark.gpu
def test_depth_limit_gpu(engine_gpu):
    cases, enc = depth()
    d = check_gpu(engine_gpu, enc)
    assert first_failing(cases, list(d.blob_status)) == {(p, k): 17 for p in TC.DEPTH_PLACES for k in ("struct", "list", "map")}


# ------------------------------------------------------------------ (e) every prefix, every byte
@functools.lru_cache(None)
def small():
    root = TC.small_history()
    b = TC.blob(root)
    cuts = TC.event_boundaries(root)
    prefixes = [b[:n] for n in range(len(b))]
    rest = [TC.restored(b, cut, k + 1) for k, cut in enumerate(cuts)]
    muts = [b[:p] + bytes([v]) + b[p + 1:] for p in range(len(b)) for v in TC.MUTATION_BYTES]
    return b, prefixes, rest, muts


def test_prefixes_and_bytes_oracle():
    """The rule: no proper prefix of a blob decodes (the History struct's stop byte is its
    last byte, and the list's count promises every event); a prefix that ends after event
    k decodes, to exactly the first k events, once the closing bytes are restored (count
    set to k, stop byte appended).  Over the prefixes and the single-byte mutations the
    statuses include every CDR_DEC_* code but DEPTH, so the inputs are not all one case."""
    b, prefixes, rest, muts = small()
    assert 250 <= len(b) <= 640, len(b)
    whole = oracle_decode(batch([b]))
    assert whole[4] == [0] and len(whole[0]) == 11
    ps = oracle_decode(batch(prefixes))[4]
    assert TD.DEC_OK not in ps and ps[0] == TD.DEC_MISSING_VERSION
    r = oracle_decode(batch(rest))
    assert r[4] == [0] * len(rest) and [r[3][k + 1] - r[3][k] for k in range(len(rest))] == list(range(1, 12))
    for k in range(len(rest)):
        assert [no_off(_by_string(e, r[6])) for e in r[0][r[3][k]:r[3][k + 1]]] == [
            no_off(_by_string(e, whole[6])) for e in whole[0][:k + 1]]
    ms = oracle_decode(batch(muts))[4]
    assert set(ps) | set(ms) == set(range(8)) - {TD.DEC_DEPTH}, (sorted(set(ps)), sorted(set(ms)))
    assert ms.count(TD.DEC_OK) > len(b)  # and many mutations still decode: their records are compared


@pytest.mark.gpu
def test_every_prefix_gpu(engine_gpu):
    b, prefixes, rest, muts = small()
    check_gpu(engine_gpu, batch(prefixes + rest), by_string=True)


@pytest.mark.gpu
def test_every_byte_gpu(engine_gpu):
    """Every byte of the blob set to 0x00, 0x0B, 0x0C, 0x0D, 0x0F, 0x7F, 0x80, 0xFF: statuses
    and the records of the blobs that still decode, by string.

    A byte set in the eventType leaves a record whose union is not the type's member, so
    each union is compared as the member its attribute struct filled (`by_union`).

    Loops driven by a wire count, read before the first run (csrc/ingest.hip): a corrupt
    count (0x7FFFFFFF after a 0x7F in its first byte) must end at the blob's end.
      - Blob::run, the events list: `i < n && r.ok()`; event() reads at least the first
        field's type byte through fields() -> u8() -> need(1), which consumes a byte or sets
        TRUNCATED.  The non-struct branch calls skip1 per element.
      - skip1 / skip_body, one value: a fixed type consumes >= 1 byte or fails need(); a
        string reads its 4-byte length; a struct reads at least its stop byte; a list / set
        reads 5 header bytes, a map 6; any other type sets BAD_TYPE.  So every element of
        every counted loop consumes >= 1 byte or sets an error, and need() fails at `end`.
      - skip_body's frames: a list's `n` / a map's `2 * n` (0xFFFFFFFE at most: no wrap in
        32 bits) count down once per value, each consuming as above; a struct frame pops on
        its stop byte.  The outer for(;;) returns on !r.ok(), the inner while tests r.ok().
      - search_attrs: `i < n && r.ok()`, per pair two str() (4 bytes each) or two skip1.
      - reset_points: `i < n && r.ok()`, per point fields() (>= 1 byte) or skip1 per element.
      - fields(): `while (r.ok())`, each turn reads a type byte.
      - Rd::hash(p, n): n is a length need() has already checked against `end`.
      - tab_insert / tab_lookup: bounded by the table's capacity, not by a wire count.
    Nothing loops on a wire count without consuming input; the worst blob costs its own
    length (a few hundred iterations here)."""
    b, prefixes, rest, muts = small()
    check_gpu(engine_gpu, batch(muts), corrupt=True)


# ------------------------------------------------------------------ (f) the reader's three paths
def small_blob(i, pad=0):
    """A well-formed ~110-byte blob whose kept strings vary with i; `pad` more bytes of string."""
    return TC.blob(TC.history([TC.cancel_initiated(1 + i % 5, control=b"c%d-" % (i % 7) + b"p" * pad)]))


def padded_wave(n, total, first=0):
    """n small blobs whose lengths sum to exactly `total` (the last one's string padded)."""
    w = [small_blob(first + i) for i in range(n - 1)]
    need = total - sum(map(len, w)) - len(small_blob(first + n - 1))
    assert need >= 0
    return w + [small_blob(first + n - 1, need)]


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_staging_boundary_gpu(engine_gpu, delta):
    """Two wavefronts of 64 blobs.  The second starts 5 (+ k) bytes past a 16-byte
    boundary and its byte range, measured from that boundary, is CDR_INGEST_STAGE + delta:
    staged in LDS up to and including the limit, through the register window one past it.
    Also one wave alone from an aligned start, its range the limit + delta."""
    for k in (0, 7):
        w0 = padded_wave(64, STAGE + 5 - k)  # k + len(w0) = STAGE + 5: wave 1 starts 5 past a boundary
        lead = (k + sum(map(len, w0))) % 16
        assert lead == 5
        w1 = padded_wave(64, STAGE + delta - lead, first=64)
        enc = batch(w0 + w1)
        if k == 0:  # wave 0 alone, exactly / one past / one short of the limit
            check_gpu(engine_gpu, batch(padded_wave(64, STAGE + delta)))
        check_gpu(engine_gpu, enc, byte_offset=k)


@pytest.mark.gpu
def test_long_blob_among_small_gpu(engine_gpu):
    """One 70,000-byte blob (a long control string) among 63 small ones: that wave reads
    through the register window, the next wave is staged; strict, so a string both waves
    hold has one handle."""
    w0 = [small_blob(i) for i in range(64)]
    w0[10] = small_blob(10, 70_000 - len(small_blob(10)))
    assert len(w0[10]) == 70_000
    check_gpu(engine_gpu, batch(w0 + [small_blob(i) for i in range(64)]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_partial_wave_and_workgroup_gpu(engine_gpu, n):
    blobs = [small_blob(i) if i % 9 else TC.blob(TC.history([TC.started(1, b"%d" % i), TC.upsert(2)])) for i in range(n)]
    check_gpu(engine_gpu, batch(blobs))


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(16))
def test_unaligned_base_gpu(engine_gpu, k):
    """blob_bytes k bytes past an aligned allocation filled with 0xA5, total lengths leaving
    0..15 bytes after the last 16-byte boundary (the byte-by-byte tail).  The last blob
    ends in a string three stop bytes before the final byte, or (odd tails) is cut right
    after that string, which then reaches the final byte: TRUNCATED, the others intact."""
    for tail in range(16):
        last = TC.blob(TC.history([TC.event(3, 330, [TC.s(10, b"new-run-%d" % tail)])]))
        last = last[:-3] if tail % 2 else last
        head = [small_blob(k), small_blob(tail)]
        pad = (tail - (k + sum(map(len, head)) + len(last))) % 16
        blobs = [small_blob(k, pad), small_blob(tail), last]
        assert (k + sum(map(len, blobs))) % 16 == tail
        ref = oracle_decode(batch(blobs))
        assert ref[4] == [0, 0, TD.DEC_TRUNCATED if tail % 2 else 0]
        check_gpu(engine_gpu, batch(blobs), ref, byte_offset=k)


# ------------------------------------------------------------------ (g) strings and entries
G_SEEDS = [b"", b"emptyUuid", b"dup", b"dup", b"", b"tl", b"cdom", b"cdom-id", b"unused", b"xdom", b"xdom-id"]


def test_seed_rules_oracle():
    """Two equal seeds: the first keeps the strings; "" above index 0 and an unused seed
    name nothing; a blob string equal to a seed takes the seed's handle; a domain-map name
    past the seeds names nothing."""
    blobs = [TC.blob(TC.history([TC.decision_scheduled(1), TC.cancel_initiated(2, b"dup", control=b""),
                                 TC.child_initiated(3), TC.cancel_initiated(4, b"xdom")]))]
    ev, kvs, rps, ev_off, st, est, S = oracle_decode(batch(blobs, G_SEEDS, [(6, 7), (len(G_SEEDS) + 1, 7)]))
    assert st == [0] and S[:len(G_SEEDS)] == G_SEEDS
    assert ev[0].a.dt_sched.task_list == 5 and ev[1].a.ext.domain == 2 and ev[1].a.ext.control == 0
    assert (ev[2].a.ext.domain, ev[2].a.ext.target_domain_id, ev[2].a.ext.flags & abi.XF_DOMAIN_MISSING) == (6, 7, 0)
    assert ev[3].a.ext.domain == 9 and ev[3].a.ext.flags & abi.XF_DOMAIN_MISSING
    assert all(h >= len(G_SEEDS) for h in (ev[1].a.ext.workflow_id, ev[2].a.ext.workflow_type))


@pytest.mark.gpu
def test_seeds_and_domains_gpu(engine_gpu):
    blobs = [TC.blob(TC.history([TC.decision_scheduled(1), TC.cancel_initiated(2, b"dup", control=b""),
                                 TC.child_initiated(3), TC.cancel_initiated(4, b"xdom"),
                                 TC.activity_scheduled(5, b"xdom"), TC.activity_scheduled(6, b"cdom")]))] * 3
    for dm in ([(6, 7)], [(6, 7), (9, 10)], [(6, 7), (len(G_SEEDS) + 1, 7), (0xFFFFFFFF, 7)], []):
        check_gpu(engine_gpu, batch(blobs, G_SEEDS, dm))


@functools.lru_cache(None)
def many_strings():
    near = [b"ab", b"abc", b"abd", b"abcd", b"abc\0", b"\0", b"\0\0", b"abc\xff", b"abC"]
    blobs = [TC.blob(TC.history([TC.cancel_initiated(1, b"d%d" % i, b"ctl-%d" % i),
                                 TC.signal_initiated(2, b"e%d" % i, near[i % len(near)])])) for i in range(1000)]
    return batch(blobs), near


def test_many_distinct_strings_oracle():
    enc, near = many_strings()
    ev, kvs, rps, ev_off, st, est, S = oracle_decode(enc)
    new = S[len(SEEDS):]
    assert len(new) == len(set(new)) >= 3000 and set(near) <= set(new)
    assert [TD.str_hash(x) for x in new] == sorted(TD.str_hash(x) for x in new)
    assert [S[ev[2 * i + 1].a.ext.control] for i in range(len(near))] == near


@pytest.mark.gpu
def test_many_distinct_strings_gpu(engine_gpu):
    """3,000 distinct strings (the collect and rank passes span many workgroups), among
    them strings that differ only in length or in the last byte: strict, so every handle
    is the rank of its hash."""
    check_gpu(engine_gpu, many_strings()[0])


def entries_case():
    good = [small_blob(i) for i in range(12)]
    trunc, nover, badv = good[0][:-1], good[1][:3] + b"\x7f" + good[1][4:], b"\x58" + good[2][1:]
    blobs = [good[0],                       # entry 0: one good blob
             trunc, good[1], good[2],       # entry 1: the first blob fails
             good[3], nover, good[4],       # entry 2: the middle one (an unknown id: no events)
             good[5], good[6], badv,        # entry 3: the last one
             trunc, good[7], badv,          # entry 4: two fail: the first failure is the entry's
             good[8], good[9], good[10]]    # entry 6 (entry 5 has no blobs): all good
    e0 = [0, 1, 4, 7, 10, 13, 13, 16, 16, 16]  # entries 7 and 8: trailing, without blobs
    want = [0, TD.DEC_TRUNCATED, TD.DEC_NO_EVENTS, TD.DEC_INVALID_VERSION, TD.DEC_TRUNCATED, 0, 0, 0, 0]
    ev_off = [0, 1, 3, 5, 7, 8, 8, 11, 11, 11]  # only the good blobs' events (one each) count
    return batch(blobs, entry_blob0=e0), want, ev_off


def test_entries_oracle():
    enc, want, ev_off = entries_case()
    r = oracle_decode(enc)
    assert r[5] == want and list(r[3]) == ev_off and len(r[0]) == 11


@pytest.mark.gpu
def test_entries_gpu(engine_gpu):
    enc, want, ev_off = entries_case()
    d = check_gpu(engine_gpu, enc)
    assert list(d.entry_status) == want and list(d.ev_off) == ev_off and d.n_bad_blobs == 5


@pytest.mark.gpu
def test_no_blobs_no_entries_gpu(engine_gpu):
    for e0 in ([0, 0, 0, 0], [0]):
        d = check_gpu(engine_gpu, batch([], entry_blob0=e0))
        assert len(d.events) == 0 and list(d.ev_off) == [0] * len(e0) and list(d.entry_status) == [0] * (len(e0) - 1)
        assert d.strings == SEEDS
