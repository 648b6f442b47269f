"""Loading the pending tables from their Cassandra map columns on the device (cdr.h
cdr_load_cql_rows, csrc/load.hip), checked against tests/cql_rows_ref.py.

CPU: the reference reader inverts the reference writer on replayed states of the synthetic
configs 2-5 — the decoded state equals the state with every timestamp FLOORED to the
millisecond, ns // 1,000,000 * 1,000,000: a CQL timestamp holds milliseconds (gocql's
marshalTimestamp, restated by oracle/cql_values.timestamp, floors), so that is all a stored
state keeps of a time — the wire edges give the statuses cdr.h names, and the ABI mirrors match.
GPU (-m gpu): the device == the reference record for record, status for status and handle for
handle on those states, on hand-made columns, on every field edge, truncation, map count and
buffer end; the SQL and Cassandra forms of one state load alike; the loaded state carries a
replay to the oracle's result.
"""
import ctypes as C
import functools
import os
import random
import re
import struct

import numpy as np
import pytest

from cadence_amd import abi, engine, rows
from oracle import cql_values as cv
from oracle import thrift_decode as TD
from tests import cql_rows_ref as ref
from tests.test_load_rows import _copy_outputs, _state
from tests.test_load_state import _state as _builder_state

TABLES = rows.TABLES
ZT = abi.ZERO_TIME_NANOS
TRUNCATED, BAD_SIZE = TD.DEC_TRUNCATED, TD.DEC_BAD_SIZE
E_SIZE, E_SHAPE, E_UUID = abi.LOAD_E_CQL_SIZE, abi.LOAD_E_SHAPE, abi.LOAD_E_UUID
I64_MIN, I64_MAX, I32_MIN, I32_MAX = -2**63, 2**63 - 1, -2**31, 2**31 - 1
U = b"0123abcd-89ef-4c5d-8a7b-fedcba987654"
RUN = bytes(range(0x10, 0x20))
TIME_FIELDS = {"act": ("scheduled_time", "started_time", "last_heartbeat_time", "expiration_time"),
               "timer": ("expiry_time",)}


def q(v):
    return struct.pack(">q", v)


def i4(v):
    return struct.pack(">i", v)


def lst(elems) -> bytes:
    return i4(len(elems)) + b"".join(cv.val(e) for e in elems)


def base(t, v=0, key=None):
    """The UDT of table t with every declared field set (values vary with v), raw values in
    declaration order."""
    k = 500 + v if key is None else key
    if t == 0:
        return [q(7 + v), q(k), q(5 + v), b"sched-event", q(1_600_000_000_000 + v), q(9 + v), b"started-event",
                q(1_600_000_000_123 + v), b"act-%d" % v, b"req-%d" % v, b"details", i4(11 + v), i4(12 + v), i4(13 + v),
                i4(14 + v), b"\x01" if v % 2 == 0 else b"\x00", q(77 + v), q(1_600_000_000_456 + v), i4(3 + v),
                i4(2 + v), b"tl-%d" % (v % 3), b"identity", b"\x01", i4(1 + v), struct.pack(">d", 1.5 + v), i4(60 + v),
                q(1_700_000_000_000 + v), i4(4 + v), lst([b"bad", b"e%d" % (v % 5)]), b"reason", b"worker", b"fdetails",
                b"thriftrw"]
    if t == 1:
        return [q(7 + v), b"timer-%d" % k if key is None else key, q(21 + v), q(1_650_000_000_000 + v), q(9000 + v)]
    if t == 2:
        return [q(7 + v), q(k), q(30 + v), b"init-event", q(33 + v), b"child-wf-%d" % v,
                bytes((x + v) & 0xFF for x in RUN), b"started-event", bytes((x + 3 * v) & 0xFF for x in RUN[::-1]),
                b"thriftrw", b"dom-%d" % (v % 2), b"type-%d" % (v % 4), i4(1 + v % 3)]
    if t == 3:
        return [q(7 + v), q(40 + v), q(k), U[:-4] + b"%04x" % (v & 0xFFFF)]
    return [q(7 + v), q(50 + v), q(k), bytes((x * 3 + v) & 0xFF for x in RUN), b"sig-%d" % (v % 7), b"input-%d" % v,
            b"ctl-%d" % v if v % 2 else None]


def pair(t, udt, key=b"map-key") -> bytes:
    """A map pair: the key (never read) and the UDT, given as its fields or as its raw [bytes]."""
    return cv.val(key) + (udt if isinstance(udt, bytes) else ref.udt_value(udt))


def raw_udt(parts) -> bytes:
    """A UDT [bytes] value from raw field encodings (bytes) — for lengths no value has."""
    body = b"".join(parts)
    return i4(len(body)) + body


def entries_of(cases) -> rows.CqlCols:
    """One entry per (table, pair): a one-pair column in its table; the entry's other tables
    are null columns or count-0 columns by turns."""
    cols = [[b"" if (w + t) % 2 else i4(0) for w in range(len(cases))] for t in range(5)]
    for w, (t, p) in enumerate(cases):
        cols[t][w] = i4(1) + p
    return rows.pack_cql(len(cases), cols)


# ---------------------------------------------------------------- the edge cases
@functools.lru_cache(maxsize=None)
def field_cases():
    """[(name, table, pair, expected)]: expected is a row status, or None where the row
    decodes and the restatement says to what."""
    out = []
    for t in range(5):
        f0, types = base(t), [ty for _, ty in ref.UDT[t]]
        n = len(f0)
        keep_id = t != 3  # a request-cancel row without its ID text is CDR_LOAD_E_UUID

        def edit(i, v, f0=f0):
            return f0[:i] + [v] + f0[i + 1:]

        def raw_at(i, enc, f0=f0):
            return raw_udt([cv.val(x) for x in f0[:i]] + [enc] + [cv.val(x) for x in f0[i + 1:]])
        out.append(("plain", t, pair(t, f0), None))
        out.append(("null key", t, pair(t, f0, None), None))
        out.append(("null UDT", t, cv.val(b"k") + i4(-1), None if keep_id else E_UUID))
        out.append(("empty UDT", t, cv.val(b"k") + i4(0), None if keep_id else E_UUID))
        for i, ty in enumerate(types):
            idless = t == 3 and i == 3
            out.append((f"{i} null", t, pair(t, edit(i, None)), E_UUID if idless else None))
            out.append((f"{i} zero-length", t, pair(t, edit(i, b"")), E_UUID if idless else None))
            out.append((f"{i} length -2", t, pair(t, raw_at(i, i4(-2))), BAD_SIZE))
            out.append((f"{i} length past the UDT", t, pair(t, raw_at(i, i4(1 << 20) + b"ab")), TRUNCATED))
            size = ref.SIZE.get(ty)
            if size:
                for m in {size - 1, size + 1, 2 * size} - {0}:
                    out.append((f"{i} {ty} of {m} bytes", t, pair(t, edit(i, bytes(m))), E_SIZE))
            if ty == "bigint":
                for v in (I64_MIN, I64_MAX, -1, 0):
                    out.append((f"{i} bigint {v}", t, pair(t, edit(i, q(v))), None))
            if ty == "int":
                for v in (I32_MIN, I32_MAX, -1):
                    out.append((f"{i} int {v}", t, pair(t, edit(i, i4(v))), None))
            if ty == "double":
                for bits in (0x8000000000000000, 0x7FF0000000000000, 0x7FF8000000000001, 1, 0xFFEFFFFFFFFFFFFF):
                    out.append((f"{i} double {bits:#x}", t, pair(t, edit(i, struct.pack(">Q", bits))), None))
            if ty == "boolean":
                for b in (b"\x00", b"\x01", b"\xff", b"\x80"):
                    out.append((f"{i} boolean {b!r}", t, pair(t, edit(i, b)), None))
            if ty == "timestamp":
                for ms, want in ((0, None), (-1, None), (ref.MS_MAX, None), (-ref.MS_MAX, None),
                                 (ref.MS_MAX + 1, E_SHAPE),  # the first value whose nanoseconds overflow
                                 (-ref.MS_MAX - 1, E_SHAPE), (I64_MAX, E_SHAPE), (I64_MIN, E_SHAPE)):
                    out.append((f"{i} timestamp {ms}", t, pair(t, edit(i, q(ms))), want))
        for i in range(n + 1):  # fewer fields
            out.append((f"cut after field {i}", t, pair(t, f0[:i]), None if keep_id or i == n else E_UUID))
            if i < n:  # ... and the next field's length word cut
                out.append((f"cut in the length of field {i}", t, pair(t, raw_udt([cv.val(x) for x in f0[:i]] + [b"\0\0"])),
                            TRUNCATED))
        out.append(("extra trailing fields", t, pair(t, f0 + [b"later-field", None, q(1)]), None))
        out.append(("trailing bytes that are no value", t, pair(t, raw_udt([cv.val(x) for x in f0] + [b"\xff\xff"])), None))
        if t == 2:
            for name, run in (("emptyRunID", ref.EMPTY_RUN_ID), ("zero", bytes(16)), ("ordinary", RUN),
                              ("emptyRunID + 1", ref.EMPTY_RUN_ID[:-1] + b"\x01"), ("all ones", b"\xff" * 16)):
                out.append((f"run ID {name}", t, pair(t, edit(6, run)), None))
        if t == 3:
            for name, text in (("uppercase", U.upper()), ("32 hex", U.replace(b"-", b"")), ("35 chars", U[:-1]),
                               ("37 chars", U + b"0"), ("braces", b"{" + U[1:-1] + b"}"),
                               ("dash moved", U[:8] + U[9:10] + b"-" + U[10:]), ("non-hex", U[:20] + b"g" + U[21:]),
                               ("mixed case", U[:3] + b"A" + U[4:])):
                out.append((f"cancel request ID {name}", t, pair(t, edit(3, text)), E_UUID))
        if t == 0:
            L = 28
            many = [b"e%d" % k * (k % 9) for k in range(40)]
            for name, v, want in (
                    ("0 elements", lst([]), None), ("1 element", lst([b"only"]), None), ("many elements", lst(many), None),
                    ("an empty element", lst([b"a", b"", b"c"]), None),
                    ("a null element", i4(2) + cv.val(b"a") + i4(-1), BAD_SIZE),
                    ("element length -5", i4(1) + i4(-5), BAD_SIZE), ("count -1", i4(-1), BAD_SIZE),
                    ("count -1 and elements", i4(-1) + cv.val(b"a"), BAD_SIZE),
                    ("count past the elements", i4(3) + cv.val(b"a") + cv.val(b"b"), TRUNCATED),
                    ("count 2^31-1 alone", i4(I32_MAX), TRUNCATED), ("2 bytes", b"\0\0", TRUNCATED),
                    ("element past the value", i4(1) + i4(9) + b"short", TRUNCATED),
                    ("element length cut", i4(2) + cv.val(b"a") + b"\0\0\0", TRUNCATED),
                    ("bytes after the last element", lst([b"a", b"b"]) + b"tail", None)):
                out.append((f"list {name}", t, pair(t, edit(L, v)), want))
    return out


def _parse(t, p):
    udts, found = ref.split(i4(1) + p)
    assert found is None and len(udts) == 1
    return ref.parse_udt(t, udts[0])


# ---------------------------------------------------------------- CPU
def _floored(t, rec) -> bytes:
    """The record as a Cassandra store gives it back: every timestamp floored to the
    millisecond; HEARTBEAT cleared where STARTED is set (as every load does)."""
    rec = type(rec).from_buffer_copy(bytes(rec))
    for f in TIME_FIELDS.get(t, ()):
        setattr(rec, f, getattr(rec, f) // 1_000_000 * 1_000_000)
    if t == "act" and rec.flags & abi.AI_STARTED_TIME_SET:
        rec.flags &= ~abi.AI_HEARTBEAT_TIME_SET
    return bytes(rec)


def _check_against_state(b, out, row0, table_of, result_of):
    n = 0
    for w in range(b.n_wfs):
        ok = out.result[w].code == abi.OK
        for i, t in enumerate(TABLES):
            want = [_floored(t, r) for r in out.rows(w, t)] if ok else []
            assert result_of(w)[1 + i] == len(want), (w, t)
            for j, rec in enumerate(want):
                assert table_of(i, int(row0[i][w]) + j) == rec, (w, t, j)
                n += 1
    return n


@pytest.mark.parametrize("builder", [abi.BUILDER_LOCAL, abi.BUILDER_2DC, abi.BUILDER_NDC])
@pytest.mark.parametrize("cfg", [2, 3, 4, 5])
def test_reference_round_trip(cfg, builder):
    """state -> CQL columns -> decoded state == the state with its timestamps floored to ms,
    for each of the three builders."""
    b, out, strs = _builder_state(cfg, builder)[:3]
    for w in range(b.n_wfs):  # what the floor rests on: a replayed row without STARTED has no times
        for r in (out.rows(w, "act") if out.result[w].code == abi.OK else []):
            if not r.flags & abi.AI_STARTED_TIME_SET:
                assert (r.started_time, r.last_heartbeat_time) == (0, 0) and not r.flags & abi.AI_HEARTBEAT_TIME_SET
    cols = ref.columns(b, out, strs)
    dec = ref.decode(cols, strs)
    assert not any(dec.entry_status) and not any(any(s) for s in dec.row_status)
    assert dec.strings == strs  # seeds = the whole table: nothing new, every handle kept
    n = _check_against_state(b, out, dec.entry_row0, lambda i, slot: dec.tables[i][slot], lambda w: dec.result[w])
    assert n > 0 and sum(dec.n_rows) == n


@pytest.mark.parametrize("builder", ["activity", "timer", "child", "cancel", "signal"])
def test_reference_writer(builder):
    """The writer's pairs against oracle/cql_values.py's builders: the UDT's fields are the
    statement's, in the schema's order, and the key is the statement's first value."""
    t = ["activity", "timer", "child", "cancel", "signal"].index(builder)
    b, out, strs = _state(3 if t != 2 else 5)
    S = cv.tb.lookup(strs)
    recs = [r for w in range(b.n_wfs) if out.result[w].code == abi.OK for r in out.rows(w, TABLES[t])][:50]
    assert recs
    for r in recs:
        values = ref.WRITER[t](r, S)
        v = cv.decode(values, ref.STATEMENT_TYPES[t])
        p = ref.pair(t, values)
        assert p.startswith(cv.val(v[0]))
        udts, found = ref.split(i4(1) + p)
        assert found is None
        f = ref.Fields(udts[0])
        got = [f.val() for _ in ref.UDT[t]]
        assert f.p == len(udts[0]) and got == [v[1 + i] for i in ref.DECLARED[t]]
        names = [nm for nm, _ in ref.UDT[t]]
        if t in (3, 4):
            assert got[names.index("initiated_id")] == q(r.initiated_id)
            assert got[names.index("initiated_event_batch_id")] == q(r.initiated_event_batch_id)
        rec, _ = ref.parse_udt(t, udts[0])
        assert ref._key(t, rec) == (0 if t == 1 else r.schedule_id if t == 0 else r.initiated_id)


def test_reference_wire_edges():
    seen = set()
    for name, t, p, want in field_cases():
        if want is None:
            _parse(t, p)
        else:
            with pytest.raises(ref.RowError) as e:
                _parse(t, p)
            assert e.value.code == want, (name, t)
            seen.add(want)
    assert seen == {TRUNCATED, BAD_SIZE, E_SIZE, E_SHAPE, E_UUID}
    # what the plain UDTs decode to, spelled out once
    a, s = _parse(0, pair(0, base(0)))
    assert (a.version, a.schedule_id, a.scheduled_event_batch_id, a.started_id) == (7, 500, 5, 9)
    assert (a.scheduled_time, a.started_time, a.last_heartbeat_time) == (
        1_600_000_000_000_000_000, 1_600_000_000_123_000_000, 1_600_000_000_456_000_000)
    assert a.flags == abi.AI_CANCEL_REQUESTED | abi.AI_HAS_RETRY | abi.AI_STARTED_TIME_SET
    assert (a.s2s, a.s2c, a.stc, a.hb, a.cancel_request_id, a.backoff_coefficient) == (11, 12, 13, 14, 77, 1.5)
    assert s == {"activity_id": b"act-0", "request_id": b"req-0", "task_list": b"tl-0",
                 "nonretriable": struct.pack(">bi", 11, 2) + b"\0\0\0\x03bad\0\0\0\x02e0"}
    a, _ = _parse(0, pair(0, base(0)[:7] + [None] + base(0)[8:]))  # started_time null: the heartbeat says so
    assert a.flags & (abi.AI_STARTED_TIME_SET | abi.AI_HEARTBEAT_TIME_SET) == abi.AI_HEARTBEAT_TIME_SET
    assert (a.started_time, a.last_heartbeat_time) == (0, 1_600_000_000_456_000_000)
    a, _ = _parse(0, cv.val(None) + i4(-1))
    assert (a.flags, a.started_time, a.last_heartbeat_time, a.scheduled_time, a.expiration_time) == (0, 0, 0, ZT, ZT)
    c, s = _parse(2, pair(2, base(2)))
    assert (c.create_request_hi, c.create_request_lo) == (0x1f1e1d1c1b1a1918, 0x1716151413121110)
    assert s["started_run_id"] == b"10111213-1415-1617-1819-1a1b1c1d1e1f"
    assert _parse(2, pair(2, base(2)[:6] + [ref.EMPTY_RUN_ID] + base(2)[7:]))[1]["started_run_id"] == b""
    g, s = _parse(4, pair(4, base(4, 1)))
    assert (g.version, g.initiated_event_batch_id, g.initiated_id) == (8, 51, 501) and s["control"] == b"ctl-1"
    x, s = _parse(1, pair(1, base(1)))
    assert (x.expiry_time, s) == (1_650_000_000_000_000_000, {"timer_id": b"timer-500"})
    # the map split's findings
    two = pair(3, base(3)) + pair(3, base(3, 1))
    assert ref.split(b"") == ([], None) and ref.split(i4(0) + b"junk") == ([], None)
    assert ref.split(b"\0\0\0") == ([], (0, TRUNCATED)) and ref.split(i4(-1)) == ([], (0, BAD_SIZE))
    assert ref.split(i4(abi.LOAD_MAX_ENTRY_ROWS + 1)) == ([], (0, abi.LOAD_E_ENTRY_ROWS))
    assert ref.split(i4(abi.LOAD_MAX_ENTRY_ROWS)) == ([], (0, TRUNCATED))
    assert [len(ref.split(i4(2) + two + b"ignored")[0]), ref.split(i4(2) + two + b"ignored")[1]] == [2, None]
    assert ref.split(i4(3) + two)[1] == (2, TRUNCATED) and len(ref.split(i4(3) + two)[0]) == 2
    assert ref.split(i4(1) + i4(-2))[1] == (0, BAD_SIZE) and ref.split(i4(2) + pair(3, base(3)) + cv.val(b"k") + i4(-9))[1] == (1, BAD_SIZE)


def test_abi_mirrors():
    L = abi.lib()
    assert L.cdr_struct_size(b"cdr_cql_rows_in") == C.sizeof(abi.CdrCqlRowsIn) == 80
    assert L.cdr_struct_size(b"cdr_cql_rows_out") == C.sizeof(abi.CdrCqlRowsOut) == 296 + 40 + 24
    assert hasattr(L, "cdr_load_cql_rows")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "cdr", "cdr.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"#define CDR_LOAD_E_([A-Z_]+) (\d+)", hdr)}
    assert codes["CQL_SIZE"] == abi.LOAD_E_CQL_SIZE == codes["CLUSTER"] + 1 == max(codes.values())
    assert abi.LOAD_STATUS[abi.LOAD_E_CQL_SIZE] == "E_CQL_SIZE"
    assert "int cdr_load_cql_rows(cdr_ctx* ctx, const cdr_cql_rows_in* in, cdr_cql_rows_out* out, void* stream);" in hdr
    assert ref.EMPTY_RUN_ID == cv.parse_uuid(cv.EMPTY_RUN_ID) and ref.ZT == cv.ZERO_TIME_NANOS


# ---------------------------------------------------------------- GPU
def _assert_equal(eng, cols, seeds, **kw):
    got = rows.load_cql(eng, cols, seeds, **kw)
    want = ref.decode(cols, seeds, kw.get("n_bytes"))
    bad = ref.compare_cql(got, want, cols)
    assert not bad, "\n".join(bad[:10])
    return got, want


@pytest.mark.gpu
def test_gpu_round_trip_batches(engine_gpu):
    """(1) the GPU encoder's values of replayed states, as columns, load to the reference's
    result and to the states' own records with their times floored."""
    started = 0
    for cfg in (2, 3, 4, 5):
        b, out, strs = _state(cfg)
        cols = rows.encode_state_cql(engine_gpu, b, out, strs)
        assert cols.bytes.tobytes() == ref.columns(b, out, strs).bytes.tobytes()
        got, _ = _assert_equal(engine_gpu, cols, strs)
        raw = {i: bytes(got.tables[t]) for i, t in enumerate(TABLES)}
        size = [C.sizeof(engine.TABLE_TYPES[t]) for t in TABLES]
        res = lambda w: (got.result[w].code, got.result[w].n_activity, got.result[w].n_timer, got.result[w].n_child,  # noqa: E731
                         got.result[w].n_cancel, got.result[w].n_signal)
        assert _check_against_state(b, out, got.entry_row0, lambda i, s: raw[i][s * size[i]:(s + 1) * size[i]], res) > 0
        assert got.strings == strs and not got.n_bad_entries
        started += sum(1 for r in got.tables["child"] if r.started_run_id)
    assert started > 0


@functools.lru_cache(maxsize=None)
def _hand_made():
    """Entries of 0 / 1 / 63 / 64 / 65 rows per table, one 1,000-row entry beside empty ones,
    null columns beside count-0 columns, keys ascending, descending and shuffled."""
    counts = [0, 1, 63, 64, 65, 0, 1000, 0, 0, 2, 7]
    rng = random.Random(0xC91)
    cols = [[None] * len(counts) for _ in range(5)]
    for t in range(5):
        v = 0
        for w, n in enumerate(counts):
            n = counts[(w + t) % len(counts)]  # the tables' big entries are different entries
            if n == 0:
                cols[t][w] = b"" if w % 2 else i4(0)
                continue
            keys = [1000 * w + 3 * j - 40 for j in range(n)]
            if w % 3 == 0:
                keys.reverse()
            elif w % 3 == 1:
                rng.shuffle(keys)
            ps = []
            for k in keys:
                ps.append(pair(t, base(t, v, b"timer %d of %d" % (k, w % 2) if t == 1 else k)))
                v += 1
            cols[t][w] = i4(n) + b"".join(ps)
    return rows.pack_cql(len(counts), cols)


@pytest.mark.gpu
def test_gpu_hand_made_columns(engine_gpu):
    """(2) row counts around the wavefront, a 1,000-row entry, null and count-0 columns, rows
    arriving in descending and shuffled key order: ascending output, a few seeds."""
    cols = _hand_made()
    seeds = [b"", b"tl-1", b"no such string", b"type-2", b"timer 23 of 1"]
    got, want = _assert_equal(engine_gpu, cols, seeds)
    assert not any(want.entry_status) and max(want.n_rows) > 1000 and len(want.strings) > 1000
    assert max(int(got.entry_row0[0][w + 1] - got.entry_row0[0][w]) for w in range(cols.n_entries)) == 1000
    for w in range(cols.n_entries):
        for t in TABLES:
            ks = [r.timer_id if t == "timer" else getattr(r, rows.KEY[t]) for r in got.rows(w, t)]
            assert ks == sorted(ks) and len(set(ks)) == len(ks), (w, t)
    assert any(x & abi.STR_REF_GEN for x in got.str_ref.tolist()) and any(x & abi.STR_REF_SEED for x in got.str_ref.tolist())


@pytest.mark.gpu
def test_gpu_field_edges(engine_gpu):
    """(3) every field of every UDT null, zero-length, at its extremes and with a wrong size;
    UDTs cut after each field and with fields appended; run IDs; request-cancel ID texts;
    lists — each in an entry of its own."""
    cases = field_cases()
    cols = entries_of([(t, p) for _, t, p, _ in cases])
    seeds = [b"", b"act-0", b"tl-0", b"timer-500", b"no such string"]
    got, _ = _assert_equal(engine_gpu, cols, seeds)
    for w, (name, t, _, want) in enumerate(cases):
        assert got.entry_status[w] == (want or 0), (name, t)
        assert got.result[w].code == (abi.E_LOAD_ROWS if want else abi.OK), (name, t)


@pytest.mark.gpu
def test_gpu_row_truncation_at_every_length(engine_gpu):
    """(4a) one UDT of each table cut at every length (its length word says the cut): a cut
    inside a field is CDR_DEC_TRUNCATED, a cut between fields leaves the rest null; the whole
    rows between them (the same wave's staged range) decode unchanged."""
    cases, inside = [], 0
    for t in range(5):
        f0 = base(t)
        body = b"".join(cv.val(x) for x in f0)
        ends, p = {0}, 0
        for x in f0:
            p += len(cv.val(x))
            ends.add(p)
        for n in range(len(body)):
            cases += [(t, pair(t, f0), 0), (t, pair(t, i4(n) + body[:n]), 0 if n in ends else TRUNCATED)]
            inside += n not in ends
    cols = entries_of([(t, p) for t, p, _ in cases])
    got, _ = _assert_equal(engine_gpu, cols, [b""])
    assert inside > 500
    for w, (t, _, want) in enumerate(cases):
        if not (t == 3 and want == 0):  # (a request-cancel row cut before its ID: CDR_LOAD_E_UUID)
            assert got.entry_status[w] == want, (w, t)
    assert set(got.entry_status.tolist()) == {0, TRUNCATED, E_UUID}


@pytest.mark.gpu
def test_gpu_column_truncation_at_every_length(engine_gpu):
    """(4b) a three-pair column of each table cut at every length through its first two pairs:
    the pairs before the cut are rows, the finding belongs to the first pair the cut hit."""
    cols, expect = [[] for _ in range(5)], []
    for t in range(5):
        ps = [pair(t, base(t, j)) for j in range(3)]
        body = i4(3) + b"".join(ps)
        first, second = 4 + len(ps[0]), 4 + len(ps[0]) + len(ps[1])
        for n in range(second + 5):
            for u in range(5):
                cols[u].append(body[:n] if u == t else b"")
            expect.append((t, 0 if n == 0 else TRUNCATED, 0 if n < first else 1 if n < second else 2))
    packed = rows.pack_cql(len(expect), cols)
    got, want = _assert_equal(engine_gpu, packed, [b""])
    for w, (t, status, n_rows) in enumerate(expect):
        assert got.entry_status[w] == status, (w, t)
        assert int(got.entry_row0[t][w + 1] - got.entry_row0[t][w]) == n_rows, (w, t)
    assert not any(any(s) for s in want.row_status)  # every finding here is the map's


@pytest.mark.gpu
def test_gpu_buffer_end(engine_gpu):
    """(5) the last column ends at n_bytes, with `bytes` ending where its allocation ends —
    whole, cut, and claiming lengths past the buffer — and offsets that lie past n_bytes."""
    plain = pair(4, base(4))
    cut = pair(4, raw_udt([cv.val(x) for x in base(4)[:4]] + [i4(1 << 20) + b"abc"]))
    for tail in (i4(1) + plain, i4(1) + cut, i4(1) + plain[:-1], i4(2) + plain, i4(1) + plain[:9], b"\0\0",
                 i4(1) + cv.val(b"k") + i4(1 << 30)):
        cols = entries_of([(4, plain), (0, pair(0, base(0))), (4, plain)])
        last = rows.pack_cql(3, [[cols.column(t, w) if (t, w) != (4, 2) else tail for w in range(3)] for t in range(5)])
        assert int(last.col_off[4][3]) == len(last.bytes)
        got, _ = _assert_equal(engine_gpu, last, [b""], at_end=True)
        assert got.entry_status.tolist()[:2] == [0, 0]
        assert got.entry_status[2] == (0 if tail == i4(1) + plain else TRUNCATED)
    # offsets past n_bytes are clamped: the call is told a shorter buffer than the offsets cover
    cols = entries_of([(4, plain), (4, plain), (3, pair(3, base(3)))])
    lo, hi = int(cols.col_off[4][1]), int(cols.col_off[4][2])
    assert hi < len(cols.bytes)
    for nb in (len(cols.bytes) - 1, hi, hi - 1, lo + 10, lo + 3, lo, 3, 0):
        got, want = _assert_equal(engine_gpu, cols, [b""], at_end=True, n_bytes=nb)
        assert got.entry_status[1] == (TRUNCATED if lo < nb < hi else 0), nb


@pytest.mark.gpu
def test_gpu_map_counts(engine_gpu):
    """(6) map counts of -1, 0, CDR_LOAD_MAX_ENTRY_ROWS and the limit + 1 with no bytes behind
    them: the limit is decided from the count word alone and fails its entry only."""
    n = abi.LOAD_MAX_ENTRY_ROWS
    bodies = [i4(-1), i4(0), i4(n), i4(n + 1), i4(I32_MIN), i4(I32_MAX), i4(1) + pair(3, base(3))]
    cols = [[b""] * len(bodies) for _ in range(5)]
    cols[3] = bodies
    cols[1][3] = i4(1) + pair(1, raw_udt([b"\0\0"]))  # a lower table's row failure comes first
    got, _ = _assert_equal(engine_gpu, rows.pack_cql(len(bodies), cols), [b""])
    assert got.entry_status.tolist() == [BAD_SIZE, 0, TRUNCATED, TRUNCATED, BAD_SIZE, abi.LOAD_E_ENTRY_ROWS, 0]
    assert got.n_rows == [0, 1, 0, 1, 0] and got.result[6].n_cancel == 1
    cols[1][3] = b""
    got, _ = _assert_equal(engine_gpu, rows.pack_cql(len(bodies), cols), [b""])
    assert got.entry_status[3] == abi.LOAD_E_ENTRY_ROWS and got.n_bad_entries == 5


@pytest.mark.gpu
def test_gpu_duplicate_keys(engine_gpu):
    """(7) one duplicate key in a single entry of each table (the map keys differ: the key is
    the UDT's field): only that entry fails, both rows say so."""
    cols = [[None] * 7 for _ in range(5)]
    for t in range(5):
        for w in range(7):
            ks = [10 * w + j for j in range(4)]
            if w == t + 1:
                ks[3] = ks[0]
            ps = [pair(t, base(t, 4 * w + j, b"id-%d" % k if t == 1 else k), b"map-key-%d" % j) for j, k in enumerate(ks)]
            cols[t][w] = i4(4) + b"".join(ps)
    got, want = _assert_equal(engine_gpu, rows.pack_cql(7, cols), [b""])
    assert got.entry_status.tolist() == [0] + [abi.LOAD_E_DUP_KEY] * 5 + [0]
    assert sum(1 for s in want.row_status for x in s if x == abi.LOAD_E_DUP_KEY) == 10 and got.n_bad_entries == 5


@pytest.mark.gpu
def test_gpu_staging(engine_gpu):
    """(8) wavefronts whose 64 rows span a byte under, exactly, and a byte over the 24 KiB the
    loader stages in LDS, and one far over it (the buffer is 256-byte aligned, so a wave's
    staged range starts at its first row's offset rounded down to 16)."""
    stage = 24576
    chunks, pos = [], 0
    for w, over in enumerate((-1, 0, 1, 40000, -200)):
        ps = [pair(4, base(4, 64 * w + j)) for j in range(63)]
        start = pos + 4
        fixed = 4 + sum(map(len, ps))
        last = base(4, 64 * w + 63)
        after = 4 if w < 4 else 0  # a wave's range ends where the next one's first row starts: past a count word
        room = stage + over - (start - (start & ~15)) - (fixed - 4) - len(pair(4, last[:5] + [b"", last[6]])) - after
        last[5] = bytes((7 * i + w) & 0xFF for i in range(room))
        ps.append(pair(4, last))
        body = i4(64) + b"".join(ps)
        assert pos + len(body) + after - (start & ~15) == stage + over
        chunks.append(body)
        pos += len(body)
    cols = [[b""] * 5 for _ in range(5)]
    cols[4] = chunks
    got, _ = _assert_equal(engine_gpu, rows.pack_cql(5, cols), [b""])
    assert not got.n_bad_entries and got.n_rows[4] == 320


@pytest.mark.gpu
def test_gpu_degenerate_sizes_and_misuse(engine_gpu):
    """(9) all-empty tables, zero entries, two calls in a row on the warm context, the
    CDR_API_EINVAL cases."""
    empty = rows.pack_cql(3, [[b"", i4(0), b""] for _ in range(5)])
    got, _ = _assert_equal(engine_gpu, empty, [b""])
    assert [(r.code, r.n_activity, r.n_signal) for r in got.result] == [(abi.OK, 0, 0)] * 3
    assert got.strings == [b""] and got.n_rows == [0] * 5 and bytes(got.caps) == bytes(len(bytes(got.caps)))
    got = rows.load_cql(engine_gpu, rows.pack_cql(0, [[] for _ in range(5)]), [b"", b"seed"])
    assert len(got.result) == 0 and got.strings == [b"", b"seed"] and got.n_bad_entries == 0 and got.n_rows == [0] * 5
    cols = _hand_made()
    one, two = rows.load_cql(engine_gpu, cols, [b"", b"tl-1"]), rows.load_cql(engine_gpu, cols, [b"", b"tl-1"])
    for t in TABLES:
        assert bytes(one.tables[t]) == bytes(two.tables[t])
    assert bytes(one.result) == bytes(two.result) and bytes(one.caps) == bytes(two.caps) and one.strings == two.strings
    assert all((a == c).all() for a, c in zip(one.row_status, two.row_status))
    L = abi.lib()
    inp, res = abi.CdrCqlRowsIn(), abi.CdrCqlRowsOut()
    assert L.cdr_load_cql_rows(engine_gpu.ctx, None, C.byref(res), None) == -1
    assert L.cdr_load_cql_rows(engine_gpu.ctx, C.byref(inp), None, None) == -1
    assert L.cdr_load_cql_rows(None, C.byref(inp), C.byref(res), None) == -1
    assert L.cdr_load_cql_rows(engine_gpu.ctx, C.byref(inp), C.byref(res), None) == -1  # no seeds
    dev = rows.DeviceBuffers()
    try:
        so = dev.up(np.zeros(2, np.uint64))
        inp.seed_off, inp.seed_bytes, inp.n_seeds = so, so, 1
        assert L.cdr_load_cql_rows(engine_gpu.ctx, C.byref(inp), C.byref(res), None) == 0  # zero entries
        inp.n_entries = 2
        assert L.cdr_load_cql_rows(engine_gpu.ctx, C.byref(inp), C.byref(res), None) == -1  # null col_off
        for t in range(5):
            inp.col_off[t] = dev.up(np.zeros(3, np.uint64))
        inp.n_bytes = 16
        assert L.cdr_load_cql_rows(engine_gpu.ctx, C.byref(inp), C.byref(res), None) == -1  # null bytes
        inp.bytes, inp.n_bytes = so, 1 << 35
        assert L.cdr_load_cql_rows(engine_gpu.ctx, C.byref(inp), C.byref(res), None) == -1  # row indices are 32 bits
        inp.n_bytes = 16
        assert L.cdr_load_cql_rows(engine_gpu.ctx, C.byref(inp), C.byref(res), None) == 0
        assert list(res.n_rows) == [0] * 5 and res.rows.n_strings == 1
    finally:
        dev.free()


def _ms_state():
    """A state whose times are whole milliseconds, with every started / heartbeat combination a
    replay leaves set by hand on its first activity rows."""
    b, out, strs = _state(5)
    out = _copy_outputs(b, out)
    k = 0
    for w in range(b.n_wfs):
        if out.result[w].code != abi.OK:
            continue
        for t, fs in TIME_FIELDS.items():
            off = getattr(out.plan.caps[w], t + "_off")
            for j in range(getattr(out.result[w], engine.TABLE_COUNT[t])):
                r = out.tables[t][off + j]
                for f in fs:
                    setattr(r, f, getattr(r, f) // 1_000_000 * 1_000_000)
                if t == "act" and k < 40:
                    r.flags &= ~(abi.AI_STARTED_TIME_SET | abi.AI_HEARTBEAT_TIME_SET)
                    r.started_time = r.last_heartbeat_time = 0
                    if k % 4:
                        r.flags |= abi.AI_STARTED_TIME_SET
                        r.started_time = (0, -7_000_000, 1_600_000_000_000_000_000)[k % 3]
                        r.last_heartbeat_time = (0, 1_600_000_001_000_000_000)[k % 2]
                    k += 1
    assert k == 40
    return b, out, strs


@pytest.mark.gpu
def test_gpu_both_forms_load_alike(engine_gpu):
    """(10) one state with whole-millisecond times, encoded both ways and loaded by
    cdr_load_rows and by cdr_load_cql_rows with the same seeds: identical records, handles and
    string tables."""
    b, out, strs = _ms_state()
    seeds = strs[:len(strs) // 4]
    sql = rows.load(engine_gpu, rows.encode_state(engine_gpu, b, out, strs), seeds)
    cql = rows.load_cql(engine_gpu, rows.encode_state_cql(engine_gpu, b, out, strs), seeds)
    assert not sql.n_bad_entries and not cql.n_bad_entries
    assert cql.strings == sql.strings and len(sql.strings) > len(seeds)
    assert any(r.nonretriable for r in sql.tables["act"]) and any(r.started_run_id for r in sql.tables["child"])
    for t in TABLES:
        assert len(cql.tables[t]) == len(sql.tables[t]) > 0 and bytes(cql.tables[t]) == bytes(sql.tables[t]), t
    assert bytes(cql.result) == bytes(sql.result) and bytes(cql.caps) == bytes(sql.caps)
    assert cql.entry_status.tolist() == sql.entry_status.tolist()


def _loaded_of(want, n_entries) -> rows.Loaded:
    """The restatement's decode as a rows.Loaded (what rows.to_carry takes)."""
    tables = {}
    for i, t in enumerate(TABLES):
        ty = engine.TABLE_TYPES[t]
        raw = b"".join(r if r is not None else bytes(C.sizeof(ty)) for r in want.tables[i])
        tables[t] = (ty * len(want.tables[i])).from_buffer_copy(raw) if raw else (ty * 0)()
    result = (abi.CdrWfResult * max(1, n_entries))()
    caps = (abi.CdrWfCaps * max(1, n_entries))()
    tot = abi.CdrTotals()
    for i, t in enumerate(TABLES):
        setattr(tot, t, want.n_rows[i])
    for w in range(n_entries):
        result[w].code = want.result[w][0]
        for i, t in enumerate(TABLES):
            setattr(result[w], engine.TABLE_COUNT[t], want.result[w][1 + i])
            setattr(caps[w], t + "_off", want.caps[w][0][i])
            setattr(caps[w], t + "_cap", want.caps[w][1][i])
    return rows.Loaded(tables, result, caps, tot, want.row_status, np.array(want.entry_status, np.int32), want.strings,
                       None, None, b"", sum(1 for s in want.entry_status if s))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [3, 5])
def test_gpu_replay_closes_the_loop(engine_gpu, cfg):
    """(11) prefix replay -> encode_state_cql -> load_cql -> to_carry -> suffix replay == the
    oracle's carry-in replay of the suffix onto the restatement's decoded state; the mutation of
    that replay == the reference diff."""
    import oracle
    from tests import mutation_ref
    b = engine.synth_batch(cfg, 300, seed=0x5EED0D00 + cfg)
    cut = engine.split_half(b)
    assert (cut > 0).sum() > 100
    pre, suf = engine.cut_batches(b, cut)
    pre_out = engine_gpu.replay(pre)
    strs = rows.state_strings(pre, pre_out)
    cols = rows.encode_state_cql(engine_gpu, pre, pre_out, strs)
    got = rows.load_cql(engine_gpu, cols, strs)  # seeds = the whole table: the batch's handles stay
    want = ref.decode(cols, strs)
    assert not ref.compare_cql(got, want, cols)
    assert sum(got.n_rows) > 500 and all(n > 0 for n in got.n_rows) and not got.n_bad_entries and got.strings == strs
    src = np.where((cut > 0) & np.array([pre_out.result[w].code == abi.OK for w in range(b.n_wfs)]),
                   np.arange(b.n_wfs), -1)
    suf.carry = rows.to_carry(got, pre_out, src)
    out = engine_gpu.replay(suf)
    carry = suf.carry
    suf.carry = rows.to_carry(_loaded_of(want, b.n_wfs), pre_out, src)
    expected = oracle.replay(suf)
    suf.carry = carry
    bad = engine.compare(suf, out, expected)
    assert not bad, bad[:5]
    assert sum(1 for w in range(b.n_wfs) if expected.result[w].code == abi.OK and src[w] >= 0) > 100
    mut = engine_gpu.mutation(suf, out)
    bad = mutation_ref.check(suf, out, mut)
    assert not bad, "\n".join(bad[:10])
