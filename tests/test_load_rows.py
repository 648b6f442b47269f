"""Loading persisted pending-table rows on the device (cdr.h cdr_load_rows, csrc/load.hip):
the inverse of the SQL row encoders, checked against tests/rows_ref.py.

CPU: the reference decoder inverts oracle/thrift_binary.py's writers on replayed states of
the synthetic configs 2-5 (records byte for byte, blobs byte for byte after re-encoding),
handles the wire edges (hand-built blobs, tests/thrift_cases.py's builders) the way
cdr/ingest.h states them, and the ABI mirrors match.  GPU (-m gpu): the device decoder ==
the reference record for record and status for status on those states, on the hand-made
edge states of tests/encode_edges.py, on shuffled rows, duplicate keys, every wire edge,
every truncation, a blob that claims to run past the buffer, and the string-table rules;
its output feeds the encoders back to the input blobs and a carry-in replay to the
oracle's final states.
"""
import ctypes as C
import functools
import os
import random
import re
import struct
from types import SimpleNamespace

import numpy as np
import pytest

from cadence_amd import abi, engine, ingest, rows
from oracle import thrift_binary as tb
from oracle import thrift_decode as TD
from tests import rows_ref as ref
from tests import thrift_cases as tc
from tests.thrift_cases import F, Lst, Raw, St

TABLES = rows.TABLES
ZT = abi.ZERO_TIME_NANOS
U = b"0123abcd-89ef-4c5d-8a7b-fedcba987654"
WRITER = {"act": tb.activity_info_blob, "child": tb.child_info_blob, "signal": tb.signal_info_blob,
          "timer": lambda r, S: tb.timer_info_blob(r), "cancel": lambda r, S: tb.request_cancel_info_blob(r)}


# ---------------------------------------------------------------- replayed states
def _copy_outputs(b, out):
    cp = engine.Outputs(b, out.plan)
    C.memmove(cp.result, out.result, C.sizeof(out.result))
    C.memmove(cp.exec, out.exec, C.sizeof(out.exec))
    C.memmove(cp.repl, out.repl, C.sizeof(out.repl))
    for t in engine.TABLES:
        C.memmove(cp.tables[t], out.tables[t], C.sizeof(out.tables[t]))
    return cp


@functools.lru_cache(maxsize=None)
def _state(cfg):
    """(batch, oracle-replayed states with the pending tables' handles renumbered densely,
    the table of distinct strings over those handles): the synthetic generator spreads its
    handles over a million values, a table the tests would spend their time hashing."""
    import oracle
    b = engine.synth_batch(cfg, 300, seed=0x5EED0900 + cfg)
    if cfg == 2:  # a finished config-2 workflow has no pending rows: its first half has
        b, _ = engine.cut_batches(b, engine.split_half(b))
    out = _copy_outputs(b, oracle.replay(b))
    full = rows.state_strings(b, out)
    used = sorted({getattr(r, f) for w in range(b.n_wfs) if out.result[w].code == abi.OK for t in TABLES
                   for r in out.rows(w, t) for f in rows.HANDLES[t]} - {0})
    dense = {h: i + 1 for i, h in enumerate(used)}
    dense[0] = 0
    for w in range(b.n_wfs):
        if out.result[w].code != abi.OK:
            continue
        for t in TABLES:
            off = getattr(out.plan.caps[w], t + "_off")
            for j in range(getattr(out.result[w], engine.TABLE_COUNT[t])):
                r = out.tables[t][off + j]
                for f in rows.HANDLES[t]:
                    setattr(r, f, dense[getattr(r, f)])
    strs = [b""] + [full[h] for h in used]
    assert len(set(strs)) == len(strs)
    return b, out, strs


def _normal(t, rec) -> bytes:
    """The record as a load gives it back: HEARTBEAT cleared where both time bits are set."""
    if t == "act" and rec.flags & abi.AI_STARTED_TIME_SET and rec.flags & abi.AI_HEARTBEAT_TIME_SET:
        rec = type(rec).from_buffer_copy(bytes(rec))
        rec.flags &= ~abi.AI_HEARTBEAT_TIME_SET
    return bytes(rec)


def _oracle_rows(b, out, strs) -> rows.Rows:
    """encode_state with the oracle's writers."""
    S = tb.lookup(strs)
    tables = []
    for t in TABLES:
        per = []
        for w in range(b.n_wfs):
            rs = []
            for r in (out.rows(w, t) if out.result[w].code == abi.OK else []):
                blob = WRITER[t](r, S)
                rs.append((strs[r.timer_id], blob) if t == "timer" else
                          (r.schedule_id, blob, rows.heartbeat_column(r)) if t == "act" else (r.initiated_id, blob))
            per.append(rs)
        tables.append(per)
    return rows.pack(b.n_wfs, tables)


def _check_against_state(b, out, R, tables_of, result_of):
    """The decoded tables hold the states' own records."""
    n = 0
    for w in range(b.n_wfs):
        ok = out.result[w].code == abi.OK
        for i, t in enumerate(TABLES):
            want = [_normal(t, r) for r in out.rows(w, t)] if ok else []
            assert result_of(w)[1 + i] == len(want), (w, t)
            base = int(R.entry_row0[i][w])
            for j, rec in enumerate(want):
                assert tables_of(i, base + j) == rec, (w, t, j)
                n += 1
    return n


# ---------------------------------------------------------------- CPU
@pytest.mark.parametrize("cfg", [2, 3, 4, 5])
def test_reference_round_trip(cfg):
    b, out, strs = _state(cfg)
    R = _oracle_rows(b, out, strs)
    dec = ref.decode(R, strs)
    assert not any(dec.entry_status) and not any(any(s) for s in dec.row_status)
    assert dec.strings == strs  # seeds = the whole table: nothing new, every handle kept
    n = _check_against_state(b, out, R, lambda i, slot: dec.tables[i][slot], lambda w: dec.result[w])
    assert n > 0
    S = tb.lookup(dec.strings)
    for i, t in enumerate(TABLES):
        ty = engine.TABLE_TYPES[t]
        for slot, raw in enumerate(dec.tables[i]):
            assert WRITER[t](ty.from_buffer_copy(raw), S) == R.blob(i, slot), (t, slot)


def _base_fields(t, v=0):
    """The row struct of table t with every IDL field set (values vary with v)."""
    s, i32, i64, b = tc.s, tc.i32, tc.i64, tc.boolean
    if t == 0:
        return [i64(10, 7 + v), i64(12, 5 + v), s(14, b"sched-event"), s(16, b"thriftrw"), i64(18, 10**18 + v),
                i64(20, 9 + v), s(22, b"started-event"), s(24, b"thriftrw"), i64(26, 10**18 + 5 + v),
                s(28, b"act-%d" % v), s(30, b"req-%d" % v), i32(32, 11 + v), i32(34, 12 + v), i32(36, 13 + v),
                i32(38, 14 + v), b(40, v == 0), i64(42, 77 + v), i32(44, 3 + v), i32(46, 2 + v), s(48, b"tl-%d" % v),
                s(50, b"identity"), b(52, True), i32(54, 1 + v), i32(56, 60 + v), i32(58, 4 + v),
                i64(60, 2 * 10**18 + v), F(tc.T_DOUBLE, 62, 1.5 + v), tc.lst(64, tc.T_STRING, [b"bad", b"e%d" % v]),
                s(66, b"reason"), s(68, b"worker"), s(70, b"details")]
    if t == 1:
        return [i64(10, 7 + v), i64(12, 21 + v), i64(14, 10**18 + v), i64(16, 9000 + v)]
    if t == 2:
        return [i64(10, 7 + v), i64(12, 30 + v), i64(14, 33 + v), s(16, b"init-event"), s(18, b"thriftrw"),
                s(20, b"child-wf-%d" % v), s(22, bytes(range(16 * v, 16 * v + 16))), s(24, b"started-event"),
                s(26, b"thriftrw"), s(28, U[:-1] + b"%d" % v), s(30, b"dom-%d" % v), s(32, b"type-%d" % v),
                i32(35, 1 + v)]
    if t == 3:
        return [i64(10, 7 + v), i64(11, 40 + v), s(12, U[:-1] + b"%d" % v)]
    return [i64(10, 7 + v), i64(11, 50 + v), s(12, U[:-1] + b"%d" % v), s(14, b"sig-%d" % v), s(16, b"input-%d" % v),
            s(18, b"ctl-%d" % v)]


def _blob(fields) -> bytes:
    return tc.value(tc.T_STRUCT, St("row", fields))


def _wrong(f):
    """The field again with a wire type the IDL does not give it."""
    return F(tc.T_STRING, f.fid, b"zz") if f.t != tc.T_STRING else F(tc.T_I64, f.fid, 5)


@functools.lru_cache(maxsize=None)
def wire_cases():
    """[(name, table, blob, expected)]: expected is a status, or the plain blob whose decode
    the edge blob must equal."""
    cases = []
    for t in range(5):
        base = _base_fields(t)
        plain = _blob(base)
        cases.append(("plain", t, plain, plain))
        cases.append(("reversed order", t, _blob(base[::-1]), plain))
        sh = list(base)
        random.Random(17 + t).shuffle(sh)
        cases.append(("shuffled order", t, _blob(sh), plain))
        unk = [F(ty, 900 + k, v) for k, (_, ty, v) in enumerate(tc.unknown_values())]
        cases.append(("unknown fields after", t, _blob(base + unk), plain))
        cases.append(("unknown fields before", t, _blob(unk + base), plain))
        mixed = [x for pair in zip(base, unk * 2) for x in pair] + base[len(unk * 2):]
        cases.append(("unknown fields between", t, _blob(mixed), plain))
        cases.append(("wrong types after", t, _blob(base + [_wrong(f) for f in base]), plain))
        cases.append(("wrong types before", t, _blob([_wrong(f) for f in base] + base), plain))
        cases.append(("repeated fields", t, _blob(base + _base_fields(t, 1)), _blob(_base_fields(t, 1))))
        cases.append(("repeated then wrong type", t, _blob(base + _base_fields(t, 1) + [_wrong(f) for f in base]),
                      _blob(_base_fields(t, 1))))
        cases.append(("trailing bytes", t, plain + b"\x0b\x00\x0a\xff\xff", plain))
        cases.append(("trailing zero", t, plain + b"\x00", plain))
        cases.append(("empty struct", t, b"\x00", abi.LOAD_E_UUID if t >= 2 else b"\x00"))  # no request ID
        for kind in ("struct", "list", "map"):
            for levels, want in ((TD.MAX_DEPTH, plain), (TD.MAX_DEPTH + 1, TD.DEC_DEPTH)):
                ty, v = tc.nested(kind, levels)
                cases.append((f"{kind} depth {levels}", t, _blob(base[:2] + [F(ty, 901, v)] + base[2:]), want))
        cases.append(("negative string length", t, _blob(base + [F(tc.T_STRING, 902, Raw(struct.pack(">i", -1)))]),
                      TD.DEC_BAD_SIZE))
        cases.append(("negative list count", t, _blob([F(tc.T_LIST, 903, Raw(struct.pack(">bi", 8, -5)))] + base),
                      TD.DEC_BAD_SIZE))
        cases.append(("negative map count", t, _blob(base + [F(tc.T_MAP, 904, Raw(struct.pack(">bbi", 8, 8, -1)))]),
                      TD.DEC_BAD_SIZE))
        for bad_type in (1, 5, 7, 9, 16, 0x7F):
            cases.append((f"wire type {bad_type}", t, _blob(base[:1] + [F(bad_type, 905, Raw(b"\0\0"))] + base[1:]),
                          TD.DEC_BAD_TYPE))
        cases.append(("no stop byte", t, plain[:-1], TD.DEC_TRUNCATED))
        cases.append(("empty blob", t, b"", TD.DEC_TRUNCATED))
        fid = {2: 28, 3: 12, 4: 12}.get(t)
        if fid:
            for name, text in (("uppercase", U.upper()), ("32 hex", U.replace(b"-", b"")), ("35 chars", U[:-1]),
                               ("37 chars", U + b"0"), ("braces", b"{" + U[1:-1] + b"}"), ("empty", b""),
                               ("dash moved", U[:8] + U[9:10] + b"-" + U[10:]), ("non-hex", U[:20] + b"g" + U[21:]),
                               ("mixed case", U[:3] + b"A" + U[4:])):
                edit = [F(tc.T_STRING, fid, text) if f.fid == fid else f for f in base]
                cases.append((f"request ID {name}", t, _blob(edit), abi.LOAD_E_UUID))
            cases.append(("request ID absent", t, _blob([f for f in base if f.fid != fid]), abi.LOAD_E_UUID))
            cases.append(("request ID canonical then wrong type", t,
                          _blob(base + [F(tc.T_I64, fid, 1)]), plain))
        if t == 2:
            no_run = _blob([f for f in base if f.fid != 22])
            for n, want in ((0, no_run), (15, abi.LOAD_E_UUID), (16, None), (17, abi.LOAD_E_UUID), (36, abi.LOAD_E_UUID)):
                blob = _blob([tc.s(22, bytes(range(200, 200 + n))) if f.fid == 22 else f for f in base])
                cases.append((f"run ID of {n} bytes", t, blob, blob if want is None else want))
        if t == 0:
            no_list = _blob([f for f in base if f.fid != 64])
            cases.append(("empty error list", t, _blob([tc.lst(64, tc.T_STRING, []) if f.fid == 64 else f for f in base]),
                          no_list))
            cases.append(("error list of i64", t, _blob([tc.lst(64, tc.T_I64, [1, 2]) if f.fid == 64 else f for f in base]),
                          no_list))
            cases.append(("error list replaced by a list of i32", t, _blob(base + [tc.lst(64, tc.T_I32, [1])]), no_list))
            cases.append(("error list as a set", t, _blob([F(tc.T_SET, 64, Lst(tc.T_STRING, [b"x"])) if f.fid == 64 else f
                                                           for f in base]), no_list))
            cases.append(("started time absent", t, _blob([f for f in base if f.fid != 26]),
                          _blob([tc.i64(26, 0) if f.fid == 26 else f for f in base])))
    return cases


KEY_OF = {0: 501, 2: 502, 3: 503, 4: 504}


def _one(t, blob):
    key = b"timer-key" if t == 1 else KEY_OF[t]
    return ref.parse_row(t, blob, 0, len(blob), key, 10**18 + 99)


def _same(a, b):
    return bytes(a[0]) == bytes(b[0]) and a[1] == b[1]


def test_reference_wire_edges():
    seen = set()
    for name, t, blob, want in wire_cases():
        if isinstance(want, int):
            with pytest.raises((TD.DecodeError, ref.RowError)) as e:
                _one(t, blob)
            assert e.value.code == want, (name, t)
            seen.add(want)
        else:
            assert _same(_one(t, blob), _one(t, want)), (name, t)
    assert seen == {TD.DEC_TRUNCATED, TD.DEC_DEPTH, TD.DEC_BAD_SIZE, TD.DEC_BAD_TYPE, abi.LOAD_E_UUID}
    # what the plain blobs decode to, spelled out once
    a, s = _one(0, _blob(_base_fields(0)))
    assert (a.version, a.schedule_id, a.scheduled_event_batch_id, a.started_id, a.started_time) == (7, 501, 5, 9, 10**18 + 5)
    assert a.flags == abi.AI_CANCEL_REQUESTED | abi.AI_HAS_RETRY | abi.AI_STARTED_TIME_SET
    assert (a.last_heartbeat_time, a.backoff_coefficient, a.expiration_time) == (10**18 + 99, 1.5, 2 * 10**18)
    assert s == {"activity_id": b"act-0", "request_id": b"req-0", "task_list": b"tl-0",
                 "nonretriable": struct.pack(">bi", 11, 2) + b"\0\0\0\x03bad\0\0\0\x02e0"}
    a, _ = _one(0, _blob([tc.i64(26, ZT)]))
    assert (a.flags, a.started_time, a.last_heartbeat_time) == (abi.AI_HEARTBEAT_TIME_SET, 0, 10**18 + 99)
    a, _ = ref.parse_row(0, b"\x00", 0, 1, 1, ZT)
    assert (a.flags, a.started_time, a.last_heartbeat_time) == (abi.AI_STARTED_TIME_SET, 0, 0)
    c, s = _one(2, _blob(_base_fields(2)))
    assert (c.create_request_hi, c.create_request_lo) == (0x0123abcd89ef4c5d, 0x8a7bfedcba987650)
    assert s["started_run_id"] == b"00010203-0405-0607-0809-0a0b0c0d0e0f"


def test_abi_mirrors():
    L = abi.lib()
    assert L.cdr_struct_size(b"cdr_rows_in") == C.sizeof(abi.CdrRowsIn) == 200
    assert L.cdr_struct_size(b"cdr_rows_out") == C.sizeof(abi.CdrRowsOut) == 296
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "cdr", "cdr.h")).read()
    sch = open(os.path.join(root, "include", "cdr", "schema.h")).read()
    ing = open(os.path.join(root, "include", "cdr", "ingest.h")).read()
    assert int(re.search(r"#define CDR_LOAD_E_UUID (\d+)", hdr).group(1)) == abi.LOAD_E_UUID == ref.E_UUID
    assert int(re.search(r"#define CDR_LOAD_E_DUP_KEY (\d+)", hdr).group(1)) == abi.LOAD_E_DUP_KEY
    assert int(re.search(r"#define CDR_LOAD_E_ENTRY_ROWS (\d+)", hdr).group(1)) == abi.LOAD_E_ENTRY_ROWS == 18
    assert int(re.search(r"#define CDR_LOAD_MAX_ENTRY_ROWS (\d+)u", hdr).group(1)) == abi.LOAD_MAX_ENTRY_ROWS
    dec = [int(v) for v in re.findall(r"#define CDR_DEC_[A-Z_]+ (\d+)", ing)]
    assert max(dec) < abi.LOAD_E_UUID < abi.LOAD_E_DUP_KEY and sorted(dec) == sorted(k for k in abi.DEC_STATUS)
    assert int(re.search(r"CDR_E_LOAD_ROWS = (\d+)", sch).group(1)) == abi.E_LOAD_ROWS
    codes = [int(v) for v in re.findall(r"\bCDR_[A-Z]+_[A-Z_0-9]+ = (\d+),? +/\*", sch.split("enum cdr_status")[1].split("};")[0])]
    assert codes.count(abi.E_LOAD_ROWS) == 1 and abi.STATUS[abi.E_LOAD_ROWS] == "E_LOAD_ROWS"
    assert abi.STR_REF_SEED == 1 << 63 and abi.STR_REF_GEN == 1 << 62


# ---------------------------------------------------------------- GPU
def _assert_equal(got, R, seeds):
    want = ref.decode(R, seeds)
    bad = ref.compare(got, want, R)
    assert not bad, "\n".join(bad[:10])
    return want


def _unpack(R):
    """rows.pack's input form of a Rows."""
    tables = []
    for t in range(5):
        per = []
        for w in range(R.n_entries):
            rs = []
            for r in range(int(R.entry_row0[t][w]), int(R.entry_row0[t][w + 1])):
                rs.append((R.timer_id(r), R.blob(t, r)) if t == 1 else
                          (int(R.key[t][r]), R.blob(t, r), int(R.act_heartbeat[r])) if t == 0 else
                          (int(R.key[t][r]), R.blob(t, r)))
            per.append(rs)
        tables.append(per)
    return tables


@pytest.mark.gpu
def test_gpu_round_trip_batches(engine_gpu):
    """(1) the GPU encoders' blobs of replayed states decode to the reference's result and to
    the states' own records; the generated run-ID path is hit."""
    started = 0
    for cfg in (2, 3, 4, 5):
        b, out, strs = _state(cfg)
        R = rows.encode_state(engine_gpu, b, out, strs)
        assert R.bytes.tobytes() == _oracle_rows(b, out, strs).bytes.tobytes()
        got = rows.load(engine_gpu, R, strs)
        _assert_equal(got, R, strs)
        raw = {i: bytes(got.tables[t]) for i, t in enumerate(TABLES)}
        size = [C.sizeof(engine.TABLE_TYPES[t]) for t in TABLES]
        res = lambda w: (got.result[w].code, got.result[w].n_activity, got.result[w].n_timer, got.result[w].n_child,  # noqa: E731
                         got.result[w].n_cancel, got.result[w].n_signal)
        assert _check_against_state(b, out, R, lambda i, s: raw[i][s * size[i]:(s + 1) * size[i]], res) > 0
        assert got.strings == strs and not got.n_bad_entries
        started += sum(1 for r in got.tables["child"] if r.started_run_id)
        assert any(x & abi.STR_REF_SEED for x in got.str_ref.tolist())
    assert started > 0


@functools.lru_cache(maxsize=None)
def _hand_made_rows(eng):
    from tests import encode_edges
    hm = encode_edges.hand_made()
    R = rows.encode_state(eng, hm.batch, hm.out, hm.T.strs)
    # the rows left out are the ones the oracle's writers refuse (a timer's blob holds no
    # string: its refusal is the key column's handle past the table)
    for i, t in enumerate(TABLES):
        want = encode_edges.expected(t, "sql")
        kept = []
        for w in range(hm.batch.n_wfs):
            if hm.out.result[w].code == abi.OK:
                base = getattr(hm.out.plan.caps[w], t + "_off")
                kept += [(w, j) for j, r in enumerate(hm.out.rows(w, t))
                         if want[base + j][1] == 0 and (t != "timer" or r.timer_id < hm.T.n)]
        assert R.src[i] == kept, t
        assert len(kept) < sum(len(hm.out.rows(w, t)) for w in range(hm.batch.n_wfs)
                               if hm.out.result[w].code == abi.OK) or t == "cancel", t
    # the hand-made rows draw their keys from short cycles of edge values: keep each key's
    # first use in an entry (the extremes stay) and give its repeats keys of their own
    tabs = _unpack(R)
    for t in range(5):
        for rs in tabs[t]:
            seen = set()
            for j, row in enumerate(rs):
                k = row[0]
                while k in seen:
                    k = k + b"#%d" % j if t == 1 else \
                        ((k * 6364136223846793005 + 1442695040888963407 + j + 2**63) % 2**64) - 2**63
                seen.add(k)
                rs[j] = (k,) + row[1:]
    R2 = rows.pack(R.n_entries, tabs)
    R2.src = R.src
    return hm, R2


@pytest.mark.gpu
def test_gpu_hand_made_states(engine_gpu):
    """(2) 0 / 1 / 63 / 64 / 65 / 1000-row entries beside empty ones, integer, double and
    timestamp extremes, strings of every length class; a few seeds, the rest new."""
    hm, R = _hand_made_rows(engine_gpu)
    assert max(int(R.entry_row0[0][w + 1] - R.entry_row0[0][w]) for w in range(R.n_entries)) == 1000
    seeds = hm.T.strs[:12]
    got = rows.load(engine_gpu, R, seeds)
    want = _assert_equal(got, R, seeds)
    assert not any(want.entry_status) and len(want.strings) > len(seeds)
    assert any(x & abi.STR_REF_GEN for x in got.str_ref.tolist())


@pytest.mark.gpu
def test_gpu_row_order(engine_gpu):
    """(3) rows shuffled within every entry (the 1000-row entry reversed): ascending output,
    equal to the unshuffled result."""
    hm, R = _hand_made_rows(engine_gpu)
    seeds = [b""]
    base = rows.load(engine_gpu, R, seeds)
    tabs = _unpack(R)
    rng = random.Random(0x10AD)
    for t in range(5):
        for w, rs in enumerate(tabs[t]):
            if len(rs) == 1000:
                rs.reverse()
            else:
                rng.shuffle(rs)
    R2 = rows.pack(R.n_entries, tabs)
    assert R2.bytes.tobytes() != R.bytes.tobytes()
    got = rows.load(engine_gpu, R2, seeds)
    assert got.strings == base.strings and not got.n_bad_entries
    for t in TABLES:
        assert bytes(got.tables[t]) == bytes(base.tables[t]), t
    for w in range(R.n_entries):
        for t in TABLES:
            ks = [r.timer_id if t == "timer" else getattr(r, rows.KEY[t]) for r in got.rows(w, t)]
            assert ks == sorted(ks) and len(set(ks)) == len(ks), (w, t)
    _assert_equal(got, R2, seeds)


@pytest.mark.gpu
def test_gpu_duplicate_key(engine_gpu):
    """(4) one duplicate key in a single entry of each table: only that entry fails."""
    b, out, strs = _state(3)
    R = _oracle_rows(b, out, strs)
    tabs = _unpack(R)
    hit = {}
    for t in range(5):
        w = next(w for w in range(R.n_entries) if len(tabs[t][w]) >= 2 and w not in hit.values()
                 and 0 < w < R.n_entries - 1)
        hit[t] = w
        rs = tabs[t][w]
        rs[-1] = (rs[0][0],) + rs[-1][1:]
    R2 = rows.pack(R.n_entries, tabs)
    got = rows.load(engine_gpu, R2, strs)
    want = _assert_equal(got, R2, strs)
    base = rows.load(engine_gpu, R, strs)
    for w in range(R.n_entries):
        if w in hit.values():
            assert got.entry_status[w] == abi.LOAD_E_DUP_KEY and got.result[w].code == abi.E_LOAD_ROWS
            assert (got.result[w].n_activity, got.result[w].n_timer, got.result[w].n_child) == (0, 0, 0)
        else:
            assert got.entry_status[w] == 0
            for t in TABLES:
                assert [bytes(r) for r in got.rows(w, t)] == [bytes(r) for r in base.rows(w, t)], (w, t)
    assert got.n_bad_entries == 5 and sum(1 for s in want.row_status for x in s if x == abi.LOAD_E_DUP_KEY) == 10


@pytest.mark.gpu
def test_gpu_entry_row_limit(engine_gpu):
    """An entry may hold CDR_LOAD_MAX_ENTRY_ROWS rows of a table and no more: the ranking walks
    an entry's rows from every one of its lanes, and the limit bounds that."""
    n = abi.LOAD_MAX_ENTRY_ROWS
    blob = _blob(_base_fields(3))
    tabs = [[[] for _ in range(3)] for _ in range(5)]
    tabs[3][0] = [(n - k, blob) for k in range(n)]
    tabs[3][1] = [(k, blob) for k in range(n + 1)]
    tabs[3][2] = [(5, blob)]
    tabs[1][1] = [(b"timer", _blob(_base_fields(1)))]
    R = rows.pack(3, tabs)
    got = rows.load(engine_gpu, R, [b""])
    assert got.entry_status.tolist() == [0, abi.LOAD_E_ENTRY_ROWS, 0]
    assert [r.code for r in got.result] == [abi.OK, abi.E_LOAD_ROWS, abi.OK] and got.result[0].n_cancel == n
    st = got.row_status[3]
    assert not st[:n].any() and (st[n:2 * n + 1] == abi.LOAD_E_ENTRY_ROWS).all() and st[-1] == 0
    assert [r.initiated_id for r in got.rows(0, "cancel")] == list(range(1, n + 1))
    _assert_equal(got, R, [b""])


def test_reference_entry_row_limit(monkeypatch):
    """The reference's rule at a limit it walks quickly: every row of the table over the limit
    has the status, a lower table's failure comes first, other tables and entries are untouched."""
    monkeypatch.setattr(abi, "LOAD_MAX_ENTRY_ROWS", 3)
    blob, tim = _blob(_base_fields(3)), _blob(_base_fields(1))
    tabs = [[[] for _ in range(3)] for _ in range(5)]
    tabs[3][0] = [(k, blob) for k in range(3)]
    tabs[3][1] = [(k % 2, blob) for k in range(4)]
    tabs[1][1] = [(b"t", tim)]
    tabs[3][2] = [(k, blob) for k in range(4)]
    tabs[1][2] = [(b"t", tim), (b"t", tim)]
    want = ref.decode(rows.pack(3, tabs), [b""])
    assert want.entry_status == [0, abi.LOAD_E_ENTRY_ROWS, abi.LOAD_E_DUP_KEY]
    assert want.row_status[3] == [0] * 3 + [abi.LOAD_E_ENTRY_ROWS] * 8
    assert want.row_status[1] == [0, abi.LOAD_E_DUP_KEY, abi.LOAD_E_DUP_KEY]


def _entries_of(cases):
    """One entry per (table, key column, blob): a Rows."""
    tabs = [[[] for _ in cases] for _ in range(5)]
    for w, (t, blob) in enumerate(cases):
        tabs[t][w].append((b"timer-%d" % (w % 3), blob) if t == 1 else (KEY_OF[t] + w, blob, 10**18 + w) if t == 0
                          else (KEY_OF[t] + w, blob))
    return rows.pack(len(cases), tabs)


@pytest.mark.gpu
def test_gpu_wire_edges(engine_gpu):
    """(5a) every wire-edge blob of the CPU test, each in an entry of its own."""
    cases = wire_cases()
    R = _entries_of([(t, blob) for _, t, blob, _ in cases])
    seeds = [b"", b"act-0", b"tl-1", b"timer-1", b"no such string"]
    got = rows.load(engine_gpu, R, seeds)
    _assert_equal(got, R, seeds)
    for w, (name, t, blob, want) in enumerate(cases):
        assert got.entry_status[w] == (want if isinstance(want, int) else 0), (name, t)


@pytest.mark.gpu
def test_gpu_truncation_at_every_length(engine_gpu):
    """(5b) one blob per table cut at every length: CDR_DEC_TRUNCATED each, and the whole
    rows between them (the same wave's staged range) decode unchanged."""
    cases = []
    for t in range(5):
        plain = _blob(_base_fields(t))
        for n in range(len(plain)):
            cases += [(t, plain), (t, plain[:n])]
        cases.append((t, plain))
    R = _entries_of(cases)
    got = rows.load(engine_gpu, R, [b""])
    _assert_equal(got, R, [b""])
    for w, (t, blob) in enumerate(cases):
        whole = len(blob) == len(_blob(_base_fields(t)))
        assert got.entry_status[w] == (0 if whole else TD.DEC_TRUNCATED), (w, t, len(blob))
        assert got.result[w].code == (abi.OK if whole else abi.E_LOAD_ROWS)


@pytest.mark.gpu
def test_gpu_buffer_end(engine_gpu):
    """(6) the last row of `bytes` is cut and its string claims to run past n_bytes, with
    `bytes` ending where its allocation ends: TRUNCATED, the call returns cleanly, and the
    rows before it decode."""
    plain = _blob(_base_fields(4))
    cut = _blob(_base_fields(4)[:3])[:-1] + struct.pack(">bhi", 11, 14, 1 << 20) + b"abc"
    for tail in (cut, cut[:-3], plain[:-1], plain[:5]):
        R = _entries_of([(4, plain), (0, _blob(_base_fields(0))), (4, tail)])
        assert R.blob(4, 1) == tail and int(R.blob_off[4][2]) == len(R.bytes)  # no timers: the signal blobs come last
        got = rows.load(engine_gpu, R, [b""], at_end=True)
        _assert_equal(got, R, [b""])
        assert got.entry_status.tolist() == [0, 0, TD.DEC_TRUNCATED]


def _sig(version, name, inp=b"", ctl=b""):
    g = SimpleNamespace(version=version, initiated_event_batch_id=version + 1, signal_request_lo=version,
                        signal_request_hi=1, signal_name=1, input=2 if inp else 0, control=3 if ctl else 0)
    return tb.signal_info_blob(g, lambda h: (b"", name, inp, ctl)[h])


@pytest.mark.gpu
def test_gpu_string_table(engine_gpu):
    """(7) seeds keep their handles, new strings are numbered by hash rank, a timer ID used
    in two entries and as an activity ID has one handle."""
    act = _blob([tc.s(28, b"shared-id"), tc.s(48, b"seeded"), tc.s(30, b"new-b")])
    tim = _blob(_base_fields(1))
    tabs = [[[] for _ in range(3)] for _ in range(5)]
    tabs[0][1] = [(5, act, ZT)]
    tabs[1][0] = [(b"shared-id", tim), (b"seeded", tim), (b"", tim)]
    tabs[1][2] = [(b"new-a", tim), (b"shared-id", tim)]
    tabs[4][2] = [(9, _sig(1, b"seeded", b"new-a", b"seeded-too"))]
    R = rows.pack(3, tabs)
    seeds = [b"", b"unused", b"seeded", b"seeded-too"]
    got = rows.load(engine_gpu, R, seeds)
    _assert_equal(got, R, seeds)
    new = sorted([b"shared-id", b"new-a", b"new-b"], key=TD.str_hash)
    assert got.strings == seeds + new
    h = {s: len(seeds) + i for i, s in enumerate(new)}
    assert got.rows(1, "act")[0].activity_id == h[b"shared-id"] and got.rows(1, "act")[0].task_list == 2
    assert sorted(r.timer_id for r in got.rows(0, "timer")) == sorted([0, 2, h[b"shared-id"]])
    assert sorted(r.timer_id for r in got.rows(2, "timer")) == sorted([h[b"new-a"], h[b"shared-id"]])
    g = got.rows(2, "signal")[0]
    assert (g.signal_name, g.input, g.control) == (2, h[b"new-a"], 3)


@pytest.mark.gpu
def test_gpu_many_strings(engine_gpu):
    """(7) more than 65,536 string fields in one call (70,000 signal rows with Input set,
    n_seeds = 1): the ranking's scan and sort cross their tiles."""
    n, per = 70_000, 100
    tabs = [[[] for _ in range(n // per)] for _ in range(5)]
    for k in range(n):
        tabs[4][k // per].append((n - k, _sig(k, b"sig-%d" % (k % 7), b"input-%05d" % k)))
    R = rows.pack(n // per, tabs)
    got = rows.load(engine_gpu, R, [b""])
    assert not got.n_bad_entries and not got.row_status[4].any()
    distinct = {b"sig-%d" % i for i in range(7)} | {b"input-%05d" % k for k in range(n)}
    assert got.strings == [b""] + sorted(distinct, key=TD.str_hash)
    for w in (0, 1, n // per - 1):  # rows arrive in descending key order
        rs = got.rows(w, "signal")
        assert [r.initiated_id for r in rs] == sorted(r.initiated_id for r in rs) and len(rs) == per
        for r in rs:
            k = n - r.initiated_id
            assert got.strings[r.input] == b"input-%05d" % k and got.strings[r.signal_name] == b"sig-%d" % (k % 7)
            assert (r.version, r.signal_request_lo, r.signal_request_hi) == (k, k, 1)


@pytest.mark.gpu
def test_gpu_strings_close_the_loop(engine_gpu):
    """(8) the decoded table, gathered on the device, and the decoded state go back through
    the encoders to the input blobs, byte for byte."""
    for cfg in (2, 3, 4, 5):
        b, out, strs = _state(cfg)
        R = rows.encode_state(engine_gpu, b, out, strs)
        seeds = strs[:len(strs) // 3]  # most strings are new: the handles differ from the states'
        got = rows.load(engine_gpu, R, seeds, gather=True)
        assert got.gathered == got.strings and sorted(got.strings[1:]) == sorted(strs[1:])
        state = rows.to_carry(got, out).state
        R2 = rows.encode_state(engine_gpu, b, state, got.gathered)
        assert R2.src == R.src and R2.n_rows == R.n_rows
        for t in range(5):
            assert [R2.blob(t, r) for r in range(R.n_rows[t])] == [R.blob(t, r) for r in range(R.n_rows[t])], t
        assert R2.bytes.tobytes() == R.bytes.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [3, 5])
def test_gpu_replay_closes_the_loop(engine_gpu, cfg):
    """(9) prefix replay -> encode_state -> load -> to_carry -> suffix replay == the oracle's
    replay of the whole histories; the mutation of that replay == the reference diff."""
    import oracle
    from tests import mutation_ref
    b = engine.synth_batch(cfg, 300, seed=0x5EED0A00 + cfg)
    cut = engine.split_half(b)
    assert (cut > 0).sum() > 100
    pre, suf = engine.cut_batches(b, cut)
    pre_out = engine_gpu.replay(pre)
    strs = rows.state_strings(pre, pre_out)
    R = rows.encode_state(engine_gpu, pre, pre_out, strs)
    assert sum(R.n_rows) > 500 and all(n > 0 for n in R.n_rows)
    got = rows.load(engine_gpu, R, strs)  # seeds = the whole table: the batch's handles stay
    assert not got.n_bad_entries and got.strings == strs
    src = np.where((cut > 0) & np.array([pre_out.result[w].code == abi.OK for w in range(b.n_wfs)]),
                   np.arange(b.n_wfs), -1)
    suf.carry = rows.to_carry(got, pre_out, src)
    out = engine_gpu.replay(suf)
    whole = oracle.replay(b)
    bad = engine.compare(b, out, whole)
    assert not bad, bad[:5]
    assert sum(1 for w in range(b.n_wfs) if whole.result[w].code == abi.OK and src[w] >= 0) > 100
    mut = engine_gpu.mutation(suf, out)
    bad = mutation_ref.check(suf, out, mut)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.gpu
def test_gpu_degenerate_sizes_and_misuse(engine_gpu):
    """(10) empty tables, zero entries, a repeated call on the warm context, null arguments."""
    empty = [[[] for _ in range(3)] for _ in range(5)]
    got = rows.load(engine_gpu, rows.pack(3, empty), [b""])
    assert [(r.code, r.n_activity, r.n_signal) for r in got.result] == [(abi.OK, 0, 0)] * 3
    assert got.entry_status.tolist() == [0, 0, 0] and got.strings == [b""] and bytes(got.caps) == bytes(len(bytes(got.caps)))
    got = rows.load(engine_gpu, rows.pack(0, [[] for _ in range(5)]), [b"", b"seed"])
    assert len(got.result) == 0 and got.strings == [b"", b"seed"] and got.n_bad_entries == 0
    b, out, strs = _state(5)
    R = _oracle_rows(b, out, strs)
    one, two = rows.load(engine_gpu, R, strs[:7]), rows.load(engine_gpu, R, strs[:7])
    for t in TABLES:
        assert bytes(one.tables[t]) == bytes(two.tables[t])
    assert bytes(one.result) == bytes(two.result) and bytes(one.caps) == bytes(two.caps) and one.strings == two.strings
    assert all((a == c).all() for a, c in zip(one.row_status, two.row_status))
    L = abi.lib()
    inp, res = abi.CdrRowsIn(), abi.CdrRowsOut()
    assert L.cdr_load_rows(engine_gpu.ctx, None, C.byref(res), None) == -1
    assert L.cdr_load_rows(engine_gpu.ctx, C.byref(inp), None, None) == -1
    assert L.cdr_load_rows(None, C.byref(inp), C.byref(res), None) == -1
    assert L.cdr_load_rows(engine_gpu.ctx, C.byref(inp), C.byref(res), None) == -1  # no seeds
    assert L.cdr_strtab_gather_async(engine_gpu.ctx, None, None, 0, None, None, None, None, None, None) == -1
    assert L.cdr_strtab_gather_async(None, None, None, 0, None, None, None, None, None, None) == -1
    bad = rows.pack(2, [[[(1, b"\x00", ZT)], []]] + [[[], []] for _ in range(4)])
    bad.entry_row0[0][2] = 2  # an entry range past the rows
    assert rows.load(engine_gpu, bad, [b""], check=False).rc == -1


@pytest.mark.gpu
def test_gpu_gather_on_an_ingest_table(engine_gpu):
    """(11) cdr_strtab_gather_async with gen_bytes == NULL on a cdr_ingest_out table."""
    b = engine.synth_batch(3, 60, seed=0x5EED0B00)
    enc = ingest.encode_batch(b)
    dec = ingest.decode(engine_gpu, enc)
    assert dec.raw.n_strings == len(dec.strings) > len(enc.seeds)
    table = rows.gather(engine_gpu, dec.raw.str_ref, dec.raw.str_len, dec.raw.n_strings, enc.blob_bytes, enc.seeds)
    assert table == [bytes(s) for s in dec.strings]
