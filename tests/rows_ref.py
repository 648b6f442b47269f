"""TEST INFRASTRUCTURE ONLY: Python reference of the persisted-row loader (cdr.h
cdr_load_rows, cadence_amd/csrc/load.hip), the parity checker for it.

It restates the contract of the header, independently of the device parser, on the
generic wire reader of oracle/thrift_decode.py (Reader / fget / Interner):

  * a blob is one bare binary-protocol struct; the bytes after its stop byte are ignored;
    fields in any order, the last occurrence of the right wire type wins, everything else
    is skipped under the depth limit of cdr/ingest.h (the row struct itself is walked, so
    each of its fields starts at level 1);
  * the field mapping is the inverse of oracle/thrift_binary.py's writers, following
    getActivityInfoMap / getTimerInfoMap / getChildExecutionInfoMap /
    getRequestCancelInfoMap / getSignalInfoMap (workflowStateMaps.go);
  * request IDs must be canonical lowercase UUID text, a child's StartedRunID 0 or 16 bytes
    (CDR_LOAD_E_UUID otherwise);
  * strings: seeds keep their handles, the others are numbered by hash rank; only rows of
    entries in which every row decoded are interned;
  * each entry's rows in ascending key order (timer key = the ID's handle), a repeated key
    is CDR_LOAD_E_DUP_KEY on every row that has it; more than CDR_LOAD_MAX_ENTRY_ROWS rows of
    an entry in one table are CDR_LOAD_E_ENTRY_ROWS, every one of them;
  * an entry fails with the status of its first failing row, lowest table then lowest row.
"""
from __future__ import annotations

import collections
import ctypes as C
import re

from cadence_amd import abi, engine
from cadence_amd.rows import TABLES
from oracle import thrift_decode as TD
from oracle.thrift_decode import T_BOOL, T_DOUBLE, T_I32, T_I64, T_LIST, T_STRING, T_STRUCT, Interner, Reader, fget

E_UUID, E_DUP_KEY, E_ENTRY_ROWS = abi.LOAD_E_UUID, abi.LOAD_E_DUP_KEY, abi.LOAD_E_ENTRY_ROWS
UUID_TEXT = re.compile(rb"[0-9a-f]{8}-[0-9a-f]{4}-[0-9a-f]{4}-[0-9a-f]{4}-[0-9a-f]{12}")
# a struct the decoder walks whose fields are all leaves or skipped values (thrift_decode.WALK)
_WALKED_LEAF = "name"
assert TD.WALK[_WALKED_LEAF] == {}


class RowError(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


def _request_id(b: bytes):
    if not UUID_TEXT.fullmatch(b):
        raise RowError(E_UUID)
    h = b.replace(b"-", b"")
    return int(h[16:], 16), int(h[:16], 16)  # lo, hi


def uuid_string(b: bytes) -> bytes:
    """sqldb.UUID(b).String() of 16 bytes."""
    h = b.hex()
    return f"{h[:8]}-{h[8:12]}-{h[12:16]}-{h[16:20]}-{h[20:]}".encode()


def parse_row(t: int, data: bytes, start: int, end: int, key, heartbeat: int = abi.ZERO_TIME_NANOS):
    """(record with its handle fields zero, {handle field: bytes}) of one row, or RowError /
    TD.DecodeError.  `key`: the key column (table 1: the timer ID's bytes)."""
    st = Reader(data, start, end).value(T_STRUCT, 0, _WALKED_LEAF)

    def g(fid, ft, default=0):
        v = fget(st, fid, ft)
        return default if v is None else v[0]
    strs = {}
    if t == 0:
        a = abi.CdrActivityInfo()
        a.schedule_id = key
        a.version, a.scheduled_event_batch_id = g(10, T_I64), g(12, T_I64)
        a.scheduled_time, a.started_id = g(18, T_I64), g(20, T_I64)
        started = g(26, T_I64)
        flags = (abi.AI_CANCEL_REQUESTED if g(40, T_BOOL) else 0) | (abi.AI_HAS_RETRY if g(52, T_BOOL) else 0)
        if started != abi.ZERO_TIME_NANOS:
            flags |= abi.AI_STARTED_TIME_SET
            a.started_time = started
        a.last_heartbeat_time = heartbeat if heartbeat != abi.ZERO_TIME_NANOS else 0
        if a.last_heartbeat_time and not flags & abi.AI_STARTED_TIME_SET:
            flags |= abi.AI_HEARTBEAT_TIME_SET
        a.flags = flags
        a.s2s, a.s2c, a.stc, a.hb = g(32, T_I32), g(34, T_I32), g(36, T_I32), g(38, T_I32)
        a.cancel_request_id, a.timer_task_status, a.attempt = g(42, T_I64), g(44, T_I32), g(46, T_I32)
        a.initial_interval, a.maximum_interval, a.maximum_attempts = g(54, T_I32), g(56, T_I32), g(58, T_I32)
        a.expiration_time = g(60, T_I64)
        d = fget(st, 62, T_DOUBLE)
        if d is not None:  # the bits, not the value (NaN payloads)
            raw = bytes(data[d[1][0]:d[1][1]])[::-1]
            C.memmove(C.addressof(a) + abi.CdrActivityInfo.backoff_coefficient.offset, raw, 8)
        strs = {"activity_id": g(28, T_STRING, b""), "request_id": g(30, T_STRING, b""),
                "task_list": g(48, T_STRING, b""), "nonretriable": b""}
        lst = fget(st, 64, T_LIST)
        if lst is not None and lst[0][1] == T_STRING and lst[0][2]:
            strs["nonretriable"] = bytes(data[lst[1][0]:lst[1][1]])
        return a, strs
    if t == 1:
        x = abi.CdrTimerInfo()
        x.version, x.started_id, x.expiry_time, x.task_id = g(10, T_I64), g(12, T_I64), g(14, T_I64), g(16, T_I64)
        return x, {"timer_id": bytes(key)}
    if t == 2:
        c = abi.CdrChildInfo()
        c.initiated_id = key
        c.version, c.initiated_event_batch_id, c.started_id = g(10, T_I64), g(12, T_I64), g(14, T_I64)
        c.parent_close_policy = g(35, T_I32)
        c.create_request_lo, c.create_request_hi = _request_id(g(28, T_STRING, b""))
        run = g(22, T_STRING, b"")
        if len(run) not in (0, 16):
            raise RowError(E_UUID)
        return c, {"started_workflow_id": g(20, T_STRING, b""), "started_run_id": uuid_string(run) if run else b"",
                   "domain_name": g(30, T_STRING, b""), "workflow_type": g(32, T_STRING, b"")}
    if t == 3:
        c = abi.CdrCancelInfo()
        c.initiated_id = key
        c.version, c.initiated_event_batch_id = g(10, T_I64), g(11, T_I64)
        c.cancel_request_lo, c.cancel_request_hi = _request_id(g(12, T_STRING, b""))
        return c, {}
    s = abi.CdrSignalInfo()
    s.initiated_id = key
    s.version, s.initiated_event_batch_id = g(10, T_I64), g(11, T_I64)
    s.signal_request_lo, s.signal_request_hi = _request_id(g(12, T_STRING, b""))
    return s, {"signal_name": g(14, T_STRING, b""), "input": g(16, T_STRING, b""), "control": g(18, T_STRING, b"")}


class Decoded:
    pass


def decode(rows, seeds: list) -> Decoded:
    """The whole cdr_load_rows contract on a cadence_amd.rows.Rows: .tables[t][slot] = record
    bytes (None where unspecified: the slices of failed entries), .row_status[t],
    .entry_status, .result [(code, n_act .. n_signal)], .caps [(offsets, counts)], .strings."""
    data = rows.bytes.tobytes()
    ne, n_rows = rows.n_entries, rows.n_rows
    parsed = [[None] * n_rows[t] for t in range(5)]
    status = [[0] * n_rows[t] for t in range(5)]
    for t in range(5):
        for r in range(n_rows[t]):
            key = rows.timer_id(r) if t == 1 else int(rows.key[t][r])
            hb = int(rows.act_heartbeat[r]) if t == 0 else 0
            try:
                parsed[t][r] = parse_row(t, data, int(rows.blob_off[t][r]), int(rows.blob_off[t][r + 1]), key, hb)
            except (TD.DecodeError, RowError) as e:
                status[t][r] = e.code

    def span(t, w):
        return range(int(rows.entry_row0[t][w]), int(rows.entry_row0[t][w + 1]))

    def first_failure(w):
        for t in range(5):
            for r in span(t, w):
                if status[t][r]:
                    return status[t][r]
        return 0
    entry_status = [first_failure(w) for w in range(ne)]
    it = Interner(seeds)
    for w in range(ne):
        if entry_status[w] == 0:
            for t in range(5):
                for r in span(t, w):
                    for s in parsed[t][r][1].values():
                        it.add(s)
    it.finish()
    out = Decoded()
    out.tables = [[None] * n_rows[t] for t in range(5)]
    for w in range(ne):
        if entry_status[w]:
            continue
        recs = []
        for t in range(5):
            done = []
            for r in span(t, w):
                rec, strs = parsed[t][r]
                for f, s in strs.items():
                    setattr(rec, f, it.handle(s))
                k = rec.timer_id if t == 1 else int(rows.key[t][r])
                done.append((k, r, rec))
            uses = collections.Counter(k for k, _, _ in done)
            for k, r, _ in done:
                if len(done) > abi.LOAD_MAX_ENTRY_ROWS:
                    status[t][r] = E_ENTRY_ROWS
                elif uses[k] > 1:
                    status[t][r] = E_DUP_KEY
            recs.append(sorted(done, key=lambda x: x[0]))
        entry_status[w] = first_failure(w)
        if entry_status[w] == 0:
            for t in range(5):
                for j, (_, _, rec) in enumerate(recs[t]):
                    out.tables[t][int(rows.entry_row0[t][w]) + j] = bytes(rec)
    out.row_status, out.entry_status = status, entry_status
    out.result, out.caps = [], []
    for w in range(ne):
        cnt = [len(span(t, w)) for t in range(5)]
        ok = entry_status[w] == 0
        out.result.append((abi.OK if ok else abi.E_LOAD_ROWS, *[c if ok else 0 for c in cnt]))
        out.caps.append(([int(rows.entry_row0[t][w]) for t in range(5)], cnt))
    out.strings = list(seeds) + [it.new[h] for h in sorted(it.new)]
    return out


def compare(got, want: Decoded, rows) -> list:
    """Mismatches between a cadence_amd.rows.Loaded and the reference: statuses, results,
    capacities, the string table, and record for record the slices of every OK entry."""
    bad = []
    for t in range(5):
        gs = [int(x) for x in got.row_status[t]]
        if gs != want.row_status[t]:
            r = next(i for i, (a, b) in enumerate(zip(gs, want.row_status[t])) if a != b)
            bad.append(f"row_status[{t}][{r}]: {gs[r]} != {want.row_status[t][r]}")
    ge = [int(x) for x in got.entry_status]
    if ge != want.entry_status:
        w = next(i for i, (a, b) in enumerate(zip(ge, want.entry_status)) if a != b)
        bad.append(f"entry_status[{w}]: {ge[w]} != {want.entry_status[w]}")
    if got.n_bad_entries != sum(1 for s in want.entry_status if s):
        bad.append(f"n_bad_entries {got.n_bad_entries}")
    zero_caps = bytes(C.sizeof(abi.CdrWfCaps))
    for w in range(rows.n_entries):
        r, c = got.result[w], got.caps[w]
        g = (r.code, r.n_activity, r.n_timer, r.n_child, r.n_cancel, r.n_signal)
        if g != want.result[w]:
            bad.append(f"result[{w}]: {g} != {want.result[w]}")
        if (r.flags, r.fail_event_id, r.fail_index, r.n_vh, r.n_reset_points, r.n_search_attr) != (0,) * 6:
            bad.append(f"result[{w}]: fields the loader leaves zero are set")
        exp = abi.CdrWfCaps()
        for i, t in enumerate(TABLES):
            setattr(exp, t + "_off", want.caps[w][0][i])
            setattr(exp, t + "_cap", want.caps[w][1][i])
        if bytes(c) != bytes(exp):
            bad.append(f"caps[{w}]")
    if list(got.strings) != want.strings:
        bad.append(f"strings: {len(got.strings)} vs {len(want.strings)}" + "".join(
            f"; [{h}] {a[:40]!r} != {b[:40]!r}" for h, (a, b) in enumerate(zip(got.strings, want.strings)) if a != b)[:300])
    for i, t in enumerate(TABLES):
        size = C.sizeof(engine.TABLE_TYPES[t])
        raw = bytes(got.tables[t])
        for slot, rec in enumerate(want.tables[i]):
            if rec is not None and raw[slot * size:(slot + 1) * size] != rec:
                bad.append(f"{t}[{slot}]: record differs")
                if len(bad) > 20:
                    return bad
    return bad
