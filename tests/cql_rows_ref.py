"""TEST INFRASTRUCTURE ONLY: Python reference of the Cassandra-form loader (cdr.h
cdr_load_cql_rows, cadence_amd/csrc/load.hip), the counterpart of tests/rows_ref.py.

It restates the header's contract independently of the device code:

  * a column body is an int32 count and that many (key, UDT) pairs of [bytes]; an empty body is
    a null column; `split` delimits the pairs and names the map-level finding, which belongs to
    the index of the first pair that could not be delimited (the count findings: index 0);
  * a UDT value is its fields' [bytes] in the schema's declaration order; fewer fields leave
    the rest null, bytes after the last declared field are ignored; null or empty fixed-size
    values are zero, another wrong length is CDR_LOAD_E_CQL_SIZE; timestamps are milliseconds
    (x 1,000,000, outside int64: CDR_LOAD_E_SHAPE; null: Go's zero time); the first finding in
    field order is the row's status;
  * keys come from the UDT; strings, order, duplicate keys and the per-entry failure rule are
    those of tests/rows_ref.py.

The writer (`pair` / `columns`) builds columns from oracle/cql_values.py's statement values:
`oracle.cql_values.decode` splits them by the statement's types and DECLARED puts the UDT's
fields into the schema's order.
"""
from __future__ import annotations

import collections
import ctypes as C
import struct

from cadence_amd import abi, rows
from cadence_amd.rows import TABLES
from oracle import cql_values as cv
from oracle import thrift_decode as TD
from oracle.thrift_decode import Interner
from tests.rows_ref import Decoded, RowError, _request_id, compare, uuid_string  # noqa: F401

TRUNCATED, BAD_SIZE = TD.DEC_TRUNCATED, TD.DEC_BAD_SIZE
E_CQL_SIZE, E_SHAPE, E_ENTRY_ROWS, E_DUP_KEY = abi.LOAD_E_CQL_SIZE, abi.LOAD_E_SHAPE, abi.LOAD_E_ENTRY_ROWS, abi.LOAD_E_DUP_KEY
ZT = abi.ZERO_TIME_NANOS
EMPTY_RUN_ID = bytes.fromhex("300000000000f000f000000000000000")  # cassandraPersistence.go:48
MS_MAX = (2**63 - 1) // 1_000_000  # the largest millisecond value whose nanoseconds fit int64

# schema.cql:149-228: the UDTs' fields in declaration order, (name, type)
UDT = {
    0: [("version", "bigint"), ("schedule_id", "bigint"), ("scheduled_event_batch_id", "bigint"),
        ("scheduled_event", "blob"), ("scheduled_time", "timestamp"), ("started_id", "bigint"),
        ("started_event", "blob"), ("started_time", "timestamp"), ("activity_id", "text"), ("request_id", "text"),
        ("details", "blob"), ("schedule_to_start_timeout", "int"), ("schedule_to_close_timeout", "int"),
        ("start_to_close_timeout", "int"), ("heart_beat_timeout", "int"), ("cancel_requested", "boolean"),
        ("cancel_request_id", "bigint"), ("last_hb_updated_time", "timestamp"), ("timer_task_status", "int"),
        ("attempt", "int"), ("task_list", "text"), ("started_identity", "text"), ("has_retry_policy", "boolean"),
        ("init_interval", "int"), ("backoff_coefficient", "double"), ("max_interval", "int"),
        ("expiration_time", "timestamp"), ("max_attempts", "int"), ("non_retriable_errors", "list<text>"),
        ("last_failure_reason", "text"), ("last_worker_identity", "text"), ("last_failure_details", "blob"),
        ("event_data_encoding", "text")],
    1: [("version", "bigint"), ("timer_id", "text"), ("started_id", "bigint"), ("expiry_time", "timestamp"),
        ("task_id", "bigint")],
    2: [("version", "bigint"), ("initiated_id", "bigint"), ("initiated_event_batch_id", "bigint"),
        ("initiated_event", "blob"), ("started_id", "bigint"), ("started_workflow_id", "text"),
        ("started_run_id", "uuid"), ("started_event", "blob"), ("create_request_id", "uuid"),
        ("event_data_encoding", "text"), ("domain_name", "text"), ("workflow_type_name", "text"),
        ("parent_close_policy", "int")],
    3: [("version", "bigint"), ("initiated_event_batch_id", "bigint"), ("initiated_id", "bigint"),
        ("cancel_request_id", "text")],
    4: [("version", "bigint"), ("initiated_event_batch_id", "bigint"), ("initiated_id", "bigint"),
        ("signal_request_id", "uuid"), ("signal_name", "text"), ("input", "blob"), ("control", "blob")],
}
SIZE = cv.FIXED
# position i of the declared UDT is field DECLARED[t][i] of the statement (after its key)
DECLARED = {0: range(33), 1: range(5), 2: range(13), 3: (0, 2, 1, 3), 4: (0, 2, 1, 3, 4, 5, 6)}
STATEMENT_TYPES = [cv.ACTIVITY_TYPES, cv.TIMER_TYPES, cv.CHILD_TYPES, cv.CANCEL_TYPES, cv.SIGNAL_TYPES]
WRITER = [cv.activity, cv.timer, cv.child, cv.cancel, cv.signal]
for _t in range(5):  # the two orders hold the same types
    assert [STATEMENT_TYPES[_t][1 + i] for i in DECLARED[_t]] == [ty for _, ty in UDT[_t]], _t


# ---------------------------------------------------------------- the writer
def udt_value(fields) -> bytes:
    """A UDT value ([bytes]) from its fields' raw values (None: null)."""
    return cv.val(b"".join(cv.val(f) for f in fields))


def pair(t: int, values: bytes) -> bytes:
    """A map pair from a row's statement values (oracle/cql_values.py)."""
    v = cv.decode(values, STATEMENT_TYPES[t])
    return cv.val(v[0]) + udt_value([v[1 + i] for i in DECLARED[t]])


def column(pairs) -> bytes:
    return rows.cql_column(pairs)


def columns(batch, out, strs) -> rows.CqlCols:
    """encode_state_cql with the oracle's writers."""
    S = cv.tb.lookup(strs)
    cols = []
    for i, t in enumerate(TABLES):
        per = []
        for w in range(batch.n_wfs):
            ps = [pair(i, WRITER[i](r, S)) for r in (out.rows(w, t) if out.result[w].code == abi.OK else [])]
            per.append(column(ps or None))
        cols.append(per)
    return rows.pack_cql(batch.n_wfs, cols)


# ---------------------------------------------------------------- the reader
def _i32(b, p):
    return struct.unpack_from(">i", b, p)[0]


def split(body: bytes):
    """(the delimited pairs' UDT values (None: null), the map-level finding (index, status) or
    None) of a column body."""
    if not body:
        return [], None
    if len(body) < 4:
        return [], (0, TRUNCATED)
    n = _i32(body, 0)
    if n < 0:
        return [], (0, BAD_SIZE)
    if n > abi.LOAD_MAX_ENTRY_ROWS:
        return [], (0, E_ENTRY_ROWS)
    p, udts = 4, []
    for k in range(n):
        v = None
        for _ in range(2):  # the key, delimited and not read; the UDT
            if len(body) - p < 4:
                return udts, (k, TRUNCATED)
            ln = _i32(body, p)
            p += 4
            if ln < -1:
                return udts, (k, BAD_SIZE)
            if ln > len(body) - p:
                return udts, (k, TRUNCATED)
            v = None if ln < 0 else body[p:p + ln]
            p += max(ln, 0)
        udts.append(v)
    return udts, None


class Fields:
    """The fields of one UDT value, read in order."""

    def __init__(self, b):
        self.b, self.p = b or b"", 0

    def val(self):
        b = self.b
        if self.p == len(b):
            return None  # fewer fields than declared
        if len(b) - self.p < 4:
            raise RowError(TRUNCATED)
        ln = _i32(b, self.p)
        self.p += 4
        if ln < 0:
            if ln != -1:
                raise RowError(BAD_SIZE)
            return None
        if ln > len(b) - self.p:
            raise RowError(TRUNCATED)
        self.p += ln
        return b[self.p - ln:self.p]

    def fixed(self, ty):
        v = self.val()
        if not v:
            return None
        if len(v) != SIZE[ty]:
            raise RowError(E_CQL_SIZE)
        return v

    def bigint(self):
        v = self.fixed("bigint")
        return struct.unpack(">q", v)[0] if v else 0

    def int(self):
        v = self.fixed("int")
        return struct.unpack(">i", v)[0] if v else 0

    def boolean(self):
        v = self.fixed("boolean")
        return bool(v and v[0])

    def double_bits(self):
        return self.fixed("double") or bytes(8)

    def uuid(self):
        return self.fixed("uuid") or bytes(16)

    def timestamp(self):
        v = self.fixed("timestamp")
        if not v:
            return ZT
        ms = struct.unpack(">q", v)[0]
        if not -MS_MAX <= ms <= MS_MAX:
            raise RowError(E_SHAPE)
        return ms * 1_000_000

    def text(self):
        return self.val() or b""

    def list_text(self):
        """The thrift list<string> body of a non-empty list, else b""."""
        v = self.val()
        if not v:
            return b""
        if len(v) < 4:
            raise RowError(TRUNCATED)
        cnt, p = _i32(v, 0), 4
        if cnt < 0:
            raise RowError(BAD_SIZE)
        for _ in range(cnt):
            if len(v) - p < 4:
                raise RowError(TRUNCATED)
            ln = _i32(v, p)
            p += 4
            if ln < 0:
                raise RowError(BAD_SIZE)
            if ln > len(v) - p:
                raise RowError(TRUNCATED)
            p += ln
        return b"\x0b" + v[:p] if cnt else b""


def _hi_lo(u: bytes):
    return int.from_bytes(u[:8], "big"), int.from_bytes(u[8:], "big")


def parse_udt(t: int, udt):
    """(record with its handle fields zero, {handle field: bytes}) of one UDT value, or RowError."""
    f = Fields(udt)
    if t == 0:
        a = abi.CdrActivityInfo()
        a.version, a.schedule_id, a.scheduled_event_batch_id = f.bigint(), f.bigint(), f.bigint()
        f.text()
        a.scheduled_time, a.started_id = f.timestamp(), f.bigint()
        f.text()
        started = f.timestamp()
        strs = {"activity_id": f.text(), "request_id": f.text()}
        f.text()
        a.s2s, a.s2c, a.stc, a.hb = f.int(), f.int(), f.int(), f.int()
        flags = abi.AI_CANCEL_REQUESTED if f.boolean() else 0
        a.cancel_request_id = f.bigint()
        hb = f.timestamp()
        a.timer_task_status, a.attempt = f.int(), f.int()
        strs["task_list"] = f.text()
        f.text()
        flags |= abi.AI_HAS_RETRY if f.boolean() else 0
        a.initial_interval = f.int()
        C.memmove(C.addressof(a) + abi.CdrActivityInfo.backoff_coefficient.offset, f.double_bits()[::-1], 8)
        a.maximum_interval, a.expiration_time, a.maximum_attempts = f.int(), f.timestamp(), f.int()
        strs["nonretriable"] = f.list_text()
        for _ in range(4):
            f.text()
        # from the nanosecond values on: cdr_load_rows' rules
        if started != ZT:
            flags |= abi.AI_STARTED_TIME_SET
            a.started_time = started
        a.last_heartbeat_time = hb if hb != ZT else 0
        if a.last_heartbeat_time and not flags & abi.AI_STARTED_TIME_SET:
            flags |= abi.AI_HEARTBEAT_TIME_SET
        a.flags = flags
        return a, strs
    if t == 1:
        x = abi.CdrTimerInfo()
        x.version = f.bigint()
        tid = f.text()
        x.started_id, x.expiry_time, x.task_id = f.bigint(), f.timestamp(), f.bigint()
        return x, {"timer_id": tid}
    if t == 2:
        c = abi.CdrChildInfo()
        c.version, c.initiated_id, c.initiated_event_batch_id = f.bigint(), f.bigint(), f.bigint()
        f.text()
        c.started_id = f.bigint()
        strs = {"started_workflow_id": f.text()}
        run = f.uuid()
        strs["started_run_id"] = b"" if run in (bytes(16), EMPTY_RUN_ID) else uuid_string(run)
        f.text()
        c.create_request_hi, c.create_request_lo = _hi_lo(f.uuid())
        f.text()
        strs["domain_name"], strs["workflow_type"] = f.text(), f.text()
        c.parent_close_policy = f.int()
        return c, strs
    if t == 3:
        c = abi.CdrCancelInfo()
        c.version, c.initiated_event_batch_id, c.initiated_id = f.bigint(), f.bigint(), f.bigint()
        c.cancel_request_lo, c.cancel_request_hi = _request_id(f.text())
        return c, {}
    g = abi.CdrSignalInfo()
    g.version, g.initiated_event_batch_id, g.initiated_id = f.bigint(), f.bigint(), f.bigint()
    g.signal_request_hi, g.signal_request_lo = _hi_lo(f.uuid())
    return g, {"signal_name": f.text(), "input": f.text(), "control": f.text()}


def _key(t, rec):
    return rec.schedule_id if t == 0 else rec.timer_id if t == 1 else rec.initiated_id


def decode(cols: rows.CqlCols, seeds: list, n_bytes: int = None) -> Decoded:
    """The whole cdr_load_cql_rows contract on a cadence_amd.rows.CqlCols: a tests/rows_ref.py
    Decoded plus .n_rows and .entry_row0, the rows the split finds.  `n_bytes`: the buffer's
    length as the call is told it (offsets are clamped to it)."""
    data = cols.bytes.tobytes()
    nb = len(data) if n_bytes is None else n_bytes
    ne = cols.n_entries
    parsed, status, row0, finding = [], [], [], []
    for t in range(5):
        ps, st, r0, fd = [], [], [0], []
        for w in range(ne):
            e = min(int(cols.col_off[t][w + 1]), nb)
            p = min(int(cols.col_off[t][w]), e)
            udts, found = split(data[p:e])
            fd.append(found)
            for u in udts:
                try:
                    ps.append(parse_udt(t, u))
                    st.append(0)
                except RowError as x:
                    ps.append(None)
                    st.append(x.code)
            r0.append(len(ps))
        parsed.append(ps)
        status.append(st)
        row0.append(r0)
        finding.append(fd)

    def span(t, w):
        return range(row0[t][w], row0[t][w + 1])

    def first_failure(w):
        for t in range(5):
            for r in span(t, w):
                if status[t][r]:
                    return status[t][r]
            if finding[t][w]:  # its index is past every row of the column
                return finding[t][w][1]
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
    out.tables = [[None] * len(parsed[t]) for t in range(5)]
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
                done.append((_key(t, rec), r, rec))
            uses = collections.Counter(k for k, _, _ in done)
            for k, r, _ in done:
                if uses[k] > 1:
                    status[t][r] = E_DUP_KEY
            recs.append(sorted(done, key=lambda x: x[0]))
        entry_status[w] = first_failure(w)
        if entry_status[w] == 0:
            for t in range(5):
                for j, (_, _, rec) in enumerate(recs[t]):
                    out.tables[t][row0[t][w] + j] = bytes(rec)
    out.row_status, out.entry_status = status, entry_status
    out.result, out.caps = [], []
    for w in range(ne):
        cnt = [len(span(t, w)) for t in range(5)]
        ok = entry_status[w] == 0
        out.result.append((abi.OK if ok else abi.E_LOAD_ROWS, *[c if ok else 0 for c in cnt]))
        out.caps.append(([row0[t][w] for t in range(5)], cnt))
    out.strings = list(seeds) + [it.new[h] for h in sorted(it.new)]
    out.n_rows = [len(parsed[t]) for t in range(5)]
    out.entry_row0 = row0
    return out


def compare_cql(got, want: Decoded, cols) -> list:
    """tests/rows_ref.compare plus the split's own outputs."""
    bad = []
    if list(got.n_rows) != want.n_rows:
        return [f"n_rows {list(got.n_rows)} != {want.n_rows}"]
    for t in range(5):
        if [int(x) for x in got.entry_row0[t][:cols.n_entries + 1]] != want.entry_row0[t] and cols.n_entries:
            bad.append(f"entry_row0[{t}]")
    return bad + compare(got, want, cols)
