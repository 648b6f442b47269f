"""TEST INFRASTRUCTURE ONLY: Python reference of the Cassandra whole-state loader (cdr.h
cdr_load_cql_state, cadence_amd/csrc/load.hip), the parity checker for it.

The header's contract restated on tests/cql_rows_ref.py's field reader (the pending tables are
that module's) and tests/exec_rows_ref.py's nested-blob walks (branch tokens, reset points,
version histories: the same thriftrw blobs as the SQL form's), independently of the device code:

  * the `execution` body is the 58 fields of workflow_execution in the schema's declaration
    order (FIELDS, checked against tests/golden/cql_workflow_execution_fields.json), each a
    [bytes] value; the first finding in field order is the row's — the list's and the two maps'
    element findings included;
  * then, in this order: the replication state's wire findings; replication state and version
    histories together (SHAPE); an unknown cluster; the branch token; the reset points; the
    maps' counts (SHAPE); the version histories;
  * strings, failure rule and outputs are cdr_load_state's; generated strings are the UUID
    texts (domain, run, parents, create request), the list body and the Memo body.

The writer (`columns`) builds the four columns from oracle/cql_values.execution's statement
values: `oracle.cql_values.decode` splits them by the statement's types and DECLARED puts the
UDT's fields into the schema's order.
"""
from __future__ import annotations

import collections
import ctypes as C
import struct
from types import SimpleNamespace

from cadence_amd import abi, rows
from oracle import cql_values as cv
from oracle import thrift_decode as TD
from oracle.thrift_decode import T_BOOL, T_I32, T_I64, T_LIST, T_STRING, T_STRUCT, Interner, fget
from tests import cql_rows_ref as ref
from tests import exec_rows_ref as xref
from tests.cql_rows_ref import BAD_SIZE, TRUNCATED, ZT, Fields, _i32
from tests.exec_rows_ref import E_CLUSTER, E_SHAPE, P_HANDLES, X_HANDLES  # noqa: F401
from tests.rows_ref import RowError, uuid_string

EMPTY_DOMAIN_ID = bytes.fromhex("100000000000f000f000000000000000")  # cassandraPersistence.go:46
EMPTY_RUN_ID = ref.EMPTY_RUN_ID
EMPTY_INITIATED_ID = cv.EMPTY_INITIATED_ID

# schema.cql:23-82: workflow_execution's fields in declaration order, (name, type)
FIELDS = [
    ("domain_id", "uuid"), ("workflow_id", "text"), ("run_id", "uuid"), ("parent_domain_id", "uuid"),
    ("parent_workflow_id", "text"), ("parent_run_id", "uuid"), ("initiated_id", "bigint"),
    ("completion_event_batch_id", "bigint"), ("completion_event", "blob"), ("completion_event_data_encoding", "text"),
    ("task_list", "text"), ("workflow_type_name", "text"), ("workflow_timeout", "int"), ("decision_task_timeout", "int"),
    ("execution_context", "blob"), ("state", "int"), ("close_status", "int"), ("last_processed_event", "bigint"),
    ("start_time", "timestamp"), ("last_updated_time", "timestamp"), ("create_request_id", "uuid"),
    ("decision_version", "bigint"), ("decision_schedule_id", "bigint"), ("decision_started_id", "bigint"),
    ("decision_request_id", "text"), ("decision_timeout", "int"), ("decision_attempt", "bigint"),
    ("decision_timestamp", "bigint"), ("decision_scheduled_timestamp", "bigint"),
    ("decision_original_scheduled_timestamp", "bigint"), ("cancel_requested", "boolean"), ("cancel_request_id", "text"),
    ("sticky_task_list", "text"), ("sticky_schedule_to_start_timeout", "int"), ("client_library_version", "text"),
    ("client_feature_version", "text"), ("client_impl", "text"), ("attempt", "int"), ("has_retry_policy", "boolean"),
    ("init_interval", "int"), ("backoff_coefficient", "double"), ("max_interval", "int"), ("expiration_time", "timestamp"),
    ("max_attempts", "int"), ("non_retriable_errors", "list<text>"), ("event_store_version", "int"),
    ("signal_count", "int"), ("branch_token", "blob"), ("history_size", "bigint"), ("last_first_event_id", "bigint"),
    ("next_event_id", "bigint"), ("cron_schedule", "text"), ("expiration_seconds", "int"), ("last_event_task_id", "bigint"),
    ("auto_reset_points", "blob"), ("auto_reset_points_encoding", "text"), ("search_attributes", "map<text,blob>"),
    ("memo", "map<text,blob>")]
NAMES = [n for n, _ in FIELDS]
# position i of the declared UDT is field DECLARED[i] of the statement (oracle/cql_values.execution)
DECLARED = rows.EXEC_DECLARED
assert [cv.EXEC_TYPES[i] for i in DECLARED] == [ty for _, ty in FIELDS]  # the two orders hold the same types


# ---------------------------------------------------------------- the writer
def body(fields) -> bytes:
    """A UDT value's body from its fields' raw values (None: null)."""
    return b"".join(cv.val(f) for f in fields)


def four_columns(builder: int, values: bytes) -> tuple:
    """(execution, replication_state, version_histories, encoding) bodies from the execution
    row's statement values (oracle/cql_values.execution)."""
    v = cv.decode(values, cv.EXEC_TYPES + cv.EXEC_TAIL[builder])
    f, tail = v[:58], v[58:]
    execution = body([f[i] for i in DECLARED])
    if builder == abi.BUILDER_2DC:  # the tail's last value is the next_event_id column: the UDT has its own
        return execution, body(tail[:5]), b"", b""
    if builder == abi.BUILDER_NDC:
        return execution, b"", tail[1] or b"", tail[2] or b""
    return execution, b"", b"", b""


def columns(batch, out, strs, persist, names) -> rows.CqlCols:
    """encode_state_cql(exec_rows=True) with the oracle's writers; an entry that is not OK, or
    whose row the writer refuses, gets a one-byte execution body."""
    S = cv.tb.lookup(strs)
    cols = ref.columns(batch, out, strs)
    per = [[cols.column(t, w) for w in range(batch.n_wfs)] for t in range(5)]
    xcols = [[], [], [], []]
    for w in range(batch.n_wfs):
        four = (b"\0", b"", b"", b"")
        if out.result[w].code == abi.OK:
            try:
                values = cv.execution(out.exec[w], batch.wfs[w].builder, S, persist[w], repl=out.repl[w],
                                      vh_items=[(v.event_id, v.version) for v in out.rows(w, "vh")],
                                      rps=[(p, S) for p in out.rows(w, "rp")],
                                      sa=[(kv.key, kv.value) for kv in out.rows(w, "sa")], cluster_names=names)
                four = four_columns(batch.wfs[w].builder, values)
            except cv.BadUUID:  # an ID the uuid columns cannot hold: the writer refuses the row
                pass
        for c in range(4):
            xcols[c].append(four[c])
    return rows.pack_cql(batch.n_wfs, per, xcols)


# ---------------------------------------------------------------- the reader
class XFields(Fields):
    def uuid_or_none(self, none: bytes) -> bytes:
        """A parent's ID: sixteen zero bytes and the writer's sentinel are b""."""
        u = self.uuid()
        return b"" if u in (bytes(16), none) else u

    def map_blob(self):
        """(pairs, the value's bytes from its count to the end of its last pair) of a
        map<text, blob>; null, empty or count 0: ([], b"")."""
        v = self.val()
        if not v:
            return [], b""
        cnt, p, elems = _count(v), 4, []
        for _ in range(2 * cnt):
            e, p = _elem(v, p, False)
            elems.append(e)
        return (list(zip(elems[0::2], elems[1::2])), v[:p]) if cnt else ([], b"")


def _count(v: bytes) -> int:
    if len(v) < 4:
        raise RowError(TRUNCATED)
    if _i32(v, 0) < 0:
        raise RowError(BAD_SIZE)
    return _i32(v, 0)


def _elem(v: bytes, p: int, null_ok: bool):
    """(element, position after it) of the [bytes] at p of collection value v."""
    if len(v) - p < 4:
        raise RowError(TRUNCATED)
    ln = _i32(v, p)
    p += 4
    if ln < 0:
        if ln != -1 or not null_ok:
            raise RowError(BAD_SIZE)
        return b"", p
    if ln > len(v) - p:
        raise RowError(TRUNCATED)
    return v[p:p + ln], p + ln


def parse_exec(execution: bytes, rs: bytes, vhb: bytes, vhenc: bytes, clusters: list) -> SimpleNamespace:
    """One execution row from its four column bodies: what tests/exec_rows_ref.parse_exec
    gives (.x / .ps / .repl records with their handle fields zero, .xs / .pss, .builder, .vh,
    .rps, .sa, .n_sa_wire, .sa_strings, .gen); RowError / TD.DecodeError where the row fails."""
    f = XFields(execution)
    x, ps, repl = abi.CdrExecInfo(), abi.CdrExecPersist(), abi.CdrReplState()
    xs, pss = dict.fromkeys(X_HANDLES, b""), dict.fromkeys(P_HANDLES, b"")
    # ---- the UDT, in declaration order
    dom = f.uuid()
    xs["workflow_id"] = f.text()
    run = f.uuid()
    pdom = f.uuid_or_none(EMPTY_DOMAIN_ID)
    xs["parent_workflow_id"] = f.text()
    prun = f.uuid_or_none(EMPTY_RUN_ID)
    x.initiated_id = f.bigint()
    x.completion_event_batch_id = f.bigint()
    f.text()  # completion_event
    f.text()
    xs["task_list"] = f.text()
    xs["workflow_type"] = f.text()
    x.workflow_timeout = f.int()
    x.decision_timeout_value = f.int()
    pss["execution_context"] = f.text()
    x.state = f.int()
    x.close_status = f.int()
    x.last_processed_event = f.bigint()
    ps.start_time = f.timestamp()
    ps.last_updated_time = f.timestamp()
    crq = f.uuid()
    x.decision_version = f.bigint()
    x.decision_schedule_id = f.bigint()
    x.decision_started_id = f.bigint()
    xs["decision_request_id"] = f.text()
    x.decision_timeout = f.int()
    x.decision_attempt = f.bigint()
    x.decision_started_ts = f.bigint()
    x.decision_scheduled_ts = f.bigint()
    x.decision_original_scheduled_ts = f.bigint()
    flags = abi.XI_STARTED | (abi.XI_CANCEL_REQUESTED if f.boolean() else 0)
    f.text()  # cancel_request_id
    pss["sticky_task_list"] = f.text()
    ps.sticky_s2s_timeout = f.int()
    pss["client_library_version"] = f.text()
    pss["client_feature_version"] = f.text()
    pss["client_impl"] = f.text()
    x.attempt = f.int()
    flags |= abi.XI_HAS_RETRY if f.boolean() else 0
    x.initial_interval = f.int()
    C.memmove(C.addressof(x) + abi.CdrExecInfo.backoff_coefficient.offset, f.double_bits()[::-1], 8)
    x.maximum_interval = f.int()
    expiration = f.timestamp()
    x.maximum_attempts = f.int()
    xs["nonretriable"] = f.list_text()
    f.int()  # event_store_version
    x.signal_count = f.int()
    token = f.text()
    ps.history_size = f.bigint()
    x.last_first_event_id = f.bigint()
    x.next_event_id = f.bigint()
    xs["cron_schedule"] = f.text()
    x.expiration_seconds = f.int()
    x.last_event_task_id = f.bigint()
    rpb = f.text()
    rpenc = f.text()
    sa_wire, _ = f.map_blob()
    memo_pairs, memo_body = f.map_blob()
    # ---- what follows from the values
    if not pdom and x.initiated_id == EMPTY_INITIATED_ID:
        x.initiated_id = abi.EMPTY_EVENT_ID
    if expiration != ZT:
        flags |= abi.XI_HAS_EXPIRATION
        x.expiration_time = expiration
    xs["domain_id"], xs["run_id"], xs["create_request_id"] = uuid_string(dom), uuid_string(run), uuid_string(crq)
    gen = [xs["domain_id"], xs["run_id"]]
    for name, b in (("parent_domain_id", pdom), ("parent_run_id", prun)):
        if b:
            xs[name] = uuid_string(b)
            gen.append(xs[name])
    gen.append(xs["create_request_id"])
    if xs["nonretriable"]:
        gen.append(xs["nonretriable"])
    # ---- the findings after the UDT's, in the header's order
    two_dc, ndc, unknown = bool(rs), bool(vhb), False
    if two_dc:
        g = XFields(rs)
        repl.current_version = g.bigint()
        repl.start_version = g.bigint()
        repl.last_write_version = g.bigint()
        repl.last_write_event_id = g.bigint()
        m = g.val()
        if m:
            p = 4
            for _ in range(_count(m)):
                key, p = _elem(m, p, False)
                u, p = _elem(m, p, True)
                uf = XFields(u)
                ver = uf.bigint()
                last = uf.bigint()
                if key not in clusters:
                    unknown = True
                    continue
                i = clusters.index(key)
                repl.lri_mask |= 1 << i
                repl.lri_version[i], repl.lri_last_event_id[i] = ver, last
    if two_dc and ndc:
        raise RowError(E_SHAPE)
    builder = abi.BUILDER_2DC if two_dc else abi.BUILDER_NDC if ndc else abi.BUILDER_LOCAL
    if two_dc:
        repl.present = 1
        ps.start_version, ps.current_version = repl.start_version, repl.current_version
        if unknown:
            raise RowError(E_CLUSTER)
    else:
        repl = abi.CdrReplState()
    tree, lo, hi = b"", 0, 0
    if token:
        flags |= abi.XI_HAS_BRANCH
        tree, lo, hi = xref._token(token)
    rps = []
    if rpb:
        pts = fget(xref._nested(rpb, rpenc), 10, T_LIST)
        if pts is not None and pts[0][1] == T_STRUCT:
            flags |= abi.XI_HAS_RESET_POINTS
            if len(pts[0][2]) > abi.LOAD_MAX_RESET_POINTS:
                raise RowError(E_SHAPE)
            for pt in pts[0][2]:
                p, pf = abi.CdrResetPoint(), 0
                for fid, ft, bit in ((10, T_STRING, abi.RP_HAS_CHECKSUM), (20, T_STRING, abi.RP_HAS_RUN_ID),
                                     (30, T_I64, abi.RP_HAS_FIRST_DC_ID), (40, T_I64, abi.RP_HAS_CREATED),
                                     (50, T_I64, abi.RP_HAS_EXPIRING), (60, T_BOOL, abi.RP_HAS_RESETTABLE)):
                    pf |= bit if fget(pt, fid, ft) is not None else 0
                val = lambda fi, t, d=0: (fget(pt, fi, t) or (d,))[0]  # noqa: E731
                p.first_decision_completed_id, p.created_time_nano = val(30, T_I64), val(40, T_I64)
                p.expiring_time_nano = val(50, T_I64)
                p.flags = pf | (abi.RP_RESETTABLE if val(60, T_BOOL) else 0)
                rps.append((p, val(10, T_STRING, b""), val(20, T_STRING, b"")))
    if len(sa_wire) > abi.LOAD_MAX_SEARCH_ATTR or len(memo_pairs) > abi.LOAD_MAX_SEARCH_ATTR:
        raise RowError(E_SHAPE)
    sa, sa_strings = [], []
    if sa_wire:
        flags |= abi.XI_HAS_SEARCH_ATTR
        sa_strings = [s for kv in sa_wire for s in kv]
        last_v = dict(sa_wire)
        sa = [(k, last_v[k]) for k in dict.fromkeys(k for k, _ in sa_wire)]
    if memo_pairs:
        flags |= abi.XI_HAS_MEMO
        xs["memo"] = b"\x0d\x00\x0a\x0b\x0b" + memo_body + b"\x00"
        gen.append(xs["memo"])
    vh = []
    if ndc:
        vst = xref._nested(vhb, vhenc)
        hs = fget(vst, 20, T_LIST)
        if (fget(vst, 10, T_I32) or (0,))[0] != 0 or hs is None or hs[0][1] != T_STRUCT or len(hs[0][2]) != 1:
            raise RowError(E_SHAPE)
        h = hs[0][2][0]
        vtok = (fget(h, 10, T_STRING) or (b"",))[0]
        if vtok:
            tree, lo, hi = xref._token(vtok)
            if token:
                raise RowError(E_SHAPE)
            flags |= abi.XI_VH_BRANCH
        its = fget(h, 20, T_LIST)
        if its is not None and its[0][1] == T_STRUCT:
            if len(its[0][2]) > abi.LOAD_MAX_VH_ITEMS:
                raise RowError(E_SHAPE)
            vh = [((fget(i, 10, T_I64) or (0,))[0], (fget(i, 20, T_I64) or (0,))[0]) for i in its[0][2]]
    xs["branch_tree_id"], x.branch_id_lo, x.branch_id_hi = tree, lo, hi
    x.flags, x.reset_points_len, x.search_attr_len = flags, len(rps), len(sa)
    return SimpleNamespace(x=x, xs=xs, ps=ps, pss=pss, repl=repl, builder=builder, vh=vh, rps=rps, sa=sa,
                           n_sa_wire=len(sa_wire), sa_strings=sa_strings, gen=gen)


def exec_columns(cols: rows.CqlCols, w: int, n_bytes: int = None) -> tuple:
    """Entry w's four column bodies, their offsets clamped to n_bytes."""
    data = cols.bytes.tobytes()
    nb = len(data) if n_bytes is None else n_bytes
    out = []
    for c in range(4):
        e = min(int(cols.exec.off[c][w + 1]), nb)
        out.append(data[min(int(cols.exec.off[c][w]), e):e])
    return tuple(out)


def decode_state(cols: rows.CqlCols, seeds: list, n_bytes: int = None, cluster_seed=None) -> SimpleNamespace:
    """The whole cdr_load_cql_state contract on a CqlCols with .exec: tests/exec_rows_ref
    decode_state's fields over the rows tests/cql_rows_ref's split finds (.n_rows,
    .entry_row0)."""
    data = cols.bytes.tobytes()
    nb = len(data) if n_bytes is None else n_bytes
    ne = cols.n_entries
    cs = cols.exec.cluster_seed if cluster_seed is None else cluster_seed
    clusters = [seeds[s] if s < len(seeds) else None for s in cs]
    parsed, status, row0, finding = [], [], [], []
    for t in range(5):
        ps, st, r0, fd = [], [], [0], []
        for w in range(ne):
            e = min(int(cols.col_off[t][w + 1]), nb)
            udts, found = ref.split(data[min(int(cols.col_off[t][w]), e):e])
            fd.append(found)
            for u in udts:
                try:
                    ps.append(ref.parse_udt(t, u))
                    st.append(0)
                except RowError as x:
                    ps.append(None)
                    st.append(x.code)
            r0.append(len(ps))
        parsed.append(ps)
        status.append(st)
        row0.append(r0)
        finding.append(fd)
    n_rows = [len(parsed[t]) for t in range(5)]
    xp, xstatus = [None] * ne, [0] * ne
    for w in range(ne):
        try:
            xp[w] = parse_exec(*exec_columns(cols, w, nb), clusters)
        except (TD.DecodeError, RowError) as e:
            xstatus[w] = e.code

    def span(t, w):
        return range(row0[t][w], row0[t][w + 1])

    def first_failure(w):
        for t in range(5):
            for r in span(t, w):
                if status[t][r]:
                    return status[t][r]
            if finding[t][w]:
                return finding[t][w][1]
        return xstatus[w]
    entry_status = [first_failure(w) for w in range(ne)]
    it = Interner(seeds)
    for w in range(ne):
        if entry_status[w] == 0:
            for t in range(5):
                for r in span(t, w):
                    for s in parsed[t][r][1].values():
                        it.add(s)
            p = xp[w]
            for s in list(p.xs.values()) + list(p.pss.values()) + [s for _, c, r in p.rps for s in (c, r)] + p.sa_strings:
                it.add(s)
    it.finish()
    out = SimpleNamespace(tables=[[None] * n_rows[t] for t in range(5)])
    cnt = [(len(p.vh), len(p.rps), p.n_sa_wire, (sum(len(s) for s in p.gen) + 3) & ~3) if p else (0, 0, 0, 0) for p in xp]
    off = [(0, 0, 0, 0)]
    for c in cnt:
        off.append(tuple(a + b for a, b in zip(off[-1], c)))
    act_lists = sum(len(parsed[0][r][1]["nonretriable"]) for r in range(n_rows[0]) if status[0][r] == 0)
    out.totals, out.gen_len = off[-1][:3], 36 * n_rows[2] + off[-1][3] + act_lists
    out.vh, out.rp, out.sa = ([None] * off[-1][i] for i in range(3))
    out.exec, out.repl, out.persist = [None] * ne, [None] * ne, [None] * ne
    out.builder = [p.builder if p else None for p in xp]
    for w in range(ne):
        if entry_status[w]:
            continue
        recs = []
        for t in range(5):
            done = []
            for r in span(t, w):
                rec, strs = parsed[t][r]
                for fld, s in strs.items():
                    setattr(rec, fld, it.handle(s))
                done.append((ref._key(t, rec), r, rec))
            uses = collections.Counter(k for k, _, _ in done)
            for k, r, _ in done:
                if uses[k] > 1:
                    status[t][r] = ref.E_DUP_KEY
            recs.append(sorted(done, key=lambda x: x[0]))
        entry_status[w] = first_failure(w)
        if entry_status[w]:
            continue
        for t in range(5):
            for j, (_, _, rec) in enumerate(recs[t]):
                out.tables[t][row0[t][w] + j] = bytes(rec)
        p = xp[w]
        for fld, s in p.xs.items():
            setattr(p.x, fld, it.handle(s))
        for fld, s in p.pss.items():
            setattr(p.ps, fld, it.handle(s))
        out.exec[w], out.repl[w], out.persist[w] = bytes(p.x), bytes(p.repl), bytes(p.ps)
        for j, (e, v) in enumerate(p.vh):
            out.vh[off[w][0] + j] = struct.pack("<qq", e, v)
        for j, (rp, c, r) in enumerate(p.rps):
            rp.binary_checksum, rp.run_id = it.handle(c), it.handle(r)
            out.rp[off[w][1] + j] = bytes(rp)
        for j, (k, v) in enumerate(p.sa):
            out.sa[off[w][2] + j] = struct.pack("<II", it.handle(k), it.handle(v))
    out.row_status, out.entry_status, out.exec_status = status, entry_status, xstatus
    out.result, out.caps = [], []
    for w in range(ne):
        c5 = [len(span(t, w)) for t in range(5)]
        ok = entry_status[w] == 0
        items = (len(xp[w].vh), len(xp[w].rps), len(xp[w].sa)) if ok else (0, 0, 0)
        out.result.append((abi.OK if ok else abi.E_LOAD_ROWS, *[c if ok else 0 for c in c5], *items))
        out.caps.append(([row0[t][w] for t in range(5)], c5, off[w][:3], cnt[w][:3]))
    out.strings = list(seeds) + [it.new[h] for h in sorted(it.new)]
    out.n_rows, out.entry_row0, out.parsed = n_rows, row0, xp
    return out


def compare_state(got, want, cols) -> list:
    """Mismatches between a cadence_amd.rows.Loaded of load_cql_state and the reference."""
    if list(got.n_rows) != want.n_rows:
        return [f"n_rows {list(got.n_rows)} != {want.n_rows}"]
    bad = []
    for t in range(5):
        if cols.n_entries and [int(x) for x in got.entry_row0[t][:cols.n_entries + 1]] != want.entry_row0[t]:
            bad.append(f"entry_row0[{t}]")
    return bad + xref.compare_state(got, want, cols)
