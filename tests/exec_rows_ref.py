"""TEST INFRASTRUCTURE ONLY: Python reference of the whole-state loader (cdr.h
cdr_load_state, cadence_amd/csrc/load.hip), the parity checker for it.

The execution row's contract restated on the generic wire reader of
oracle/thrift_decode.py, independently of the device parser; the pending tables are
tests/rows_ref.py's.  The mapping is the inverse of oracle/thrift_binary.py exec_info_blob,
following sqlExecutionManager.GetWorkflowExecution, DeserializeResetPoints /
DeserializeVersionHistories and NewVersionHistoriesFromThrift:

  * the row's blob is one bare struct; nested blobs (reset points, version histories, branch
    tokens) are the 0x59 preamble and a struct, each walked level by level: a level's wire
    errors come before any finding inside it;
  * the findings come in the header's order: wire errors, parent ID lengths, fields 44 and 122
    together, an unknown cluster, field 104's token, the reset points, the search attributes,
    the version histories;
  * strings: one interner for the pending rows and the execution rows; the key columns'
    and parent IDs' UUID texts and the Memo struct body are generated strings;
  * a failing execution row fails its entry after the pending tables (table 5).
"""
from __future__ import annotations

import collections
import ctypes as C
import struct
from types import SimpleNamespace

from cadence_amd import abi, engine
from cadence_amd.rows import TABLES
from oracle import thrift_decode as TD
from oracle.thrift_decode import T_BOOL, T_DOUBLE, T_I32, T_I64, T_LIST, T_MAP, T_STRING, T_STRUCT, Interner, Reader, fget
from tests import rows_ref
from tests.rows_ref import UUID_TEXT, RowError, uuid_string

E_UUID, E_ENCODING, E_SHAPE, E_CLUSTER = abi.LOAD_E_UUID, abi.LOAD_E_ENCODING, abi.LOAD_E_SHAPE, abi.LOAD_E_CLUSTER
_LEAF = rows_ref._WALKED_LEAF
X_HANDLES = ("domain_id", "workflow_id", "run_id", "create_request_id", "parent_domain_id", "parent_workflow_id",
             "parent_run_id", "task_list", "workflow_type", "cron_schedule", "memo", "nonretriable", "branch_tree_id",
             "decision_request_id")
P_HANDLES = ("execution_context", "sticky_task_list", "client_library_version", "client_feature_version",
             "client_impl")


def _i32(v: int) -> int:
    """Go's int32(v) of an int64."""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def _struct(b: bytes, start: int):
    return Reader(b, start, len(b)).value(T_STRUCT, 0, _LEAF)


def _token(b: bytes):
    """(tree ID bytes, lo, hi) of a branch token."""
    if not b or b[0] != 0x59:
        raise RowError(E_ENCODING)
    st = _struct(b, 1)
    anc = fget(st, 30, T_LIST)
    if anc is not None and anc[0][2]:
        raise RowError(E_SHAPE)
    bid = (fget(st, 20, T_STRING) or (b"",))[0]
    if not UUID_TEXT.fullmatch(bid):
        raise RowError(E_UUID)
    h = bid.replace(b"-", b"")
    return (fget(st, 10, T_STRING) or (b"",))[0], int(h[16:], 16), int(h[:16], 16)


def _nested(blob: bytes, encoding: bytes):
    if encoding != b"thriftrw" or not blob or blob[0] != 0x59:
        raise RowError(E_ENCODING)
    return _struct(blob, 1)


def parse_exec(data: bytes, start: int, end: int, col, clusters: list) -> SimpleNamespace:
    """One execution row: .x / .ps / .repl records with their handle fields zero, .xs / .pss
    {handle field: bytes}, .builder, .vh [(event ID, version)], .rps [(record, checksum, run
    ID)], .sa [(key, value)] (distinct keys), .n_sa_wire, .sa_strings (every pair's), .gen
    [generated strings in gen_bytes order]; RowError / TD.DecodeError where the row fails.  `col`: the row's columns (domain_id
    / run_id 16 bytes, workflow_id, next_event_id, last_write_version); `clusters`: cluster i's
    name (None: its seed index names no seed)."""
    st = Reader(data, start, end).value(T_STRUCT, 0, _LEAF)

    def g(fid, ft, default=0):
        v = fget(st, fid, ft)
        return default if v is None else v[0]

    def has(fid, ft):
        return fget(st, fid, ft) is not None
    x, ps, repl = abi.CdrExecInfo(), abi.CdrExecPersist(), abi.CdrReplState()
    xs = dict.fromkeys(X_HANDLES, b"")
    gen = [uuid_string(col.domain_id), uuid_string(col.run_id)]
    xs["domain_id"], xs["run_id"], xs["workflow_id"] = gen[0], gen[1], bytes(col.workflow_id)
    pdom = prun = b""
    x.initiated_id = abi.EMPTY_EVENT_ID
    if has(10, T_STRING):
        pdom, prun = g(10, T_STRING), g(14, T_STRING, b"")
        xs["parent_workflow_id"] = g(12, T_STRING, b"")
        x.initiated_id = g(16, T_I64)
    if len(pdom) not in (0, 16) or len(prun) not in (0, 16):
        raise RowError(E_UUID)
    for f, b in (("parent_domain_id", pdom), ("parent_run_id", prun)):
        if b:
            xs[f] = uuid_string(b)
            gen.append(xs[f])
    x.completion_event_batch_id = g(18, T_I64) if has(18, T_I64) else abi.EMPTY_EVENT_ID
    xs["task_list"], xs["workflow_type"] = g(24, T_STRING, b""), g(26, T_STRING, b"")
    x.workflow_timeout, x.decision_timeout_value = g(28, T_I32), g(30, T_I32)
    x.state, x.close_status = g(34, T_I32), g(36, T_I32)
    ps.start_version, ps.current_version = g(38, T_I64), g(40, T_I64)
    ps.start_time, ps.last_updated_time, ps.history_size = g(54, T_I64), g(56, T_I64), g(108, T_I64)
    ps.sticky_s2s_timeout = _i32(g(80, T_I64))
    pss = {"execution_context": g(32, T_STRING, b""), "sticky_task_list": g(78, T_STRING, b""),
           "client_library_version": g(110, T_STRING, b""), "client_feature_version": g(112, T_STRING, b""),
           "client_impl": g(114, T_STRING, b"")}
    x.next_event_id, x.last_event_task_id = col.next_event_id, 0
    x.last_first_event_id, x.last_processed_event = g(50, T_I64), g(52, T_I64)
    x.decision_version, x.decision_schedule_id, x.decision_started_id = g(58, T_I64), g(60, T_I64), g(62, T_I64)
    x.decision_timeout, x.decision_attempt = g(64, T_I32), g(66, T_I64)
    x.decision_started_ts, x.decision_scheduled_ts = g(68, T_I64), g(69, T_I64)
    x.decision_original_scheduled_ts = g(71, T_I64)
    xs["create_request_id"], xs["decision_request_id"] = g(72, T_STRING, b""), g(74, T_STRING, b"")
    x.attempt, x.signal_count = _i32(g(82, T_I64)), _i32(g(106, T_I64))
    x.initial_interval, x.maximum_interval = g(84, T_I32), g(86, T_I32)
    x.maximum_attempts, x.expiration_seconds = g(88, T_I32), g(90, T_I32)
    d = fget(st, 92, T_DOUBLE)
    if d is not None:  # the bits, not the value
        C.memmove(C.addressof(x) + abi.CdrExecInfo.backoff_coefficient.offset, bytes(data[d[1][0]:d[1][1]])[::-1], 8)
    flags = abi.XI_STARTED | (abi.XI_CANCEL_REQUESTED if g(70, T_BOOL) else 0) | (abi.XI_HAS_RETRY if g(98, T_BOOL) else 0)
    if g(94, T_I64) != abi.ZERO_TIME_NANOS:
        flags |= abi.XI_HAS_EXPIRATION
        x.expiration_time = g(94, T_I64)
    lst = fget(st, 96, T_LIST)
    if lst is not None and lst[0][1] == T_STRING and lst[0][2]:
        xs["nonretriable"] = bytes(data[lst[1][0]:lst[1][1]])
    xs["cron_schedule"] = g(100, T_STRING, b"")
    # ---- the findings, in the header's order
    two_dc, ndc = has(44, T_I64), has(122, T_STRING)
    if two_dc and ndc:
        raise RowError(E_SHAPE)
    builder = abi.BUILDER_2DC if two_dc else abi.BUILDER_NDC if ndc else abi.BUILDER_LOCAL
    if two_dc:
        repl.present = 1
        repl.start_version, repl.current_version = ps.start_version, ps.current_version
        repl.last_write_version, repl.last_write_event_id = col.last_write_version, g(44, T_I64)
        m = fget(st, 46, T_MAP)
        if m is not None and m[0][1] == T_STRING and m[0][2] == T_STRUCT:
            for k, v in m[0][3]:
                if k not in clusters:
                    raise RowError(E_CLUSTER)
                i = clusters.index(k)
                repl.lri_mask |= 1 << i
                repl.lri_version[i] = (fget(v, 10, T_I64) or (0,))[0]
                repl.lri_last_event_id[i] = (fget(v, 12, T_I64) or (0,))[0]
    tree, lo, hi = b"", 0, 0
    if has(104, T_STRING):
        flags |= abi.XI_HAS_BRANCH
        tree, lo, hi = _token(g(104, T_STRING))
    rps = []
    rpb = g(115, T_STRING, b"")
    if rpb:
        pts = fget(_nested(rpb, g(116, T_STRING, b"")), 10, T_LIST)
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
                val = lambda f, t, d=0: (fget(pt, f, t) or (d,))[0]  # noqa: E731
                p.first_decision_completed_id, p.created_time_nano = val(30, T_I64), val(40, T_I64)
                p.expiring_time_nano = val(50, T_I64)
                p.flags = pf | (abi.RP_RESETTABLE if val(60, T_BOOL) else 0)
                rps.append((p, val(10, T_STRING, b""), val(20, T_STRING, b"")))
    sa, n_sa_wire, sa_strings = [], 0, []
    m = fget(st, 118, T_MAP)
    if m is not None:
        flags |= abi.XI_HAS_SEARCH_ATTR
        if m[0][1] == T_STRING and m[0][2] == T_STRING:
            n_sa_wire = len(m[0][3])
            if n_sa_wire > abi.LOAD_MAX_SEARCH_ATTR:
                raise RowError(E_SHAPE)
            sa_strings = [s for kv in m[0][3] for s in kv]  # every pair's, a superseded value included
            last = dict(m[0][3])
            sa = [(k, last[k]) for k in dict.fromkeys(k for k, _ in m[0][3])]
    m = fget(st, 120, T_MAP)
    if m is not None:
        flags |= abi.XI_HAS_MEMO
        xs["memo"] = b"\x0d\x00\x0a" + bytes(data[m[1][0]:m[1][1]]) + b"\x00"
    vh = []
    if ndc:
        vst = _nested(g(122, T_STRING), g(124, T_STRING, b""))
        hs = fget(vst, 20, T_LIST)
        if (fget(vst, 10, T_I32) or (0,))[0] != 0 or hs is None or hs[0][1] != T_STRUCT or len(hs[0][2]) != 1:
            raise RowError(E_SHAPE)
        h = hs[0][2][0]
        vtok = (fget(h, 10, T_STRING) or (b"",))[0]
        if vtok:
            tree, lo, hi = _token(vtok)
            if has(104, T_STRING):
                raise RowError(E_SHAPE)
            flags |= abi.XI_VH_BRANCH
        its = fget(h, 20, T_LIST)
        if its is not None and its[0][1] == T_STRUCT:
            if len(its[0][2]) > abi.LOAD_MAX_VH_ITEMS:
                raise RowError(E_SHAPE)
            vh = [((fget(i, 10, T_I64) or (0,))[0], (fget(i, 20, T_I64) or (0,))[0]) for i in its[0][2]]
    xs["branch_tree_id"], x.branch_id_lo, x.branch_id_hi = tree, lo, hi
    x.flags, x.reset_points_len, x.search_attr_len = flags, len(rps), len(sa)
    if xs["memo"]:
        gen.append(xs["memo"])
    return SimpleNamespace(x=x, xs=xs, ps=ps, pss=pss, repl=repl, builder=builder, vh=vh, rps=rps, sa=sa,
                           n_sa_wire=n_sa_wire, sa_strings=sa_strings, gen=gen)


def columns(rows, w: int) -> SimpleNamespace:
    X = rows.exec
    return SimpleNamespace(domain_id=X.domain_id[16 * w:16 * w + 16].tobytes(), run_id=X.run_id[16 * w:16 * w + 16].tobytes(),
                           workflow_id=rows.bytes[int(X.workflow_id_off[w]):int(X.workflow_id_off[w + 1])].tobytes(),
                           next_event_id=int(X.next_event_id[w]), last_write_version=int(X.last_write_version[w]))


def decode_state(rows, seeds: list) -> SimpleNamespace:
    """The whole cdr_load_state contract on a cadence_amd.rows.Rows with .exec: rows_ref.decode's
    fields, .result with n_vh / n_reset_points / n_search_attr appended, .caps with (vh, rp, sa)
    offsets and capacities appended, and per entry .exec / .repl / .persist (record bytes, None
    where unspecified) / .builder / .exec_status, item tables .vh / .rp / .sa by slot, .totals
    (vh, rp, sa) and .gen_len."""
    data = rows.bytes.tobytes()
    ne, n_rows, X = rows.n_entries, rows.n_rows, rows.exec
    clusters = [seeds[s] if s < len(seeds) else None for s in X.cluster_seed]
    parsed = [[None] * n_rows[t] for t in range(5)]
    status = [[0] * n_rows[t] for t in range(5)]
    for t in range(5):
        for r in range(n_rows[t]):
            key = rows.timer_id(r) if t == 1 else int(rows.key[t][r])
            hb = int(rows.act_heartbeat[r]) if t == 0 else 0
            try:
                parsed[t][r] = rows_ref.parse_row(t, data, int(rows.blob_off[t][r]), int(rows.blob_off[t][r + 1]), key, hb)
            except (TD.DecodeError, RowError) as e:
                status[t][r] = e.code
    xp, xstatus = [None] * ne, [0] * ne
    for w in range(ne):
        try:
            xp[w] = parse_exec(data, min(int(X.blob_off[w]), len(data)), min(int(X.blob_off[w + 1]), len(data)),
                               columns(rows, w), clusters)
        except (TD.DecodeError, RowError) as e:
            xstatus[w] = e.code

    def span(t, w):
        return range(int(rows.entry_row0[t][w]), int(rows.entry_row0[t][w + 1]))

    def first_failure(w):
        for t in range(5):
            for r in span(t, w):
                if status[t][r]:
                    return status[t][r]
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
    # the item tables' slots: every entry whose execution row decoded owns its wire counts
    cnt = [(len(p.vh), len(p.rps), p.n_sa_wire, (sum(len(s) for s in p.gen) + 3) & ~3) if p else (0, 0, 0, 0) for p in xp]
    off = [(0, 0, 0, 0)]
    for c in cnt:
        off.append(tuple(a + b for a, b in zip(off[-1], c)))
    out.totals, out.gen_len = off[-1][:3], 36 * n_rows[2] + off[-1][3]
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
                for f, s in strs.items():
                    setattr(rec, f, it.handle(s))
                k = rec.timer_id if t == 1 else int(rows.key[t][r])
                done.append((k, r, rec))
            uses = collections.Counter(k for k, _, _ in done)
            for k, r, _ in done:
                if len(done) > abi.LOAD_MAX_ENTRY_ROWS:
                    status[t][r] = rows_ref.E_ENTRY_ROWS
                elif uses[k] > 1:
                    status[t][r] = rows_ref.E_DUP_KEY
            recs.append(sorted(done, key=lambda x: x[0]))
        entry_status[w] = first_failure(w)
        if entry_status[w]:
            continue
        for t in range(5):
            for j, (_, _, rec) in enumerate(recs[t]):
                out.tables[t][int(rows.entry_row0[t][w]) + j] = bytes(rec)
        p = xp[w]
        for f, s in p.xs.items():
            setattr(p.x, f, it.handle(s))
        for f, s in p.pss.items():
            setattr(p.ps, f, it.handle(s))
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
        out.caps.append(([int(rows.entry_row0[t][w]) for t in range(5)], c5, off[w][:3], cnt[w][:3]))
    out.strings = list(seeds) + [it.new[h] for h in sorted(it.new)]
    return out


def compare_state(got, want, rows) -> list:
    """Mismatches between a cadence_amd.rows.Loaded of load_state and the reference."""
    bad = []
    for t in range(5):
        gs = [int(x) for x in got.row_status[t]]
        if gs != want.row_status[t]:
            r = next(i for i, (a, b) in enumerate(zip(gs, want.row_status[t])) if a != b)
            bad.append(f"row_status[{t}][{r}]: {gs[r]} != {want.row_status[t][r]}")
    for name in ("entry_status", "exec_status"):
        g, e = [int(x) for x in getattr(got, name)], getattr(want, name)
        if g != e:
            w = next(i for i, (a, b) in enumerate(zip(g, e)) if a != b)
            bad.append(f"{name}[{w}]: {g[w]} != {e[w]}")
    if got.n_bad_entries != sum(1 for s in want.entry_status if s):
        bad.append(f"n_bad_entries {got.n_bad_entries}")
    if (got.totals.vh, got.totals.rp, got.totals.sa) != tuple(want.totals):
        bad.append(f"totals {(got.totals.vh, got.totals.rp, got.totals.sa)} != {want.totals}")
    if len(got.gen_bytes) != want.gen_len:
        bad.append(f"n_gen_bytes {len(got.gen_bytes)} != {want.gen_len}")
    for w in range(rows.n_entries):
        r, c = got.result[w], got.caps[w]
        g = (r.code, r.n_activity, r.n_timer, r.n_child, r.n_cancel, r.n_signal, r.n_vh, r.n_reset_points, r.n_search_attr)
        if g != want.result[w]:
            bad.append(f"result[{w}]: {g} != {want.result[w]}")
        if (r.flags, r.fail_event_id, r.fail_index) != (0, 0, 0):
            bad.append(f"result[{w}]: fields the loader leaves zero are set")
        exp = abi.CdrWfCaps()
        offs, cnts, xoff, xcnt = want.caps[w]
        for i, t in enumerate(TABLES):
            setattr(exp, t + "_off", offs[i])
            setattr(exp, t + "_cap", cnts[i])
        for i, t in enumerate(("vh", "rp", "sa")):
            setattr(exp, t + "_off", xoff[i])
            setattr(exp, t + "_cap", xcnt[i])
        if bytes(c) != bytes(exp):
            bad.append(f"caps[{w}]")
        if want.entry_status[w] == 0:
            if int(got.builder[w]) != want.builder[w]:
                bad.append(f"builder[{w}]: {got.builder[w]} != {want.builder[w]}")
            for name, ty in (("exec", abi.CdrExecInfo), ("repl", abi.CdrReplState), ("persist", abi.CdrExecPersist)):
                a, b = bytes(getattr(got, name)[w]), getattr(want, name)[w]
                if a != b:
                    ga, wb = ty.from_buffer_copy(a), ty.from_buffer_copy(b)
                    diff = [f for f, *_ in ty._fields_ if bytes(C.string_at(C.addressof(ga) + getattr(ty, f).offset,
                                                                                   getattr(ty, f).size)) !=
                            bytes(C.string_at(C.addressof(wb) + getattr(ty, f).offset, getattr(ty, f).size))]
                    bad.append(f"{name}[{w}] differs in {diff}")
    if list(got.strings) != want.strings:
        bad.append(f"strings: {len(got.strings)} vs {len(want.strings)}" + "".join(
            f"; [{h}] {a[:40]!r} != {b[:40]!r}" for h, (a, b) in enumerate(zip(got.strings, want.strings)) if a != b)[:300])
    for i, t in enumerate(TABLES + ("vh", "rp", "sa")):
        size = C.sizeof(engine.TABLE_TYPES[t])
        raw = bytes(got.tables[t])
        for slot, rec in enumerate(want.tables[i] if i < 5 else getattr(want, t)):
            if rec is not None and raw[slot * size:(slot + 1) * size] != rec:
                bad.append(f"{t}[{slot}]: record differs")
                if len(bad) > 20:
                    return bad
    return bad
