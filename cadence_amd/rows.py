"""Host side of the persisted-row loader (cdr.h cdr_load_rows, csrc/load.hip).

``encode_state`` runs the existing row encoders over the five pending tables of replayed
states — and, with ``exec_rows=True``, over their execution rows — and packs the blobs the
way a store would hand them back (a ``Rows``, the host form of cdr_rows_in and
cdr_exec_rows_in); ``load`` decodes the pending tables of a ``Rows`` on the device
(cdr_load_rows) and ``load_state`` the execution rows with them (cdr_load_state), both
returning host copies of every output; ``to_carry`` turns a decode into an ``engine.Carry``
a batch can replay onto — a ``load_state`` result as it is, a ``load`` result with the
caller's exec / repl / vh / rp / sa records.  ``gather`` runs cdr_strtab_gather_async on
any decoded string table.  The Cassandra form of the pending tables (cdr_load_cql_rows):
``encode_state_cql`` wraps the CQL encoder's rows as map columns (a ``CqlCols``, built by
``pack_cql``) and ``load_cql`` decodes them on the device into the same ``Loaded``; with
``exec_rows=True`` the execution row's four columns go with them (a ``CqlExec``) and
``load_cql_state`` decodes the whole state (cdr_load_cql_state), which ``to_carry`` takes as
it takes a ``load_state`` result.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import struct
from types import SimpleNamespace

import numpy as np

from . import abi, engine
from .ingest import stand_in, string_table

TABLES = ("act", "timer", "child", "cancel", "signal")  # cdr.h table numbers 0 .. 4
KEY = {"act": "schedule_id", "child": "initiated_id", "cancel": "initiated_id", "signal": "initiated_id"}
HANDLES = {"act": ("activity_id", "request_id", "task_list", "nonretriable"), "timer": ("timer_id",),
           "child": ("started_workflow_id", "started_run_id", "domain_name", "workflow_type"), "cancel": (),
           "signal": ("signal_name", "input", "control")}


@dataclasses.dataclass
class ExecRows:
    """cdr_exec_rows_in on the host: entry w's execution row is bytes[blob_off[w]:blob_off[w+1]]
    of the Rows that holds it, its workflow ID bytes[workflow_id_off[w]:workflow_id_off[w+1]]."""
    blob_off: np.ndarray            # uint64 [n_entries + 1]
    domain_id: np.ndarray           # uint8 [16 * n_entries]
    run_id: np.ndarray              # uint8 [16 * n_entries]
    workflow_id_off: np.ndarray     # uint64 [n_entries + 1]
    next_event_id: np.ndarray       # int64 [n_entries]
    last_write_version: np.ndarray  # int64 [n_entries]
    cluster_seed: list              # seed index of cluster i's name


@dataclasses.dataclass
class Rows:
    """cdr_rows_in on the host.  Row r of table t: blob bytes[blob_off[t][r]:blob_off[t][r+1]],
    key[t][r] (tables 0, 2-4) or the timer ID bytes[timer_id_off[r]:timer_id_off[r+1]]
    (table 1); entry w owns rows [entry_row0[t][w], entry_row0[t][w+1])."""
    bytes: np.ndarray          # uint8
    blob_off: list             # 5 x uint64 [n_rows + 1]
    entry_row0: list           # 5 x uint32 [n_entries + 1]
    key: list                  # 5 x int64 [n_rows] (key[1] is empty)
    timer_id_off: np.ndarray   # uint64 [n_rows[1] + 1]
    act_heartbeat: np.ndarray  # int64 [n_rows[0]]
    n_entries: int
    src: list = None           # encode_state: 5 x [(entry, row j of the entry)] per packed row
    exec: ExecRows = None      # the execution rows (cdr_load_state)

    @property
    def n_rows(self):
        return [len(o) - 1 for o in self.blob_off]

    def blob(self, t: int, r: int) -> bytes:
        return self.bytes[int(self.blob_off[t][r]):int(self.blob_off[t][r + 1])].tobytes()

    def timer_id(self, r: int) -> bytes:
        return self.bytes[int(self.timer_id_off[r]):int(self.timer_id_off[r + 1])].tobytes()


def pack(n_entries: int, tables, exec_rows=None, cluster_seed=()) -> Rows:
    """tables[t][w] = entry w's rows of table t in arrival order: (key, blob) for tables 0,
    2, 3, 4 — table 0 may add a third item, the heartbeat column (default: Go's zero time) —
    and (timer ID bytes, blob) for table 1.  Each table's blobs are contiguous in `bytes`,
    the timer IDs follow the last blob.  exec_rows[w] = (blob, domain ID's 16 bytes, run ID's
    16 bytes, workflow ID, next_event_id, last_write_version) adds the execution rows: the
    workflow IDs follow the timer IDs and the execution blobs come last."""
    chunks, pos = [], 0
    offs, row0, keys, hb, ids = [], [], [], [], []
    for t in range(5):
        off, r0, ks = [pos], [0], []
        for w in range(n_entries):
            for row in tables[t][w]:
                if t == 1:
                    ids.append(bytes(row[0]))
                else:
                    ks.append(row[0])
                    if t == 0:
                        hb.append(row[2] if len(row) > 2 else abi.ZERO_TIME_NANOS)
                chunks.append(bytes(row[1]))
                pos += len(row[1])
                off.append(pos)
            r0.append(len(off) - 1)
        offs.append(np.array(off, np.uint64))
        row0.append(np.array(r0, np.uint32))
        keys.append(np.array(ks, np.int64))
    tid_off = [pos]
    for s in ids:
        chunks.append(s)
        pos += len(s)
        tid_off.append(pos)
    xr = None
    if exec_rows is not None:
        assert len(exec_rows) == n_entries and all(len(x[1]) == 16 and len(x[2]) == 16 for x in exec_rows)
        wid_off = [pos]
        for x in exec_rows:
            chunks.append(bytes(x[3]))
            pos += len(x[3])
            wid_off.append(pos)
        xoff = [pos]
        for x in exec_rows:
            chunks.append(bytes(x[0]))
            pos += len(x[0])
            xoff.append(pos)
        xr = ExecRows(np.array(xoff, np.uint64), np.frombuffer(b"".join(bytes(x[1]) for x in exec_rows), np.uint8).copy(),
                      np.frombuffer(b"".join(bytes(x[2]) for x in exec_rows), np.uint8).copy(),
                      np.array(wid_off, np.uint64), np.array([x[4] for x in exec_rows], np.int64),
                      np.array([x[5] for x in exec_rows], np.int64), list(cluster_seed))
    data = np.frombuffer(b"".join(chunks) or b"\0", np.uint8).copy()
    return Rows(data[:pos], offs, row0, keys, np.array(tid_off, np.uint64), np.array(hb, np.int64), n_entries,
                exec=xr)


def heartbeat_column(a) -> int:
    """The LastHeartbeatUpdatedTime column of an activity record: its heartbeat time when
    either time bit says it is a real instant, else Go's zero time."""
    if a.flags & (abi.AI_STARTED_TIME_SET | abi.AI_HEARTBEAT_TIME_SET):
        return a.last_heartbeat_time
    return abi.ZERO_TIME_NANOS


def run_id_text(h: int) -> bytes:
    return b"%08x-0000-4000-8000-%012x" % (h & 0xFFFFFFFF, h)


def state_strings(batch: engine.Batch, out: engine.Outputs, strings=None) -> list:
    """A table of distinct strings covering every handle the pending tables of `out` name:
    ingest.stand_in's string per handle (or `strings`), canonical UUID text for the handles
    used as a child's started run ID, a one-element list<string> body for the handles used
    as RetryNonRetryableErrors."""
    hmax, runs, lists = 1, set(), set()
    for w in range(batch.n_wfs):
        if out.result[w].code != abi.OK:
            continue
        for t in TABLES:
            for r in out.rows(w, t):
                hmax = max([hmax] + [getattr(r, f) for f in HANDLES[t]])
                if t == "child" and r.started_run_id:
                    runs.add(r.started_run_id)
                if t == "act" and r.nonretriable:
                    lists.add(r.nonretriable)
    tab = [b""] + [stand_in(h, strings) for h in range(1, hmax + 1)]
    for h in runs:
        tab[h] = run_id_text(h)
    for h in lists - runs:
        s = stand_in(h, strings)
        tab[h] = struct.pack(">bi", 11, 1) + struct.pack(">i", len(s)) + s
    return tab


X_HANDLES = ("domain_id", "workflow_id", "run_id", "create_request_id", "parent_domain_id", "parent_workflow_id",
             "parent_run_id", "task_list", "workflow_type", "cron_schedule", "memo", "nonretriable", "branch_tree_id",
             "decision_request_id")
X_UUIDS = ("domain_id", "run_id", "parent_domain_id", "parent_run_id")
ITEM_HANDLES = {"rp": ("binary_checksum", "run_id"), "sa": ("key", "value")}


def whole_state_strings(batch: engine.Batch, out: engine.Outputs, extra: int = 0, strings=None) -> list:
    """state_strings extended to the execution rows: a table of distinct strings covering every
    handle the OK entries of `out` name anywhere (and `extra` more handles after them, for a
    persistence context or cluster names), with canonical UUID text for the handles used as a
    domain, run or parent ID, a Memo struct body for Memo handles and a list<string> body for
    RetryNonRetryableErrors handles."""
    hmax, uuids, memos, lists = 1, set(), set(), set()
    for w in range(batch.n_wfs):
        if out.result[w].code != abi.OK:
            continue
        x = out.exec[w]
        hmax = max([hmax] + [getattr(x, f) for f in X_HANDLES])
        uuids |= {getattr(x, f) for f in X_UUIDS}
        memos.add(x.memo)
        lists.add(x.nonretriable)
        for t in TABLES + ("rp", "sa"):
            for r in out.rows(w, t):
                hmax = max([hmax] + [getattr(r, f) for f in {**HANDLES, **ITEM_HANDLES}[t]])
                if t == "child":
                    uuids.add(r.started_run_id)
                if t == "act":
                    lists.add(r.nonretriable)
    tab = [b""] + [stand_in(h, strings) for h in range(1, hmax + 1 + extra)]
    for h in lists - {0}:
        s = stand_in(h, strings)
        tab[h] = struct.pack(">bi", 11, 1) + struct.pack(">i", len(s)) + s
    for h in memos - {0}:
        k = b"memo-%d" % h
        tab[h] = b"\x0d\x00\x0a" + struct.pack(">bbi", 11, 11, 1) + struct.pack(">i", len(k)) + k + \
            struct.pack(">i", 2) + b"mv" + b"\x00"
    for h in uuids - {0}:
        tab[h] = run_id_text(h)
    return tab


def uuid_bytes(text: bytes) -> bytes:
    """The 16 bytes of a key column from an ID's text (sqldb.MustParseUUID); an ID that is no
    UUID — a row the store could not hold — becomes its first 16 bytes, zero-padded."""
    h = bytes(text).replace(b"-", b"")
    try:
        if len(h) == 32:
            return bytes.fromhex(h.decode("ascii"))
    except (ValueError, UnicodeDecodeError):
        pass
    return bytes(text)[:16].ljust(16, b"\0")


def encode_state(eng: engine.Engine, batch: engine.Batch, out: engine.Outputs, strings: list, exec_rows: bool = False,
                 persist=None, cluster_names=None) -> Rows:
    """The five pending tables of the OK entries of `out` as the SQL persistence stores
    them: the device encoders' blobs (cdr_encode_blobs_async / cdr_encode_rows_async), the
    key columns and the activity heartbeat column from the records, timer IDs from
    `strings`.  A row an encoder refuses (status != 0) is left out of its entry.
    `.src[t]` names each packed row's (entry, row of the entry).
    exec_rows=True adds the execution rows: cdr_encode_blobs_async table 5 with `persist` (a
    cdr_exec_persist array; default: zeros but a 2DC entry's start / current version) and `cluster_names` (handles), the key columns from
    the exec records' strings, next_event_id and last_write_version from the records; an entry
    that is not OK, or whose row the encoder refuses, gets an empty blob (it fails to load)."""
    blobs = {}
    for t in TABLES:
        if t in ("timer", "cancel"):
            blobs[t] = eng.encode_rows(batch, out, t)
        else:
            got, codes = eng.encode_blobs(batch, out, t, strings)
            blobs[t] = {r: b for r, b in got.items() if codes[r] == 0}
    tables, src = [], []
    for t in TABLES:
        per_entry, s = [], []
        for w in range(batch.n_wfs):
            rows = []
            if out.result[w].code == abi.OK:
                base = getattr(out.plan.caps[w], t + "_off")
                for j, rec in enumerate(out.rows(w, t)):
                    if base + j not in blobs[t]:
                        continue
                    if t == "timer":
                        if rec.timer_id >= len(strings):
                            continue
                        rows.append((strings[rec.timer_id], blobs[t][base + j]))
                    elif t == "act":
                        rows.append((rec.schedule_id, blobs[t][base + j], heartbeat_column(rec)))
                    else:
                        rows.append((getattr(rec, KEY[t]), blobs[t][base + j]))
                    s.append((w, j))
            per_entry.append(rows)
        tables.append(per_entry)
        src.append(s)
    xrows = None
    if exec_rows:
        names = list(cluster_names if cluster_names is not None else [])
        if persist is None:  # buildExecutionRow's start / current version are the replication state's
            persist = (abi.CdrExecPersist * max(1, batch.n_wfs))()
            for w in range(batch.n_wfs):
                if batch.wfs[w].builder == abi.BUILDER_2DC:
                    persist[w].start_version = out.repl[w].start_version
                    persist[w].current_version = out.repl[w].current_version
        got, codes = eng.encode_blobs(batch, out, "exec", strings, persist, names)
        S = lambda h: strings[h] if h < len(strings) else b""  # noqa: E731
        xrows = []
        for w in range(batch.n_wfs):
            x = out.exec[w]
            blob = got[w] if w in got and codes[w] == 0 else b""
            xrows.append((blob, uuid_bytes(S(x.domain_id)), uuid_bytes(S(x.run_id)), S(x.workflow_id), x.next_event_id,
                          out.repl[w].last_write_version))
    rows = pack(batch.n_wfs, tables, xrows, cluster_names or ())
    rows.src = src
    return rows


@dataclasses.dataclass
class Loaded:
    tables: dict              # "act" .. "signal" -> ctypes record arrays [n_rows[t]]
    result: C.Array           # cdr_wf_result [n_entries]
    caps: C.Array             # cdr_wf_caps [n_entries]
    totals: abi.CdrTotals
    row_status: list          # 5 x int32 [n_rows[t]]
    entry_status: np.ndarray  # int32 [n_entries]
    strings: list             # bytes per handle
    str_ref: np.ndarray
    str_len: np.ndarray
    gen_bytes: bytes
    n_bad_entries: int
    gathered: list = None     # load(gather=True): the table cdr_strtab_gather_async built
    rc: int = 0
    # load_state with execution rows: the records per entry (tables also holds "vh", "rp", "sa")
    exec: C.Array = None
    repl: C.Array = None
    persist: C.Array = None
    builder: np.ndarray = None      # uint32 [n_entries]
    exec_status: np.ndarray = None  # int32 [n_entries]
    # load_cql: the rows the device split the map columns into
    n_rows: list = None             # 5 counts
    entry_row0: list = None         # 5 x uint32 [n_entries + 1]

    def rows(self, w: int, t: str):
        off = getattr(self.caps[w], t + "_off")
        return [self.tables[t][off + j] for j in range(getattr(self.result[w], engine.TABLE_COUNT[t]))]


class DeviceBuffers:
    """Device buffers of one call, freed together."""

    def __init__(self):
        self.hip, self.ptrs = engine._hip(), []

    def alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        if self.hip.hipMalloc(C.byref(p), C.c_size_t(max(8, nbytes))) != 0:
            raise RuntimeError("hipMalloc failed")
        self.ptrs.append(p)
        return p.value

    def up(self, a: np.ndarray, at_end: bool = False) -> int:
        a = np.ascontiguousarray(a)
        if at_end:  # the array's last byte is the last byte of its allocation
            size = (a.nbytes + 4095) // 4096 * 4096 or 4096
            p = self.alloc(size) + size - a.nbytes
        else:
            p = self.alloc(a.nbytes)
        if a.nbytes and self.hip.hipMemcpy(C.c_void_p(p), a.ctypes.data, C.c_size_t(a.nbytes), 1) != 0:
            raise RuntimeError("hipMemcpy H2D failed")
        return p

    def down(self, ptr, dtype, n: int) -> np.ndarray:
        out = np.zeros(max(1, n), dtype)
        if n and self.hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), C.c_size_t(n * out.itemsize), 2) != 0:
            raise RuntimeError("hipMemcpy D2H failed")
        return out[:n]

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


def _gather(eng, dev: DeviceBuffers, str_ref, str_len, n: int, d_bytes, d_seeds, d_gen) -> list:
    L = abi.lib()
    off = dev.alloc(8 * (n + 1))
    rc = L.cdr_strtab_gather_async(eng.ctx, str_ref, str_len, n, d_bytes, d_seeds, d_gen, off, None, None)
    if rc:
        raise RuntimeError(f"cdr_strtab_gather_async (sizes) rc={rc}")
    offs = dev.down(off, np.uint64, n + 1)
    total = int(offs[-1]) if n else 0
    buf = dev.alloc(total)
    rc = L.cdr_strtab_gather_async(eng.ctx, str_ref, str_len, n, d_bytes, d_seeds, d_gen, off, buf, None)
    if rc:
        raise RuntimeError(f"cdr_strtab_gather_async (copy) rc={rc}")
    raw = dev.down(buf, np.uint8, total).tobytes()
    return [raw[int(offs[h]):int(offs[h + 1])] for h in range(n)]


def gather(eng: engine.Engine, str_ref: int, str_len: int, n: int, blob_bytes: np.ndarray, seeds: list) -> list:
    """cdr_strtab_gather_async on a decoded table still resident in the context (device
    pointers str_ref / str_len, e.g. a cdr_ingest_out's; gen_bytes NULL): bytes per handle."""
    dev = DeviceBuffers()
    try:
        sb, _ = string_table(seeds)
        return _gather(eng, dev, str_ref, str_len, n, dev.up(blob_bytes), dev.up(sb), None)
    finally:
        dev.free()


def load(eng: engine.Engine, rows: Rows, seeds: list, at_end: bool = False, gather: bool = False,
         check: bool = True) -> Loaded:
    """cdr_load_rows on the device; host copies of every output.  `at_end`: `bytes` is
    uploaded so that it ends where its allocation ends.  `gather`: also build the
    contiguous string table on the device (cdr_strtab_gather_async) -> .gathered.
    check=False returns the call's status in .rc instead of raising."""
    return _load(eng, rows, seeds, at_end, gather, check, False)


def load_state(eng: engine.Engine, rows: Rows, seeds: list, at_end: bool = False, gather: bool = False,
               check: bool = True, cluster_seed=None) -> Loaded:
    """cdr_load_state on the device: as `load`, with the execution rows of `rows.exec` decoded
    too (rows.exec None: exec == NULL, cdr_load_rows' results).  `cluster_seed` overrides
    rows.exec.cluster_seed: the index in `seeds` of each cluster's name."""
    return _load(eng, rows, seeds, at_end, gather, check, True, cluster_seed)


def _load(eng, rows, seeds, at_end, gather, check, state, cluster_seed=None) -> Loaded:
    L = abi.lib()
    dev = DeviceBuffers()
    try:
        sb, so = string_table(seeds)
        inp = abi.CdrRowsIn()
        inp.bytes = dev.up(rows.bytes if len(rows.bytes) else np.zeros(1, np.uint8), at_end and len(rows.bytes) > 0)
        inp.n_bytes = len(rows.bytes)
        n_rows = rows.n_rows
        for t in range(5):
            inp.blob_off[t] = dev.up(rows.blob_off[t])
            inp.entry_row0[t] = dev.up(rows.entry_row0[t])
            inp.key[t] = dev.up(rows.key[t]) if t != 1 else None
            inp.n_rows[t] = n_rows[t]
        inp.timer_id_off = dev.up(rows.timer_id_off)
        inp.act_heartbeat = dev.up(rows.act_heartbeat)
        inp.seed_bytes, inp.seed_off = dev.up(sb), dev.up(so)
        inp.n_entries, inp.n_seeds = rows.n_entries, len(seeds)
        X = rows.exec if state else None
        if state:
            sout, xin = abi.CdrStateOut(), None
            if X is not None:
                xin = abi.CdrExecRowsIn()
                xin.blob_off, xin.workflow_id_off = dev.up(X.blob_off), dev.up(X.workflow_id_off)
                xin.domain_id, xin.run_id = dev.up(X.domain_id), dev.up(X.run_id)
                xin.next_event_id, xin.last_write_version = dev.up(X.next_event_id), dev.up(X.last_write_version)
                cs = list(X.cluster_seed if cluster_seed is None else cluster_seed)
                xin.n_clusters = len(cs)
                for i, h in enumerate(cs[:abi.MAX_CLUSTERS]):
                    xin.cluster_seed[i] = h
            rc = L.cdr_load_state(eng.ctx, C.byref(inp), C.byref(xin) if xin is not None else None, C.byref(sout), None)
            out = sout.rows
        else:
            out = abi.CdrRowsOut()
            rc = L.cdr_load_rows(eng.ctx, C.byref(inp), C.byref(out), None)
        if rc:
            if check:
                raise RuntimeError(f"cdr_load_{'state' if state else 'rows'} rc={rc}")
            return Loaded({}, None, None, abi.CdrTotals(), [], np.zeros(0, np.int32), [], None, None, b"", 0, rc=rc)
        ne = rows.n_entries

        def recs(ptr, ty, n):
            raw = dev.down(ptr, np.uint8, n * C.sizeof(ty)).tobytes()
            return (ty * n).from_buffer_copy(raw) if n else (ty * 0)()
        tables = {t: recs(getattr(out.state, t), engine.TABLE_TYPES[t], n_rows[i]) for i, t in enumerate(TABLES)}
        result = recs(out.state.result, abi.CdrWfResult, ne)
        caps = recs(out.caps, abi.CdrWfCaps, ne)
        status = [dev.down(out.row_status[t], np.int32, n_rows[t]) for t in range(5)]
        est = dev.down(out.entry_status, np.int32, ne)
        ref = dev.down(out.str_ref, np.uint64, out.n_strings)
        ln = dev.down(out.str_len, np.uint32, out.n_strings)
        gen = dev.down(out.gen_bytes, np.uint8, out.n_gen_bytes).tobytes()
        raw, sraw = rows.bytes.tobytes(), sb.tobytes()
        strings = []
        for h in range(out.n_strings):
            r, n = int(ref[h]), int(ln[h])
            src = sraw if r & abi.STR_REF_SEED else gen if r & abi.STR_REF_GEN else raw
            r &= abi.STR_REF_GEN - 1
            strings.append(src[r:r + n])
        res = Loaded(tables, result, caps, out.totals, status, est, strings, ref, ln, gen, out.n_bad_entries)
        if X is not None:
            for t in ("vh", "rp", "sa"):
                tables[t] = recs(getattr(out.state, t), engine.TABLE_TYPES[t], getattr(out.totals, t))
            res.exec = recs(out.state.exec, abi.CdrExecInfo, ne)
            res.repl = recs(out.state.repl, abi.CdrReplState, ne)
            res.persist = recs(sout.persist, abi.CdrExecPersist, ne)
            res.builder = dev.down(sout.builder, np.uint32, ne)
            res.exec_status = dev.down(sout.exec_status, np.int32, ne)
        if gather:
            res.gathered = _gather(eng, dev, out.str_ref, out.str_len, out.n_strings, inp.bytes, inp.seed_bytes,
                                   out.gen_bytes)
        return res
    finally:
        dev.free()


def to_carry(loaded: Loaded, other: engine.Outputs = None, src=None) -> engine.Carry:
    """A Carry over a decode.  A `load_state` result with its execution rows is a whole state:
    `other` is not needed, and src defaults to every entry that loaded (-1: fresh builder).
    A `load` result holds the pending tables alone: the exec / repl / vh / rp / sa records come
    from the caller (`other`, entry for entry), and src defaults to every entry that loaded
    and whose `other` record is OK."""
    n = len(loaded.result)
    if other is None:
        if loaded.exec is None:
            raise ValueError("a decode without execution rows needs the caller's records (other)")
        caps = (abi.CdrWfCaps * max(1, n))()
        tot = abi.CdrTotals()
        for t in TABLES + ("vh", "rp", "sa"):
            setattr(tot, t, getattr(loaded.totals, t))
        st = engine.Outputs(SimpleNamespace(n_wfs=n), engine.Plan(caps, tot))
        if n:
            C.memmove(caps, loaded.caps, C.sizeof(abi.CdrWfCaps) * n)
            C.memmove(st.result, loaded.result, C.sizeof(abi.CdrWfResult) * n)
            C.memmove(st.exec, loaded.exec, C.sizeof(abi.CdrExecInfo) * n)
            C.memmove(st.repl, loaded.repl, C.sizeof(abi.CdrReplState) * n)
            for t in TABLES + ("vh", "rp", "sa"):
                C.memmove(st.tables[t], loaded.tables[t], C.sizeof(loaded.tables[t]))
        if src is None:
            src = np.array([w if st.result[w].code == abi.OK else -1 for w in range(n)], np.int32)
        return engine.Carry(src=np.asarray(src, np.int32), state=st)
    assert n == other.n_wfs
    caps = (abi.CdrWfCaps * max(1, n))()
    tot = abi.CdrTotals()
    for t in TABLES:
        setattr(tot, t, getattr(loaded.totals, t))
    for t in ("vh", "rp", "sa"):
        setattr(tot, t, getattr(other.plan.totals, t))
    st = engine.Outputs(SimpleNamespace(n_wfs=n), engine.Plan(caps, tot))
    for w in range(n):
        for t in TABLES:
            setattr(caps[w], t + "_off", getattr(loaded.caps[w], t + "_off"))
            setattr(caps[w], t + "_cap", getattr(loaded.caps[w], t + "_cap"))
        for t in ("vh", "rp", "sa"):
            setattr(caps[w], t + "_off", getattr(other.plan.caps[w], t + "_off"))
            setattr(caps[w], t + "_cap", getattr(other.plan.caps[w], t + "_cap"))
        r, lo, oo = st.result[w], loaded.result[w], other.result[w]
        C.memmove(C.addressof(r), C.addressof(oo), C.sizeof(r))
        if lo.code != abi.OK and oo.code == abi.OK:
            r.code = lo.code
        for t in TABLES:
            setattr(r, engine.TABLE_COUNT[t], getattr(lo, engine.TABLE_COUNT[t]) if r.code == abi.OK else 0)
    C.memmove(st.exec, other.exec, C.sizeof(abi.CdrExecInfo) * n)
    C.memmove(st.repl, other.repl, C.sizeof(abi.CdrReplState) * n)
    for t in TABLES:
        C.memmove(st.tables[t], loaded.tables[t], C.sizeof(loaded.tables[t]))
    for t in ("vh", "rp", "sa"):
        C.memmove(st.tables[t], other.tables[t], C.sizeof(engine.TABLE_TYPES[t]) * getattr(tot, t))
    if src is None:
        src = np.array([w if st.result[w].code == abi.OK else -1 for w in range(n)], np.int32)
    return engine.Carry(src=np.asarray(src, np.int32), state=st)


# ---------------------------------------------------------------- the Cassandra form
# (cdr.h cdr_load_cql_rows) A row's bound values, as cdr_encode_cql_async emits them, are the
# map key and then the UDT's fields in the statement's order; a column Cassandra returns holds
# each UDT's fields in the order the schema declares them.  Position i of the declared UDT is
# statement field CQL_DECLARED[t][i] (tables not named: the orders agree).
CQL_DECLARED = {"cancel": (0, 2, 1, 3), "signal": (0, 2, 1, 3, 4, 5, 6)}
# The execution row (cdr.h cdr_load_cql_state): the workflow_execution UDT's 58 fields in the
# order the update statement binds them (cdr_encode_cql_async table 5), and in the order the
# schema declares them; EXEC_DECLARED[i] is the statement field at declared position i.
EXEC_STATEMENT = (
    "domain_id", "workflow_id", "run_id", "parent_domain_id", "parent_workflow_id", "parent_run_id", "initiated_id",
    "completion_event_batch_id", "completion_event", "completion_event_data_encoding", "task_list",
    "workflow_type_name", "workflow_timeout", "decision_task_timeout", "execution_context", "state", "close_status",
    "last_first_event_id", "last_event_task_id", "next_event_id", "last_processed_event", "start_time",
    "last_updated_time", "create_request_id", "signal_count", "history_size", "decision_version",
    "decision_schedule_id", "decision_started_id", "decision_request_id", "decision_timeout", "decision_attempt",
    "decision_timestamp", "decision_scheduled_timestamp", "decision_original_scheduled_timestamp", "cancel_requested",
    "cancel_request_id", "sticky_task_list", "sticky_schedule_to_start_timeout", "client_library_version",
    "client_feature_version", "client_impl", "auto_reset_points", "auto_reset_points_encoding", "attempt",
    "has_retry_policy", "init_interval", "backoff_coefficient", "max_interval", "expiration_time", "max_attempts",
    "non_retriable_errors", "event_store_version", "branch_token", "cron_schedule", "expiration_seconds",
    "search_attributes", "memo")
EXEC_DECLARED_NAMES = (
    "domain_id", "workflow_id", "run_id", "parent_domain_id", "parent_workflow_id", "parent_run_id", "initiated_id",
    "completion_event_batch_id", "completion_event", "completion_event_data_encoding", "task_list",
    "workflow_type_name", "workflow_timeout", "decision_task_timeout", "execution_context", "state", "close_status",
    "last_processed_event", "start_time", "last_updated_time", "create_request_id", "decision_version",
    "decision_schedule_id", "decision_started_id", "decision_request_id", "decision_timeout", "decision_attempt",
    "decision_timestamp", "decision_scheduled_timestamp", "decision_original_scheduled_timestamp", "cancel_requested",
    "cancel_request_id", "sticky_task_list", "sticky_schedule_to_start_timeout", "client_library_version",
    "client_feature_version", "client_impl", "attempt", "has_retry_policy", "init_interval", "backoff_coefficient",
    "max_interval", "expiration_time", "max_attempts", "non_retriable_errors", "event_store_version", "signal_count",
    "branch_token", "history_size", "last_first_event_id", "next_event_id", "cron_schedule", "expiration_seconds",
    "last_event_task_id", "auto_reset_points", "auto_reset_points_encoding", "search_attributes", "memo")
EXEC_DECLARED = tuple(EXEC_STATEMENT.index(n) for n in EXEC_DECLARED_NAMES)
assert sorted(EXEC_DECLARED) == list(range(58))
EXEC_COLUMNS = ("execution", "replication_state", "version_histories", "version_histories_encoding")


@dataclasses.dataclass
class CqlExec:
    """cdr_cql_exec_in on the host: entry w's body of column c (EXEC_COLUMNS) is
    bytes[off[c][w]:off[c][w+1]] of the CqlCols that holds it (empty: null)."""
    off: list           # 4 x uint64 [n_entries + 1]
    cluster_seed: list  # seed index of cluster i's name


@dataclasses.dataclass
class CqlCols:
    """cdr_cql_rows_in on the host: entry w's column body of table t is
    bytes[col_off[t][w]:col_off[t][w+1]] (empty: a null column)."""
    bytes: np.ndarray    # uint8
    col_off: list        # 5 x uint64 [n_entries + 1]
    n_entries: int
    src: list = None     # encode_state_cql: 5 x [(entry, row j of the entry)] per pair, in column order
    exec: CqlExec = None  # the execution row's columns (cdr_load_cql_state)

    def column(self, t: int, w: int) -> bytes:
        return self.bytes[int(self.col_off[t][w]):int(self.col_off[t][w + 1])].tobytes()

    def exec_column(self, c: int, w: int) -> bytes:
        return self.bytes[int(self.exec.off[c][w]):int(self.exec.off[c][w + 1])].tobytes()


def cql_values(b: bytes) -> list:
    """The [bytes] values (length words included) a run of CQL values consists of."""
    out, p = [], 0
    while p < len(b):
        n = struct.unpack_from(">i", b, p)[0]
        q = p + 4 + max(n, 0)
        if q > len(b):
            raise ValueError("a CQL value runs past its row")
        out.append(b[p:q])
        p = q
    return out


def cql_pair(table: str, values: bytes) -> bytes:
    """One map pair from a row's bound values: the key, then the UDT value with its fields in
    declaration order."""
    v = cql_values(values)
    key, f = v[0], v[1:]
    perm = CQL_DECLARED.get(table)
    if perm is not None:
        f = [f[i] for i in perm]
    udt = b"".join(f)
    return key + struct.pack(">i", len(udt)) + udt


def cql_column(pairs) -> bytes:
    """A map column's body from its pairs; None: a null column."""
    return b"" if pairs is None else struct.pack(">i", len(pairs)) + b"".join(pairs)


def cql_exec_columns(builder: int, values: bytes) -> tuple:
    """The execution row's four column bodies (EXEC_COLUMNS) from the values its update
    statement binds (cdr_encode_cql_async table 5): the UDT's 58 fields put into declaration
    order; a 2DC row's replication tail wrapped as a replication_state body (its trailing
    next_event_id column is the UDT's own); an NDC row's version_histories and encoding."""
    v = cql_values(values)
    f, tail = v[:58], v[58:]
    assert len(f) == 58 and len(tail) == {abi.BUILDER_2DC: 6, abi.BUILDER_NDC: 3}.get(builder, 1)
    execution = b"".join(f[i] for i in EXEC_DECLARED)
    if builder == abi.BUILDER_2DC:
        return execution, b"".join(tail[:5]), b"", b""
    if builder == abi.BUILDER_NDC:
        return execution, b"", tail[1][4:], tail[2][4:]
    return execution, b"", b"", b""


def pack_cql(n_entries: int, cols, exec_cols=None, cluster_seed=()) -> CqlCols:
    """cols[t][w] = entry w's column body of table t (b"": null).  The buffer is column-major:
    a table's columns lie one after another, so the rows a wavefront takes are one byte range.
    exec_cols[c][w] = entry w's body of the execution row's column c (EXEC_COLUMNS): the four
    columns follow the tables, laid out the same way."""
    chunks, pos, offs = [], 0, []
    for col in list(cols[:5]) + list(exec_cols or []):
        off = [pos]
        for w in range(n_entries):
            chunks.append(bytes(col[w]))
            pos += len(col[w])
            off.append(pos)
        offs.append(np.array(off, np.uint64))
    data = np.frombuffer(b"".join(chunks) or b"\0", np.uint8).copy()
    res = CqlCols(data[:pos], offs[:5], n_entries)
    if exec_cols is not None:
        assert len(exec_cols) == 4
        res.exec = CqlExec(offs[5:], list(cluster_seed))
    return res


def encode_state_cql(eng: engine.Engine, batch: engine.Batch, out: engine.Outputs, strings: list,
                     exec_rows: bool = False, persist=None, cluster_names=None) -> CqlCols:
    """The five pending tables of the OK entries of `out` as the Cassandra persistence returns
    them: the device encoder's values (cdr_encode_cql_async) with each row's fields put into
    declaration order, wrapped as map columns.  A row the encoder refuses is left out of its
    map; an entry without rows in a table gets a null column.  `.src[t]` names each pair's
    (entry, row of the entry).
    exec_rows=True adds the execution row's columns (cql_exec_columns of the encoder's table-5
    values; `persist` and `cluster_names` as in encode_state); an entry that is not OK, or whose
    row the encoder refuses, gets a one-byte execution body (it fails to load)."""
    cols, src = [], []
    for t in TABLES:
        got, codes = eng.encode_blobs(batch, out, t, strings, form="cql")
        per, s = [], []
        for w in range(batch.n_wfs):
            pairs = []
            if out.result[w].code == abi.OK:
                base = getattr(out.plan.caps[w], t + "_off")
                for j in range(len(out.rows(w, t))):
                    if base + j in got and codes[base + j] == 0:
                        pairs.append(cql_pair(t, got[base + j]))
                        s.append((w, j))
            per.append(cql_column(pairs or None))
        cols.append(per)
        src.append(s)
    xcols = None
    if exec_rows:
        names = list(cluster_names if cluster_names is not None else [])
        if persist is None:
            persist = (abi.CdrExecPersist * max(1, batch.n_wfs))()
        got, codes = eng.encode_blobs(batch, out, "exec", strings, persist, names, form="cql")
        xcols = [[], [], [], []]
        for w in range(batch.n_wfs):
            ok = out.result[w].code == abi.OK and w in got and codes[w] == 0
            four = cql_exec_columns(batch.wfs[w].builder, got[w]) if ok else (b"\0", b"", b"", b"")
            for c in range(4):
                xcols[c].append(four[c])
    res = pack_cql(batch.n_wfs, cols, xcols, cluster_names or ())
    res.src = src
    return res


def load_cql(eng: engine.Engine, cols: CqlCols, seeds: list, at_end: bool = False, check: bool = True,
             n_bytes: int = None) -> Loaded:
    """cdr_load_cql_rows on the device; host copies of every output, as `load` — with
    .n_rows and .entry_row0 (5 x uint32 [n_entries + 1]), the rows the device found.
    `n_bytes` overrides the buffer's length as the call is told it (offsets may lie past it)."""
    return _load_cql(eng, cols, seeds, at_end, check, n_bytes, False)


def load_cql_state(eng: engine.Engine, cols: CqlCols, seeds: list, at_end: bool = False, check: bool = True,
                   n_bytes: int = None, cluster_seed=None) -> Loaded:
    """cdr_load_cql_state on the device: as `load_cql`, with the execution rows of `cols.exec`
    decoded too, the outputs `load_state` has (cols.exec None: exec == NULL, cdr_load_cql_rows'
    results).  `cluster_seed` overrides cols.exec.cluster_seed."""
    return _load_cql(eng, cols, seeds, at_end, check, n_bytes, True, cluster_seed)


def _load_cql(eng, cols, seeds, at_end, check, n_bytes, state, cluster_seed=None) -> Loaded:
    L = abi.lib()
    dev = DeviceBuffers()
    try:
        sb, so = string_table(seeds)
        nb = len(cols.bytes) if n_bytes is None else n_bytes
        buf = cols.bytes[:nb]
        inp = abi.CdrCqlRowsIn()
        inp.bytes = dev.up(buf if len(buf) else np.zeros(1, np.uint8), at_end and len(buf) > 0)
        inp.n_bytes = nb
        for t in range(5):
            inp.col_off[t] = dev.up(cols.col_off[t])
        inp.seed_bytes, inp.seed_off = dev.up(sb), dev.up(so)
        inp.n_entries, inp.n_seeds = cols.n_entries, len(seeds)
        X = cols.exec if state else None
        if state:
            sout, xin = abi.CdrCqlStateOut(), None
            if X is not None:
                xin = abi.CdrCqlExecIn()
                xin.execution_off, xin.replication_state_off = dev.up(X.off[0]), dev.up(X.off[1])
                xin.version_histories_off, xin.vh_encoding_off = dev.up(X.off[2]), dev.up(X.off[3])
                cs = list(X.cluster_seed if cluster_seed is None else cluster_seed)
                xin.n_clusters = len(cs)
                for i, h in enumerate(cs[:abi.MAX_CLUSTERS]):
                    xin.cluster_seed[i] = h
            rc = L.cdr_load_cql_state(eng.ctx, C.byref(inp), C.byref(xin) if xin is not None else None, C.byref(sout),
                                      None)
            cout = sout.rows
        else:
            cout = abi.CdrCqlRowsOut()
            rc = L.cdr_load_cql_rows(eng.ctx, C.byref(inp), C.byref(cout), None)
        if rc:
            if check:
                raise RuntimeError(f"cdr_load_cql_{'state' if state else 'rows'} rc={rc}")
            return Loaded({}, None, None, abi.CdrTotals(), [], np.zeros(0, np.int32), [], None, None, b"", 0, rc=rc)
        out, ne = cout.rows, cols.n_entries
        n_rows = [int(n) for n in cout.n_rows]

        def recs(ptr, ty, n):
            raw = dev.down(ptr, np.uint8, n * C.sizeof(ty)).tobytes()
            return (ty * n).from_buffer_copy(raw) if n else (ty * 0)()
        tables = {t: recs(getattr(out.state, t), engine.TABLE_TYPES[t], n_rows[i]) for i, t in enumerate(TABLES)}
        result = recs(out.state.result, abi.CdrWfResult, ne)
        caps = recs(out.caps, abi.CdrWfCaps, ne)
        status = [dev.down(out.row_status[t], np.int32, n_rows[t]) for t in range(5)]
        est = dev.down(out.entry_status, np.int32, ne)
        ref = dev.down(out.str_ref, np.uint64, out.n_strings)
        ln = dev.down(out.str_len, np.uint32, out.n_strings)
        gen = dev.down(out.gen_bytes, np.uint8, out.n_gen_bytes).tobytes()
        raw, sraw = buf.tobytes(), sb.tobytes()
        strings = []
        for h in range(out.n_strings):
            r, n = int(ref[h]), int(ln[h])
            s = sraw if r & abi.STR_REF_SEED else gen if r & abi.STR_REF_GEN else raw
            r &= abi.STR_REF_GEN - 1
            strings.append(s[r:r + n])
        res = Loaded(tables, result, caps, out.totals, status, est, strings, ref, ln, gen, out.n_bad_entries)
        res.n_rows = n_rows
        res.entry_row0 = [dev.down(cout.entry_row0[t], np.uint32, ne + 1) if ne else np.zeros(1, np.uint32)
                          for t in range(5)]
        if X is not None:
            for t in ("vh", "rp", "sa"):
                tables[t] = recs(getattr(out.state, t), engine.TABLE_TYPES[t], getattr(out.totals, t))
            res.exec = recs(out.state.exec, abi.CdrExecInfo, ne)
            res.repl = recs(out.state.repl, abi.CdrReplState, ne)
            res.persist = recs(sout.persist, abi.CdrExecPersist, ne)
            res.builder = dev.down(sout.builder, np.uint32, ne)
            res.exec_status = dev.down(sout.exec_status, np.int32, ne)
        return res
    finally:
        dev.free()
