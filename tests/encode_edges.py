"""The hand-made batch of tests/test_encode_edges.py: encoder inputs no replay produces.

A hand-written string table (every length class up to one string past 64 KiB, every byte
value, valid and broken UUID texts, Memo and list<string> bodies), and N_ENTRIES entries
whose records take the edge values of every field.  Layout of the entries:

  * every seventh entry (w % 7 == 6) failed (code != CDR_OK) with nonzero counts and rows
    full of out-of-range handles: the encoders must give it zero-length rows / untouched slots;
  * entries below the tail are clean: every row encodes with status 0 in both forms, so the
    row offsets up to the tail follow from the oracle's sizes alone;
  * each OK entry of the tail carries one failure case per table: a clean row with exactly
    one field overridden (a handle == n or 0xFFFFFFFF, a broken UUID text, a broken Memo
    body, handle 0 where a CQL uuid column reads it).  Never two in one row: cdr.h defines no
    precedence between two failures.

The entry count follows from the cases: 81 execution-row cases, one per entry, and at most
15 % of a table's rows may be compared by status alone.
"""
import functools
import struct
import zlib

from cadence_amd import abi, engine
from oracle import cql_values as cq
from oracle import thrift_binary as tb
from tests.states import make_state

N_ENTRIES = 745  # 11 * 64 + 41 = 2 * 256 + 233
FILL = 0xA5
BAD_CODE = 4  # E_INVALID_STATE_TRANSITION
I64_MIN, I64_MAX, I32_MIN, I32_MAX = -2**63, 2**63 - 1, -2**31, 2**31 - 1
V64 = (0, 1, -1, 2**31 - 1, 2**31, 2**32, 2**53 + 1, -23, I64_MIN, I64_MAX, abi.ZERO_TIME_NANOS,
       -999_999, -1_000_000, -1_000_001, 999_999, 1_000_000)
V32 = (0, 1, -1, I32_MAX, I32_MIN)
U64S = (0, 2**64 - 1, 0x0123456789ABCDEF, 0xFEDCBA9876543210) + tuple(0xF << (4 * i) for i in range(16))
DBL_BITS = (0x0000000000000000, 0x8000000000000000, 0x3FF0000000000000, 0x4004000000000000, 0x0000000000000001,
            0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000001)
PLAIN_LENS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 35, 36, 37, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097,
              70001)
ROW_COUNTS = {0: 1000, 1: 0, 2: 63, 3: 0, 4: 64, 5: 65, 8: 1, 9: 0, 10: 1000, 11: 0}
TABLE_ID = {"act": 0, "timer": 1, "child": 2, "cancel": 3, "signal": 4, "exec": 5}

# handle fields by kind: plain bytes, UUID text (a uuid column / MustParseUUID reads it in at
# least one form), Memo struct body, list<string> body
PLAIN = {"act": ("activity_id", "request_id", "task_list"), "timer": ("timer_id",),
         "child": ("started_workflow_id", "domain_name", "workflow_type"), "cancel": (),
         "signal": ("signal_name", "input", "control"), "rp": ("binary_checksum", "run_id"), "sa": ("key", "value"),
         "exec": ("workflow_id", "parent_workflow_id", "task_list", "workflow_type", "cron_schedule", "branch_tree_id",
                  "decision_request_id"),
         "persist": ("execution_context", "sticky_task_list", "client_library_version", "client_feature_version",
                     "client_impl")}
UUIDS = {"child": ("started_run_id",),
         "exec": ("domain_id", "run_id", "create_request_id", "parent_domain_id", "parent_run_id")}
# "" is a value of its own there (nil run ID / no parent); a "" parent run ID under a parent
# is nil in the SQL form and no UUID in the CQL form: a tail case, not a clean row
MAY_BE_EMPTY = ("started_run_id", "parent_domain_id")
LISTS = {"act": ("nonretriable",), "exec": ("nonretriable",)}
MEMOS = {"exec": ("memo",)}


def pick(tag: str, k: int, n: int) -> int:
    """A fixed pseudo-random choice in [0, n): flag words and pools, uncorrelated with the
    cyclic value lists."""
    return zlib.crc32(f"{tag}/{k}".encode()) % n


def plain_bytes(n: int, k: int) -> bytes:
    return bytes((i * (2 * k + 1) + 13 * k) & 0xFF for i in range(n))


def memo_body(n_entries: int) -> bytes:
    ents = b"".join(struct.pack(">i", 2) + f"k{i}".encode() + struct.pack(">i", 3 + 70 * i) + plain_bytes(3 + 70 * i, i)
                    for i in range(n_entries))
    return tb.field(tb.T_MAP, 10, struct.pack(">bbi", tb.T_STRING, tb.T_STRING, n_entries) + ents) + b"\x00"


def list_body(n_elems: int) -> bytes:
    elems = [plain_bytes(5 + 11 * i, 40 + i) for i in range(n_elems)]
    return struct.pack(">bi", tb.T_STRING, len(elems)) + b"".join(struct.pack(">i", len(e)) + e for e in elems)


class Strings:
    """The hand-written handle table and the pools the rows draw from."""

    def __init__(self):
        self.strs = [b""]
        self.plain = {0: 0}
        for k, n in enumerate(PLAIN_LENS):
            self.plain[n] = self.add(plain_bytes(n, k))
        self.small = [h for n, h in self.plain.items() if n <= 257]
        self.big = [h for n, h in self.plain.items() if n > 257]
        u = "0123abcd-89ef-4c5d-8a7b-fedcba987654"
        mixed = "".join(c.upper() if i % 2 else c for i, c in enumerate(u))
        self.uuid_ok = [self.add(s.encode()) for s in (u, u.upper(), u.replace("-", ""), mixed)]
        self.uuid_bad = {
            "dash+1": self.add((u[:8] + u[9] + "-" + u[10:]).encode()),     # after an odd digit count: both parsers fail
            "dash+2": self.add((u[:8] + u[9:11] + "-" + u[11:]).encode()),  # after an even count: gocql skips it
            "nonhex": self.add((u[:20] + "g" + u[21:]).encode()),
            "len35": self.add(u[:-1].encode()),
            "len37": self.add((u + "0").encode()),
        }
        assert all(len(self.strs[h]) == 36 for k, h in self.uuid_bad.items() if k in ("dash+1", "dash+2", "nonhex"))
        m1 = memo_body(1)
        self.memo_ok = [self.add(memo_body(0)), self.add(m1), self.add(memo_body(3)), self.add(b"\x00")]
        self.memo_bad = {
            "empty": self.add(b""),  # a nonzero handle of no bytes
            "cut header": self.add(m1[:2]),
            "count 2, 1 entry": self.add(m1[:5] + struct.pack(">i", 2) + m1[9:-1]),  # ends with the entry
            "count 2, 1 entry, stop": self.add(m1[:5] + struct.pack(">i", 2) + m1[9:]),
            "length past the end": self.add(m1[:15] + struct.pack(">i", 4000) + m1[19:]),
            "length 0xFFFFFFFF": self.add(m1[:9] + b"\xff\xff\xff\xff" + m1[13:]),
        }
        self.lists = [self.add(list_body(n)) for n in (0, 1, 3)]
        self.cluster_names = [self.plain[5], self.plain[1], self.plain[17]]
        self.n = len(self.strs)
        self.S = tb.lookup(self.strs)

    def add(self, s: bytes) -> int:
        self.strs.append(s)
        return len(self.strs) - 1

    def bad_handles(self):
        return (self.n, 0xFFFFFFFF)


def set_double(rec, name: str, bits: int):
    """A copy of `rec` with the double field `name` set by bit pattern."""
    raw = bytearray(bytes(rec))
    o = getattr(type(rec), name).offset
    raw[o:o + 8] = struct.pack("<Q", bits)
    return type(rec).from_buffer_copy(bytes(raw))


def fill_scalars(rec, k: int, skip=()):
    """Every int64 / int32 / uint64 field of `rec` from the edge-value lists, field fi of row
    k taking value (k + 3 * fi) of its list, so that every field takes every value."""
    for fi, (name, ty) in enumerate(rec._fields_):
        if name.startswith("_pad") or name in skip or name == "flags":
            continue
        if ty is abi.i64:
            setattr(rec, name, V64[(k + 3 * fi) % len(V64)])
        elif ty is abi.i32:
            setattr(rec, name, V32[(k + 3 * fi) % len(V32)])
        elif ty is abi.u64:
            setattr(rec, name, U64S[(k + 3 * fi) % len(U64S)])


def _handles(kind: str):
    return PLAIN.get(kind, ()) + UUIDS.get(kind, ()) + LISTS.get(kind, ()) + MEMOS.get(kind, ())


def fill_handles(rec, kind: str, k: int, T: Strings):
    """Valid handles of every length class: plain fields from the strings up to 257 bytes
    (every 14th or 70th row: one field takes a long string instead), UUID fields from the
    valid texts (and "" where that is a value), Memo / list fields from their bodies or 0."""
    names = PLAIN.get(kind, ())
    for name in names:
        setattr(rec, name, T.small[pick(f"{kind}.{name}", k, len(T.small))])
    # one thread writes an entry's rows byte by byte: long strings are kept rare in the
    # tables with 1000-row entries (both periods are multiples of 7: never a failed entry)
    period = 14 if kind in ("exec", "persist") else 70
    if names and k % period == 0:
        m = k // period
        setattr(rec, names[m % len(names)], T.big[(m // len(names)) % len(T.big)])
    for name in UUIDS.get(kind, ()):
        pool = T.uuid_ok + ([0] if name in MAY_BE_EMPTY else [])
        setattr(rec, name, pool[pick(f"{kind}.{name}", k, len(pool))])
    for name in LISTS.get(kind, ()):
        pool = T.lists + [0]
        setattr(rec, name, pool[pick(f"{kind}.{name}", k, len(pool))])
    for name in MEMOS.get(kind, ()):
        pool = T.memo_ok + [0]
        setattr(rec, name, pool[pick(f"{kind}.{name}", k, len(pool))])


def clean_row(kind: str, k: int, T: Strings):
    """Row k of a pending table, rp, sa or vh: edge values everywhere, valid handles."""
    rec = engine.TABLE_TYPES[kind]()
    fill_scalars(rec, k, skip=_handles(kind))
    fill_handles(rec, kind, k, T)
    if kind == "act":
        rec.flags = pick("act.flags", k, 8)
        rec = set_double(rec, "backoff_coefficient", DBL_BITS[k % len(DBL_BITS)])
    if kind == "rp":
        rec.flags = pick("rp.flags", k, 128)
    return rec


def bad_row(kind: str, k: int, T: Strings):
    """A row of a failed entry: every handle out of range."""
    rec = clean_row(kind, k, T)
    for i, name in enumerate(_handles(kind)):
        setattr(rec, name, T.bad_handles()[(k + i) % 2])
    if kind == "rp":
        rec.flags = 0x7F
    return rec


def clean_exec(w: int, T: Strings):
    """(cdr_exec_info, cdr_exec_persist, cdr_repl_state) of entry w."""
    x = abi.CdrExecInfo()
    fill_scalars(x, w, skip=_handles("exec") + ("reset_points_len", "search_attr_len"))
    fill_handles(x, "exec", w, T)
    x.flags = pick("exec.flags", w, 0x200)
    x = set_double(x, "backoff_coefficient", DBL_BITS[w % len(DBL_BITS)])
    ps = abi.CdrExecPersist()
    fill_scalars(ps, w + 5, skip=PLAIN["persist"])
    fill_handles(ps, "persist", w, T)
    # an int32 in the reference's ExecutionInfo (StickyScheduleToStartTimeout), widened by the SQL blob
    ps.sticky_s2s_timeout = V32[w % len(V32)]
    rs = abi.CdrReplState()
    fill_scalars(rs, w + 9)
    for i in range(abi.MAX_CLUSTERS):
        rs.lri_version[i] = V64[(w + i) % len(V64)]
        rs.lri_last_event_id[i] = V64[(w + 5 * i + 2) % len(V64)]
    rs.lri_mask = (0, 0b001, 0b101, 0b111)[pick("lri", w, 4)]  # bits at or above n_clusters stay clear
    return x, ps, rs


# ---------------------------------------------------------------- the failure cases
def pending_cases(T: Strings) -> dict:
    """{table: [(field, handle)]}: the one field a tail row overrides."""
    cases = {t: [] for t in ("act", "timer", "child", "cancel", "signal")}
    for t in cases:
        for name in _handles(t):
            cases[t] += [(name, h) for h in T.bad_handles()]
    cases["child"] += [("started_run_id", h) for h in T.uuid_bad.values()]
    return cases


def exec_cases(T: Strings) -> list:
    """[(where, field, handle)] with where in exec / persist / rp / sa."""
    cases = []
    for where in ("exec", "persist", "rp", "sa"):
        for name in _handles(where):
            cases += [(where, name, h) for h in T.bad_handles()]
    for name in UUIDS["exec"]:
        cases += [("exec", name, h) for h in T.uuid_bad.values()]
    # "" where a CQL uuid column reads the string
    cases += [("exec", name, 0) for name in ("domain_id", "run_id", "create_request_id", "parent_run_id")]
    cases += [("exec", "memo", h) for h in T.memo_bad.values()]
    return cases


class HandMade:
    pass


@functools.lru_cache(maxsize=None)
def hand_made() -> HandMade:
    """The batch (built once per session; nothing modifies it)."""
    T = Strings()
    n = N_ENTRIES
    pc, xc = pending_cases(T), exec_cases(T)
    n_tail = max([len(xc)] + [len(v) for v in pc.values()])
    oks = [w for w in range(n) if w % 7 != 6]
    tail = oks[-n_tail:]  # the last n_tail OK entries: case i in tail[i]
    hm = HandMade()
    hm.T, hm.first_tail, hm.tail = T, tail[0], tail
    hm.failed = [w for w in range(n) if w % 7 == 6]
    hm.case_of = {}  # (table, row) / ("exec", w) -> the overridden (field, handle)
    counter = {t: 0 for t in engine.TABLES}
    per_entry, execs = [], []

    def rows(kind, cnt, make):
        out = []
        for _ in range(cnt):
            out.append(make(kind, counter[kind], T))
            counter[kind] += 1
        return out
    for w in range(n):
        failed = w % 7 == 6
        make = bad_row if failed else clean_row
        cnt = 3 if failed else ROW_COUNTS.get(w, (w * 5 + 1) % 4)
        tabs = {t: rows(t, cnt, make) for t in ("act", "timer", "child", "cancel", "signal")}
        tabs["vh"] = rows("vh", 3 if failed else (0, 1, 40)[pick("n_vh", w, 3)], make)
        tabs["rp"] = rows("rp", 3 if failed else (0, 1, 20)[pick("n_rp", w, 3)], make)
        tabs["sa"] = rows("sa", 3 if failed else (0, 5, 2)[pick("n_sa", w, 3)], make)
        x, ps, rs = clean_exec(w, T)
        if failed:
            for i, name in enumerate(_handles("exec")):
                setattr(x, name, T.bad_handles()[i % 2])
            x.flags = 0x1FF
        if w in tail:
            i = tail.index(w)
            for t, cases in pc.items():
                if i < len(cases):
                    name, h = cases[i]
                    r = clean_row(t, counter[t], T)
                    counter[t] += 1
                    setattr(r, name, h)
                    tabs[t].append(r)
                    hm.case_of[(t, w, len(tabs[t]) - 1)] = (name, h)
            if i < len(xc):
                where, name, h = xc[i]
                # the entry reads the field in both forms: a parent, every optional part
                # present, a branch token, one reset point with both strings, one attribute
                x.flags |= 0x008 | 0x010 | 0x020 | 0x040 | 0x100
                x.parent_domain_id = x.parent_run_id = T.uuid_ok[i % 4]
                x.memo = T.memo_ok[1]
                if not tabs["rp"]:
                    tabs["rp"] = rows("rp", 1, clean_row)
                tabs["rp"][0].flags |= 0x03
                if not tabs["sa"]:
                    tabs["sa"] = rows("sa", 1, clean_row)
                setattr({"exec": x, "persist": ps, "rp": tabs["rp"][0], "sa": tabs["sa"][0]}[where], name, h)
                hm.case_of[("exec", w)] = (where, name, h)
        per_entry.append(tabs)
        execs.append((x, ps, rs))
    batch, out = make_state(per_entry, lambda w: (w + 1) % 4, tables=engine.TABLES)
    persist = (abi.CdrExecPersist * n)()
    for w, (x, ps, rs) in enumerate(execs):
        batch.wfs[w].builder = w % 3
        out.exec[w], out.repl[w], persist[w] = x, rs, ps
        if w % 7 == 6:
            out.result[w].code = BAD_CODE
    hm.batch, hm.out, hm.persist, hm.n_cases = batch, out, persist, {**{t: len(v) for t, v in pc.items()},
                                                                     "exec": len(xc)}
    return hm


# ---------------------------------------------------------------- expected bytes and statuses
def expect(fn):
    """(bytes, 0) or (None, status): the oracle's failure classes, nothing else caught."""
    try:
        return fn(), 0
    except (tb.BadUUID, cq.BadUUID):
        return None, 1
    except tb.BadHandle:
        return None, 2
    except tb.BadMemo:
        return None, 3


SQL_ROW = {"act": tb.activity_info_blob, "child": tb.child_info_blob, "signal": tb.signal_info_blob,
           "timer": lambda r, S: tb.timer_info_blob(r), "cancel": lambda r, S: tb.request_cancel_info_blob(r)}
CQL_ROW = {"act": cq.activity, "timer": cq.timer, "child": cq.child, "cancel": cq.cancel, "signal": cq.signal}


def expected_rows(batch, out, table: str, form: str, S, persist=None, cluster_names=()) -> dict:
    """{capacity row: (bytes or None, status)} for the rows of OK entries (exec: row = entry)."""
    want = {}
    for w in range(batch.n_wfs):
        if out.result[w].code != abi.OK:
            continue
        if table == "exec":
            mk = cq.execution if form == "cql" else tb.exec_info_blob
            want[w] = expect(lambda: mk(
                out.exec[w], batch.wfs[w].builder, S, persist[w], repl=out.repl[w],
                vh_items=[(v.event_id, v.version) for v in out.rows(w, "vh")],
                rps=[(p, S) for p in out.rows(w, "rp")], sa=[(kv.key, kv.value) for kv in out.rows(w, "sa")],
                cluster_names=cluster_names))
            continue
        mk = (CQL_ROW if form == "cql" else SQL_ROW)[table]
        base = getattr(out.plan.caps[w], table + "_off")
        for j, row in enumerate(out.rows(w, table)):
            want[base + j] = expect(lambda: mk(row, S))
    return want


@functools.lru_cache(maxsize=None)
def expected(table: str, form: str) -> dict:
    hm = hand_made()
    return expected_rows(hm.batch, hm.out, table, form, hm.T.S, hm.persist, hm.T.cluster_names)


def n_capacity_rows(batch, out, table: str) -> int:
    return batch.n_wfs if table == "exec" else max(1, getattr(out.plan.totals, table))


def oracle_offsets(want: dict, n_rows: int):
    """(row_off[0 .. first], first): the offsets the oracle's sizes give up to the first row
    it has no size for (a row with a status != 0), or all n_rows + 1 of them."""
    off, first = [0], n_rows
    for r in range(n_rows):
        blob, code = want.get(r, (b"", 0))
        if code:
            first = r
            break
        off.append(off[-1] + len(blob))
    return off, first
