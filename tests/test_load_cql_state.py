"""Loading whole stored states from the Cassandra execution row on the device (cdr.h
cdr_load_cql_state, csrc/load.hip), checked against tests/cql_exec_ref.py.

CPU: the reference reader inverts oracle/cql_values.execution on replayed states of the
synthetic configs 2-5 under all three builders.  The decoded records are the states' own with
exactly these differences: every timestamp is FLOORED to the millisecond (a CQL timestamp holds
milliseconds), CDR_XI_HAS_SEARCH_ATTR / _HAS_MEMO are clear where the map is empty (Cassandra
stores an empty map as null), and last_event_task_id is kept (the SQL form gives 0); what no
stored row carries is at the loader's value as in tests/test_load_state.py, and start / current
version come back from the replication state.  The name-derived permutation equals the
schema's field names (tests/golden/cql_workflow_execution_fields.json), every wire edge of the
contract gives the stated status and precedence on hand-built bytes, and the ABI mirrors match.
GPU (-m gpu): the device == the reference record for record, status for status and handle for
handle on those states, on every entry count around the wavefront and workgroup, on every wire
edge, truncation, buffer end and staging size; the SQL and Cassandra forms of one state load
alike; the loaded state alone carries a replay to the oracle's whole replay.
"""
import ctypes as C
import functools
import json
import os
import re
import struct

import numpy as np
import pytest

from cadence_amd import abi, engine, rows
from oracle import cql_values as cv
from oracle import thrift_decode as TD
from tests import cql_exec_ref as cx
from tests import cql_rows_ref as ref
from tests.rows_ref import UUID_TEXT, RowError
from tests.test_load_cql import base as pending_base
from tests.test_load_cql import i4, lst, pair, q
from tests.test_load_state import CLUSTERS, _as_written, _histories, _points, _sa_rows, _token
from tests.test_load_state import _state as _builder_state

ZT = abi.ZERO_TIME_NANOS
TRUNCATED, BAD_SIZE = TD.DEC_TRUNCATED, TD.DEC_BAD_SIZE
E_SIZE, E_SHAPE, E_CLUSTER, E_ENCODING = abi.LOAD_E_CQL_SIZE, abi.LOAD_E_SHAPE, abi.LOAD_E_CLUSTER, abi.LOAD_E_ENCODING
ITEMS = ("vh", "rp", "sa")
SEEDS = [b""] + CLUSTERS + [b"tl-0", b"no such string"]
CSEED = [1, 2, 3]
MS = 1_000_000
STAGE, BLOCK = 24576, 128  # CDR_LOAD_STAGE, CDR_LOAD_BLOCK (csrc/load.hip)


def _copy(rec):
    return type(rec).from_buffer_copy(bytes(rec))


# ---------------------------------------------------------------- replayed states
@functools.lru_cache(maxsize=None)
def _state(cfg, builder):
    """tests/test_load_state._state with what the Cassandra writer needs: the create request
    IDs are UUID texts (a uuid column), and a 2DC entry's persistence context holds its
    replication state's versions (the Cassandra row has no others)."""
    b, out, strs, persist, names = _builder_state(cfg, builder)
    strs = list(strs)
    persist = (abi.CdrExecPersist * b.n_wfs)(*[_copy(p) for p in persist])
    ok = [w for w in range(b.n_wfs) if out.result[w].code == abi.OK]
    bodies = {out.exec[w].memo for w in ok} | {out.exec[w].nonretriable for w in ok}
    bodies |= {r.nonretriable for w in ok for r in out.rows(w, "act")}
    for w in ok:
        h = out.exec[w].create_request_id
        if h and h not in bodies and not UUID_TEXT.fullmatch(strs[h]):
            strs[h] = b"c0de%04x-0000-4000-8000-%012x" % (h & 0xFFFF, h)
        two_dc = b.wfs[w].builder == abi.BUILDER_2DC
        persist[w].start_version = out.repl[w].start_version if two_dc else 0
        persist[w].current_version = out.repl[w].current_version if two_dc else 0
    assert len(set(strs)) == len(strs)
    return b, out, strs, persist, names


def _storable(b, out, strs, w):
    """Entry w is OK and the Cassandra writer takes it (its IDs are UUIDs)."""
    if out.result[w].code != abi.OK:
        return False
    x = out.exec[w]
    return all(UUID_TEXT.fullmatch(strs[getattr(x, f)]) for f in ("domain_id", "run_id", "create_request_id"))


def _as_stored(b, out, persist, w):
    """(exec, repl, persist) records of entry w as a Cassandra load gives them back:
    tests/test_load_state._as_written with the three differences of this form."""
    x, repl = _as_written(b, out, persist, w)
    x.last_event_task_id = out.exec[w].last_event_task_id
    x.expiration_time = x.expiration_time // MS * MS
    if not out.rows(w, "sa"):
        x.flags &= ~abi.XI_HAS_SEARCH_ATTR
    ps = _copy(persist[w])
    for f in ("start_time", "last_updated_time"):
        if getattr(ps, f) != ZT:
            setattr(ps, f, getattr(ps, f) // MS * MS)
    return x, repl, ps


def _check_against_state(b, out, strs, persist, get):
    """get(w) -> (exec, repl, persist, builder, vh, rp, sa) record bytes of a decode."""
    n = 0
    for w in range(b.n_wfs):
        if not _storable(b, out, strs, w):
            continue
        x, repl, ps = _as_stored(b, out, persist, w)
        gx, gr, gp, gb, gvh, grp, gsa = get(w)
        assert gx == bytes(x), (w, [f for f, *_ in abi.CdrExecInfo._fields_
                                    if getattr(abi.CdrExecInfo.from_buffer_copy(gx), f) != getattr(x, f)])
        assert gr == bytes(repl) and gb == b.wfs[w].builder, w
        assert gp == bytes(ps), (w, [f for f, *_ in abi.CdrExecPersist._fields_
                                     if getattr(abi.CdrExecPersist.from_buffer_copy(gp), f) != getattr(ps, f)])
        assert gvh == [bytes(r) for r in out.rows(w, "vh")] and grp == [bytes(r) for r in out.rows(w, "rp")], w
        assert gsa == [bytes(abi.CdrKV(key=k, value=v)) for k, v in _sa_rows(out, w)], w
        n += 1
    return n


# ---------------------------------------------------------------- hand-built rows
def cmap(pairs) -> bytes:
    """A map<text, blob> value."""
    return i4(len(pairs)) + b"".join(cv.val(k) + cv.val(v) for k, v in pairs)


def xvals(kind="local", v=0, n_rp=2, sa=((b"k1", b"v1"), (b"k2", b"v2")), mp=((b"mk", b"mv"),), **over) -> dict:
    """The execution UDT with every declared field set (values vary with v), by field name."""
    d = {
        "domain_id": bytes(range(v, 16 + v)), "workflow_id": b"workflow-%d" % v, "run_id": bytes(range(200 + v, 216 + v)),
        "parent_domain_id": bytes(range(16 + v, 32 + v)), "parent_workflow_id": b"parent-wf-%d" % v,
        "parent_run_id": bytes(range(64 + v, 80 + v)), "initiated_id": q(33 + v), "completion_event_batch_id": q(90 + v),
        "completion_event": b"completion-event", "completion_event_data_encoding": b"thriftrw", "task_list": b"tl-%d" % v,
        "workflow_type_name": b"type-%d" % v, "workflow_timeout": i4(3600 + v), "decision_task_timeout": i4(10 + v),
        "execution_context": b"context-%d" % v, "state": i4(1 + v), "close_status": i4(v), "last_processed_event": q(80 + v),
        "start_time": q(1_600_000_000_000 + v), "last_updated_time": q(1_600_000_000_009 + v),
        "create_request_id": bytes(range(128 + v, 144 + v)), "decision_version": q(6 + v), "decision_schedule_id": q(91 + v),
        "decision_started_id": q(92 + v), "decision_request_id": b"decision-req-%d" % v, "decision_timeout": i4(15 + v),
        "decision_attempt": q(2 + v), "decision_timestamp": q(10**18 + 3), "decision_scheduled_timestamp": q(10**18 + 2),
        "decision_original_scheduled_timestamp": q(10**18 + 1), "cancel_requested": b"\x01" if v == 0 else b"\x00",
        "cancel_request_id": b"cancel-req", "sticky_task_list": b"sticky-%d" % v,
        "sticky_schedule_to_start_timeout": i4(25 + v), "client_library_version": b"lib-%d" % v,
        "client_feature_version": b"feat-%d" % v, "client_impl": b"impl-%d" % v, "attempt": i4(3 + v),
        "has_retry_policy": b"\x01", "init_interval": i4(1 + v), "backoff_coefficient": struct.pack(">d", 1.5 + v),
        "max_interval": i4(60 + v), "expiration_time": q(2_000_000_000_000 + v), "max_attempts": i4(4 + v),
        "non_retriable_errors": lst([b"bad", b"e%d" % v]), "event_store_version": i4(-1), "signal_count": i4(-2 - v),
        "branch_token": _token(b"tree-%d" % v) if kind != "ndc" else None, "history_size": q(5000 + v),
        "last_first_event_id": q(88 + v), "next_event_id": q(101 + v), "cron_schedule": b"* * * * %d" % v,
        "expiration_seconds": i4(600 + v), "last_event_task_id": q(777 + v), "auto_reset_points": _points(n_rp, v),
        "auto_reset_points_encoding": b"thriftrw", "search_attributes": None if sa is None else cmap(sa),
        "memo": None if mp is None else cmap(mp)}
    assert list(d) == cx.NAMES and set(over) <= set(d), set(over) - set(d)
    d.update(over)
    return d


def xbody(d) -> bytes:
    return cx.body([d[n] for n in cx.NAMES])


def lri_map(pairs) -> bytes:
    return i4(len(pairs)) + b"".join(cv.val(k) + cv.val(cx.body([q(ver), q(ev)])) for k, ver, ev in pairs)


def rs_body(v=0, lri=None) -> bytes:
    lri = [(CLUSTERS[0], 3 + v, 30), (CLUSTERS[2], 4 + v, 40)] if lri is None else lri
    return cx.body([q(7 + v), q(5 + v), q(55 + v), q(41 + v), lri_map(lri)])


def four(kind="local", v=0, n_items=3, rs=None, vh=None, enc=None, **kw) -> tuple:
    """The four column bodies of a hand-built row of builder `kind`."""
    d = xvals(kind, v, **kw)
    rs = (rs_body(v) if kind == "2dc" else b"") if rs is None else rs
    vh = (_histories(n_items=n_items, v=v) if kind == "ndc" else b"") if vh is None else vh
    enc = (b"thriftrw" if kind == "ndc" else b"") if enc is None else enc
    return xbody(d), rs, vh, enc


def raw_at(d, name, enc) -> bytes:
    """The execution body with field `name`'s whole [bytes] replaced by the raw bytes `enc`."""
    return b"".join(enc if n == name else cv.val(d[n]) for n in cx.NAMES)


def entries(fours, pending=None, seed=CSEED) -> rows.CqlCols:
    """One entry per (execution, replication_state, version_histories, encoding); null pending
    columns unless given (pending[t][w] = a column body)."""
    n = len(fours)
    cols = pending or [[b""] * n for _ in range(5)]
    return rows.pack_cql(n, cols, [[f[c] for f in fours] for c in range(4)], seed)


def _one(f):
    return cx.parse_exec(*f, CLUSTERS)


def _outcome(f):
    """What a row decodes to, as something to compare: its status, or its records and strings."""
    try:
        p = _one(f)
    except (TD.DecodeError, RowError) as e:
        return e.code
    return (bytes(p.x), p.xs, bytes(p.ps), p.pss, bytes(p.repl), p.builder, p.vh, p.sa, [(bytes(r), c, u) for r, c, u in p.rps])


def _status(want):
    """The status a wire case expects (a case may expect what another failing row gives)."""
    if isinstance(want, int):
        return want
    o = _outcome(want)
    return o if isinstance(o, int) else 0


@functools.lru_cache(maxsize=None)
def wire_cases():
    """[(name, four columns, expected)]: expected is a status, or the four columns whose decode
    the edge's must equal."""
    cases = []
    for kind in ("local", "2dc", "ndc"):
        plain = four(kind)
        cases.append((f"{kind} plain", plain, plain))
        cases.append((f"{kind} extra trailing fields", (plain[0] + cv.val(b"later") + cv.val(None) + cv.val(q(1)),) + plain[1:], plain))
        cases.append((f"{kind} trailing bytes that are no value", (plain[0] + b"\xff\xff",) + plain[1:], plain))
    d = xvals()
    plain = four()
    types = dict(cx.FIELDS)
    # every field: null, zero-length, bad lengths, wrong sizes
    for i, name in enumerate(cx.NAMES):
        null, empty = four(**{name: None}), four(**{name: b""})
        cases += [(f"{name} null", null, null), (f"{name} zero-length", empty, null)]
        cases.append((f"{name} length -2", (raw_at(d, name, i4(-2)),) + plain[1:], BAD_SIZE))
        cases.append((f"{name} length past the UDT", (raw_at(d, name, i4(1 << 20) + b"ab"),) + plain[1:], TRUNCATED))
        size = ref.SIZE.get(types[name])
        if size:
            for m in (size - 1, size + 1):
                if m:
                    cases.append((f"{name} of {m} bytes", four(**{name: bytes(m)}), E_SIZE))
        cut = cx.body([d[n] for n in cx.NAMES[:i]])  # fewer fields: the rest null
        cases.append((f"cut before {name}", (cut,) + plain[1:], four(**{n: None for n in cx.NAMES[i:]})))
        cases.append((f"cut in the length of {name}", (cut + b"\0\0",) + plain[1:], TRUNCATED))
    cases.append(("every field absent", (b"", b"", b"", b""), four(**{n: None for n in cx.NAMES})))
    # timestamps
    for name in ("start_time", "last_updated_time", "expiration_time"):
        for ms, want in ((ref.MS_MAX, None), (-ref.MS_MAX, None), (ref.MS_MAX + 1, E_SHAPE), (-ref.MS_MAX - 1, E_SHAPE), (-2**63, E_SHAPE)):
            f = four(**{name: q(ms)})
            cases.append((f"{name} {ms}", f, f if want is None else want))
    # parents
    for name, sentinel, other in (("parent_domain_id", cx.EMPTY_DOMAIN_ID, cx.EMPTY_RUN_ID),
                                  ("parent_run_id", cx.EMPTY_RUN_ID, cx.EMPTY_DOMAIN_ID)):
        cases.append((f"{name} sentinel", four(**{name: sentinel}), four(**{name: None})))
        cases.append((f"{name} zero", four(**{name: bytes(16)}), four(**{name: None})))
        cases.append((f"{name} the other sentinel", four(**{name: other}), four(**{name: other})))
        cases.append((f"{name} sentinel + 1", four(**{name: sentinel[:-1] + b"\x01"}), four(**{name: sentinel[:-1] + b"\x01"})))
    cases.append(("no parent: emptyInitiatedID", four(parent_domain_id=cx.EMPTY_DOMAIN_ID, initiated_id=q(-7)),
                  four(parent_domain_id=None, initiated_id=q(abi.EMPTY_EVENT_ID))))
    cases.append(("a parent: -7 stays", four(initiated_id=q(-7)), four(initiated_id=q(-7))))
    # branch token
    cases.append(("empty branch_token", four(branch_token=b""), four(branch_token=None)))
    cases.append(("branch_token without preamble", four(branch_token=_token()[1:]), E_ENCODING))
    cases.append(("branch_token truncated inside", four(branch_token=_token()[:-2]), TRUNCATED))
    cases.append(("BranchID uppercase", four(branch_token=_token(bid=b"0123ABCD-89ef-4c5d-8a7b-fedcba987654")), abi.LOAD_E_UUID))
    cases.append(("branch_token and a version-history token", four("ndc", branch_token=_token()), E_SHAPE))
    # reset points
    cases.append(("empty reset points, json", four(auto_reset_points=b"", auto_reset_points_encoding=b"json"),
                  four(auto_reset_points=None, auto_reset_points_encoding=b"json")))
    cases.append(("reset points, json", four(auto_reset_points_encoding=b"json"), E_ENCODING))
    cases.append(("reset points, null encoding", four(auto_reset_points_encoding=None), E_ENCODING))
    cases.append(("reset points at the bound", four(n_rp=abi.LOAD_MAX_RESET_POINTS), four(n_rp=abi.LOAD_MAX_RESET_POINTS)))
    cases.append(("reset points over the bound", four(n_rp=abi.LOAD_MAX_RESET_POINTS + 1), E_SHAPE))
    # the two maps
    M = abi.LOAD_MAX_SEARCH_ATTR
    many = tuple((b"k%d" % k, b"v%d" % k) for k in range(M))
    for name, kw in (("search_attributes", "sa"), ("memo", "mp")):
        cases.append((f"{name} count 0", four(**{kw: ()}), four(**{kw: None})))
        cases.append((f"{name} one pair", four(**{kw: ((b"k", b"v"),)}), four(**{kw: ((b"k", b"v"),)})))
        cases.append((f"{name} empty key and value", four(**{kw: ((b"", b""),)}), four(**{kw: ((b"", b""),)})))
        cases.append((f"{name} at the bound", four(**{kw: many}), four(**{kw: many})))
        cases.append((f"{name} over the bound", four(**{kw: many + ((b"one", b"more"),)}), E_SHAPE))
        cases.append((f"{name} bytes after the last pair", four(**{name: cmap(many[:2]) + b"tail"}), four(**{kw: many[:2]})))
        for edge, value, want in (
                ("2 bytes", b"\0\0", TRUNCATED), ("count -1", i4(-1), BAD_SIZE), ("count past the pairs", i4(2) + cmap(many[:1])[4:], TRUNCATED),
                ("count 2^31-1 alone", i4(2**31 - 1), TRUNCATED), ("a null key", i4(1) + i4(-1) + cv.val(b"v"), BAD_SIZE),
                ("a null value", i4(1) + cv.val(b"k") + i4(-1), BAD_SIZE), ("length -5", i4(1) + i4(-5), BAD_SIZE),
                ("a value past the map", i4(1) + cv.val(b"k") + i4(9) + b"short", TRUNCATED),
                ("a length cut", i4(1) + cv.val(b"k") + b"\0\0\0", TRUNCATED)):
            cases.append((f"{name} {edge}", four(**{name: value}), want))
    rep = ((b"k1", b"a"), (b"k2", b"b"), (b"k1", b"c"), (b"", b"d"), (b"", b""))
    cases.append(("repeated search-attribute key", four(sa=rep), four(sa=((b"k1", b"c"), (b"k2", b"b"), (b"", b"")))))
    # the list
    L = "non_retriable_errors"
    cases.append(("list count 0", four(**{L: lst([])}), four(**{L: None})))
    cases.append(("list a null element", four(**{L: i4(2) + cv.val(b"a") + i4(-1)}), BAD_SIZE))
    cases.append(("list element past the value", four(**{L: i4(1) + i4(9) + b"short"}), TRUNCATED))
    cases.append(("list bytes after the last element", four(**{L: lst([b"a"]) + b"tail"}), four(**{L: lst([b"a"])})))
    # the replication state
    two = four("2dc")
    rs = lambda *f: cx.body(list(f))  # noqa: E731
    cases.append(("replication state of one field", four("2dc", rs=rs(q(9))), four("2dc", rs=rs(q(9), None, None, None, None))))
    head = rs_body(lri=[])[:48]  # the four versions
    cases.append(("replication state, null map", four("2dc", rs=head + cv.val(None)), four("2dc", rs=head + cv.val(i4(0)))))
    cases.append(("replication state, trailing field", four("2dc", rs=rs_body() + cv.val(b"later")), two))
    cases.append(("last_write_version of 4 bytes", four("2dc", rs=rs(q(1), q(2), bytes(4))), E_SIZE))
    cases.append(("replication state cut in a length", four("2dc", rs=rs_body()[:14]), TRUNCATED))
    cases.append(("replication state length -2", four("2dc", rs=rs(q(1)) + i4(-2)), BAD_SIZE))
    cases.append(("unknown cluster", four("2dc", rs=rs_body(lri=[(CLUSTERS[0], 1, 2), (b"cluster-nowhere", 3, 4)])), E_CLUSTER))
    cases.append(("empty cluster name", four("2dc", rs=rs_body(lri=[(b"", 1, 2)])), E_CLUSTER))
    cases.append(("repeated cluster", four("2dc", rs=rs_body(lri=[(CLUSTERS[1], 1, 2), (CLUSTERS[0], 5, 6), (CLUSTERS[1], 3, 4)])),
                  four("2dc", rs=rs_body(lri=[(CLUSTERS[0], 5, 6), (CLUSTERS[1], 3, 4)]))))
    for edge, m, want in (("2 bytes", b"\0\0", TRUNCATED), ("count -1", i4(-1), BAD_SIZE), ("count past the pairs", i4(2) + lri_map([(CLUSTERS[0], 1, 2)])[4:], TRUNCATED),
                          ("a null key", i4(1) + i4(-1) + cv.val(cx.body([q(1), q(2)])), BAD_SIZE),
                          ("version of 4 bytes", i4(1) + cv.val(CLUSTERS[0]) + cv.val(cx.body([bytes(4), q(2)])), E_SIZE),
                          ("info cut inside", i4(1) + cv.val(CLUSTERS[0]) + cv.val(cx.body([q(1)]) + b"\0\0"), TRUNCATED),
                          ("info past the map", i4(1) + cv.val(CLUSTERS[0]) + i4(24) + b"short", TRUNCATED)):
        cases.append((f"replication info {edge}", four("2dc", rs=head + cv.val(m)), want))
    null_info = head + cv.val(i4(2) + cv.val(CLUSTERS[0]) + i4(-1) + cv.val(CLUSTERS[1]) + cv.val(cx.body([q(8)])))
    cases.append(("replication info null and short", four("2dc", rs=null_info),
                  four("2dc", rs=head + cv.val(lri_map([(CLUSTERS[0], 0, 0), (CLUSTERS[1], 8, 0)])))))
    # version histories
    ndc = four("ndc")
    cases.append(("version histories, json", four("ndc", enc=b"json"), E_ENCODING))
    cases.append(("version histories, no encoding", four("ndc", enc=b""), E_ENCODING))
    cases.append(("version histories without preamble", four("ndc", vh=ndc[2][1:]), E_ENCODING))
    cases.append(("version histories truncated inside", four("ndc", vh=ndc[2][:-3]), TRUNCATED))
    cases.append(("an encoding without version histories", four(enc=b"thriftrw"), plain))
    cases.append(("two histories", four("ndc", vh=_histories(n_hist=2)), E_SHAPE))
    cases.append(("index 1", four("ndc", vh=_histories(index=1)), E_SHAPE))
    cases.append(("items over the bound", four("ndc", n_items=abi.LOAD_MAX_VH_ITEMS + 1), E_SHAPE))
    # precedence: the UDT, the replication state's wire, both set, the cluster, the token, the
    # reset points, the maps' counts, the version histories
    both = dict(rs=rs_body(), vh=ndc[2], enc=b"thriftrw")
    bad_cluster = rs_body(lri=[(b"cluster-nowhere", 3, 4)])
    over = many + ((b"one", b"more"),)
    cases.append(("both set", four(**both), E_SHAPE))
    cases.append(("UDT before the replication state", four(rs=rs_body()[:14], state=bytes(3)), E_SIZE))
    cases.append(("a later UDT finding loses", four(state=bytes(3), memo=i4(-1)), E_SIZE))
    cases.append(("replication wire before both set", four(**{**both, "rs": rs_body()[:14]}), TRUNCATED))
    cases.append(("both set before the cluster", four(**{**both, "rs": bad_cluster}), E_SHAPE))
    cases.append(("replication wire before the cluster", four("2dc", rs=rs_body(lri=[(b"nowhere", 1, 2)])[:-3]), TRUNCATED))
    cases.append(("cluster before the token", four("2dc", rs=bad_cluster, branch_token=b"\x00"), E_CLUSTER))
    cases.append(("token before the reset points", four(branch_token=b"\x00", n_rp=abi.LOAD_MAX_RESET_POINTS + 1), E_ENCODING))
    cases.append(("reset points before the maps", four(auto_reset_points_encoding=b"json", sa=over), E_ENCODING))
    cases.append(("maps before the version histories", four("ndc", enc=b"json", mp=over), E_SHAPE))
    return cases


# ---------------------------------------------------------------- CPU
@pytest.mark.parametrize("builder", [abi.BUILDER_LOCAL, abi.BUILDER_2DC, abi.BUILDER_NDC])
@pytest.mark.parametrize("cfg", [2, 3, 4, 5])
def test_reference_round_trip(cfg, builder):
    """state -> oracle/cql_values.execution -> declared order -> reference decode == the state
    with the three differences of the form."""
    b, out, strs, persist, names = _state(cfg, builder)
    H = {s: h for h, s in enumerate(strs)}
    S = cv.tb.lookup(strs)
    clusters = [strs[h] for h in names]

    def get(w):
        values = cv.execution(out.exec[w], b.wfs[w].builder, S, persist[w], repl=out.repl[w],
                              vh_items=[(v.event_id, v.version) for v in out.rows(w, "vh")],
                              rps=[(p, S) for p in out.rows(w, "rp")],
                              sa=[(kv.key, kv.value) for kv in out.rows(w, "sa")], cluster_names=names)
        cols = cx.four_columns(b.wfs[w].builder, values)
        assert cols == rows.cql_exec_columns(b.wfs[w].builder, values)
        p = cx.parse_exec(*cols, clusters)
        for f, s in p.xs.items():
            setattr(p.x, f, H[s])
        for f, s in p.pss.items():
            setattr(p.ps, f, H[s])
        rps = []
        for rp, c, run in p.rps:
            rp.binary_checksum, rp.run_id = H[c], H[run]
            rps.append(rp)
        assert p.n_sa_wire == len(out.rows(w, "sa"))
        return (bytes(p.x), bytes(p.repl), bytes(p.ps), p.builder, [struct.pack("<qq", *i) for i in p.vh],
                [bytes(r) for r in rps], [bytes(abi.CdrKV(key=H[k], value=H[v])) for k, v in p.sa])
    assert _check_against_state(b, out, strs, persist, get) > 100


def test_declared_order_is_the_schema():
    """The name-derived permutation against the schema's field names."""
    root = os.path.dirname(os.path.abspath(__file__))
    names = json.load(open(os.path.join(root, "golden", "cql_workflow_execution_fields.json")))["fields"]
    assert len(names) == 58 and tuple(names) == rows.EXEC_DECLARED_NAMES and names == cx.NAMES
    assert sorted(rows.EXEC_STATEMENT) == sorted(names) and len(rows.EXEC_STATEMENT) == len(cv.EXEC_TYPES)
    assert rows.EXEC_DECLARED == tuple(rows.EXEC_STATEMENT.index(n) for n in names)
    # last_first_event_id: the statement's 18th field, the declaration's 50th
    assert rows.EXEC_STATEMENT[17] == names[49] == "last_first_event_id" and rows.EXEC_DECLARED[49] == 17
    assert rows.EXEC_DECLARED != tuple(range(58))
    assert cx.EMPTY_DOMAIN_ID == cv.parse_uuid(cv.EMPTY_DOMAIN_ID) and cx.EMPTY_RUN_ID == cv.parse_uuid(cv.EMPTY_RUN_ID)


def test_reference_wire_edges():
    seen = set()
    for name, f, want in wire_cases():
        if isinstance(want, int):
            assert _outcome(f) == want, name
            seen.add(want)
        else:
            assert _outcome(f) == _outcome(want), name
    assert seen == {TRUNCATED, BAD_SIZE, E_SIZE, E_SHAPE, E_CLUSTER, E_ENCODING, abi.LOAD_E_UUID}
    # what the plain rows decode to, spelled out once
    p = _one(four("2dc"))
    x = p.x
    assert p.xs["domain_id"] == b"00010203-0405-0607-0809-0a0b0c0d0e0f" and p.xs["workflow_id"] == b"workflow-0"
    assert p.xs["create_request_id"] == b"80818283-8485-8687-8889-8a8b8c8d8e8f"
    assert p.xs["parent_domain_id"] == b"10111213-1415-1617-1819-1a1b1c1d1e1f" and p.xs["parent_workflow_id"] == b"parent-wf-0"
    assert (x.initiated_id, x.completion_event_batch_id, x.next_event_id, x.last_event_task_id) == (33, 90, 101, 777)
    assert (x.attempt, x.signal_count, p.ps.sticky_s2s_timeout, x.backoff_coefficient) == (3, -2, 25, 1.5)
    assert x.flags == (abi.XI_CANCEL_REQUESTED | abi.XI_HAS_RETRY | abi.XI_HAS_EXPIRATION | abi.XI_HAS_BRANCH | abi.XI_HAS_MEMO |
                       abi.XI_HAS_SEARCH_ATTR | abi.XI_HAS_RESET_POINTS | abi.XI_STARTED)
    assert (p.ps.start_time, p.ps.last_updated_time, x.expiration_time) == (16 * 10**17, 16 * 10**17 + 9 * MS, 2 * 10**18)
    assert (p.ps.history_size, x.last_first_event_id, x.expiration_seconds) == (5000, 88, 600)
    assert p.builder == abi.BUILDER_2DC and (p.repl.present, p.repl.current_version, p.repl.start_version) == (1, 7, 5)
    assert (p.ps.current_version, p.ps.start_version, p.repl.last_write_version, p.repl.last_write_event_id) == (7, 5, 55, 41)
    assert (p.repl.lri_mask, list(p.repl.lri_version)[:3], list(p.repl.lri_last_event_id)[:3]) == (5, [3, 0, 4], [30, 0, 40])
    assert p.xs["memo"] == b"\x0d\x00\x0a\x0b\x0b\0\0\0\x01\0\0\0\x02mk\0\0\0\x02mv\x00"
    assert p.xs["nonretriable"] == b"\x0b\0\0\0\x02\0\0\0\x03bad\0\0\0\x02e0" and p.sa == [(b"k1", b"v1"), (b"k2", b"v2")]
    assert [len(s) for s in p.gen] == [36] * 5 + [len(p.xs["nonretriable"]), len(p.xs["memo"])]
    p = _one(four("ndc"))
    assert p.builder == abi.BUILDER_NDC and p.vh == [(3, 1), (7, 2), (11, 3)] and p.x.flags & abi.XI_VH_BRANCH
    assert not p.x.flags & abi.XI_HAS_BRANCH and p.xs["branch_tree_id"] == b"vh-tree-0" and not bytes(p.repl).strip(b"\0")
    p = _one((b"", b"", b"", b""))
    assert p.x.flags == abi.XI_STARTED and (p.ps.start_time, p.x.expiration_time, p.x.initiated_id) == (ZT, 0, 0)
    assert p.xs["domain_id"] == b"00000000-0000-0000-0000-000000000000" == p.xs["create_request_id"]


def test_abi_mirrors():
    L = abi.lib()
    assert L.cdr_struct_size(b"cdr_cql_exec_in") == C.sizeof(abi.CdrCqlExecIn) == 32 + 4 * abi.MAX_CLUSTERS + 8
    assert L.cdr_struct_size(b"cdr_cql_state_out") == C.sizeof(abi.CdrCqlStateOut) == 360 + 24
    assert L.cdr_struct_size(b"cdr_cql_rows_in") == 80 and L.cdr_struct_size(b"cdr_cql_rows_out") == 360
    assert (abi.CdrCqlExecIn.cluster_seed.offset, abi.CdrCqlExecIn.n_clusters.offset) == (32, 32 + 4 * abi.MAX_CLUSTERS)
    assert (abi.CdrCqlStateOut.persist.offset, abi.CdrCqlStateOut.builder.offset, abi.CdrCqlStateOut.exec_status.offset) == (360, 368, 376)
    assert hasattr(L, "cdr_load_cql_state")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "cdr", "cdr.h")).read()
    flat = " ".join(hdr.split())
    assert ("int cdr_load_cql_state(cdr_ctx* ctx, const cdr_cql_rows_in* rows, const cdr_cql_exec_in* exec, "
            "cdr_cql_state_out* out, void* stream);") in flat
    codes = {k: int(v) for k, v in re.findall(r"#define CDR_LOAD_E_([A-Z_]+) (\d+)", hdr)}
    assert max(codes.values()) == codes["CQL_SIZE"] == 22
    assert "is the next step and not built" not in open(os.path.join(root, "DESIGN.md")).read()


# ---------------------------------------------------------------- GPU
def _assert_equal(eng, cols, seeds, **kw):
    got = rows.load_cql_state(eng, cols, seeds, **kw)
    want = cx.decode_state(cols, seeds, kw.get("n_bytes"), kw.get("cluster_seed"))
    bad = cx.compare_state(got, want, cols)
    assert not bad, "\n".join(bad[:10])
    return got, want


def _getter(got):
    size = {t: C.sizeof(engine.TABLE_TYPES[t]) for t in ITEMS}
    raw = {t: bytes(got.tables[t]) for t in ITEMS}

    def get(w):
        c, r = got.caps[w], got.result[w]
        items = [[raw[t][(getattr(c, t + "_off") + j) * size[t]:(getattr(c, t + "_off") + j + 1) * size[t]]
                  for j in range(getattr(r, engine.TABLE_COUNT[t]))] for t in ITEMS]
        return (bytes(got.exec[w]), bytes(got.repl[w]), bytes(got.persist[w]), int(got.builder[w]), *items)
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("builder", [abi.BUILDER_LOCAL, abi.BUILDER_2DC, abi.BUILDER_NDC])
@pytest.mark.parametrize("cfg", [2, 3, 4, 5])
def test_gpu_round_trip(engine_gpu, cfg, builder):
    """Replayed states through cdr_encode_cql_async -> columns -> cdr_load_cql_state: the
    columns are the oracle writer's, the records the reference's and the states' own (modulo
    the three differences); with most strings new, other handles and the same bytes."""
    b, out, strs, persist, names = _state(cfg, builder)
    cols = rows.encode_state_cql(engine_gpu, b, out, strs, exec_rows=True, persist=persist, cluster_names=names)
    assert cols.bytes.tobytes() == cx.columns(b, out, strs, persist, names).bytes.tobytes()
    ok = [w for w in range(b.n_wfs) if _storable(b, out, strs, w)]
    got, _ = _assert_equal(engine_gpu, cols, strs)  # seeds = the whole table: every handle kept
    assert got.strings == strs and got.n_bad_entries == b.n_wfs - len(ok)
    assert _check_against_state(b, out, strs, persist, _getter(got)) == len(ok) > 100
    seeds = strs[:len(strs) // 3] + CLUSTERS
    cs = [len(seeds) - len(CLUSTERS) + i for i in range(len(names))]
    got, _ = _assert_equal(engine_gpu, cols, seeds, cluster_seed=cs)
    assert set(got.strings) == set(strs) and len(set(got.strings)) == len(got.strings)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [3, 5])
def test_gpu_loaded_state_alone_carries_a_replay(engine_gpu, cfg):
    """Prefix replay -> encode_state_cql -> load_cql_state -> to_carry with nothing else ->
    suffix replay == the oracle's replay of the whole histories, once the times on both sides
    are floored to the millisecond: a time the prefix set went through a CQL timestamp, one the
    suffix set did not, and no replayed value is computed from a stored time."""
    import oracle
    b = engine.synth_batch(cfg, 300, seed=0x5EED0D00 + cfg)
    cut = engine.split_half(b)
    pre, suf = engine.cut_batches(b, cut)
    pre_out = engine_gpu.replay(pre)
    n_cl = b.cluster.n_clusters
    strs = rows.whole_state_strings(pre, pre_out, extra=n_cl)
    for w in range(b.n_wfs):  # the create request IDs go into a uuid column
        h = pre_out.exec[w].create_request_id
        if pre_out.result[w].code == abi.OK and h and not UUID_TEXT.fullmatch(strs[h]):
            strs[h] = b"c0de%04x-0000-4000-8000-%012x" % (h & 0xFFFF, h)
    assert len(set(strs)) == len(strs)
    names = list(range(len(strs) - n_cl, len(strs)))
    cols = rows.encode_state_cql(engine_gpu, pre, pre_out, strs, exec_rows=True, cluster_names=names)
    got = rows.load_cql_state(engine_gpu, cols, strs)
    assert got.strings == strs
    ok = np.array([_storable(pre, pre_out, strs, w) for w in range(b.n_wfs)])
    assert [int(s) == 0 for s in got.entry_status] == ok.tolist()
    assert {int(got.builder[w]) for w in range(b.n_wfs) if ok[w]} == {pre.wfs[w].builder for w in range(b.n_wfs) if ok[w]}
    # (a repeated search-attribute key is two rows of the replay and one of any stored map: see
    # tests/test_load_state.py; those entries replay whole)
    storable = np.array([len({kv.key for kv in pre_out.rows(w, "sa")}) == pre_out.result[w].n_search_attr
                         for w in range(b.n_wfs)])
    src = np.where((cut > 0) & ok & storable, np.arange(b.n_wfs), -1)
    cut = np.where(storable & ok, cut, 0)
    pre, suf = engine.cut_batches(b, cut)
    suf.carry = rows.to_carry(got, src=src)
    out = engine_gpu.replay(suf)
    whole = oracle.replay(b)
    floored = 0
    for res in (out, whole):
        for w in range(b.n_wfs):
            if src[w] >= 0:
                floored += _floor_times(res, w)
    bad = engine.compare(b, out, whole)
    assert not bad, bad[:5]
    assert sum(1 for w in range(b.n_wfs) if whole.result[w].code == abi.OK and src[w] >= 0) > 100 and floored > 0


TIME_FIELDS = {"act": ("scheduled_time", "started_time", "last_heartbeat_time", "expiration_time"),
               "timer": ("expiry_time",)}


def _floor_times(res, w) -> int:
    """Floor entry w's stored times to the millisecond in place; how many changed."""
    recs = [(res.exec[w], ("expiration_time",))]
    for t, fs in TIME_FIELDS.items():
        off = getattr(res.plan.caps[w], t + "_off")
        recs += [(res.tables[t][off + j], fs) for j in range(getattr(res.result[w], engine.TABLE_COUNT[t]))]
    n = 0
    for r, fs in recs:
        for f in fs:
            v = getattr(r, f)
            n += v != v // MS * MS
            setattr(r, f, v // MS * MS)
    return n


def _named(rec, strings, handles):
    """A record's fields with its handle fields as strings."""
    return {f: (strings[getattr(rec, f)] if f in handles else getattr(rec, f)) for f, *_ in type(rec)._fields_
            if not f.startswith("_") and not hasattr(getattr(rec, f), "__len__")}


@pytest.mark.gpu
def test_gpu_both_forms_load_alike(engine_gpu):
    """The same states (config 4: the three builders mixed) through cdr_load_state and
    cdr_load_cql_state agree record for record once handles are strings; the only differences
    are the millisecond floor, the empty maps' flags and last_event_task_id."""
    b, out, strs, persist, names = _state(4, abi.BUILDER_NDC)
    seeds = strs[:len(strs) // 4] + CLUSTERS
    cs = [len(seeds) - len(CLUSTERS) + i for i in range(len(names))]
    R = rows.encode_state(engine_gpu, b, out, strs, exec_rows=True, persist=persist, cluster_names=names)
    sql = rows.load_state(engine_gpu, R, seeds, cluster_seed=cs)
    cols = rows.encode_state_cql(engine_gpu, b, out, strs, exec_rows=True, persist=persist, cluster_names=names)
    cql = rows.load_cql_state(engine_gpu, cols, seeds, cluster_seed=cs)
    n, builders = 0, set()
    for w in range(b.n_wfs):
        if not _storable(b, out, strs, w):
            continue
        assert sql.entry_status[w] == 0 == cql.entry_status[w], w
        a, c = _named(sql.exec[w], sql.strings, rows.X_HANDLES), _named(cql.exec[w], cql.strings, rows.X_HANDLES)
        assert a["last_event_task_id"] == 0 and c["last_event_task_id"] == out.exec[w].last_event_task_id
        a["last_event_task_id"] = c["last_event_task_id"]
        a["expiration_time"] = a["expiration_time"] // MS * MS
        if not sql.result[w].n_search_attr:
            a["flags"] &= ~abi.XI_HAS_SEARCH_ATTR
        assert a == c, (w, [f for f in a if a[f] != c[f]])
        pa = _named(sql.persist[w], sql.strings, cx.P_HANDLES)
        pc = _named(cql.persist[w], cql.strings, cx.P_HANDLES)
        for f in ("start_time", "last_updated_time"):
            pa[f] = pa[f] if pa[f] == ZT else pa[f] // MS * MS
        assert pa == pc, (w, [f for f in pa if pa[f] != pc[f]])
        assert bytes(sql.repl[w]) == bytes(cql.repl[w]) and sql.builder[w] == cql.builder[w], w
        assert bytes(sql.result[w]) == bytes(cql.result[w]), w
        assert [bytes(r) for r in sql.rows(w, "vh")] == [bytes(r) for r in cql.rows(w, "vh")], w
        for t, hs in rows.ITEM_HANDLES.items():
            assert [_named(r, sql.strings, hs) for r in sql.rows(w, t)] == [_named(r, cql.strings, hs) for r in cql.rows(w, t)], (w, t)
        builders.add(int(cql.builder[w]))
        n += 1
    assert n > 100 and len(builders) > 1


def _varied(w, **kw):
    """A row whose item counts, builder and values vary with w."""
    kind = ("local", "2dc", "ndc")[w % 3]
    return four(kind, w % 5, n_rp=w % 4, sa=[(b"key-%d" % k, b"value-%d" % (w + k)) for k in range(w % 3)],
                mp=[(b"m", b"%d" % w)] if w % 2 else None, n_items=w % 6, **kw)


def _pending(n):
    """Pending columns for n entries: a signal row in every third entry, an activity row with
    an error list in every fifth."""
    cols = [[b""] * n for _ in range(5)]
    for w in range(n):
        if w % 3 == 0:
            cols[4][w] = i4(1) + pair(4, pending_base(4, w, w))
        if w % 5 == 0:
            cols[0][w] = i4(1) + pair(0, pending_base(0, w, w))
    return cols


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, BLOCK + 1])
def test_gpu_entry_counts(engine_gpu, n):
    """Entry counts around a wavefront and one past a workgroup, with pending rows beside the
    execution rows (one string table: the activity rows' list bodies follow the entries'
    shares of gen_bytes)."""
    got, want = _assert_equal(engine_gpu, entries([_varied(w) for w in range(n)], _pending(n)), SEEDS)
    assert not any(want.entry_status) and len(got.result) == n
    if n > 5:
        assert any(r.nonretriable for r in got.tables["act"]) and all(x.nonretriable for x in got.exec)


@pytest.mark.gpu
def test_gpu_failing_rows_stay_in_their_lane(engine_gpu):
    """A failing execution row in lanes 0 / 31 / 32 / 63 of a wave: its neighbours are
    unaffected and none of its strings is interned, its pending rows' included; a failing
    pending row wins the entry status (the execution row is table 5)."""
    n = BLOCK + 1
    bad_lanes = (64, 64 + 31, 64 + 32, 64 + 63)
    fours = [_varied(w) for w in range(n)]
    for w in bad_lanes:
        fours[w] = _varied(w, workflow_id=b"workflow-of-a-failing-row-%d" % w, auto_reset_points_encoding=b"json")
    pend = _pending(n)
    for w in bad_lanes:
        pend[4][w] = i4(1) + pair(4, pending_base(4, w, w)[:4] + [b"signal-of-a-failing-row-%d" % w])
    pend[3][64 + 31] = i4(1) + pair(3, pending_base(3)[:3] + [b"not-a-uuid"])
    got, want = _assert_equal(engine_gpu, entries(fours, pend), SEEDS)
    for w in range(n):
        assert got.exec_status[w] == (E_ENCODING if w in bad_lanes else 0), w
        assert got.entry_status[w] == (0 if w not in bad_lanes else abi.LOAD_E_UUID if w == 64 + 31 else E_ENCODING), w
    assert got.n_bad_entries == 4 and [got.result[w].code for w in bad_lanes] == [abi.E_LOAD_ROWS] * 4
    assert not any(b"failing-row" in s for s in got.strings) and b"workflow-3" in got.strings


@pytest.mark.gpu
def test_gpu_wire_edges(engine_gpu):
    """Every wire-edge row of the CPU test, each in an entry of its own."""
    cases = wire_cases()
    got, _ = _assert_equal(engine_gpu, entries([f for _, f, _ in cases]), SEEDS)
    for w, (name, _, want) in enumerate(cases):
        assert got.exec_status[w] == got.entry_status[w] == _status(want), name


@pytest.mark.gpu
@pytest.mark.parametrize("column", [0, 1, 2])
def test_gpu_truncation_at_every_length(engine_gpu, column):
    """One full execution UDT (or replication_state body, or version_histories blob) cut at
    every length, one entry per length in a single launch; whole rows between them."""
    kind = ("ndc", "2dc", "ndc")[column]
    plain = four(kind, n_rp=1, n_items=2)
    d = xvals(kind, n_rp=1)
    ends, p, no_encoding = {0}, 0, -1
    if column == 0:
        for name in cx.NAMES:
            p += len(cv.val(d[name]))
            ends.add(p)
            if name == "auto_reset_points":  # a cut here leaves the reset points without their encoding
                no_encoding = p
    elif column == 1:
        for v in (q(7), q(5), q(55), q(41)):
            p += len(cv.val(v))
            ends.add(p)
    fours, expect = [], []
    for n in range(len(plain[column])):
        fours.append(plain[:column] + (plain[column][:n],) + plain[column + 1:])
        # (an empty version_histories blob is a null column: not NDC)
        expect.append(E_ENCODING if n == no_encoding else 0 if n in ends else TRUNCATED)
        if n % 16 == 0:
            fours.append(plain)
            expect.append(0)
    got, _ = _assert_equal(engine_gpu, entries(fours), SEEDS)
    assert got.entry_status.tolist() == expect and expect.count(TRUNCATED) > len(expect) // 2


@pytest.mark.gpu
def test_gpu_buffer_end(engine_gpu):
    """`bytes` ends where its allocation ends and n_bytes is short of the offsets: the offsets
    are clamped, the cut column is TRUNCATED or null, the rows before it decode; lengths inside
    the last column that claim bytes past the buffer."""
    fours = [four("ndc"), _varied(4), four("ndc")]
    cols = entries(fours)
    assert int(cols.exec.off[3][3]) == len(cols.bytes)  # the encoding column comes last
    total = len(cols.bytes)
    x_end, vh_lo, vh_hi = int(cols.exec.off[0][3]), int(cols.exec.off[2][2]), int(cols.exec.off[2][3])
    for nb, want in ((total, 0), (total - 1, E_ENCODING), (total - 8, E_ENCODING), (vh_hi - 1, E_ENCODING), (vh_lo + 1, E_ENCODING),
                     (vh_lo, 0), (x_end - 1, TRUNCATED), (x_end - 40, TRUNCATED), (3, None), (0, None)):
        got, _ = _assert_equal(engine_gpu, cols, SEEDS, at_end=True, n_bytes=nb)
        if want is not None:
            assert got.entry_status.tolist()[2] == want, nb
    cols.exec.off[3][3] += 1 << 20  # the last offset far past the buffer
    _assert_equal(engine_gpu, cols, SEEDS, at_end=True)
    d = xvals()
    tails = [raw_at(d, "memo", i4(1 << 30) + b"abc"), raw_at(d, "memo", cv.val(i4(1) + cv.val(b"k") + i4(1 << 30))),
             raw_at(d, "memo", cv.val(i4(2**31 - 1)))]
    for tail in tails:
        cols = rows.pack_cql(2, [[b"", b""] for _ in range(5)], [[b"", b""], [b"", b""], [b"", b""], [four()[0], tail]], CSEED)
        assert int(cols.exec.off[3][2]) == len(cols.bytes)
        cols.exec.off = [cols.exec.off[3], cols.exec.off[1], cols.exec.off[2], cols.exec.off[0]]  # execution last
        got, _ = _assert_equal(engine_gpu, cols, SEEDS, at_end=True)
        assert got.entry_status.tolist() == [0, TRUNCATED]


def _sized(size, w):
    """A short execution body (most fields null) padded to exactly `size` bytes."""
    d = {n: None for n in cx.NAMES}
    d.update(workflow_id=b"", task_list=b"tl-%d" % (w % 3), state=i4(1), next_event_id=q(9 + w), domain_id=bytes([w % 251] * 16))
    pad = size - len(xbody(d))
    assert pad >= 0
    d["workflow_id"] = b"p" * pad
    assert len(xbody(d)) == size
    return xbody(d), b"", b"", b""


@pytest.mark.gpu
def test_gpu_staging(engine_gpu):
    """Waves whose 64 execution columns span a byte under, exactly, and a byte over the 24 KiB
    the loader stages in LDS (the buffer is 256-byte aligned, so a wave's staged range starts at
    its first column's offset rounded down to 16), and a 70 KB memo."""
    fours, pos = [], 0
    share = STAGE // 64
    for over in (-1, 0, 1):
        lead = pos - (pos & ~15)
        last = STAGE + over - lead - 63 * share
        fours += [_sized(share, w) for w in range(63)] + [_sized(last, 63)]
        assert pos + 63 * share + last - (pos & ~15) == STAGE + over
        pos += 63 * share + last
    big = len(fours)
    fours.append(four(mp=((b"big", bytes(range(256)) * 273 + b"x" * 113), (b"k", b"v"))))
    fours += [_varied(w) for w in range(5)]
    cols = entries(fours)
    assert int(cols.exec.off[0][0]) == 0 and int(cols.exec.off[0][192]) == pos
    got, want = _assert_equal(engine_gpu, cols, SEEDS)
    assert not got.n_bad_entries and len(got.strings[got.exec[big].memo]) > 70_000
    assert got.strings[got.exec[big].memo] == want.parsed[big].xs["memo"]


@pytest.mark.gpu
def test_gpu_misuse_and_degenerate_sizes(engine_gpu):
    """exec == NULL is cdr_load_cql_rows byte for byte; zero entries; a second call on the warm
    context gives the first one's results; the CDR_API_EINVAL cases."""
    from tests.test_load_cql import _hand_made
    cols = _hand_made()
    one, two = rows.load_cql(engine_gpu, cols, SEEDS), rows.load_cql_state(engine_gpu, cols, SEEDS)
    for t in rows.TABLES:
        assert bytes(one.tables[t]) == bytes(two.tables[t])
    assert bytes(one.result) == bytes(two.result) and bytes(one.caps) == bytes(two.caps) and one.strings == two.strings
    assert all((a == c).all() for a, c in zip(one.row_status, two.row_status)) and one.gen_bytes == two.gen_bytes
    assert (one.entry_status == two.entry_status).all() and bytes(one.totals) == bytes(two.totals) and two.exec is None
    assert one.n_rows == two.n_rows and all((a == c).all() for a, c in zip(one.entry_row0, two.entry_row0))
    assert (one.str_len == two.str_len).all()  # (str_ref names whichever occurrence was interned first)
    none = rows.load_cql_state(engine_gpu, entries([]), SEEDS)
    assert len(none.result) == 0 and none.strings == SEEDS and none.n_bad_entries == 0 and none.n_rows == [0] * 5
    cx_cols = entries([_varied(w) for w in range(70)], _pending(70))
    first, again = rows.load_cql_state(engine_gpu, cx_cols, SEEDS), rows.load_cql_state(engine_gpu, cx_cols, SEEDS)
    assert bytes(first.exec) == bytes(again.exec) and first.strings == again.strings and first.gen_bytes == again.gen_bytes
    assert all(bytes(first.tables[t]) == bytes(again.tables[t]) for t in ITEMS + rows.TABLES)
    L = abi.lib()
    ctx = engine_gpu.ctx
    inp, xin, res = abi.CdrCqlRowsIn(), abi.CdrCqlExecIn(), abi.CdrCqlStateOut()
    assert L.cdr_load_cql_state(ctx, None, C.byref(xin), C.byref(res), None) == -1
    assert L.cdr_load_cql_state(ctx, C.byref(inp), C.byref(xin), None, None) == -1
    assert L.cdr_load_cql_state(None, C.byref(inp), C.byref(xin), C.byref(res), None) == -1
    assert L.cdr_load_cql_state(ctx, C.byref(inp), C.byref(xin), C.byref(res), None) == -1  # no seeds
    assert rows.load_cql_state(engine_gpu, cx_cols, SEEDS, check=False, cluster_seed=list(range(abi.MAX_CLUSTERS + 1))).rc == -1
    dev = rows.DeviceBuffers()
    try:
        so = dev.up(np.zeros(3, np.uint64))
        inp.seed_off, inp.seed_bytes, inp.n_seeds = so, so, 1
        assert L.cdr_load_cql_state(ctx, C.byref(inp), C.byref(xin), C.byref(res), None) == 0  # zero entries
        inp.n_entries = 2
        for t in range(5):
            inp.col_off[t] = so
        assert L.cdr_load_cql_state(ctx, C.byref(inp), C.byref(xin), C.byref(res), None) == -1  # null columns
        xin.execution_off = xin.replication_state_off = xin.version_histories_off = so
        assert L.cdr_load_cql_state(ctx, C.byref(inp), C.byref(xin), C.byref(res), None) == -1  # one column null
        xin.vh_encoding_off = so
        assert L.cdr_load_cql_state(ctx, C.byref(inp), C.byref(xin), C.byref(res), None) == 0
        assert res.rows.rows.n_bad_entries == 0 and res.rows.rows.totals.vh == 0 and res.exec_status
    finally:
        dev.free()
