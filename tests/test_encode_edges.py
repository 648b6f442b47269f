"""The persisted-row encoders (encode.hip, encode_var.hip; SQL thriftrw and CQL forms) on
hand-made states and edge values — what no synthetic replay feeds them:
the local builder, failed entries, strings up to 70,001 bytes, out-of-range handles in every
handle field, broken UUID texts and Memo bodies, integer / double / timestamp extremes,
every flag word, 0 .. 1000 rows per entry beside empty ones, a scan over many tiles,
guarded buffers, a NULL row_status and the argument checks.

The batch is tests/encode_edges.py; expected bytes and statuses come only from
oracle/thrift_binary.py and oracle/cql_values.py (BadUUID / BadHandle / BadMemo -> status;
no other exception is caught).  CPU: the batch holds what it claims.  GPU (-m gpu): every
row's status == the oracle's, every status-0 row byte-identical, the row set exactly the
rows of OK entries, zero-length rows / untouched slots everywhere else.
"""
import ctypes as C

import numpy as np
import pytest

from cadence_amd import abi, engine
from oracle import cql_values as cq
from oracle import thrift_binary as tb
from tests import encode_edges as ee
from tests.states import make_state
from tests.test_encode_cql import check_cql_values
from tests.test_encode_var import ACTIVITY, CHILD, EXEC, SIGNAL, check_variable_row_blobs, parse

SQL_VAR = ("act", "child", "signal", "exec")
CQL_ALL = ("act", "timer", "child", "cancel", "signal", "exec")
FORMS = [("sql", t) for t in SQL_VAR] + [("cql", t) for t in CQL_ALL]
# the statuses a table can produce, per form (cdr.h CDR_BLOB_*): E_UUID where a UUID text is
# parsed, E_MEMO for the execution row's Memo, E_HANDLE wherever a handle is read
CAN = {("sql", "act"): {0, 2}, ("sql", "child"): {0, 1, 2}, ("sql", "signal"): {0, 2}, ("sql", "exec"): {0, 1, 2, 3},
       ("cql", "act"): {0, 2}, ("cql", "timer"): {0, 2}, ("cql", "child"): {0, 1, 2}, ("cql", "cancel"): {0},
       ("cql", "signal"): {0, 2}, ("cql", "exec"): {0, 1, 2, 3}}
IDL = {"act": ACTIVITY, "child": CHILD, "signal": SIGNAL, "exec": EXEC}
CQL_TYPES = {"act": cq.ACTIVITY_TYPES, "timer": cq.TIMER_TYPES, "child": cq.CHILD_TYPES, "cancel": cq.CANCEL_TYPES,
             "signal": cq.SIGNAL_TYPES}


# ---------------------------------------------------------------- CPU
def test_oracle_failure_classes():
    S = tb.lookup([b"", b"x"])
    assert S(1) == b"x"
    for h in (2, 0xFFFFFFFF):
        with pytest.raises(tb.BadHandle):
            S(h)
    T = ee.Strings()
    for name, h in T.memo_bad.items():
        with pytest.raises(tb.BadMemo):
            tb._memo_fields(T.strs[h])
    assert [tb._memo_fields(T.strs[h]) is None for h in T.memo_ok] == [False, False, False, True]
    assert cq.BadHandle is tb.BadHandle and cq.BadMemo is tb.BadMemo
    # the two UUID parsers differ on a dash after an even digit count
    s = T.strs[T.uuid_bad["dash+2"]]
    with pytest.raises(tb.BadUUID):
        tb.parse_uuid(s)
    assert cq.parse_uuid(s) == cq.parse_uuid(T.strs[T.uuid_ok[0]])
    for k in ("dash+1", "nonhex", "len35", "len37"):
        with pytest.raises(tb.BadUUID):
            tb.parse_uuid(T.strs[T.uuid_bad[k]])
        with pytest.raises(cq.BadUUID):
            cq.parse_uuid(T.strs[T.uuid_bad[k]])
    for h in T.uuid_ok:
        assert tb.parse_uuid(T.strs[h]) == cq.parse_uuid(T.strs[h]) == bytes.fromhex("0123abcd89ef4c5d8a7bfedcba987654")


def test_string_table_holds_what_it_claims():
    T = ee.Strings()
    assert sorted(len(T.strs[h]) for h in T.plain.values()) == [0] + list(ee.PLAIN_LENS)
    assert set(b"".join(T.strs[h] for h in T.plain.values())) == set(range(256))
    assert max(len(s) for s in T.strs) == 70001 > 1 << 16
    assert [len(T.strs[h]) for h in T.uuid_ok] == [36, 36, 32, 36]
    assert [len(parse(b"\x0d\x00\x0a" + tb._memo_fields(T.strs[h]) + b"\x00", {10: 13})[10]) for h in T.memo_ok[:3]] \
        == [0, 1, 3]
    assert [cq.decode(cq.list_text(T.strs[h]), ["list<text>"])[0][:4] for h in T.lists] == \
        [(n).to_bytes(4, "big") for n in (0, 1, 3)]


def _values(recs, name):
    return {getattr(r, name) for r in recs}


def _bits(recs, name):
    o = getattr(type(recs[0]), name).offset
    return {int.from_bytes(bytes(r)[o:o + 8], "little") for r in recs}


def test_hand_made_batch_holds_what_it_claims():
    """Shape, values and flags of the batch (see the module docstring of tests/encode_edges.py)."""
    hm = ee.hand_made()
    b, out, T = hm.batch, hm.out, hm.T
    assert b.n_wfs == ee.N_ENTRIES and b.n_wfs % 64 and b.n_wfs % 256
    ok = [w for w in range(b.n_wfs) if out.result[w].code == abi.OK]
    assert hm.failed == [w for w in range(b.n_wfs) if w % 7 == 6] and len(ok) + len(hm.failed) == b.n_wfs
    for w in hm.failed:
        r = out.result[w]
        assert r.code != abi.OK and min(r.n_activity, r.n_timer, r.n_child, r.n_cancel, r.n_signal, r.n_vh,
                                        r.n_reset_points, r.n_search_attr) > 0
        assert all(getattr(row, f) >= T.n for t in ("act", "timer", "child", "signal", "rp", "sa")
                   for row in out.rows(w, t) for f in ee._handles(t))
    counts = {out.result[w].n_signal for w in ok}
    assert {0, 1, 63, 64, 65, 1000} <= counts
    assert out.result[0].n_activity == 1000 and out.result[1].n_activity == 0 == out.result[9].n_activity
    for t in engine.TABLES:  # slack (w + 1) % 4 rows
        assert all(getattr(out.plan.caps[w], t + "_cap") == getattr(out.result[w], engine.TABLE_COUNT[t]) + (w + 1) % 4
                   for w in range(b.n_wfs))
    # scalars: every int64 / int32 field of every record type takes every edge value, the
    # UUID halves their patterns, the doubles their bit patterns
    recs = {t: [r for w in ok for r in out.rows(w, t)] for t in engine.TABLES}
    recs["exec"] = [out.exec[w] for w in ok]
    recs["persist"] = [hm.persist[w] for w in ok]
    recs["repl"] = [out.repl[w] for w in ok]
    for kind, rows in recs.items():
        for name, ty in type(rows[0])._fields_:
            if name.startswith("_pad") or name in ee._handles(kind) or name == "flags":
                continue
            if ty is abi.i64 and name != "sticky_s2s_timeout":
                assert _values(rows, name) >= set(ee.V64), (kind, name)
            if ty is abi.i32 or name == "sticky_s2s_timeout":
                assert _values(rows, name) >= set(ee.V32), (kind, name)
            if ty is abi.u64:
                assert _values(rows, name) >= set(ee.U64S), (kind, name)
            if ty is abi.f64:
                assert _bits(rows, name) == set(ee.DBL_BITS), (kind, name)
    # handles: every handle field takes 0, every valid class, n and 0xFFFFFFFF
    for kind, rows in recs.items():
        for name in ee._handles(kind):
            seen = _values(rows, name)
            assert {0, T.n, 0xFFFFFFFF} <= seen, (kind, name)
            if name in ee.PLAIN.get(kind, ()):
                assert set(T.plain.values()) <= seen, (kind, name)
            if name in ee.UUIDS.get(kind, ()):
                assert set(T.uuid_ok) | set(T.uuid_bad.values()) <= seen, (kind, name)
            if name in ee.LISTS.get(kind, ()):
                assert set(T.lists) <= seen, (kind, name)
            if name in ee.MEMOS.get(kind, ()):
                assert set(T.memo_ok) | set(T.memo_bad.values()) <= seen, (kind, name)
    # timestamps under both CDR_AI_STARTED_TIME_SET states
    ts = (-1, -999_999, -1_000_000, -1_000_001, 999_999, 1_000_000, ee.I64_MIN, ee.I64_MAX)
    for name in ("started_time", "last_heartbeat_time"):
        for bit in (0, abi.AI_STARTED_TIME_SET):
            assert {getattr(a, name) for a in recs["act"] if a.flags & abi.AI_STARTED_TIME_SET == bit} >= set(ts)
    assert _values(recs["persist"], "start_time") >= set(ts) | {abi.ZERO_TIME_NANOS}
    # flags
    assert {a.flags & 7 for a in recs["act"]} == set(range(8))
    assert {p.flags & 0x7F for p in recs["rp"]} == set(range(128))
    for bld in (abi.BUILDER_LOCAL, abi.BUILDER_2DC, abi.BUILDER_NDC):
        fl = [out.exec[w].flags for w in ok if b.wfs[w].builder == bld and w < hm.first_tail]
        for bit in (1 << i for i in range(9)):
            assert any(f & bit for f in fl) and any(not f & bit for f in fl), (bld, bit)
    clean = [w for w in ok if w < hm.first_tail]
    X, R = out.exec, out.result
    assert any(not X[w].flags & abi.XI_HAS_RESET_POINTS and R[w].n_reset_points > 0 for w in clean)
    assert {R[w].n_search_attr for w in clean if X[w].flags & abi.XI_HAS_SEARCH_ATTR} >= {0, 5}
    assert any(X[w].flags & abi.XI_HAS_MEMO and X[w].memo == 0 for w in clean)
    assert any(b.wfs[w].builder == abi.BUILDER_NDC and not X[w].flags & abi.XI_VH_BRANCH for w in clean)
    assert b.cluster.n_clusters == 3
    assert {out.repl[w].lri_mask for w in clean if b.wfs[w].builder == abi.BUILDER_2DC} == {0, 0b001, 0b101, 0b111}
    assert {R[w].n_vh for w in clean if b.wfs[w].builder == abi.BUILDER_NDC} == {0, 1, 40}
    assert {R[w].n_reset_points for w in clean} == {0, 1, 20}


@pytest.mark.parametrize("form,table", FORMS)
def test_expected_rows_cover(form, table):
    """Per table and form: every status it can produce occurs; at most 15 % of the rows are
    compared by status alone; every status-0 row parses (SQL: under the IDL, CQL: under the
    schema's column types); and all 16 classes of (row start offset mod 4, row length mod 4)
    occur among the status-0 rows whose offsets the oracle's sizes determine."""
    hm = ee.hand_made()
    want = ee.expected(table, form)
    assert {code for _, code in want.values()} == CAN[form, table]
    bad = sum(1 for _, code in want.values() if code)
    print(form, table, "rows", len(want), "by status only", bad)
    assert bad <= 0.15 * len(want)
    # no failure outside the case rows, each a clean row with one field overridden
    caps = hm.out.plan.caps
    case_rows = {w for key, w in ((k, k[1]) for k in hm.case_of) if key[0] == "exec"} if table == "exec" else \
        {getattr(caps[k[1]], table + "_off") + k[2] for k in hm.case_of if k[0] == table}
    assert {r for r, (_, code) in want.items() if code} <= case_rows and len(case_rows) == hm.n_cases[table]
    for r, (blob, code) in want.items():
        if code == 0 and form == "sql":
            parse(blob, IDL[table])
        elif code == 0:
            cq.decode(blob, CQL_TYPES[table] if table != "exec" else
                      cq.EXEC_TYPES + cq.EXEC_TAIL[hm.batch.wfs[r].builder])
    # clean rows stay clean: no failure outside the case rows
    first = min(r for r, (_, code) in want.items() if code) if bad else None
    if table == "exec":
        assert first is None or first >= hm.first_tail
    if table in SQL_VAR:
        off, first = ee.oracle_offsets(want, ee.n_capacity_rows(hm.batch, hm.out, table))
        classes = {(off[r] % 4, len(want[r][0]) % 4) for r in want if r < first}
        assert len(classes) == 16, sorted(classes)


# ---------------------------------------------------------------- GPU
def _check_rows(eng, batch, out, want, got, codes):
    """Statuses, bytes, the row set and the zero-length rows of one encode_blobs call."""
    assert set(got) == set(want) == set(codes)
    bad = [(r, codes[r], want[r][1]) for r in sorted(want) if codes[r] != want[r][1]]
    assert not bad, f"{len(bad)} statuses differ, first (row, got, oracle) {bad[:5]}"
    bad = [r for r in sorted(want) if want[r][1] == 0 and got[r] != want[r][0]]
    assert not bad, f"{len(bad)} rows differ, first {bad[:5]}"
    enc = eng.encoded
    off = enc.row_off.astype(np.int64)
    assert len(off) == enc.n_rows + 1 and off[0] == 0 and off[-1] == len(enc.raw) and (np.diff(off) >= 0).all()
    empty = np.ones(enc.n_rows, bool)
    empty[sorted(want)] = False
    assert (np.diff(off)[empty] == 0).all(), "a row past an entry's count or of a failed entry has bytes"
    assert (enc.status[empty] == 0).all()
    ref, first = ee.oracle_offsets(want, enc.n_rows)
    assert off[:len(ref)].tolist() == ref, "row offsets up to the first failing row"


@pytest.mark.gpu
@pytest.mark.parametrize("form,table", FORMS)
def test_gpu_hand_made_variable(engine_gpu, form, table):
    hm = ee.hand_made()
    want = ee.expected(table, form)
    got, codes = engine_gpu.encode_blobs(hm.batch, hm.out, table, hm.T.strs, hm.persist, hm.T.cluster_names,
                                         form=form, fill=ee.FILL, guard=64)
    _check_rows(engine_gpu, hm.batch, hm.out, want, got, codes)


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["timer", "cancel"])
def test_gpu_hand_made_fixed(engine_gpu, table):
    """encode.hip: rows byte-identical; the slots of slack rows and failed entries keep the fill."""
    hm = ee.hand_made()
    want = ee.expected_rows(hm.batch, hm.out, table, "sql", hm.T.S)
    got = engine_gpu.encode_rows(hm.batch, hm.out, table, fill=ee.FILL)
    assert set(got) == set(want) and all(code == 0 for _, code in want.values())
    bad = [r for r in sorted(want) if got[r] != want[r][0]]
    assert not bad, f"{len(bad)} rows differ, first {bad[:5]}"
    enc = engine_gpu.encoded
    slots = np.frombuffer(enc.raw, np.uint8).reshape(enc.n_rows, enc.stride)
    untouched = np.ones(enc.n_rows, bool)
    untouched[sorted(want)] = False
    assert untouched.sum() > len(hm.failed) and (slots[untouched] == ee.FILL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("builder", [abi.BUILDER_LOCAL, abi.BUILDER_2DC, abi.BUILDER_NDC])
def test_gpu_replay_failed_entries_and_builders(engine_gpu, builder):
    """A real replay with failed entries under each builder (BUILDER_LOCAL among them) through
    the comparison code of test_encode_var.py / test_encode_cql.py."""
    b = engine.synth_batch(0, 300, seed=0x5EED0800 + builder, error_rate=0.1, builder=builder)
    out = engine_gpu.replay(b)
    n_failed = sum(out.result[w].code != abi.OK for w in range(b.n_wfs))
    n_forced = sum(out.result[w].code == abi.OK and b.wfs[w].builder == builder for w in range(b.n_wfs))
    assert n_failed > 0 and n_forced > 100, (n_failed, n_forced)
    assert check_variable_row_blobs(engine_gpu, b, out, nonempty=False) > 0
    assert check_cql_values(engine_gpu, b, out, nonempty=False) > 0


def _sparse_signals(n_rows_total=65_537):
    """Signal rows only: 1000 rows first, 1000 last, 0-3 rows in 3-row slices between; the
    capacity rows add up to n_rows_total."""
    T = ee.Strings()
    mid, rest = divmod(n_rows_total - 2000, 3)
    assert rest == 0
    counts = [1000] + [(0, 0, 1, 0, 0, 2, 0, 3)[w % 8] for w in range(mid)] + [1000]
    k, per_entry = 0, []
    for c in counts:
        per_entry.append({"signal": [ee.clean_row("signal", k + j, T) for j in range(c)]})
        k += c
    slack = lambda w: 0 if w in (0, len(counts) - 1) else 3 - counts[w]  # noqa: E731
    batch, out = make_state(per_entry, slack, tables=("signal",))
    return T, batch, out


@pytest.mark.gpu
def test_gpu_scan_across_tiles(engine_gpu):
    """Row offsets over many scan tiles.  hipcub::DeviceScan::ExclusiveSum forwards to
    rocprim::exclusive_scan, whose default config for 8-byte items has no gfx950 entry in
    rocprim/device/detail/config/device_scan.hpp and so is default_scan_config_base
    (device_config_helper.hpp): block size 256 x 16 / ceil(8 / 4) = 8 items per thread =
    2,048 items per tile (gfx942's tuned entry, 256 x 15 = 3,840, were it chosen).  The scan
    runs over n_rows + 1 = 65,538 items: 33 tiles of 2,048 (18 of 3,840), more than four
    either way.  Most tiles hold empty rows only."""
    tile = 256 * 15  # the larger of the two
    T, batch, out = _sparse_signals()
    n_rows = ee.n_capacity_rows(batch, out, "signal")
    assert n_rows == 65_537 and n_rows + 1 > 4 * tile
    assert out.result[0].n_signal == 1000 == out.result[batch.n_wfs - 1].n_signal
    for form in ("sql", "cql"):
        want = ee.expected_rows(batch, out, "signal", form, T.S)
        assert all(code == 0 for _, code in want.values())
        got, codes = engine_gpu.encode_blobs(batch, out, "signal", T.strs, form=form, fill=ee.FILL, guard=64)
        _check_rows(engine_gpu, batch, out, want, got, codes)
        ref, first = ee.oracle_offsets(want, n_rows)
        assert first == n_rows and engine_gpu.encoded.row_off.tolist() == ref


@pytest.mark.gpu
@pytest.mark.parametrize("form,table", [("sql", "signal"), ("sql", "exec"), ("cql", "act"), ("cql", "exec")])
def test_gpu_guards_repeats_nullable_status(engine_gpu, form, table):
    """The write pass inside a guarded buffer (engine.encode_blobs checks both 64-byte guards,
    so `blobs` points 64 bytes into its allocation); the same calls again give the same bytes;
    row_status == NULL changes neither the offsets nor the blobs."""
    hm = ee.hand_made()
    args = (hm.batch, hm.out, table, hm.T.strs, hm.persist, hm.T.cluster_names)
    runs = []
    for with_status in (True, True, False):
        got, codes = engine_gpu.encode_blobs(*args, form=form, fill=ee.FILL, guard=64, with_status=with_status)
        assert (codes == {}) == (not with_status)
        runs.append((got, engine_gpu.encoded.row_off.tolist(), engine_gpu.encoded.raw))
    assert runs[0] == runs[1], "repeated calls differ"
    assert runs[0][1] == runs[2][1] and runs[0][2] == runs[2][2], "row_status == NULL changes the output"
    assert runs[0][1][-1] == len(runs[0][2]) > 0


@pytest.mark.gpu
def test_gpu_argument_errors(engine_gpu):
    """Every documented argument check returns CDR_API_EINVAL before any launch.  All
    pointers that are passed are real, zeroed device allocations."""
    L, hip = abi.lib(), engine._hip()
    EINVAL = -1
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(1 << 16)) == 0
    try:
        assert hip.hipMemset(p, 0, C.c_size_t(1 << 16)) == 0
        dev = p.value

        def dbatch(n_wfs=0):
            db = abi.CdrDevBatch()
            db.n_wfs, db.caps, db.wfs = n_wfs, dev, dev
            return db

        def outs(**null):
            o = abi.CdrOut()
            for name in ("result", "exec", "repl", "vh", "act", "timer", "child", "cancel", "signal", "rp", "sa"):
                setattr(o, name, None if name in null else dev)
            return o

        def strtab(n=4):
            return abi.CdrStrtab(bytes=dev, off=dev, n=n)

        def var(fn, table, db=None, o=None, st="default", persist=dev, n_rows=0, row_off=dev):
            st = strtab() if st == "default" else st
            return getattr(L, fn)(engine_gpu.ctx, table, C.byref(db or dbatch()), C.byref(o or outs()),
                                  C.byref(st) if st is not None else None, persist, dev, n_rows, row_off, None, dev,
                                  None)
        for table in (1, 3, -1, 6):
            assert var("cdr_encode_blobs_async", table) == EINVAL, table
        for table in (-1, 6):
            assert var("cdr_encode_cql_async", table) == EINVAL, table
        for fn in ("cdr_encode_blobs_async", "cdr_encode_cql_async"):
            assert var(fn, 4, st=None) == EINVAL
            assert var(fn, 4, st=strtab(n=0)) == EINVAL
            assert var(fn, 4, row_off=None) == EINVAL
            assert var(fn, 5, db=dbatch(1), n_rows=0) == EINVAL  # n_rows < n_wfs
            assert var(fn, 5, persist=None) == EINVAL
            for table, name in ((0, "act"), (2, "child"), (4, "signal"), (5, "exec"), (5, "repl"), (5, "vh"), (5, "rp"),
                                (5, "sa")):
                assert var(fn, table, o=outs(**{name: 1})) == EINVAL, (fn, name)
            assert var(fn, 4, o=outs(result=1)) == EINVAL
        for table, name in ((1, "timer"), (3, "cancel")):
            assert var("cdr_encode_cql_async", table, o=outs(**{name: 1})) == EINVAL
            assert L.cdr_encode_rows_async(engine_gpu.ctx, table, C.byref(dbatch()), C.byref(outs(**{name: 1})), dev,
                                           None) == EINVAL
        assert L.cdr_encode_rows_async(engine_gpu.ctx, 0, C.byref(dbatch()), C.byref(outs()), dev, None) == EINVAL
        assert L.cdr_encode_rows_async(engine_gpu.ctx, 1, C.byref(dbatch()), C.byref(outs()), None, None) == EINVAL
        # the same arguments without the fault are accepted (n_wfs == 0: nothing is launched
        # for the rows; the scan covers the single total)
        assert var("cdr_encode_blobs_async", 4) == 0
        assert L.cdr_encode_rows_async(engine_gpu.ctx, 1, C.byref(dbatch()), C.byref(outs()), dev, None) == 0
    finally:
        hip.hipFree(p)
