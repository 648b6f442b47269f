"""Loading whole stored states on the device (cdr.h cdr_load_state, csrc/load.hip): the
execution row decoded with the five pending tables, checked against tests/exec_rows_ref.py.

CPU: the reference decoder inverts oracle/thrift_binary.py exec_info_blob on replayed states
of the synthetic configs 2-5 under all three builders (records byte for byte with
last_event_task_id zeroed and CDR_XI_STARTED set, blobs byte for byte after re-encoding), it
handles the hand-built wire edges the way the header states them, and the ABI mirrors match.
GPU (-m gpu): the device decoder == the reference record for record and status for status on
those states, on every size class, every wire edge, every truncation and a blob that claims to
run past the buffer; the string table is one handle space; the loaded state alone carries a
replay to the oracle's final states and goes back through the encoders to the input bytes.
"""
import ctypes as C
import dataclasses
import functools
import os
import random
import re
import struct

import numpy as np
import pytest

from cadence_amd import abi, engine, rows
from oracle import thrift_binary as tb
from oracle import thrift_decode as TD
from tests import exec_rows_ref as xref
from tests import rows_ref
from tests import thrift_cases as tc
from tests.thrift_cases import F, Raw, St

ZT = abi.ZERO_TIME_NANOS
U = b"0123abcd-89ef-4c5d-8a7b-fedcba987654"
ITEMS = ("vh", "rp", "sa")
CLUSTERS = [b"cluster-active", b"cluster-standby", b"cluster-third"]


def _copy(rec):
    return type(rec).from_buffer_copy(bytes(rec))


# ---------------------------------------------------------------- replayed states
@functools.lru_cache(maxsize=None)
def _state(cfg, builder):
    """(batch, oracle-replayed states with every handle renumbered densely, the table of
    distinct strings over those handles with the cluster names appended, persistence
    contexts, the cluster names' handles)."""
    import oracle
    b = engine.synth_batch(cfg, 300, seed=0x5EED0C00 + cfg, builder=builder)
    if cfg == 2:  # a finished config-2 workflow has no pending rows: its first half has
        b, _ = engine.cut_batches(b, engine.split_half(b))
    res = oracle.replay(b)
    out = engine.Outputs(b, res.plan)
    for name in ("result", "exec", "repl"):
        C.memmove(getattr(out, name), getattr(res, name), C.sizeof(getattr(res, name)))
    for t in engine.TABLES:
        C.memmove(out.tables[t], res.tables[t], C.sizeof(res.tables[t]))
    full = rows.whole_state_strings(b, out)
    fields = {**rows.HANDLES, **rows.ITEM_HANDLES}
    ok = [w for w in range(b.n_wfs) if out.result[w].code == abi.OK]
    used = {getattr(out.exec[w], f) for w in ok for f in rows.X_HANDLES}
    used |= {getattr(r, f) for w in ok for t in fields for r in out.rows(w, t) for f in fields[t]}
    used = sorted(used - {0})
    dense = {h: i + 1 for i, h in enumerate(used)}
    dense[0] = 0
    for w in ok:
        for f in rows.X_HANDLES:
            setattr(out.exec[w], f, dense[getattr(out.exec[w], f)])
        for t in fields:
            off = getattr(out.plan.caps[w], t + "_off")
            for j in range(getattr(out.result[w], engine.TABLE_COUNT[t])):
                for f in fields[t]:
                    setattr(out.tables[t][off + j], f, dense[getattr(out.tables[t][off + j], f)])
    strs = [b""] + [full[h] for h in used]
    names = list(range(len(strs), len(strs) + len(CLUSTERS)))
    strs += CLUSTERS
    assert len(set(strs)) == len(strs) and b.cluster.n_clusters <= len(CLUSTERS)
    n = len(strs)
    persist = (abi.CdrExecPersist * b.n_wfs)(*[abi.CdrExecPersist(
        start_version=w % 5 - 1, current_version=w % 7, start_time=1_600_000_000_000_000_000 + w,
        last_updated_time=ZT if w % 3 == 0 else 1_700_000_000_000_000_000 + w, history_size=1000 + w,
        sticky_s2s_timeout=(w % 11) - 2, execution_context=(w * 5) % n if w % 4 else 0, sticky_task_list=(w * 3) % n,
        client_library_version=w % min(13, n), client_feature_version=0, client_impl=(w * 7) % min(17, n))
        for w in range(b.n_wfs)])
    return b, out, strs, persist, names[:b.cluster.n_clusters]


def _sa_rows(out, w):
    """Entry w's search attributes as a stored map can hold them: a key's first position and
    last value (the synthetic Started events repeat keys, which no Go map does)."""
    last = {kv.key: kv.value for kv in out.rows(w, "sa")}
    return [(k, last[k]) for k in dict.fromkeys(kv.key for kv in out.rows(w, "sa"))]


def _as_written(b, out, persist, w):
    """Entry w's records as a load gives them back: what the row does not carry is at the
    loader's value — last_event_task_id 0 (never read), CDR_XI_STARTED set, and, as the writer
    drops them, the parent fields of an entry without a parent domain, a Memo flag without a
    Memo, branch fields no token carries, a replication state of another builder, a repeated
    search-attribute key; start / current version come back from the persistence context."""
    x, bld = _copy(out.exec[w]), b.wfs[w].builder
    x.last_event_task_id = 0
    x.flags |= abi.XI_STARTED
    x.search_attr_len = len(_sa_rows(out, w))
    if not x.parent_domain_id:
        x.parent_workflow_id, x.parent_run_id, x.initiated_id = 0, 0, abi.EMPTY_EVENT_ID
    if not x.memo:
        x.flags &= ~abi.XI_HAS_MEMO
    if bld == abi.BUILDER_NDC:
        x.flags &= ~abi.XI_HAS_BRANCH
    else:
        x.flags &= ~abi.XI_VH_BRANCH
    if not x.flags & (abi.XI_HAS_BRANCH | abi.XI_VH_BRANCH):
        x.branch_tree_id = x.branch_id_lo = x.branch_id_hi = 0
    repl = _copy(out.repl[w]) if bld == abi.BUILDER_2DC else abi.CdrReplState()
    if bld == abi.BUILDER_2DC:
        repl.start_version, repl.current_version = persist[w].start_version, persist[w].current_version
    return x, repl


def _oracle_blob(b, out, strs, persist, names, w, x=None, distinct=False):
    """The oracle writer's execution row of entry w (`distinct`: of its distinct search
    attributes; x: another exec record)."""
    S = tb.lookup(strs)
    sa = _sa_rows(out, w) if distinct else [(kv.key, kv.value) for kv in out.rows(w, "sa")]
    return tb.exec_info_blob(x if x is not None else out.exec[w], b.wfs[w].builder, S, persist[w], repl=out.repl[w],
                             vh_items=[(v.event_id, v.version) for v in out.rows(w, "vh")],
                             rps=[(p, S) for p in out.rows(w, "rp")],
                             sa=sa, cluster_names=names)


def _columns(out, strs, w):
    x = out.exec[w]
    return (rows.uuid_bytes(strs[x.domain_id]), rows.uuid_bytes(strs[x.run_id]), strs[x.workflow_id], x.next_event_id,
            out.repl[w].last_write_version)


def _check_against_state(b, out, persist, get):
    """The decoded records hold the states' own.  get(w) -> (exec, repl, persist, builder, vh
    items, reset points, search attributes) as record bytes / lists of record bytes."""
    n = 0
    for w in range(b.n_wfs):
        if out.result[w].code != abi.OK:
            continue
        x, repl = _as_written(b, out, persist, w)
        gx, gr, gp, gb, gvh, grp, gsa = get(w)
        assert gx == bytes(x), (w, [f for f, *_ in abi.CdrExecInfo._fields_
                                    if getattr(abi.CdrExecInfo.from_buffer_copy(gx), f) != getattr(x, f)])
        assert gr == bytes(repl) and gp == bytes(persist[w]) and gb == b.wfs[w].builder, w
        assert gvh == [bytes(r) for r in out.rows(w, "vh")] and grp == [bytes(r) for r in out.rows(w, "rp")], w
        assert gsa == [bytes(abi.CdrKV(key=k, value=v)) for k, v in _sa_rows(out, w)], w
        n += 1
    return n


# ---------------------------------------------------------------- CPU
COVERED = set()  # what the replayed states exercised, over all configs and builders


@pytest.mark.parametrize("builder", [abi.BUILDER_LOCAL, abi.BUILDER_2DC, abi.BUILDER_NDC])
@pytest.mark.parametrize("cfg", [2, 3, 4, 5])
def test_reference_round_trip(cfg, builder):
    b, out, strs, persist, names = _state(cfg, builder)
    H = {s: h for h, s in enumerate(strs)}
    S = tb.lookup(strs)
    clusters = [strs[h] for h in names]
    seen = {"parent": 0, "memo": 0, "rp": 0, "sa": 0, "vh": 0, "lri": 0}

    def get(w):
        blob = _oracle_blob(b, out, strs, persist, names, w)
        d, r, wid, nxt, lwv = _columns(out, strs, w)
        col = xref.SimpleNamespace(domain_id=d, run_id=r, workflow_id=wid, next_event_id=nxt, last_write_version=lwv)
        p = xref.parse_exec(blob, 0, len(blob), col, clusters)
        for f, s in p.xs.items():
            setattr(p.x, f, H[s])
        for f, s in p.pss.items():
            setattr(p.ps, f, H[s])
        rps = []
        for rp, c, run in p.rps:
            rp.binary_checksum, rp.run_id = H[c], H[run]
            rps.append(rp)
        sa = [abi.CdrKV(key=H[k], value=H[v]) for k, v in p.sa]
        for k, hit in (("parent", p.x.parent_domain_id), ("memo", p.x.memo), ("rp", rps), ("sa", sa), ("vh", p.vh),
                       ("lri", p.repl.lri_mask)):
            seen[k] += 1 if hit else 0
        # re-encoding the decoded records gives the input bytes back, apart from field 48
        x0 = _copy(out.exec[w])
        x0.last_event_task_id = 0
        again = tb.exec_info_blob(p.x, p.builder, S, p.ps, repl=p.repl, vh_items=p.vh, rps=[(rp, S) for rp in rps],
                                  sa=[(kv.key, kv.value) for kv in sa], cluster_names=names)
        assert again == _oracle_blob(b, out, strs, persist, names, w, x0, distinct=True), w
        assert p.n_sa_wire == len(out.rows(w, "sa")) and sum(len(s) for s in p.gen) == 36 * (2 + bool(p.x.parent_domain_id) + bool(
            p.x.parent_run_id)) + len(strs[p.x.memo])
        return (bytes(p.x), bytes(p.repl), bytes(p.ps), p.builder, [struct.pack("<qq", *i) for i in p.vh],
                [bytes(r) for r in rps], [bytes(kv) for kv in sa])
    assert _check_against_state(b, out, persist, get) > 100
    builders = {b.wfs[w].builder for w in range(b.n_wfs) if out.result[w].code == abi.OK}  # (config 4 mixes them)
    assert builder in builders and seen["rp"] and seen["sa"], seen
    assert (seen["vh"] > 0) == (abi.BUILDER_NDC in builders) and (abi.BUILDER_2DC in builders or not seen["lri"]), seen
    COVERED.update(k for k, n in seen.items() if n)


def test_replayed_states_cover_the_row():
    for cfg in (2, 3, 4, 5):
        for builder in (abi.BUILDER_LOCAL, abi.BUILDER_2DC, abi.BUILDER_NDC):
            test_reference_round_trip(cfg, builder)
    assert COVERED == {"parent", "memo", "rp", "sa", "vh", "lri"}


def _token(tree=b"tree-0", bid=U, ancestors=()):
    return tb.PREAMBLE + tc.value(tc.T_STRUCT, St("HistoryBranch", [
        tc.s(10, tree), tc.s(20, bid), tc.lst(30, tc.T_STRUCT, list(ancestors))]))


def _points(n, v=0):
    pts = [tc.reset_point(b"cks-%d-%d" % (v, k), b"0000%04d-aaaa-4bbb-8ccc-%012d" % (v, k % 3), k) for k in range(n)]
    return tb.PREAMBLE + tc.value(tc.T_STRUCT, St("ResetPoints", [tc.lst(10, tc.T_STRUCT, pts)]))


def _history(token, items):
    return St("VersionHistory", [tc.s(10, token), tc.lst(20, tc.T_STRUCT, [
        St("Item", [tc.i64(10, e), tc.i64(20, ver)]) for e, ver in items])])


def _histories(token=None, n_items=3, index=0, n_hist=1, v=0):
    token = _token(b"vh-tree-%d" % v) if token is None else token
    hs = [_history(token, [(4 * k + 3 + v, k + 1) for k in range(n_items)]) for _ in range(n_hist)]
    return tb.PREAMBLE + tc.value(tc.T_STRUCT, St("VersionHistories", [tc.i32(10, index), tc.lst(20, tc.T_STRUCT, hs)]))


def _lri(pairs):
    return tc.mp(46, tc.T_STRING, tc.T_STRUCT, [(k, St("ReplicationInfo", [tc.i64(10, ver), tc.i64(12, ev)]))
                                                for k, ver, ev in pairs])


def _x_fields(kind="local", v=0, n_rp=2, sa=((b"k1", b"v1"), (b"k2", b"v2")), memo=((b"mk", b"mv"),), n_items=3):
    """The execution row's struct with every IDL field set (values vary with v)."""
    s, i32, i64, bl = tc.s, tc.i32, tc.i64, tc.boolean
    f = [s(10, bytes(range(16 + v, 32 + v))), s(12, b"parent-wf-%d" % v), s(14, bytes(range(64 + v, 80 + v))), i64(16, 33 + v),
         i64(18, 90 + v), s(20, b"completion-event"), s(22, b"thriftrw"), s(24, b"tl-%d" % v), s(26, b"type-%d" % v),
         i32(28, 3600 + v), i32(30, 10 + v), s(32, b"context-%d" % v), i32(34, 1 + v), i32(36, v), i64(38, 5 + v), i64(40, 7 + v)]
    if kind == "2dc":
        f += [i64(44, 41 + v), _lri([(CLUSTERS[0], 3 + v, 30), (CLUSTERS[2], 4 + v, 40)])]
    f += [i64(48, 777), i64(50, 88 + v), i64(52, 80 + v), i64(54, 10**18 + v), i64(56, 10**18 + 9 + v), i64(58, 6 + v),
          i64(60, 91 + v), i64(62, 92 + v), i32(64, 15 + v), i64(66, 2 + v), i64(68, 10**18 + 3), i64(69, 10**18 + 2),
          bl(70, v == 0), i64(71, 10**18 + 1), s(72, b"create-req-%d" % v), s(74, b"decision-req-%d" % v), s(76, b"cancel-req"),
          s(78, b"sticky-%d" % v), i64(80, (1 << 32) + 25 + v), i64(82, (1 << 33) + 3 + v), i32(84, 1 + v), i32(86, 60 + v),
          i32(88, 4 + v), i32(90, 600 + v), F(tc.T_DOUBLE, 92, 1.5 + v), i64(94, 2 * 10**18 + v),
          tc.lst(96, tc.T_STRING, [b"bad", b"e%d" % v]), bl(98, True), s(100, b"* * * * %d" % v)]
    if kind != "ndc":
        f.append(s(104, _token(b"tree-%d" % v)))
    f += [i64(106, (1 << 32) - 2 - v), i64(108, 5000 + v), s(110, b"lib-%d" % v), s(112, b"feat-%d" % v), s(114, b"impl-%d" % v),
          s(115, _points(n_rp, v)), s(116, b"thriftrw")]
    if sa is not None:
        f.append(tc.mp(118, tc.T_STRING, tc.T_STRING, list(sa)))
    if memo is not None:
        f.append(tc.mp(120, tc.T_STRING, tc.T_STRING, list(memo)))
    if kind == "ndc":
        f += [s(122, _histories(n_items=n_items, v=v)), s(124, b"thriftrw")]
    return f


def _blob(fields) -> bytes:
    return tc.value(tc.T_STRUCT, St("row", fields))


def _with(fields, **by_fid):
    """The fields with those of id f<N> replaced (None: removed; a list: several in its place)."""
    out = []
    for f in fields:
        key = "f%d" % f.fid
        if key not in by_fid:
            out.append(f)
        elif by_fid[key] is not None:
            out += by_fid[key] if isinstance(by_fid[key], list) else [by_fid[key]]
    return out


def _wrong(f):
    return F(tc.T_STRING, f.fid, b"zz") if f.t != tc.T_STRING else F(tc.T_I64, f.fid, 5)


@functools.lru_cache(maxsize=None)
def wire_cases():
    """[(name, blob, expected)]: expected is a status, or the plain blob whose decode the edge
    blob's must equal."""
    s = tc.s
    cases = []
    for kind in ("local", "2dc", "ndc"):
        base = _x_fields(kind)
        plain = _blob(base)
        cases.append((f"{kind} plain", plain, plain))
        cases.append((f"{kind} reversed order", _blob(base[::-1]), plain))
        sh = list(base)
        random.Random(31).shuffle(sh)
        cases.append((f"{kind} shuffled order", _blob(sh), plain))
        unk = [F(ty, 900 + k, v) for k, (_, ty, v) in enumerate(tc.unknown_values())]
        cases.append((f"{kind} unknown fields", _blob(unk + base + unk), plain))
        cases.append((f"{kind} wrong types after", _blob(base + [_wrong(f) for f in base]), plain))
        cases.append((f"{kind} wrong types before", _blob([_wrong(f) for f in base] + base), plain))
        cases.append((f"{kind} repeated fields", _blob(base + _x_fields(kind, 1)), _blob(_x_fields(kind, 1))))
        cases.append((f"{kind} trailing bytes", plain + b"\x0b\x00\x0a\xff\xff", plain))
        cases.append((f"{kind} no stop byte", plain[:-1], TD.DEC_TRUNCATED))
    base = _x_fields("local")
    plain = _blob(base)
    ndc = _x_fields("ndc")
    cases.append(("every optional field absent", b"\x00", b"\x00"))
    cases.append(("empty blob", b"", TD.DEC_TRUNCATED))
    for kind in ("struct", "list", "map"):
        for levels, want in ((TD.MAX_DEPTH, plain), (TD.MAX_DEPTH + 1, TD.DEC_DEPTH)):
            ty, v = tc.nested(kind, levels)
            cases.append((f"{kind} depth {levels}", _blob(base[:2] + [F(ty, 901, v)] + base[2:]), want))
    cases.append(("negative string length", _blob(base + [F(tc.T_STRING, 902, Raw(struct.pack(">i", -1)))]), TD.DEC_BAD_SIZE))
    cases.append(("wire type 9", _blob(base[:1] + [F(9, 905, Raw(b"\0\0"))] + base[1:]), TD.DEC_BAD_TYPE))
    # builders and shapes
    cases.append(("fields 44 and 122", _blob(_x_fields("2dc") + ndc[-2:]), abi.LOAD_E_SHAPE))
    cases.append(("field 104 and a version-history token", _blob(ndc + [s(104, _token())]), abi.LOAD_E_SHAPE))
    cases.append(("field 104 and an empty version-history token",
                  _blob(_with(ndc, f122=s(122, _histories(token=b""))) + [s(104, _token(b"vh-tree-0"))]),
                  _blob(_with(ndc, f122=s(122, _histories(token=b""))) + [s(104, _token(b"vh-tree-0"))])))
    cases.append(("two histories", _blob(_with(ndc, f122=s(122, _histories(n_hist=2)))), abi.LOAD_E_SHAPE))
    cases.append(("no history", _blob(_with(ndc, f122=s(122, _histories(n_hist=0)))), abi.LOAD_E_SHAPE))
    cases.append(("index 1", _blob(_with(ndc, f122=s(122, _histories(index=1)))), abi.LOAD_E_SHAPE))
    anc = [St("HistoryBranchRange", [s(10, b"branch"), tc.i64(20, 1), tc.i64(30, 5)])]
    cases.append(("ancestors in field 104", _blob(_with(base, f104=s(104, _token(ancestors=anc)))), abi.LOAD_E_SHAPE))
    cases.append(("ancestors in the version-history token",
                  _blob(_with(ndc, f122=s(122, _histories(token=_token(ancestors=anc))))), abi.LOAD_E_SHAPE))
    # encodings and preambles
    for fid, enc, src in ((115, 116, base), (122, 124, ndc)):
        blob = next(f.v for f in src if f.fid == fid)
        cases.append((f"encoding json on {fid}", _blob(_with(src, **{"f%d" % enc: s(enc, b"json")})), abi.LOAD_E_ENCODING))
        cases.append((f"encoding absent on {fid}", _blob(_with(src, **{"f%d" % enc: None})), abi.LOAD_E_ENCODING))
        cases.append((f"no preamble on {fid}", _blob(_with(src, **{"f%d" % fid: s(fid, blob[1:])})), abi.LOAD_E_ENCODING))
        cases.append((f"{fid} truncated inside", _blob(_with(src, **{"f%d" % fid: s(fid, blob[:-3])})), TD.DEC_TRUNCATED))
        cases.append((f"{fid} with trailing bytes", _blob(_with(src, **{"f%d" % fid: s(fid, blob + b"\x0b\xff")})), _blob(src)))
    cases.append(("empty 115 with a json encoding", _blob(_with(base, f115=s(115, b""), f116=s(116, b"json"))),
                  _blob(_with(base, f115=None))))
    cases.append(("reset points without Points", _blob(_with(base, f115=s(115, tb.PREAMBLE + b"\x00"))),
                  _blob(_with(base, f115=s(115, tb.PREAMBLE + b"\x00")))))
    cases.append(("empty 122", _blob(_with(ndc, f122=s(122, b""))), abi.LOAD_E_ENCODING))
    cases.append(("empty 104", _blob(_with(base, f104=s(104, b""))), abi.LOAD_E_ENCODING))
    cases.append(("no preamble on 104", _blob(_with(base, f104=s(104, _token()[1:]))), abi.LOAD_E_ENCODING))
    cases.append(("104 truncated inside", _blob(_with(base, f104=s(104, _token()[:-2]))), TD.DEC_TRUNCATED))
    for name, text in (("uppercase", U.upper()), ("32 hex", U.replace(b"-", b"")), ("empty", b""), ("37 chars", U + b"0")):
        cases.append((f"BranchID {name}", _blob(_with(base, f104=s(104, _token(bid=text)))), abi.LOAD_E_UUID))
        cases.append((f"version-history BranchID {name}",
                      _blob(_with(ndc, f122=s(122, _histories(token=_token(bid=text))))), abi.LOAD_E_UUID))
    # parent IDs
    for fid in (10, 14):
        for n, want in ((0, None), (15, abi.LOAD_E_UUID), (16, None), (17, abi.LOAD_E_UUID)):
            blob = _blob(_with(base, **{"f%d" % fid: s(fid, bytes(range(100, 100 + n)))}))
            cases.append((f"field {fid} of {n} bytes", blob, blob if want is None else want))
    cases.append(("parent fields without field 10", _blob(_with(base, f10=None)), _blob(_with(base, f10=None, f12=None, f14=None, f16=None))))
    cases.append(("a bad parent run ID without field 10", _blob(_with(base, f10=None, f14=s(14, b"short"))),
                  _blob(_with(base, f10=None, f12=None, f14=None, f16=None))))
    # clusters and maps
    two = _x_fields("2dc")
    cases.append(("unknown cluster", _blob(_with(two, f46=_lri([(CLUSTERS[0], 1, 2), (b"cluster-nowhere", 3, 4)]))), abi.LOAD_E_CLUSTER))
    cases.append(("empty cluster name", _blob(_with(two, f46=_lri([(b"", 1, 2)]))), abi.LOAD_E_CLUSTER))
    cases.append(("repeated cluster", _blob(_with(two, f46=_lri([(CLUSTERS[1], 1, 2), (CLUSTERS[0], 5, 6), (CLUSTERS[1], 3, 4)]))),
                  _blob(_with(two, f46=_lri([(CLUSTERS[0], 5, 6), (CLUSTERS[1], 3, 4)])))))
    cases.append(("replication info of another value type", _blob(_with(two, f46=tc.mp(46, tc.T_STRING, tc.T_I64, [(b"x", 1)]))),
                  _blob(_with(two, f46=None))))
    cases.append(("field 46 without field 44", _blob(base + [_lri([(b"cluster-nowhere", 3, 4)])]), plain))
    cases.append(("repeated map key", _blob(_x_fields(sa=((b"k1", b"a"), (b"k2", b"b"), (b"k1", b"c"), (b"", b"d"), (b"", b"")))),
                  _blob(_x_fields(sa=((b"k1", b"c"), (b"k2", b"b"), (b"", b""))))))
    cases.append(("search attributes of another value type", _blob(_with(base, f118=tc.mp(118, tc.T_STRING, tc.T_I64, [(b"k", 1)]))),
                  _blob(_x_fields(sa=()))))
    cases.append(("empty maps", _blob(_x_fields(sa=(), memo=())), _blob(_x_fields(sa=(), memo=()))))
    cases.append(("no maps", _blob(_x_fields(sa=None, memo=None)), _blob(_x_fields(sa=None, memo=None))))
    cases.append(("empty error list", _blob(_with(base, f96=tc.lst(96, tc.T_STRING, []))), _blob(_with(base, f96=None))))
    cases.append(("error list of i64", _blob(_with(base, f96=tc.lst(96, tc.T_I64, [1, 2]))), _blob(_with(base, f96=None))))
    cases.append(("zero expiration time", _blob(_with(base, f94=tc.i64(94, ZT))), _blob(_with(base, f94=tc.i64(94, ZT)))))
    cases.append(("expiration time absent", _blob(_with(base, f94=None)), _blob(_with(base, f94=tc.i64(94, 0)))))
    # the bounds
    for name, at, over in (("reset points", _x_fields(n_rp=abi.LOAD_MAX_RESET_POINTS), _x_fields(n_rp=abi.LOAD_MAX_RESET_POINTS + 1)),
                           ("search attributes", _x_fields(sa=[(b"k%d" % k, b"v") for k in range(abi.LOAD_MAX_SEARCH_ATTR)]),
                            _x_fields(sa=[(b"k", b"v")] * (abi.LOAD_MAX_SEARCH_ATTR + 1))),
                           ("version-history items", _x_fields("ndc", n_items=abi.LOAD_MAX_VH_ITEMS),
                            _x_fields("ndc", n_items=abi.LOAD_MAX_VH_ITEMS + 1))):
        cases.append((f"{name} at the bound", _blob(at), _blob(at)))
        cases.append((f"{name} over the bound", _blob(over), abi.LOAD_E_SHAPE))
    return cases


COL = xref.SimpleNamespace(domain_id=bytes(range(16)), run_id=bytes(range(240, 256)), workflow_id=b"workflow-7",
                           next_event_id=101, last_write_version=55)


def _one(blob):
    return xref.parse_exec(blob, 0, len(blob), COL, CLUSTERS)


def _same(a, b):
    return (bytes(a.x), a.xs, bytes(a.ps), a.pss, bytes(a.repl), a.builder, a.vh, a.sa,
            [(bytes(r), c, u) for r, c, u in a.rps]) == \
        (bytes(b.x), b.xs, bytes(b.ps), b.pss, bytes(b.repl), b.builder, b.vh, b.sa, [(bytes(r), c, u) for r, c, u in b.rps])


def test_reference_wire_edges():
    seen = set()
    for name, blob, want in wire_cases():
        if isinstance(want, int):
            with pytest.raises((TD.DecodeError, xref.RowError)) as e:
                _one(blob)
            assert e.value.code == want, name
            seen.add(want)
        else:
            assert _same(_one(blob), _one(want)), name
    assert seen == {TD.DEC_TRUNCATED, TD.DEC_DEPTH, TD.DEC_BAD_SIZE, TD.DEC_BAD_TYPE, abi.LOAD_E_UUID, abi.LOAD_E_ENCODING,
                    abi.LOAD_E_SHAPE, abi.LOAD_E_CLUSTER}
    # what the plain blobs decode to, spelled out once
    p = _one(_blob(_x_fields("2dc")))
    x = p.x
    assert p.xs["domain_id"] == b"00010203-0405-0607-0809-0a0b0c0d0e0f" and p.xs["workflow_id"] == b"workflow-7"
    assert p.xs["parent_domain_id"] == b"10111213-1415-1617-1819-1a1b1c1d1e1f" and p.xs["parent_workflow_id"] == b"parent-wf-0"
    assert (x.initiated_id, x.completion_event_batch_id, x.next_event_id, x.last_event_task_id) == (33, 90, 101, 0)
    assert (x.attempt, x.signal_count, p.ps.sticky_s2s_timeout) == (3, -2, 25)  # the low 32 bits
    assert x.flags == (abi.XI_CANCEL_REQUESTED | abi.XI_HAS_RETRY | abi.XI_HAS_EXPIRATION | abi.XI_HAS_BRANCH | abi.XI_HAS_MEMO |
                       abi.XI_HAS_SEARCH_ATTR | abi.XI_HAS_RESET_POINTS | abi.XI_STARTED)
    assert (x.backoff_coefficient, x.expiration_time, x.branch_id_hi, x.branch_id_lo) == (1.5, 2 * 10**18, 0x0123abcd89ef4c5d,
                                                                                         0x8a7bfedcba987654)
    assert p.xs["memo"] == b"\x0d\x00\x0a\x0b\x0b\0\0\0\x01\0\0\0\x02mk\0\0\0\x02mv\x00" and p.xs["branch_tree_id"] == b"tree-0"
    assert p.xs["nonretriable"] == struct.pack(">bi", 11, 2) + b"\0\0\0\x03bad\0\0\0\x02e0"
    r = p.repl
    assert (p.builder, r.present, r.start_version, r.current_version, r.last_write_version, r.last_write_event_id) == (
        abi.BUILDER_2DC, 1, 5, 7, 55, 41)
    assert (r.lri_mask, r.lri_version[0], r.lri_last_event_id[2], r.lri_version[1]) == (0b101, 3, 40, 0)
    assert len(p.rps) == 2 and p.rps[1][0].flags == 0x3F and p.sa == [(b"k1", b"v1"), (b"k2", b"v2")]
    p = _one(_blob(_x_fields("ndc")))
    assert p.builder == abi.BUILDER_NDC and p.vh == [(3, 1), (7, 2), (11, 3)] and bytes(p.repl) == bytes(abi.CdrReplState())
    assert p.x.flags & (abi.XI_VH_BRANCH | abi.XI_HAS_BRANCH) == abi.XI_VH_BRANCH and p.xs["branch_tree_id"] == b"vh-tree-0"
    p = _one(b"\x00")
    assert (p.x.flags, p.x.completion_event_batch_id, p.builder) == (abi.XI_STARTED | abi.XI_HAS_EXPIRATION, abi.EMPTY_EVENT_ID,
                                                                     abi.BUILDER_LOCAL)
    assert p.x.initiated_id == abi.EMPTY_EVENT_ID and p.xs["parent_domain_id"] == b""
    assert p.gen == [b"00010203-0405-0607-0809-0a0b0c0d0e0f", b"f0f1f2f3-f4f5-f6f7-f8f9-fafbfcfdfeff"]


def test_abi_mirrors():
    L = abi.lib()
    assert L.cdr_struct_size(b"cdr_exec_rows_in") == C.sizeof(abi.CdrExecRowsIn) == 88
    assert L.cdr_struct_size(b"cdr_state_out") == C.sizeof(abi.CdrStateOut) == 296 + 24
    assert (abi.CdrExecRowsIn.cluster_seed.offset, abi.CdrExecRowsIn.n_clusters.offset) == (48, 80)
    assert (abi.CdrStateOut.rows.offset, abi.CdrStateOut.persist.offset, abi.CdrStateOut.exec_status.offset) == (0, 296, 312)
    assert hasattr(L, "cdr_load_state")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "cdr", "cdr.h")).read()
    for name, value in (("E_ENCODING", abi.LOAD_E_ENCODING), ("E_SHAPE", abi.LOAD_E_SHAPE), ("E_CLUSTER", abi.LOAD_E_CLUSTER)):
        assert int(re.search(r"#define CDR_LOAD_%s (\d+)" % name, hdr).group(1)) == value
    assert (abi.LOAD_E_ENTRY_ROWS, abi.LOAD_E_ENCODING, abi.LOAD_E_SHAPE, abi.LOAD_E_CLUSTER) == (18, 19, 20, 21)
    for name, value in (("VH_ITEMS", abi.LOAD_MAX_VH_ITEMS), ("RESET_POINTS", abi.LOAD_MAX_RESET_POINTS),
                        ("SEARCH_ATTR", abi.LOAD_MAX_SEARCH_ATTR)):
        assert int(re.search(r"#define CDR_LOAD_MAX_%s (\d+)u" % name, hdr).group(1)) == value
    assert "execution row stays with the caller" not in " ".join(hdr.replace("*", " ").split())


# ---------------------------------------------------------------- GPU
SEEDS = [b""] + CLUSTERS + [b"tl-0", b"no such string"]
CSEED = [1, 2, 3]


def _assert_equal(got, R, seeds):
    want = xref.decode_state(R, seeds)
    bad = xref.compare_state(got, want, R)
    assert not bad, "\n".join(bad[:10])
    return want


def _entries(blobs, pending=None, cols=None):
    """One entry per execution blob (no pending rows unless given): a Rows."""
    n = len(blobs)
    tabs = pending or [[[] for _ in range(n)] for _ in range(5)]
    xr = [(blob, bytes((w * 7 + i) & 0xFF for i in range(16)), bytes((w * 13 + 5 * i) & 0xFF for i in range(16)),
           b"workflow-%d" % (w % 50), 100 + w, 50 + w) for w, blob in enumerate(blobs)]
    for w, c in (cols or {}).items():
        xr[w] = (xr[w][0],) + tuple(c)
    return rows.pack(n, tabs, xr, CSEED)


@pytest.mark.gpu
@pytest.mark.parametrize("builder", [abi.BUILDER_LOCAL, abi.BUILDER_2DC, abi.BUILDER_NDC])
@pytest.mark.parametrize("cfg", [2, 3, 4, 5])
def test_gpu_round_trip(engine_gpu, cfg, builder):
    """Device-encoded rows of replayed states -> load_state == the reference and the states' own
    records; the gathered string table and the loaded state go back through the table-5 encoder
    to the input bytes, apart from field 48."""
    b, out, strs, persist, names = _state(cfg, builder)
    R = rows.encode_state(engine_gpu, b, out, strs, exec_rows=True, persist=persist, cluster_names=names)
    ok = [w for w in range(b.n_wfs) if out.result[w].code == abi.OK]
    for w in ok[:40]:
        assert R.bytes[int(R.exec.blob_off[w]):int(R.exec.blob_off[w + 1])].tobytes() == \
            _oracle_blob(b, out, strs, persist, names, w), w
    got = rows.load_state(engine_gpu, R, strs)  # seeds = the whole table: every handle kept
    _assert_equal(got, R, strs)
    assert got.strings == strs and got.n_bad_entries == b.n_wfs - len(ok)
    size = {t: C.sizeof(engine.TABLE_TYPES[t]) for t in ITEMS}
    raw = {t: bytes(got.tables[t]) for t in ITEMS}

    def get(w):
        c, r = got.caps[w], got.result[w]
        items = [[raw[t][(getattr(c, t + "_off") + j) * size[t]:(getattr(c, t + "_off") + j + 1) * size[t]]
                  for j in range(getattr(r, engine.TABLE_COUNT[t]))] for t in ITEMS]
        return (bytes(got.exec[w]), bytes(got.repl[w]), bytes(got.persist[w]), int(got.builder[w]), *items)
    assert _check_against_state(b, out, persist, get) == len(ok) > 100
    # most strings new: other handles, the same bytes
    seeds = strs[:len(strs) // 3] + CLUSTERS
    cs = [len(seeds) - len(CLUSTERS) + i for i in range(len(names))]
    R = dataclasses.replace(R, exec=dataclasses.replace(R.exec, cluster_seed=cs))
    got = rows.load_state(engine_gpu, R, seeds, gather=True)
    _assert_equal(got, R, seeds)
    assert got.gathered == got.strings and set(got.strings) == set(strs)
    state = rows.to_carry(got).state
    back, codes = engine_gpu.encode_blobs(b, state, "exec", got.gathered, got.persist,
                                          [got.strings.index(strs[h]) for h in names])
    for w in ok:
        x0 = _copy(out.exec[w])
        x0.last_event_task_id = 0
        assert codes[w] == 0 and back[w] == _oracle_blob(b, out, strs, persist, names, w, x0, distinct=True), w


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [3, 5])
def test_gpu_loaded_state_alone_carries_a_replay(engine_gpu, cfg):
    """Prefix replay -> encode_state -> load_state -> to_carry with nothing else -> suffix
    replay == the oracle's replay of the whole histories; the mutation and the encoders on the
    result produce blobs that parse."""
    import oracle
    from tests import mutation_ref
    b = engine.synth_batch(cfg, 300, seed=0x5EED0D00 + cfg)
    cut = engine.split_half(b)
    pre, suf = engine.cut_batches(b, cut)
    pre_out = engine_gpu.replay(pre)
    n_cl = b.cluster.n_clusters
    strs = rows.whole_state_strings(pre, pre_out, extra=n_cl)
    names = list(range(len(strs) - n_cl, len(strs)))
    R = rows.encode_state(engine_gpu, pre, pre_out, strs, exec_rows=True, cluster_names=names)
    got = rows.load_state(engine_gpu, R, strs)
    assert got.strings == strs
    ok = np.array([pre_out.result[w].code == abi.OK for w in range(b.n_wfs)])
    assert [int(s) == 0 for s in got.entry_status] == ok.tolist()
    assert {int(got.builder[w]) for w in range(b.n_wfs) if ok[w]} == {pre.wfs[w].builder for w in range(b.n_wfs) if ok[w]}
    # the synthetic Started events now and then repeat a search-attribute key, which the replay
    # keeps as two rows and no stored map can hold (the load keeps one): those entries replay whole
    storable = np.array([len({kv.key for kv in pre_out.rows(w, "sa")}) == pre_out.result[w].n_search_attr
                         for w in range(b.n_wfs)])
    assert (~storable).sum() < 15
    src = np.where((cut > 0) & ok & storable, np.arange(b.n_wfs), -1)
    cut = np.where(storable, cut, 0)
    pre, suf = engine.cut_batches(b, cut)
    suf.carry = rows.to_carry(got, src=src)
    out = engine_gpu.replay(suf)
    whole = oracle.replay(b)
    bad = engine.compare(b, out, whole)
    assert not bad, bad[:5]
    assert sum(1 for w in range(b.n_wfs) if whole.result[w].code == abi.OK and src[w] >= 0) > 100
    mut = engine_gpu.mutation(suf, out)
    bad = mutation_ref.check(suf, out, mut)
    assert not bad, "\n".join(bad[:10])
    strs2 = rows.whole_state_strings(suf, out, extra=n_cl)
    names2 = list(range(len(strs2) - n_cl, len(strs2)))
    blobs, codes = engine_gpu.encode_blobs(suf, mut.upsert, "exec", strs2, (abi.CdrExecPersist * b.n_wfs)(), names2)
    n = 0
    for w, blob in blobs.items():
        if codes[w] == 0:
            p = xref.parse_exec(blob, 0, len(blob), COL, [strs2[h] for h in names2])
            assert p.builder == suf.wfs[w].builder and p.x.state == out.exec[w].state, w
            n += 1
    assert n > 100
    acts, codes = engine_gpu.encode_blobs(suf, mut.upsert, "act", strs2)
    for r, blob in acts.items():
        if codes[r] == 0:
            rows_ref.parse_row(0, blob, 0, len(blob), 1)


def _varied(w):
    """A row whose item counts, builder and values vary with w."""
    kind = ("local", "2dc", "ndc")[w % 3]
    return _blob(_x_fields(kind, w % 5, n_rp=w % 4, sa=[(b"key-%d" % k, b"value-%d" % (w + k)) for k in range(w % 3)],
                           memo=[(b"m", b"%d" % w)] if w % 2 else None, n_items=w % 6))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_gpu_entry_counts(engine_gpu, n):
    R = _entries([_varied(w) for w in range(n)])
    got = rows.load_state(engine_gpu, R, SEEDS)
    want = _assert_equal(got, R, SEEDS)
    assert not any(want.entry_status) and len(got.result) == n


def _sized(size, w):
    """A short row (a few of the fields) padded to exactly `size` bytes."""
    f = [x for x in _x_fields("local", w % 3, n_rp=0, sa=None, memo=None) if x.fid in (18, 24, 26, 34, 50, 72, 82, 98, 115, 116)]
    pad = size - len(_blob(f)) - 7
    assert pad >= 0
    blob = _blob(f + [tc.s(950, b"p" * pad)])
    assert len(blob) == size
    return blob


@pytest.mark.gpu
def test_gpu_sizes(engine_gpu):
    """Item counts on both sides of a wavefront and of the register-table bounds, Memo sizes up
    to one value past 64 KiB, rows a byte below / at / above a lane's share of the LDS stage
    (waves that fit it exactly, by a byte, and not), and an entry over each bound."""
    blobs = []
    for n_items in (0, 1, 64, 65, 1000):
        blobs.append(_blob(_x_fields("ndc", n_items=n_items)))
    for n_rp in (0, 1, 12, 13):
        blobs.append(_blob(_x_fields("local", 1, n_rp=n_rp)))
    for n_sa in (0, 1, 8, 9):
        blobs.append(_blob(_x_fields("2dc", 2, sa=[(b"k-%d" % k, b"v-%d" % k) for k in range(n_sa)])))
    big = len(blobs) + 2
    for memo in ((), ((b"a", b"1"), (b"b", b"2"), (b"c", b"3")), ((b"big", bytes(range(256)) * 273 + b"x" * 113),)):
        blobs.append(_blob(_x_fields("local", 3, memo=memo)))
    assert len(blobs[big]) > 70_001 and len(dict(_one(blobs[big]).xs)["memo"]) > 70_001
    blobs += [_varied(w) for w in range(len(blobs), 64)]  # the first wave: the global window
    share = 24576 // 64  # a lane's share of CDR_LOAD_STAGE
    for last in (share - 1, share, share + 1):  # three waves: a byte under, exactly, a byte over the stage
        blobs += [_sized(share, w) for w in range(63)] + [_sized(last, 63)]
    over = len(blobs)
    blobs.append(_blob(_x_fields(n_rp=abi.LOAD_MAX_RESET_POINTS + 1)))
    blobs.append(_blob(_x_fields(sa=[(b"k", b"v")] * (abi.LOAD_MAX_SEARCH_ATTR + 1))))
    blobs.append(_blob(_x_fields("ndc", n_items=abi.LOAD_MAX_VH_ITEMS + 1)))
    blobs.append(_blob(_x_fields("ndc", n_items=abi.LOAD_MAX_VH_ITEMS)))
    R = _entries(blobs)
    got = rows.load_state(engine_gpu, R, SEEDS)
    want = _assert_equal(got, R, SEEDS)
    assert [int(s) for s in got.exec_status[over:]] == [abi.LOAD_E_SHAPE] * 3 + [0] and not any(want.entry_status[:over])
    assert [got.result[w].n_vh for w in range(5)] == [0, 1, 64, 65, 1000] and got.result[over + 3].n_vh == abi.LOAD_MAX_VH_ITEMS
    assert [got.result[w].n_reset_points for w in range(5, 9)] == [0, 1, 12, 13]
    assert [got.result[w].n_search_attr for w in range(9, 13)] == [0, 1, 8, 9]
    assert len(got.strings[got.exec[big].memo]) == len(blobs[big]) - len(_blob(_x_fields("local", 3, memo=()))) + 10


@pytest.mark.gpu
def test_gpu_wire_edges(engine_gpu):
    """Every wire-edge blob of the CPU test, each in an entry of its own."""
    cases = wire_cases()
    R = _entries([blob for _, blob, _ in cases])
    got = rows.load_state(engine_gpu, R, SEEDS)
    _assert_equal(got, R, SEEDS)
    for w, (name, blob, want) in enumerate(cases):
        assert got.exec_status[w] == got.entry_status[w] == (want if isinstance(want, int) else 0), name


@pytest.mark.gpu
def test_gpu_truncation_at_every_length(engine_gpu):
    """One blob with every nested blob, cut at every length: CDR_DEC_TRUNCATED each, and the
    whole rows between them decode unchanged."""
    plain = _blob(_x_fields("ndc", n_rp=1, n_items=2))
    blobs = []
    for n in range(len(plain)):
        blobs += [plain[:n]] + ([plain] if n % 16 == 0 else [])
    R = _entries(blobs)
    got = rows.load_state(engine_gpu, R, SEEDS)
    _assert_equal(got, R, SEEDS)
    for w, blob in enumerate(blobs):
        assert got.entry_status[w] == (0 if len(blob) == len(plain) else TD.DEC_TRUNCATED), (w, len(blob))


@pytest.mark.gpu
def test_gpu_buffer_end(engine_gpu):
    """The last execution row is cut and its offsets claim to run past n_bytes, with `bytes`
    ending where its allocation ends: the offsets are clamped, the row is TRUNCATED, the rows
    before it decode."""
    plain = _blob(_x_fields("ndc"))
    for tail in (plain[:-1], plain[:len(plain) // 2], plain[:5]):
        R = _entries([plain, _varied(4), tail])
        assert int(R.exec.blob_off[3]) == len(R.bytes)  # the execution blobs come last
        R.exec.blob_off[3] += 1 << 20
        got = rows.load_state(engine_gpu, R, SEEDS, at_end=True)
        _assert_equal(got, R, SEEDS)
        assert got.entry_status.tolist() == [0, 0, TD.DEC_TRUNCATED]
    R = _entries([plain, plain])
    R.exec.blob_off[1] = R.exec.blob_off[2] = len(R.bytes) + 77  # both ends past the buffer: an empty row
    got = rows.load_state(engine_gpu, R, SEEDS, at_end=True)
    _assert_equal(got, R, SEEDS)
    assert got.entry_status.tolist() == [0, TD.DEC_TRUNCATED]


@pytest.mark.gpu
def test_gpu_one_handle_space(engine_gpu):
    """A UUID that is a child's StartedRunID, an execution's run_id and a reset point's run_id
    has one handle; a Memo body equal to a seed keeps the seed's handle; seeds keep theirs."""
    run = bytes(range(0x20, 0x30))
    text = rows_ref.uuid_string(run)
    child = tc.value(tc.T_STRUCT, St("row", [tc.i64(10, 1), tc.s(20, b"child-wf"), tc.s(22, run), tc.s(28, U)]))
    pts = tb.PREAMBLE + tc.value(tc.T_STRUCT, St("ResetPoints", [tc.lst(10, tc.T_STRUCT, [tc.reset_point(b"cks", text, 0)])]))
    memo_body = b"\x0d\x00\x0a\x0b\x0b\0\0\0\x01\0\0\0\x02mk\0\0\0\x02mv\x00"
    x0 = _blob(_with(_x_fields("local"), f115=tc.s(115, pts)))
    x1 = _blob(_x_fields("ndc", 1))
    tabs = [[[], []] for _ in range(5)]
    tabs[2][1] = [(9, child)]
    R = _entries([x0, x1], tabs, {0: (bytes(16), run, b"child-wf", 10, 0), 1: (bytes(16), bytes(range(16)), text, 11, 0)})
    seeds = [b"", b"unused"] + CLUSTERS + [memo_body, b"tl-1"]
    got = rows.load_state(engine_gpu, R, seeds, cluster_seed=[2, 3, 4])
    _assert_equal(got, R, seeds)
    h = got.strings.index(text)
    assert h >= len(seeds) and got.strings.count(text) == 1
    assert got.exec[0].run_id == h == got.rows(1, "child")[0].started_run_id == got.exec[1].workflow_id
    assert got.tables["rp"][got.caps[0].rp_off].run_id == h
    assert got.exec[0].memo == 5 and got.exec[1].memo == 5 and got.exec[1].task_list == 6
    assert got.exec[0].workflow_id == got.rows(1, "child")[0].started_workflow_id
    assert got.exec[0].domain_id == got.exec[1].domain_id == got.strings.index(b"00000000-0000-0000-0000-000000000000")
    new = got.strings[len(seeds):]
    assert new == sorted(new, key=TD.str_hash) and len(set(got.strings)) == len(got.strings)


def _scalars(x) -> bytes:
    x = _copy(x)
    for f in rows.X_HANDLES:
        setattr(x, f, 0)
    return bytes(x)


@pytest.mark.gpu
def test_gpu_failures_stay_in_their_entry(engine_gpu):
    """A failing execution row fails only its entry and withholds all of its strings, the
    pending rows' included; a failing pending row in the same entry wins the entry status."""
    sig = lambda name: tc.value(tc.T_STRUCT, St("row", [tc.i64(10, 1), tc.s(12, U), tc.s(14, name)]))  # noqa: E731
    good = [_blob(_x_fields(k, v)) for v, k in enumerate(("local", "2dc", "ndc", "local"))]
    bad_x = _blob(_with(_x_fields("local", 4), f116=tc.s(116, b"json")) + [tc.s(960, b"x")])
    tabs = [[[] for _ in range(4)] for _ in range(5)]
    tabs[4][0] = [(1, sig(b"sig-in-entry-0"))]
    tabs[4][1] = [(1, sig(b"sig-in-entry-1"))]
    tabs[4][2] = [(1, sig(b"sig-in-entry-2")), (2, sig(b"cut")[:-4])]
    tabs[4][3] = [(1, sig(b"sig-in-entry-3"))]
    R = _entries([good[0], bad_x, bad_x, good[3]], tabs)
    got = rows.load_state(engine_gpu, R, SEEDS)
    _assert_equal(got, R, SEEDS)
    assert got.entry_status.tolist() == [0, abi.LOAD_E_ENCODING, TD.DEC_TRUNCATED, 0]
    assert got.exec_status.tolist() == [0, abi.LOAD_E_ENCODING, abi.LOAD_E_ENCODING, 0] and got.n_bad_entries == 2
    assert [r.code for r in got.result] == [abi.OK, abi.E_LOAD_ROWS, abi.E_LOAD_ROWS, abi.OK]
    assert (got.result[1].n_signal, got.result[1].n_reset_points, got.result[2].n_search_attr) == (0, 0, 0)
    for s in (b"sig-in-entry-1", b"sig-in-entry-2", b"tl-4", b"create-req-4"):
        assert s not in got.strings
    for s in (b"sig-in-entry-0", b"sig-in-entry-3", b"type-3", b"create-req-0"):
        assert s in got.strings
    alone = rows.load_state(engine_gpu, _entries([good[0]], [[t[0]] for t in tabs]), SEEDS)
    assert _scalars(alone.exec[0]) == _scalars(got.exec[0])  # (the handles differ: fewer strings ranked)
    # a duplicate key fails the entry after its strings were interned, execution row included
    tabs[4][3] = [(1, sig(b"dup")), (1, sig(b"dup"))]
    R = _entries([good[0], good[1], good[2], good[3]], tabs[:4] + [[tabs[4][0], [], [], tabs[4][3]]])
    got = rows.load_state(engine_gpu, R, SEEDS)
    _assert_equal(got, R, SEEDS)
    assert got.entry_status.tolist() == [0, 0, 0, abi.LOAD_E_DUP_KEY] and b"create-req-3" in got.strings


@pytest.mark.gpu
def test_gpu_without_execution_rows_and_misuse(engine_gpu):
    """exec == NULL gives cdr_load_rows' results; null arguments return CDR_API_EINVAL; a second
    call on the warm context gives the first one's results."""
    from tests import test_load_rows as tlr
    b, out, strs = tlr._state(5)
    R = tlr._oracle_rows(b, out, strs)
    one, two = rows.load(engine_gpu, R, strs[:7]), rows.load_state(engine_gpu, R, strs[:7])
    for t in rows.TABLES:
        assert bytes(one.tables[t]) == bytes(two.tables[t])
    assert bytes(one.result) == bytes(two.result) and bytes(one.caps) == bytes(two.caps) and one.strings == two.strings
    assert all((a == c).all() for a, c in zip(one.row_status, two.row_status)) and one.gen_bytes == two.gen_bytes
    assert (one.entry_status == two.entry_status).all() and bytes(one.totals) == bytes(two.totals) and two.exec is None
    Rx = _entries([_varied(w) for w in range(70)])
    first, again = rows.load_state(engine_gpu, Rx, SEEDS), rows.load_state(engine_gpu, Rx, SEEDS)
    assert bytes(first.exec) == bytes(again.exec) and first.strings == again.strings and first.gen_bytes == again.gen_bytes
    assert all(bytes(first.tables[t]) == bytes(again.tables[t]) for t in ITEMS)
    L = abi.lib()
    inp, xin, res = abi.CdrRowsIn(), abi.CdrExecRowsIn(), abi.CdrStateOut()
    ctx = engine_gpu.ctx
    assert L.cdr_load_state(ctx, None, C.byref(xin), C.byref(res), None) == -1
    assert L.cdr_load_state(ctx, C.byref(inp), C.byref(xin), None, None) == -1
    assert L.cdr_load_state(None, C.byref(inp), C.byref(xin), C.byref(res), None) == -1
    assert L.cdr_load_state(ctx, C.byref(inp), C.byref(xin), C.byref(res), None) == -1  # no seeds
    Rx.exec.cluster_seed = list(range(abi.MAX_CLUSTERS + 1))
    assert rows.load_state(engine_gpu, Rx, SEEDS, check=False).rc == -1  # more clusters than the records hold
    dev = rows.DeviceBuffers()
    try:  # entries, seeds, and an execution column missing
        so = dev.up(np.array([0, 0], np.uint64))
        inp.seed_off, inp.seed_bytes, inp.n_seeds, inp.n_entries = so, so, 1, 1
        assert L.cdr_load_state(ctx, C.byref(inp), C.byref(xin), C.byref(res), None) == -1
    finally:
        dev.free()
