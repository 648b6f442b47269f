#!/usr/bin/env python3
"""Throughput of the persisted-row loader (cdr_load_rows) and the whole-state loader
(cdr_load_state: the same rows plus every workflow's execution row) beside the history ingest
(cdr_ingest_decode), the comparable lane-per-blob thrift walk, on the same populations.

States: the final states of a config-3 and a config-5 replay.  --base workflows are
generated, replayed on the GPU and encoded on the host side of the encoders
(rows.encode_state walks every row in Python), then tiled --tile times on the way to the
device, so the loader runs over base * tile workflows (1M by default).  Tiling repeats the
strings: the loader interns base-many distinct strings however many rows name them, as a
store full of shared task lists and types would, but the per-workflow IDs of a real store
would add distinct strings the tiles do not have: a second run appends the entry number to
every timer ID, which makes the timer table's key strings distinct per workflow.  Seeds: "" alone, so every string is new.
Each population is loaded again with its execution rows (cdr_load_state, "load_state" in the
record); in the distinct run every workflow also has a run ID of its own, one more distinct
string per workflow.  "added" is the execution rows' cost: the whole-state call's wall time
less cdr_load_rows' on the same pending rows, and the execution rows' bytes over it.

Each call is timed wall-clock (it is synchronous) on a warm context over --reps repeats;
the passes inside it by the HIP events cdr_load_pass_ms reads.  The ingest decodes the same
base population's history blobs, tiled up to --ingest-bytes, in the same process.
Writes one JSON record (--out).

    python tools/load_bench.py --out profiles/load_rows.json

--form cql measures the Cassandra form instead (cdr_load_cql_rows): the same four populations
(configs 3 and 5, shared and distinct timer IDs) as map columns, each beside cdr_load_rows on
the same states' SQL rows in the same process — the yardstick — with the ratio per population
and per pass.  The map split counts into the first pass.

    python tools/load_bench.py --form cql --out profiles/load_cql.json

--form cql --exec-rows measures whole stored states from Cassandra (cdr_load_cql_state): the
same four populations with their execution rows (the `execution` / `replication_state` /
`version_histories` columns behind the tables', column-major; in the distinct run every
workflow has a run ID of its own), beside cdr_load_state on the same states' SQL rows — the
yardstick — and cdr_load_cql_rows alone on the same columns, so the execution rows' added
time is a difference within one process and session.

    python tools/load_bench.py --form cql --exec-rows --out profiles/load_cql_state.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cadence_amd import abi, engine, ingest, rows  # noqa: E402

PASSES = ("count", "intern_and_rank_strings", "rank_rows", "fill_and_epilogue")


def tile_offsets(off: np.ndarray, tile: int, base: int, dtype) -> np.ndarray:
    """`tile` copies of a run of n contiguous items (off: n + 1 offsets), back to back from `base`."""
    n, span = len(off) - 1, int(off[-1] - off[0])
    rel = (off[:-1] - off[0]).astype(np.int64)
    out = np.empty(n * tile + 1, dtype)
    out[:-1] = (rel[None, :] + (np.arange(tile, dtype=np.int64) * span)[:, None]).reshape(-1) + base
    out[-1] = base + span * tile
    return out


def tile_rows(R: rows.Rows, tile: int) -> rows.Rows:
    """The rows `tile` times over: each table's blobs stay contiguous, timer IDs follow."""
    segs, offs, row0, keys, pos = [], [], [], [], 0
    for t in range(5):
        o = R.blob_off[t]
        seg = R.bytes[int(o[0]):int(o[-1])]
        offs.append(tile_offsets(o, tile, pos, np.uint64))
        segs.append(np.tile(seg, tile))
        pos += len(seg) * tile
        row0.append(tile_offsets(R.entry_row0[t], tile, 0, np.uint32))
        keys.append(np.tile(R.key[t], tile))
    o = R.timer_id_off
    tid = tile_offsets(o, tile, pos, np.uint64)
    segs.append(np.tile(R.bytes[int(o[0]):int(o[-1])], tile))
    return rows.Rows(np.concatenate(segs), offs, row0, keys, tid, np.tile(R.act_heartbeat, tile), R.n_entries * tile)


def stats(xs) -> dict:
    xs = sorted(float(x) for x in xs)
    return {"median": float(np.median(xs)), "min": xs[0], "max": xs[-1]}


def distinct_timer_ids(R: rows.Rows) -> rows.Rows:
    """The rows with every timer ID made its workflow's own (the entry number appended): the
    timer table's key strings are then distinct per workflow, as IDs in a real store are."""
    lo = int(R.timer_id_off[0])
    entry = np.repeat(np.arange(R.n_entries), np.diff(R.entry_row0[1].astype(np.int64)))
    ids = [R.timer_id(r) + b"#%07d" % w for r, w in enumerate(entry.tolist())]
    off = np.zeros(len(ids) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in ids])
    data = np.concatenate([R.bytes[:lo], np.frombuffer(b"".join(ids) or b"\0", np.uint8)])
    return rows.Rows(data[:lo + int(off[-1])], R.blob_off, R.entry_row0, R.key, off + np.uint64(lo), R.act_heartbeat,
                     R.n_entries)


def with_exec_rows(R: rows.Rows, X: rows.Rows, tile: int, distinct: bool) -> rows.Rows:
    """R (tiled) with the execution rows of X (one population, untiled) `tile` times over behind
    its bytes: workflow IDs, then the blobs.  distinct: every entry's run ID is its own."""
    x = X.exec
    pos = len(R.bytes)
    wid = tile_offsets(x.workflow_id_off, tile, pos, np.uint64)
    wseg = np.tile(X.bytes[int(x.workflow_id_off[0]):int(x.workflow_id_off[-1])], tile)
    off = tile_offsets(x.blob_off, tile, pos + len(wseg), np.uint64)
    bseg = np.tile(X.bytes[int(x.blob_off[0]):int(x.blob_off[-1])], tile)
    run = np.tile(x.run_id, tile)
    if distinct:
        run = run.reshape(-1, 16).copy()
        run[:, :4] = np.arange(len(run), dtype=">u4").view(np.uint8).reshape(-1, 4)
        run = run.reshape(-1)
    xr = rows.ExecRows(off, np.tile(x.domain_id, tile), run, wid, np.tile(x.next_event_id, tile),
                       np.tile(x.last_write_version, tile), x.cluster_seed)
    return rows.Rows(np.concatenate([R.bytes, wseg, bseg]), R.blob_off, R.entry_row0, R.key, R.timer_id_off,
                     R.act_heartbeat, R.n_entries, exec=xr)


def time_load(eng, R: rows.Rows, reps: int) -> dict:
    """cdr_load_rows over R — cdr_load_state where R has execution rows — (seeds: "" alone),
    wall clock and passes."""
    L = abi.lib()
    n_rows, n_bytes = R.n_rows, int(len(R.bytes))
    dev = rows.DeviceBuffers()
    try:
        seeds = [b""] + (list(R.exec.cluster_seed) if R.exec is not None else [])  # (held as names here)
        sb, so = ingest.string_table(seeds)
        inp = abi.CdrRowsIn()
        inp.bytes, inp.n_bytes = dev.up(R.bytes), n_bytes
        for t in range(5):
            inp.blob_off[t], inp.entry_row0[t] = dev.up(R.blob_off[t]), dev.up(R.entry_row0[t])
            inp.key[t] = dev.up(R.key[t]) if t != 1 else None
            inp.n_rows[t] = n_rows[t]
        inp.timer_id_off, inp.act_heartbeat = dev.up(R.timer_id_off), dev.up(R.act_heartbeat)
        inp.seed_bytes, inp.seed_off = dev.up(sb), dev.up(so)
        inp.n_entries, inp.n_seeds = R.n_entries, len(seeds)
        wall, passes = [], [[] for _ in PASSES]
        res = abi.CdrRowsOut()
        X = R.exec
        if X is not None:
            sout, xin = abi.CdrStateOut(), abi.CdrExecRowsIn()
            xin.blob_off, xin.workflow_id_off = dev.up(X.blob_off), dev.up(X.workflow_id_off)
            xin.domain_id, xin.run_id = dev.up(X.domain_id), dev.up(X.run_id)
            xin.next_event_id, xin.last_write_version = dev.up(X.next_event_id), dev.up(X.last_write_version)
            xin.n_clusters = len(seeds) - 1
            for i in range(xin.n_clusters):
                xin.cluster_seed[i] = 1 + i
        for rep in range(reps + 1):
            assert dev.hip.hipDeviceSynchronize() == 0
            t0 = time.perf_counter()
            if X is not None:
                rc = L.cdr_load_state(eng.ctx, C.byref(inp), C.byref(xin), C.byref(sout), None)
                res = sout.rows
            else:
                rc = L.cdr_load_rows(eng.ctx, C.byref(inp), C.byref(res), None)
            t1 = time.perf_counter()
            assert rc == 0 and res.n_bad_entries == 0, (rc, res.n_bad_entries)
            ms = (C.c_float * 4)()
            assert L.cdr_load_pass_ms(eng.ctx, ms) == 0
            if rep:  # the first call grows the workspace
                wall.append(t1 - t0)
                for i in range(4):
                    passes[i].append(ms[i] / 1e3)
        n_strings = int(res.n_strings)
    finally:
        dev.free()
    total_rows = sum(n_rows) + (R.n_entries if X is not None else 0)
    w = stats(wall)
    rec = {"bytes": n_bytes, "strings": n_strings, "load_wall_s": w, "load_gbs": n_bytes / w["median"] / 1e9,
           "load_rows_per_s": total_rows / w["median"], "passes": {}}
    for name, xs in zip(PASSES, passes):
        s = stats(xs)
        rec["passes"][name] = {"s": s, "rows_per_s": total_rows / s["median"]}
        if name != "rank_rows":  # (it reads keys, not blob bytes)
            rec["passes"][name]["gbs"] = n_bytes / s["median"] / 1e9
    if X is not None:
        rec["exec_rows"] = R.n_entries
        rec["exec_bytes"] = int(X.blob_off[-1] - X.workflow_id_off[0])
    return rec


def tile_cols(cols: rows.CqlCols, tile: int, timer_suffix: bool = False) -> rows.CqlCols:
    """The map columns `tile` times over, table-major.  timer_suffix: every timer ID (the map
    key and the UDT's field) gets its tiled entry's number appended, as distinct_timer_ids."""
    import struct
    segs, offs, pos = [], [], 0
    n = cols.n_entries
    for t in range(5):
        o = cols.col_off[t]
        if t == 1 and timer_suffix:
            parts = []  # per base entry: [(id, version value, the fields after timer_id)]
            for w in range(n):
                body, rs = cols.column(1, w), []
                if body:
                    p = 4
                    for _ in range(struct.unpack_from(">i", body, 0)[0]):
                        kl = struct.unpack_from(">i", body, p)[0]
                        ul = struct.unpack_from(">i", body, p + 4 + kl)[0]
                        u = body[p + 8 + kl:p + 8 + kl + ul]
                        il = struct.unpack_from(">i", u, 12)[0]
                        rs.append((u[16:16 + il], u[:12], u[16 + il:]))
                        p += 8 + kl + ul
                parts.append(rs)
            out, lens = [], np.zeros(n * tile + 1, np.uint64)
            for e in range(n * tile):
                rs = parts[e % n]
                if rs:
                    sfx = b"#%07d" % e
                    col = [struct.pack(">i", len(rs))]
                    for tid, ver, rest in rs:
                        v = struct.pack(">i", len(tid) + len(sfx)) + tid + sfx
                        col += [v, struct.pack(">i", len(ver) + len(v) + len(rest)), ver, v, rest]
                    col = b"".join(col)
                    out.append(col)
                    lens[e + 1] = len(col)
            seg = np.frombuffer(b"".join(out) or b"\0", np.uint8)[:int(lens.sum())]
            offs.append(np.cumsum(lens).astype(np.uint64) + np.uint64(pos))
            segs.append(seg)
            pos += len(seg)
            continue
        seg = cols.bytes[int(o[0]):int(o[-1])]
        offs.append(tile_offsets(o, tile, pos, np.uint64))
        segs.append(np.tile(seg, tile))
        pos += len(seg) * tile
    return rows.CqlCols(np.concatenate(segs), offs, n * tile)


def with_exec_cols(T: rows.CqlCols, cols: rows.CqlCols, tile: int, distinct: bool) -> rows.CqlCols:
    """T (tiled) with the execution row's four columns of `cols` (one population, untiled)
    `tile` times over behind its bytes, column-major.  distinct: every entry's run ID (the
    UDT's third field) is its own."""
    import struct
    segs, offs, pos = [T.bytes], [], len(T.bytes)
    n = cols.n_entries
    for c in range(4):
        o = cols.exec.off[c]
        seg = np.tile(cols.bytes[int(o[0]):int(o[-1])], tile)
        off = tile_offsets(o, tile, pos, np.uint64)
        if c == 0 and distinct:
            at = np.zeros(n, np.int64)  # the run ID's place in each base entry's body
            for w in range(n):
                body = cols.exec_column(0, w)
                p = 4 + max(0, struct.unpack_from(">i", body, 0)[0])
                p += 4 + max(0, struct.unpack_from(">i", body, p)[0])
                assert struct.unpack_from(">i", body, p)[0] == 16
                at[w] = p + 4
            where = (off[:-1].astype(np.int64) - pos) + np.tile(at, tile)
            ids = np.arange(n * tile, dtype=">u4").view(np.uint8).reshape(-1, 4)
            seg[where[:, None] + np.arange(4)[None, :]] = ids
        offs.append(off)
        segs.append(seg)
        pos += len(seg)
    return rows.CqlCols(np.concatenate(segs), T.col_off, T.n_entries, exec=rows.CqlExec(offs, cols.exec.cluster_seed))


def time_load_cql(eng, cols: rows.CqlCols, reps: int, exec_rows: bool = False) -> dict:
    """cdr_load_cql_rows over `cols` — cdr_load_cql_state with exec_rows, where cols.exec holds
    the execution row's columns and, as cluster_seed, the clusters' names — (seeds: "" and those
    names), wall clock and passes."""
    L = abi.lib()
    n_bytes = int(len(cols.bytes))
    dev = rows.DeviceBuffers()
    try:
        seeds = [b""] + (list(cols.exec.cluster_seed) if exec_rows else [])
        sb, so = ingest.string_table(seeds)
        inp = abi.CdrCqlRowsIn()
        inp.bytes, inp.n_bytes = dev.up(cols.bytes), n_bytes
        for t in range(5):
            inp.col_off[t] = dev.up(cols.col_off[t])
        inp.seed_bytes, inp.seed_off = dev.up(sb), dev.up(so)
        inp.n_entries, inp.n_seeds = cols.n_entries, len(seeds)
        wall, passes = [], [[] for _ in PASSES]
        res = abi.CdrCqlRowsOut()
        if exec_rows:
            sout, xin = abi.CdrCqlStateOut(), abi.CdrCqlExecIn()
            X = cols.exec
            xin.execution_off, xin.replication_state_off = dev.up(X.off[0]), dev.up(X.off[1])
            xin.version_histories_off, xin.vh_encoding_off = dev.up(X.off[2]), dev.up(X.off[3])
            xin.n_clusters = len(seeds) - 1
            for i in range(xin.n_clusters):
                xin.cluster_seed[i] = 1 + i
        for rep in range(reps + 1):
            assert dev.hip.hipDeviceSynchronize() == 0
            t0 = time.perf_counter()
            if exec_rows:
                rc = L.cdr_load_cql_state(eng.ctx, C.byref(inp), C.byref(xin), C.byref(sout), None)
                res = sout.rows
            else:
                rc = L.cdr_load_cql_rows(eng.ctx, C.byref(inp), C.byref(res), None)
            t1 = time.perf_counter()
            assert rc == 0 and res.rows.n_bad_entries == 0, (rc, res.rows.n_bad_entries)
            ms = (C.c_float * 4)()
            assert L.cdr_load_pass_ms(eng.ctx, ms) == 0
            if rep:  # the first call grows the workspace
                wall.append(t1 - t0)
                for i in range(4):
                    passes[i].append(ms[i] / 1e3)
        n_rows, n_strings = [int(x) for x in res.n_rows], int(res.rows.n_strings)
    finally:
        dev.free()
    w = stats(wall)
    rec = {"bytes": n_bytes, "strings": n_strings, "rows": dict(zip(rows.TABLES, n_rows)), "load_wall_s": w,
           "load_gbs": n_bytes / w["median"] / 1e9, "load_rows_per_s": sum(n_rows) / w["median"], "passes": {}}
    for name, xs in zip(PASSES, passes):
        s = stats(xs)
        rec["passes"][name] = {"s": s, "rows_per_s": sum(n_rows) / s["median"]}
    if exec_rows:
        rec["exec_rows"] = cols.n_entries
        rec["exec_bytes"] = int(cols.exec.off[3][-1] - cols.exec.off[0][0])
    return rec


def versus(cql: dict, sql: dict) -> dict:
    """cdr_load_cql_rows over cdr_load_rows on the same states: medians' ratios."""
    return {"wall": cql["load_wall_s"]["median"] / sql["load_wall_s"]["median"], "bytes": cql["bytes"] / sql["bytes"],
            "passes": {p: cql["passes"][p]["s"]["median"] / sql["passes"][p]["s"]["median"] for p in PASSES}}


def bench_config_cql(eng, cfg: int, base: int, tile: int, reps: int) -> dict:
    b = engine.synth_batch(cfg, base, seed=0x5EED0000 + cfg)
    out = eng.replay(b)
    strs = rows.state_strings(b, out)
    R = tile_rows(rows.encode_state(eng, b, out, strs), tile)
    cols = rows.encode_state_cql(eng, b, out, strs)
    rec = {"config": cfg, "workflows": R.n_entries, "base_workflows": base, "tile": tile, "populations": {}}
    for name, sql_rows, cql_cols in (("shared", R, tile_cols(cols, tile)),
                                     ("distinct_timer_ids", distinct_timer_ids(R), tile_cols(cols, tile, True))):
        sql = time_load(eng, sql_rows, reps)
        cql = time_load_cql(eng, cql_cols, reps)
        assert sum(cql["rows"].values()) == sum(sql_rows.n_rows) and cql["strings"] == sql["strings"]
        rec["populations"][name] = {"load_rows": sql, "load_cql_rows": cql, "cql_over_sql": versus(cql, sql)}
    return rec


def cql_state_strings(b, out, extra: int) -> list:
    """rows.whole_state_strings with the create request IDs as UUID texts: the Cassandra writer
    binds them to a uuid column."""
    strs = rows.whole_state_strings(b, out, extra=extra)
    for w in range(b.n_wfs):
        h = out.exec[w].create_request_id
        if out.result[w].code == abi.OK and h and len(strs[h]) != 36:
            strs[h] = b"c0de%04x-0000-4000-8000-%012x" % (h & 0xFFFF, h)
    assert len(set(strs)) == len(strs)
    return strs


def bench_config_cql_state(eng, cfg: int, base: int, tile: int, reps: int) -> dict:
    b = engine.synth_batch(cfg, base, seed=0x5EED0000 + cfg)
    out = eng.replay(b)
    n_cl = b.cluster.n_clusters
    xs = cql_state_strings(b, out, n_cl)
    names = list(range(len(xs) - n_cl, len(xs)))
    X = rows.encode_state(eng, b, out, xs, exec_rows=True, cluster_names=names)
    X.exec.cluster_seed = xs[len(xs) - n_cl:]
    R = tile_rows(X, tile)
    cols = rows.encode_state_cql(eng, b, out, xs, exec_rows=True, cluster_names=names)
    cols.exec.cluster_seed = xs[len(xs) - n_cl:]
    rec = {"config": cfg, "workflows": R.n_entries, "base_workflows": base, "tile": tile, "populations": {}}
    for name, distinct in (("shared", False), ("distinct_timer_ids", True)):
        sql = time_load(eng, with_exec_rows(distinct_timer_ids(R) if distinct else R, X, tile, distinct), reps)
        T = with_exec_cols(tile_cols(cols, tile, distinct), cols, tile, distinct)
        tables = time_load_cql(eng, T, reps)
        state = time_load_cql(eng, T, reps, exec_rows=True)
        assert sum(state["rows"].values()) == sum(R.n_rows)
        rec["populations"][name] = {"load_state": sql, "load_cql_rows": tables, "load_cql_state": state,
                                    "cql_over_sql": versus(state, sql), "added": added(state, tables)}
    return rec


def added(state: dict, plain: dict) -> dict:
    """What the execution rows add to the call."""
    s = state["load_wall_s"]["median"] - plain["load_wall_s"]["median"]
    return {"ms": s * 1e3, "gbs": state["exec_bytes"] / s / 1e9 if s > 0 else None,
            "passes_ms": {p: (state["passes"][p]["s"]["median"] - plain["passes"][p]["s"]["median"]) * 1e3 for p in PASSES}}


def bench_config(eng, cfg: int, base: int, tile: int, reps: int, ingest_bytes: int) -> dict:
    L = abi.lib()
    b = engine.synth_batch(cfg, base, seed=0x5EED0000 + cfg)
    out = eng.replay(b)
    strs = rows.state_strings(b, out)
    R = tile_rows(rows.encode_state(eng, b, out, strs), tile)
    rec = {"config": cfg, "workflows": R.n_entries, "base_workflows": base, "tile": tile,
           "rows": dict(zip(rows.TABLES, R.n_rows)), "rows_total": sum(R.n_rows)}
    rec.update(time_load(eng, R, reps))
    # the same rows with the timer IDs distinct per workflow: the intern pass inserts and the
    # ranking sorts millions of strings instead of finding a few thousand again and again
    D = distinct_timer_ids(R)
    rec["distinct_timer_ids"] = time_load(eng, D, reps)
    # ---- the same two populations with their execution rows (cdr_load_state); the cluster
    # names are the only seeds beside ""
    n_cl = b.cluster.n_clusters
    xs = rows.whole_state_strings(b, out, extra=n_cl)
    X = rows.encode_state(eng, b, out, xs, exec_rows=True, cluster_names=list(range(len(xs) - n_cl, len(xs))))
    X.exec.cluster_seed = xs[len(xs) - n_cl:]
    rec["load_state"] = time_load(eng, with_exec_rows(R, X, tile, False), reps)
    rec["load_state"]["added"] = added(rec["load_state"], rec)
    rec["distinct_timer_ids"]["load_state"] = time_load(eng, with_exec_rows(D, X, tile, True), reps)
    rec["distinct_timer_ids"]["load_state"]["added"] = added(rec["distinct_timer_ids"]["load_state"],
                                                             rec["distinct_timer_ids"])
    # ---- the history ingest of the same population
    enc = ingest.encode_batch(b, threads=16)
    raw = enc.blob_bytes[:int(enc.blob_off[-1])]
    itile = max(1, min(tile, ingest_bytes // max(1, len(raw))))
    dev = rows.DeviceBuffers()
    try:
        sb, so = ingest.string_table(enc.seeds)
        dm = np.array(enc.domain_map, np.uint32).reshape(-1) if enc.domain_map else np.zeros(2, np.uint32)
        ii = abi.CdrIngestIn()
        ii.blob_bytes = dev.up(np.tile(raw, itile))
        ii.blob_off = dev.up(tile_offsets(enc.blob_off, itile, 0, np.uint64))
        ii.entry_blob0 = dev.up(tile_offsets(enc.entry_blob0, itile, 0, np.uint32))
        ii.seed_bytes, ii.seed_off, ii.domain_map = dev.up(sb), dev.up(so), dev.up(dm)
        ii.n_blobs, ii.n_entries = (len(enc.blob_off) - 1) * itile, b.n_wfs * itile
        ii.n_seeds, ii.n_domains = len(enc.seeds), len(enc.domain_map)
        dec = []
        for rep in range(reps + 1):
            io = abi.CdrIngestOut()
            assert dev.hip.hipDeviceSynchronize() == 0
            t0 = time.perf_counter()
            rc = L.cdr_ingest_decode(eng.ctx, C.byref(ii), C.byref(io), None)
            t1 = time.perf_counter()
            assert rc == 0 and io.n_bad_blobs == 0, (rc, io.n_bad_blobs)
            if rep:
                dec.append(t1 - t0)
        d = stats(dec)
        rec["ingest"] = {"workflows": b.n_wfs * itile, "tile": itile, "blobs": int(ii.n_blobs),
                         "bytes": len(raw) * itile, "events": int(io.n_events), "strings": int(io.n_strings),
                         "decode_wall_s": d, "decode_gbs": len(raw) * itile / d["median"] / 1e9}
    finally:
        dev.free()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="3,5")
    ap.add_argument("--base", type=int, default=10_000)
    ap.add_argument("--tile", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ingest-bytes", type=int, default=2_000_000_000)
    ap.add_argument("--out", default="")
    ap.add_argument("--form", default="sql", choices=("sql", "cql"))
    ap.add_argument("--exec-rows", action="store_true", help="--form cql: whole states (cdr_load_cql_state)")
    args = ap.parse_args()
    try:
        import torch
        box = torch.cuda.get_device_name(0)
    except Exception:  # noqa: BLE001
        box = "unknown"
    eng = engine.Engine(0)
    rec = {"tool": "tools/load_bench.py", "device": box, "libcdr": abi.lib().cdr_version().decode(),
           "build_flags": int(abi.lib().cdr_build_flags()), "reps": args.reps,
           "timing": "wall clock around the synchronous calls on a warm context (first call dropped); passes: HIP "
                     "events inside cdr_load_rows / cdr_load_state (the intern interval holds its two host round trips)",
           "seeds": 1, "form": args.form + ("+exec-rows" if args.exec_rows else ""), "configs": []}
    for cfg in (int(c) for c in args.configs.split(",")):
        if args.form == "cql" and args.exec_rows:
            r = bench_config_cql_state(eng, cfg, args.base, args.tile, args.reps)
        elif args.form == "cql":
            r = bench_config_cql(eng, cfg, args.base, args.tile, args.reps)
        else:
            r = bench_config(eng, cfg, args.base, args.tile, args.reps, args.ingest_bytes)
        rec["configs"].append(r)
        print(json.dumps(r), flush=True)
    eng.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
