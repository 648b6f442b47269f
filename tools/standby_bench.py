#!/usr/bin/env python3
"""Measure the standby task kernel (cdr_standby_tasks_async) for every group size.

States: as tools/sync_bench.py — the prefixes of a config-3 batch as engine.split_batch cuts
them, replayed on the GPU with their task lists; --base workflows are generated and cut on the
host and tiled --tile times on the way to the device.  Requests: the prefixes' own emitted
transfer and timer tasks (standby.tasks_to_requests' records, built with numpy here), in two
populations: the first task of every workflow, and all of them; every other request carries
the global-domain bit, the version is 0 as the replay leaves it, and the clock stands two
standby delays after the median timer task (between the push and the discard threshold).  For
each group size G the kernel is timed with HIP events from the same pristine rows (restored,
then evicted from the caches by a stream copy, before every launch), the G's alternating over
--reps rounds.  The yardstick is k_sync_activity (cdr_sync_activity_async, its shipped group
size) on the same states at one sync.synth_requests request per workflow, timed in the same
rounds; the bytes the kernel must touch (requests, results, the rows of the tables the addressed
states' requests look up) over the median time is set against cdr_stream_copy_async.  All G
must give the same result and row bytes.  Writes one JSON record (--out).

    python tools/standby_bench.py --out profiles/standby_tasks.json
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

from cadence_amd import abi, engine, standby, sync  # noqa: E402
from sync_bench import D2D, D2H, Dev, raw, tiled_requests  # noqa: E402

TABLES = (("act", abi.CdrActivityInfo), ("timer", abi.CdrTimerInfo), ("child", abi.CdrChildInfo),
          ("cancel", abi.CdrCancelInfo), ("signal", abi.CdrSignalInfo), ("vh", abi.CdrVHItem))
# the table a task type looks up (the kernel reads no row for the others)
READS = {abi.TT_ACTIVITY: "act", abi.TT_ACTIVITY_TIMEOUT: "act", abi.TT_USER_TIMER: "timer",
         abi.TT_START_CHILD: "child", abi.TT_CANCEL_EXECUTION: "cancel", abi.TT_SIGNAL_EXECUTION: "signal"}
DELAY = 600 * 1_000_000_000


def tiled_state(st, tile):
    """The base state's records `tile` times over as uint8 matrices, every table offset of the
    copies' caps shifted by the base totals."""
    n, tot = st.n_wfs, st.plan.totals
    caps = np.tile(raw(st.plan.caps, abi.CdrWfCaps, n), (tile, 1)).copy()
    for name, _ in TABLES:
        o = getattr(abi.CdrWfCaps, name + "_off").offset
        col = caps[:, o:o + 8].copy().view(np.uint64).reshape(tile, n)
        col += (np.arange(tile, dtype=np.uint64) * np.uint64(getattr(tot, name)))[:, None]
        caps[:, o:o + 8] = col.reshape(-1, 1).view(np.uint8)
    out = dict(caps=caps, result=np.tile(raw(st.result, abi.CdrWfResult, n), (tile, 1)),
               exec=np.tile(raw(st.exec, abi.CdrExecInfo, n), (tile, 1)),
               repl=np.tile(raw(st.repl, abi.CdrReplState, n), (tile, 1)))
    for name, ty in TABLES:
        out[name] = np.tile(raw(st.tables[name], ty, max(1, getattr(tot, name))), (tile, 1))
    return out


def task_requests(st, per_wf, xfer_visibility):
    """standby.tasks_to_requests(st, per_wf=per_wf, xfer_visibility=...) as a uint8 matrix of
    cdr_standby_task records, built without a Python loop over the tasks; odd requests get
    CDR_SBT_GLOBAL_DOMAIN."""
    n = st.n_wfs
    counts = np.frombuffer(st.tasks["n"], np.uint32)[:2 * n].reshape(n, 2).astype(np.int64)
    ok = np.array([st.result[w].code == abi.OK for w in range(n)])
    caps = raw(st.plan.caps, abi.CdrWfCaps, n)
    parts = []
    for k, (kind, field) in enumerate((("xfer", "xfer_off"), ("ttask", "ttask_off"))):
        o = getattr(abi.CdrWfCaps, field).offset
        off = caps[:, o:o + 8].copy().view(np.uint64).ravel().astype(np.int64)
        cnt = np.where(ok, counts[:, k], 0)
        wf = np.repeat(np.arange(n), cnt)
        ordinal = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        rows = raw(st.tasks[kind], abi.CdrTask, len(st.tasks[kind]))[off[wf] + ordinal]
        parts.append((wf, ordinal + (0 if k == 0 else np.repeat(np.where(ok, counts[:, 0], 0), cnt)), rows, k))
    wf = np.concatenate([p[0] for p in parts])
    ordinal = np.concatenate([p[1] for p in parts])
    keep = np.lexsort((ordinal, wf))  # entry w's transfer tasks, then its timer tasks
    if per_wf is not None:
        keep = keep[ordinal[keep] < per_wf]
    m = np.zeros((len(keep), C.sizeof(abi.CdrStandbyTask)), np.uint8)
    tasks = np.concatenate([p[2] for p in parts])[keep]
    is_xfer = np.concatenate([np.full(len(p[0]), p[3] == 0) for p in parts])[keep]
    vo = abi.CdrTask.visibility_ts.offset
    tasks[is_xfer, vo:vo + 8] = np.frombuffer(np.int64(xfer_visibility).tobytes(), np.uint8)
    m[:, :C.sizeof(abi.CdrTask)] = tasks
    for field, val, dt in (("wf", wf[keep], np.int32), ("flags", np.arange(len(keep)) % 2, np.uint32),
                           ("tag", (wf[keep] << 16) | ordinal[keep], np.int64)):
        o = getattr(abi.CdrStandbyTask, field).offset
        m[:, o:o + np.dtype(dt).itemsize] = val.astype(dt).reshape(-1, 1).view(np.uint8)
    return m


def tile_and_plan(base, n_base, tile):
    """The base requests `tile` times over (wf shifted by the copy), grouped by cdr_plan_standby."""
    allr = np.tile(base, (tile, 1))
    o = abi.CdrStandbyTask.wf.offset
    wf = allr[:, o:o + 4].copy().view(np.int32).reshape(tile, len(base))
    wf += (np.arange(tile, dtype=np.int64) * n_base)[:, None].astype(np.int32)
    allr[:, o:o + 4] = wf.reshape(-1, 1).view(np.uint8)
    n, ns = len(allr), n_base * tile
    order, off = np.zeros(max(1, n), np.uint32), np.zeros(ns + 2, np.uint32)
    if abi.lib().cdr_plan_standby(allr.ctypes.data, n, ns, order.ctypes.data, off.ctypes.data):
        raise RuntimeError("cdr_plan_standby failed")
    return np.ascontiguousarray(allr[order[:n]]), off


def must_touch(st, base, tile):
    """Requests + results + the rows of the tables the addressed states' requests look up."""
    to = abi.CdrTask.type.offset
    types = base[:, to:to + 4].copy().view(np.uint32).ravel()
    wo = abi.CdrStandbyTask.wf.offset
    wf = base[:, wo:wo + 4].copy().view(np.int32).ravel()
    total = len(base) * (C.sizeof(abi.CdrStandbyTask) + C.sizeof(abi.CdrStandbyResult))
    sizes = dict((n, C.sizeof(t)) for n, t in TABLES)
    count = dict(act="n_activity", timer="n_timer", child="n_child", cancel="n_cancel", signal="n_signal")
    for name in ("act", "timer", "child", "cancel", "signal"):
        hit = np.zeros(st.n_wfs, bool)
        hit[wf[np.isin(types, [t for t, tab in READS.items() if tab == name])]] = True
        rows = np.array([getattr(st.result[w], count[name]) if st.result[w].code == abi.OK else 0
                         for w in range(st.n_wfs)], np.int64)
        total += int((rows * hit).sum()) * sizes[name]
    return total * tile


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base", type=int, default=100_000, help="workflows generated and cut on the host")
    ap.add_argument("--tile", type=int, default=10, help="copies of the base states on the device")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=0x5EED0300 + 3)
    ap.add_argument("--copy-mib", type=int, default=1024, help="size of the stream-copy yardstick")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "standby_tasks.json"))
    ap.add_argument("--dry", action="store_true", help="host preparation only (states from the CPU oracle)")
    a = ap.parse_args()

    t = time.time()
    b = engine.synth_batch(3, a.base, seed=a.seed)
    pre, _ = engine.split_batch(b, 2)
    print(f"synth + split_batch: {a.base} workflows, {len(b.events)} events, {time.time() - t:.1f}s", flush=True)
    if a.dry:
        import oracle
        eng, st = None, oracle.replay(pre, threads=16, tasks=True)
    else:
        eng = engine.Engine(0)
        st = eng.replay(pre, tasks=True)
    n_states = a.base * a.tile
    host = tiled_state(st, a.tile)
    tt = raw(st.tasks["ttask"], abi.CdrTask, len(st.tasks["ttask"]))
    vo = abi.CdrTask.visibility_ts.offset
    vis = tt[:, vo:vo + 8].copy().view(np.int64).ravel()
    base_ts = int(np.median(vis[vis != 0]))
    now = base_ts + 2 * DELAY
    runs = {}
    for name, per_wf in (("one task per workflow", 1), ("all tasks", None)):
        t = time.time()
        base = task_requests(st, per_wf, base_ts)
        if per_wf == 1:  # the numpy builder is tasks_to_requests, record for record
            want = standby.tasks_to_requests(st, per_wf=1, xfer_visibility=base_ts)
            for i in range(min(len(want), 2000)):
                want.arr[i].flags = i % 2
            k = min(len(want), 2000) * C.sizeof(abi.CdrStandbyTask)
            assert bytes(memoryview(want.arr).cast("B")[:k]) == base.tobytes()[:k]
        grouped, off = tile_and_plan(base, a.base, a.tile)
        runs[name] = (base, grouped, off)
        print(f"{name}: {len(grouped)} requests, {time.time() - t:.1f}s", flush=True)
    sreqs = sync.synth_requests(st, seed=1001, per_wf=1, increment=b.cluster.failover_version_increment)
    s_grouped, s_off = tiled_requests(sreqs, a.base, a.tile)
    ok = sum(1 for w in range(st.n_wfs) if st.result[w].code == abi.OK)
    rec = {"workload": "config 3 prefixes (engine.split_batch, seed 2), their own emitted tasks",
           "base_workflows": a.base, "tile": a.tile, "n_states": n_states, "ok_states": ok * a.tile,
           "rows": {n: int(getattr(st.plan.totals, n)) * a.tile for n, _ in TABLES},
           "states_note": "base_workflows distinct workflows, tiled `tile` times",
           "clock": {"standby_delay_s": DELAY // 10**9, "now": "median timer-task visibility + 2 delays",
                     "transfer_visibility": "the median timer-task visibility"},
           "cache": "a stream copy of copy-mib runs between restoring the rows and every timed launch",
           "reps": a.reps, "timing": "HIP events around one launch, median of reps, the G's and the sync "
                                     "yardstick alternating per round", "measured": True, "runs": []}
    if a.dry:
        print(json.dumps(rec))
        return
    L = abi.lib()
    dev = Dev()
    try:
        o = abi.CdrOut()
        o.result, o.exec, o.repl = dev.up(host["result"]), dev.up(host["exec"]), dev.up(host["repl"])
        for name in ("vh", "timer", "child", "cancel", "signal"):
            setattr(o, name, dev.up(host[name]))
        act0 = dev.up(host["act"])  # pristine rows
        act_bytes = host["act"].nbytes
        o.act = dev.alloc(act_bytes)
        d_caps = dev.up(host["caps"])
        cb = a.copy_mib << 20
        src, dst = dev.alloc(cb), dev.alloc(cb)
        dev.hip.hipMemset(src, 1, C.c_size_t(cb))
        copy_ms = sorted(dev.timed(lambda: L.cdr_stream_copy_async(dst, src, cb, None)) for _ in range(a.reps + 2))
        copy_gbs = 2 * cb / (copy_ms[len(copy_ms) // 2] * 1e-3) / 1e9
        rec["stream_copy"] = {"mib": a.copy_mib, "ms_median": copy_ms[len(copy_ms) // 2], "gb_per_s": copy_gbs}
        print("stream copy", rec["stream_copy"], flush=True)
        cl = b.cluster
        ds_req, ds_off = dev.up(s_grouped), dev.up(s_off)
        ds_res = dev.alloc(len(s_grouped) * C.sizeof(abi.CdrSyncResult))

        def sync_launch():
            if L.cdr_sync_activity_async(eng.ctx, ds_req, ds_off, len(s_grouped), n_states, d_caps, C.byref(o),
                                         C.byref(cl), ds_res, None):
                raise RuntimeError("cdr_sync_activity_async failed")
        for name, (base, grouped, off) in runs.items():
            n = len(grouped)
            d_req, d_off = dev.up(grouped), dev.up(off)
            res_bytes = n * C.sizeof(abi.CdrStandbyResult)
            d_res = dev.alloc(res_bytes)

            def launch():
                if L.cdr_standby_tasks_async(eng.ctx, d_req, d_off, n, n_states, d_caps, C.byref(o), C.byref(cl),
                                             now, DELAY, d_res, None):
                    raise RuntimeError("cdr_standby_tasks_async failed")

            def cold():
                dev.copy(o.act, act0, act_bytes, D2D)
                L.cdr_stream_copy_async(dst, src, cb, None)
            ms = {g: [] for g in abi.STANDBY_GROUPS}
            sync_ms, digest, hres = [], {}, None
            for rep in range(a.reps + 1):  # round 0 warms every instantiation up and is checked
                for g in abi.STANDBY_GROUPS:
                    eng.set_standby_group(g)
                    cold()
                    if rep == 0:
                        dev.ok(dev.hip.hipMemset(d_res, 0xFF, C.c_size_t(res_bytes)), "hipMemset")
                    t_ms = dev.timed(launch)
                    if rep == 0:
                        hres, hact = np.empty(res_bytes, np.uint8), np.empty(act_bytes, np.uint8)
                        dev.copy(hres.ctypes.data, d_res, res_bytes, D2H)
                        dev.copy(hact.ctypes.data, o.act, act_bytes, D2H)
                        digest[g] = hashlib.sha256(hres.tobytes() + hact.tobytes()).hexdigest()
                    else:
                        ms[g].append(t_ms)
                cold()
                t_ms = dev.timed(sync_launch)
                if rep:
                    sync_ms.append(t_ms)
            assert len(set(digest.values())) == 1, f"group sizes disagree: {digest}"
            must = must_touch(st, base, a.tile)
            r = hres.reshape(n, -1)
            actions = np.bincount(r[:, :4].copy().view(np.int32).ravel(), minlength=13)
            reasons = np.bincount(r[:, 4:8].copy().view(np.int32).ravel(), minlength=len(abi.SB_REASONS))
            sv = sorted(sync_ms)
            run = {"population": name, "n_requests": n, "must_touch_bytes": must,
                   "actions": {abi.SB_ACTIONS[i]: int(c) for i, c in enumerate(actions) if c},
                   "reasons": {abi.SB_REASONS[i]: int(c) for i, c in enumerate(reasons) if c},
                   "results_sha256": digest[abi.STANDBY_GROUP], "groups": {},
                   "sync_yardstick": {"kernel": "k_sync_activity", "group": abi.SYNC_GROUP, "n_requests": len(s_grouped),
                                      "ms_median": sv[len(sv) // 2], "ms_min": sv[0], "ms_max": sv[-1]}}
            for g in abi.STANDBY_GROUPS:
                v = sorted(ms[g])
                med = v[len(v) // 2]
                gbs = must / (med * 1e-3) / 1e9
                run["groups"][str(g)] = {"ms_median": med, "ms_min": v[0], "ms_max": v[-1],
                                         "must_touch_gb_per_s": gbs, "share_of_stream_copy": gbs / copy_gbs,
                                         "requests_per_s": n / (med * 1e-3),
                                         "ratio_to_sync_yardstick": med / sv[len(sv) // 2]}
            run["fastest_group"] = int(min(abi.STANDBY_GROUPS, key=lambda g: run["groups"][str(g)]["ms_median"]))
            rec["runs"].append(run)
            print(json.dumps(run), flush=True)
        eng.set_standby_group(abi.STANDBY_GROUP)
        rec["shipped_group"] = abi.STANDBY_GROUP
    finally:
        dev.free()
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
