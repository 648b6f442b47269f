#!/usr/bin/env python3
"""Measure the SyncActivity kernel (cdr_sync_activity_async) for every group size.

States: the prefixes of a config-3 batch as engine.split_batch cuts them, replayed on the GPU;
--base workflows are generated and cut on the host (split_batch walks every event in Python)
and tiled --tile times on the way to the device, so the kernel runs over base * tile states.
Requests: sync.synth_requests over the base states, tiled with them; one run with one request
per workflow and one with four.  For each group size G (4, 8, 16, 64) the kernel is timed with
HIP events from the same pristine rows (restored, then evicted from the caches by a stream
copy, before every launch), the G's alternating over --reps rounds; the bytes the
kernel must touch (requests, results, the activity rows of the addressed states) over the
median time is set against cdr_stream_copy_async timed in the same process.  All G must give
the same result and row bytes.  Writes one JSON record (--out).

    python tools/sync_bench.py --out profiles/sync_activity.json
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

from cadence_amd import abi, engine, sync  # noqa: E402

H2D, D2H, D2D = 1, 2, 3


def raw(x, ty, n):
    """(n, sizeof ty) uint8 view of a ctypes array."""
    return np.frombuffer(x, dtype=np.uint8)[:n * C.sizeof(ty)].reshape(n, C.sizeof(ty))


def tiled_state(st, tile):
    """The base state's records `tile` times over: result, exec, repl, caps, vh and act as
    uint8 matrices, the copies' act_off / vh_off shifted by the base totals."""
    n, tot = st.n_wfs, st.plan.totals
    caps = np.tile(raw(st.plan.caps, abi.CdrWfCaps, n), (tile, 1)).copy()
    for name, rows in (("act_off", tot.act), ("vh_off", tot.vh)):
        o = getattr(abi.CdrWfCaps, name).offset
        col = caps[:, o:o + 8].copy().view(np.uint64).reshape(tile, n)
        col += (np.arange(tile, dtype=np.uint64) * np.uint64(rows))[:, None]
        caps[:, o:o + 8] = col.reshape(-1, 1).view(np.uint8)
    return dict(
        caps=caps, result=np.tile(raw(st.result, abi.CdrWfResult, n), (tile, 1)),
        exec=np.tile(raw(st.exec, abi.CdrExecInfo, n), (tile, 1)),
        repl=np.tile(raw(st.repl, abi.CdrReplState, n), (tile, 1)),
        vh=np.tile(raw(st.tables["vh"], abi.CdrVHItem, max(1, tot.vh)), (tile, 1)),
        act=np.tile(raw(st.tables["act"], abi.CdrActivityInfo, max(1, tot.act)), (tile, 1)))


def tiled_requests(reqs, n_base, tile):
    """The base requests `tile` times over (wf shifted by the copy), grouped by cdr_plan_sync:
    (grouped requests as a uint8 matrix, req_off)."""
    sz = C.sizeof(abi.CdrSyncActivity)
    base = raw(reqs.arr, abi.CdrSyncActivity, len(reqs))
    allr = np.tile(base, (tile, 1)).copy()
    o = abi.CdrSyncActivity.wf.offset
    wf = allr[:, o:o + 4].copy().view(np.int32).reshape(tile, len(reqs))
    wf += np.where(wf >= 0, (np.arange(tile, dtype=np.int64) * n_base)[:, None], 0).astype(np.int32)
    allr[:, o:o + 4] = wf.reshape(-1, 1).view(np.uint8)
    n, ns = len(allr), n_base * tile
    order = np.zeros(max(1, n), np.uint32)
    off = np.zeros(ns + 2, np.uint32)
    rc = abi.lib().cdr_plan_sync(allr.ctypes.data, n, ns, order.ctypes.data, off.ctypes.data)
    if rc:
        raise RuntimeError(f"cdr_plan_sync rc={rc}")
    assert sz == allr.shape[1]
    return np.ascontiguousarray(allr[order[:n]]), off


def describe_difference(x, y, grouped):
    """Print where two group sizes' results and rows differ (they never should)."""
    (gx, rx, ax), (gy, ry, ay) = x, y
    rs, as_ = C.sizeof(abi.CdrSyncResult), C.sizeof(abi.CdrActivityInfo)
    dr = np.nonzero((rx.reshape(-1, rs) != ry.reshape(-1, rs)).any(axis=1))[0]
    da = np.nonzero((ax.reshape(-1, as_) != ay.reshape(-1, as_)).any(axis=1))[0]
    print(f"G={gx} vs G={gy}: {len(dr)} results and {len(da)} rows differ", flush=True)
    for i in dr[:6]:
        q = abi.CdrSyncActivity.from_buffer_copy(grouped[i].tobytes())
        print(" request", i, engine._rec(q, None))
        for g, r in ((gx, rx), (gy, ry)):
            print("  G", g, engine._rec(abi.CdrSyncResult.from_buffer_copy(r[i * rs:(i + 1) * rs].tobytes()), None))
    for j in da[:6]:
        for g, r in ((gx, ax), (gy, ay)):
            print(" row", j, "G", g, engine._rec(abi.CdrActivityInfo.from_buffer_copy(r[j * as_:(j + 1) * as_].tobytes()),
                                                 None), flush=True)


class Dev:
    def __init__(self):
        self.hip = engine._hip()
        h = self.hip
        h.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        h.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        h.hipEventSynchronize.argtypes = [C.c_void_p]
        h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.ptrs = []
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        self.ok(h.hipEventCreate(C.byref(self.e0)), "hipEventCreate")
        self.ok(h.hipEventCreate(C.byref(self.e1)), "hipEventCreate")

    @staticmethod
    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {rc}")

    def alloc(self, nbytes):
        p = C.c_void_p()
        self.ok(self.hip.hipMalloc(C.byref(p), C.c_size_t(max(64, nbytes))), "hipMalloc")
        self.ptrs.append(p)
        return p.value

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        if a.nbytes:
            self.ok(self.hip.hipMemcpy(p, a.ctypes.data, C.c_size_t(a.nbytes), H2D), "hipMemcpy H2D")
        return p

    def copy(self, dst, src, nbytes, kind):
        self.ok(self.hip.hipMemcpy(dst, src, C.c_size_t(nbytes), kind), "hipMemcpy")

    def timed(self, launch):
        """Kernel milliseconds between two events around `launch()` on the null stream."""
        self.ok(self.hip.hipEventRecord(self.e0, None), "hipEventRecord")
        launch()
        self.ok(self.hip.hipEventRecord(self.e1, None), "hipEventRecord")
        self.ok(self.hip.hipEventSynchronize(self.e1), "hipEventSynchronize")
        ms = C.c_float()
        self.ok(self.hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1), "hipEventElapsedTime")
        return float(ms.value)

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base", type=int, default=100_000, help="workflows generated and cut on the host")
    ap.add_argument("--tile", type=int, default=10, help="copies of the base states on the device")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=0x5EED0300 + 3)
    ap.add_argument("--copy-mib", type=int, default=1024, help="size of the stream-copy yardstick")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sync_activity.json"))
    ap.add_argument("--dry", action="store_true", help="host preparation only (states from the CPU oracle)")
    a = ap.parse_args()

    t = time.time()
    b = engine.synth_batch(3, a.base, seed=a.seed)
    pre, _ = engine.split_batch(b, 2)
    print(f"synth + split_batch: {a.base} workflows, {len(b.events)} events, {time.time() - t:.1f}s", flush=True)
    if a.dry:
        import oracle
        eng, st = None, oracle.replay(pre, threads=16)
    else:
        eng = engine.Engine(0)
        st = eng.replay(pre)
    n_states = a.base * a.tile
    inc = b.cluster.failover_version_increment
    host = tiled_state(st, a.tile)
    ok = sum(1 for w in range(st.n_wfs) if st.result[w].code == abi.OK)
    rows = sum(st.result[w].n_activity for w in range(st.n_wfs) if st.result[w].code == abi.OK)
    runs = {}
    for per_wf in (1, 4):
        t = time.time()
        reqs = sync.synth_requests(st, seed=1000 + per_wf, per_wf=per_wf, increment=inc)
        grouped, off = tiled_requests(reqs, a.base, a.tile)
        runs[per_wf] = (grouped, off)
        print(f"requests per workflow {per_wf}: {len(grouped)} requests, {time.time() - t:.1f}s", flush=True)
    rec = {"workload": "config 3 prefixes (engine.split_batch, seed 2)", "base_workflows": a.base, "tile": a.tile,
           "n_states": n_states, "ok_states": ok * a.tile, "activity_rows": rows * a.tile,
           "states_note": "base_workflows distinct workflows, tiled `tile` times: n_states records, not "
                          "n_states distinct workflows",
           "cache": "a stream copy of copy-mib runs between restoring the rows and every timed launch: the "
                    "launch starts with none of its data in L2 / Infinity Cache",
           "reps": a.reps, "timing": "HIP events around one launch, median of reps, G alternating per round",
           "runs": []}
    if a.dry:
        print(json.dumps(rec))
        return
    L = abi.lib()
    dev = Dev()
    try:
        o = abi.CdrOut()
        o.result, o.exec, o.repl = dev.up(host["result"]), dev.up(host["exec"]), dev.up(host["repl"])
        o.vh = dev.up(host["vh"])
        act0 = dev.up(host["act"])  # pristine rows
        act_bytes = host["act"].nbytes
        o.act = dev.alloc(act_bytes)
        d_caps = dev.up(host["caps"])
        # the yardstick: cdr_stream_copy_async over --copy-mib (read + write bytes)
        cb = a.copy_mib << 20
        src, dst = dev.alloc(cb), dev.alloc(cb)
        dev.hip.hipMemset(src, 1, C.c_size_t(cb))
        copy_ms = sorted(dev.timed(lambda: L.cdr_stream_copy_async(dst, src, cb, None)) for _ in range(a.reps + 2))
        copy_gbs = 2 * cb / (copy_ms[len(copy_ms) // 2] * 1e-3) / 1e9
        rec["stream_copy"] = {"mib": a.copy_mib, "ms_median": copy_ms[len(copy_ms) // 2], "gb_per_s": copy_gbs}
        print("stream copy", rec["stream_copy"], flush=True)
        for per_wf, (grouped, off) in runs.items():
            n = len(grouped)
            d_req, d_off = dev.up(grouped), dev.up(off)
            d_res = dev.alloc(n * C.sizeof(abi.CdrSyncResult))
            cl = b.cluster

            def launch():
                rc = L.cdr_sync_activity_async(eng.ctx, d_req, d_off, n, n_states, d_caps, C.byref(o), C.byref(cl),
                                               d_res, None)
                if rc:
                    raise RuntimeError(f"cdr_sync_activity_async rc={rc}")
            ms = {g: [] for g in abi.SYNC_GROUPS}
            digest, first = {}, None
            res_bytes = n * C.sizeof(abi.CdrSyncResult)
            for rep in range(a.reps + 1):  # round 0 warms every instantiation up and is checked
                for g in abi.SYNC_GROUPS:
                    eng.set_sync_group(g)
                    dev.copy(o.act, act0, act_bytes, D2D)
                    # evict what the restore and the previous launch left in L2 / Infinity Cache
                    L.cdr_stream_copy_async(dst, src, cb, None)
                    if rep == 0:  # a result the kernel does not write shows as action -1
                        dev.ok(dev.hip.hipMemset(d_res, 0xFF, C.c_size_t(res_bytes)), "hipMemset")
                    t_ms = dev.timed(launch)
                    if rep == 0:
                        hres = np.empty(res_bytes, np.uint8)
                        hact = np.empty(act_bytes, np.uint8)
                        dev.copy(hres.ctypes.data, d_res, res_bytes, D2H)
                        dev.copy(hact.ctypes.data, o.act, act_bytes, D2H)
                        digest[g] = hashlib.sha256(hres.tobytes() + hact.tobytes()).hexdigest()
                        if first is None:
                            first = (g, hres, hact)
                        elif digest[g] != digest[first[0]]:
                            describe_difference(first, (g, hres, hact), grouped)
                    else:
                        ms[g].append(t_ms)
            assert len(set(digest.values())) == 1, f"group sizes disagree: {digest}"
            # bytes the kernel must touch: requests in, results out, the rows of the addressed states
            addressed = np.diff(off[:n_states + 1].astype(np.int64)) > 0
            base_rows = np.array([st.result[w].n_activity if st.result[w].code == abi.OK else 0
                                  for w in range(st.n_wfs)], np.int64)
            must = n * (C.sizeof(abi.CdrSyncActivity) + C.sizeof(abi.CdrSyncResult)) + int(
                (np.tile(base_rows, a.tile) * addressed).sum()) * C.sizeof(abi.CdrActivityInfo)
            actions = np.bincount(hres.reshape(n, -1)[:, :4].copy().view(np.int32).ravel(), minlength=11)
            run = {"requests_per_workflow": per_wf, "n_requests": n, "must_touch_bytes": must,
                   "actions": {abi.SYNC_ACTIONS[i]: int(c) for i, c in enumerate(actions)},
                   "results_sha256": digest[abi.SYNC_GROUP], "groups": {}}
            for g in abi.SYNC_GROUPS:
                v = sorted(ms[g])
                med = v[len(v) // 2]
                gbs = must / (med * 1e-3) / 1e9
                run["groups"][str(g)] = {"ms_median": med, "ms_min": v[0], "ms_max": v[-1],
                                         "must_touch_gb_per_s": gbs, "share_of_stream_copy": gbs / copy_gbs,
                                         "requests_per_s": n / (med * 1e-3)}
            run["fastest_group"] = int(min(abi.SYNC_GROUPS, key=lambda g: run["groups"][str(g)]["ms_median"]))
            rec["runs"].append(run)
            print(json.dumps(run), flush=True)
        eng.set_sync_group(abi.SYNC_GROUP)
        rec["shipped_group"] = abi.SYNC_GROUP
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
