#!/usr/bin/env python3
"""Time of cdr_mutation_async (the WorkflowMutation of a carry-in replay) at full size.

A device-resident half-split carry batch as `bench.py --carry` builds it: the config's
population is synthesised, every history cut at the call boundary nearest after its middle,
the first halves replayed into the loaded-state buffer and the second halves replayed onto
it.  Then cdr_mutation_async over those two states is timed with device events, alternated
launch by launch with cdr_stream_copy_async moving the same number of bytes, and compared
with the carry replay step of the same batch.  One JSON line per config:

  ms            mean time of a cdr_mutation_async call
  bytes         what the algorithm has to move, from the counts: IN rows + OUT rows read,
                upsert rows + delete keys + info + upsert result written, and the result /
                caps records of both states read
  copy_ms       cdr_stream_copy_async with read + write traffic equal to `bytes`
  x_copy        ms / copy_ms
  replay_ms     the carry replay step (cdr_replay_sliced_async of the second halves)
  share         ms / replay_ms

usage: python tools/mutation_bench.py [--configs 3,5] [--wfs 1000000] [--steps 20] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch  # first: its HIP runtime is the process's (tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cadence_amd import abi, engine, ndc  # noqa: E402

ROW_BYTES = {t: C.sizeof(engine.TABLE_TYPES[t]) for t in engine.MUT_TABLES}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    return a, b


def run(cfg: int, n_wf: int, steps: int, warmup: int) -> dict:
    L = abi.lib()
    eng = engine.Engine(torch.cuda.current_device())
    dev = ndc._Dev()
    tstream = torch.cuda.current_stream()
    stream = C.c_void_p(tstream.cuda_stream)
    t0 = time.perf_counter()
    b = engine.synth_batch(cfg, n_wf, 0x5EED0000 + cfg)
    n = b.n_wfs
    cut = engine.split_half(b)
    pre, suf = engine.cut_batches(b, cut)
    pre_pl = engine.plan(pre)
    pre_db = ndc.upload_batch(dev, pre, pre_pl.caps, cls=True)
    pre_out = ndc.alloc_out(dev, n, pre_pl.totals)
    rc = L.cdr_replay_sliced_async(eng.ctx, C.byref(pre_db), C.byref(pre_out), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    pre_host = ndc.download_out(dev, pre_out, n, pre_pl)
    codes = np.frombuffer(pre_host.result, dtype=np.int32).reshape(n, -1)[:, 0]
    src = np.where((cut > 0) & (codes == abi.OK), np.arange(n), -1).astype(np.int32)
    for w in np.nonzero((cut > 0) & (codes != abi.OK))[0]:  # a failed prefix: the whole history, fresh
        suf.wfs[w] = b.wfs[w]
    suf.carry = engine.Carry(src=src, state=pre_host)
    spl = engine.plan(suf)
    suf.carry = None
    suf_db = ndc.upload_batch(dev, suf, spl.caps)
    dc = abi.CdrCarry()
    dc.src, dc.caps, dc.n_src, dc.totals, dc.state = dev.up(src), pre_db.caps, n, pre_pl.totals, pre_out
    suf_db.carry = dev.up(dc)
    suf_out = ndc.alloc_out(dev, n, spl.totals)
    log(f"C{cfg}: {n} entries, {int((src >= 0).sum())} carried, setup {time.perf_counter() - t0:.0f}s")

    def replay():
        assert L.cdr_replay_sliced_async(eng.ctx, C.byref(suf_db), C.byref(suf_out), stream) == 0
    for _ in range(2):
        replay()
    torch.cuda.synchronize()
    ev = [timed(replay, tstream) for _ in range(5)]
    torch.cuda.synchronize()
    replay_ms = float(np.mean([a.elapsed_time(z) for a, z in ev]))

    # the mutation's buffers: an upsert view with the replay's capacities, delete keys sized
    # by the loaded states' totals
    m = abi.CdrMutation()
    m.upsert = ndc.alloc_out(dev, n, spl.totals)
    m.upsert.exec, m.upsert.repl = suf_out.exec, suf_out.repl
    m.upsert.vh, m.upsert.rp, m.upsert.sa = suf_out.vh, suf_out.rp, suf_out.sa
    for t in engine.MUT_TABLES:
        setattr(m, "del_" + t, dev.alloc(8 * max(1, getattr(pre_pl.totals, t))))
    m.info = dev.alloc(C.sizeof(abi.CdrMutInfo) * n)

    def mutate():
        assert L.cdr_mutation_async(eng.ctx, C.byref(suf_db), C.byref(suf_out), C.byref(m), stream) == 0
    mutate()
    torch.cuda.synchronize()
    # bytes from the counts
    info = (abi.CdrMutInfo * n)()
    up_res = (abi.CdrWfResult * n)()
    out_res = (abi.CdrWfResult * n)()
    dev.down(info, m.info)
    dev.down(up_res, m.upsert.result)
    dev.down(out_res, suf_out.result)
    inf = np.frombuffer(info, dtype=np.uint32).reshape(n, -1)
    ures = np.frombuffer(up_res, dtype=np.uint32).reshape(n, -1)
    ores = np.frombuffer(out_res, dtype=np.uint32).reshape(n, -1)
    pres = np.frombuffer(pre_host.result, dtype=np.uint32).reshape(n, -1)
    ok = ores[:, 0] == abi.OK
    stored = ok & (src >= 0)
    c0 = abi.CdrWfResult.n_activity.offset // 4
    d0 = abi.CdrMutInfo.n_del_act.offset // 4
    counts, nbytes = {}, 0
    for k, t in enumerate(engine.MUT_TABLES):
        n_in, n_out = int(pres[stored, c0 + k].sum()), int(ores[ok, c0 + k].sum())
        n_up, n_del = int(ures[ok, c0 + k].sum()), int(inf[:, d0 + k].sum())
        counts[t] = {"in": n_in, "out": n_out, "upsert": n_up, "delete": n_del}
        nbytes += (n_in + n_out + n_up) * ROW_BYTES[t] + n_del * 8
    rec = C.sizeof(abi.CdrWfResult) + C.sizeof(abi.CdrWfCaps)
    nbytes += n * (rec + 4) + int(stored.sum()) * (rec + 8)          # both states' result / caps, src, condition
    nbytes += n * (C.sizeof(abi.CdrMutInfo) + C.sizeof(abi.CdrWfResult))  # written per entry
    codes_m = {int(c): int(k) for c, k in zip(*np.unique(inf[:, 0], return_counts=True))}

    half = max(64, (nbytes // 2) // 64 * 64)  # the copy reads and writes `half` bytes each
    ca, cb = dev.alloc(half, zero=True), dev.alloc(half, zero=False)

    def copy():
        assert L.cdr_stream_copy_async(cb, ca, half, stream) == 0
    for _ in range(warmup):
        mutate()
        copy()
    torch.cuda.synchronize()
    em, ec = [], []
    for _ in range(steps):
        em.append(timed(mutate, tstream))
        ec.append(timed(copy, tstream))
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(z) for a, z in em])
    cms = np.array([a.elapsed_time(z) for a, z in ec])
    line = {
        "tool": "mutation_bench", "workload": f"C{cfg}-{n_wf}wf-carry-half-mutation", "entries": n,
        "carried": int((src >= 0).sum()), "steps": steps, "ms": round(float(ms.mean()), 4),
        "ms_min": round(float(ms.min()), 4), "ms_max": round(float(ms.max()), 4), "bytes": int(nbytes),
        "gbs": round(nbytes / ms.mean() / 1e6, 1), "copy_ms": round(float(cms.mean()), 4),
        "copy_gbs": round(2 * half / cms.mean() / 1e6, 1), "x_copy": round(float(ms.mean() / cms.mean()), 2),
        "replay_ms": round(replay_ms, 3), "share": round(float(ms.mean()) / replay_ms, 4), "codes": codes_m,
        "rows": counts, "lib_flags": int(L.cdr_build_flags()),
    }
    dev.close()
    eng.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="3,5")
    ap.add_argument("--wfs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    for cfg in (int(c) for c in args.configs.split(",")):
        line = json.dumps(run(cfg, args.wfs, max(20, args.steps), args.warmup))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
