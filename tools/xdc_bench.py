#!/usr/bin/env python3
"""Measure the 2DC replication round (cdr_xdc_admit_async, cdr_xdc_replicate_async).

States: --n workflows, copies of --base distinct config-3 histories (2DC builder), each cut at
the call boundary nearest its middle — the checkpoint.  The state buffer holds every workflow's prefix, written by this cluster; the
incoming task carries the rest at the remote cluster's version.  Three mixes of tasks over the
same reset (prefix, page calls) and apply (suffix) batches differ in their ReplicationInfo
alone: a task that finds the event ids matching is applied (APPLY); one whose ReplicationInfo
lacks this cluster resets to the remote's checkpoint — the same prefix — and is then applied
(RESET_APPLY).  Timed with HIP events, the state restored from a pristine copy before every
launch, the mixes alternating over --reps rounds:

  admit     k_xdc_admit alone
  round     cdr_xdc_replicate_async
  direct    the same reset (masked alike) and apply batches through cdr_replay_sliced_async,
            with a carry descriptor built on the host: what admission, masking, the post-reset
            check and the adoption of the states cost is round - direct

Writes one JSON record (--out); run it in several processes for the spread.

    python tools/xdc_bench.py --out profiles/xdc_replicate.json
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

from cadence_amd import abi, engine, ndc, xdc  # noqa: E402

V_LOCAL, V_REMOTE, V_ALT = 1, 12, 2  # default cluster metadata: increment 10, clusters 0 (current), 1, 2
MIXES = (("all_apply", 0.0), ("reset_10pct", 0.1), ("all_reset", 1.0))
D2D = 3


def raw(x, ty, n):
    return np.frombuffer(x, dtype=np.uint8)[:n * C.sizeof(ty)].reshape(n, C.sizeof(ty))


def col(m, field, dt):
    return m[:, field.offset:field.offset + field.size].view(dt)[:, 0]


def build(base_n, n, seed):
    """(reset batch, apply batch, the base histories' tasks as a uint8 matrix, their checkpoint event
    ids, events and prefix events of the base histories)"""
    whole = engine.synth_batch(3, base_n, seed, builder=abi.BUILDER_2DC)
    assert whole.n_wfs == base_n
    cut = engine.split_half(whole)
    ev = (abi.CdrEvent * len(whole.events))()
    C.memmove(ev, whole.events, C.sizeof(ev))
    em = raw(ev, abi.CdrEvent, len(ev))
    wf = raw(whole.wfs, abi.CdrWfDesc, base_n)
    off = col(wf, abi.CdrWfDesc.ev_off, np.uint64).astype(np.int64)
    ln = col(wf, abi.CdrWfDesc.ev_len, np.uint64).astype(np.int64)
    cut = np.where(cut > 0, cut, ln)  # an entry of one call: the prefix is all of it, the task is empty
    owner = np.repeat(np.arange(base_n), ln)
    pos = np.arange(len(ev), dtype=np.int64) - off[owner]
    in_prefix = pos < cut[owner]
    col(em, abi.CdrEvent.version, np.int64)[:] = np.where(in_prefix, V_LOCAL, V_REMOTE)
    flags = col(em, abi.CdrEvent.flags, np.uint32)
    paged = np.where(pos % xdc.PAGE_SIZE == 0, abi.EVF_BATCH_FIRST, 0).astype(np.uint32)
    flags[:] = np.where(in_prefix, (flags & ~np.uint32(abi.EVF_BATCH_FIRST)) | paged, flags)
    ids = col(em, abi.CdrEvent.event_id, np.int64)

    # the copies: events and descriptors `tiles` times over (the packer sizes its arena by the
    # events it is given, so copies cannot share them)
    tiles = n // base_n
    n_ev = len(ev)
    if tiles > 1:
        big = (abi.CdrEvent * (n_ev * tiles))()
        bm = raw(big, abi.CdrEvent, n_ev * tiles)
        for k in range(tiles):
            bm[k * n_ev:(k + 1) * n_ev] = em
        ev = big
    tile_of = np.arange(n, dtype=np.int64) // base_n

    def descs(lo, length):
        d = np.tile(wf, (tiles, 1))
        col(d, abi.CdrWfDesc.ev_off, np.uint64)[:] = (np.tile(lo, tiles) + tile_of * n_ev).astype(np.uint64)
        col(d, abi.CdrWfDesc.ev_len, np.uint64)[:] = np.tile(length, tiles).astype(np.uint64)
        col(d, abi.CdrWfDesc.wf_key, np.uint64)[:] += tile_of.astype(np.uint64) << np.uint64(40)
        out = (abi.CdrWfDesc * n)()
        C.memmove(out, d.ctypes.data, d.nbytes)
        return out

    def batch(wfs):
        return engine.Batch(events=ev, wfs=wfs, kvs=whole.kvs, rps=whole.rps, cluster=whole.cluster,
                            now_ns=whole.now_ns, uuid_seed=whole.uuid_seed, empty_uuid=whole.empty_uuid)
    reset = batch(descs(off, cut))
    apply = batch(descs(off + cut, ln - cut))
    tasks = xdc.new_tasks(base_n)
    for w in range(base_n):
        if ln[w] > cut[w]:
            xdc.task_from_entry(tasks[w], apply, w, version=V_REMOTE)
        # (else: n_events 0, an empty task)
    e_c = ids[off + cut - 1]
    return reset, apply, raw(tasks, abi.CdrXdcTask, base_n), e_c, int(ln.sum()), int(cut.sum())


def mix_tasks(base_tasks, e_c, n, share, seed):
    """The base tasks tiled to n, `share` of them without this cluster's ReplicationInfo (the
    remote's entry names the checkpoint): RESET_APPLY; the rest with it: APPLY."""
    base_n = len(base_tasks)
    t = np.tile(base_tasks, (-(-n // base_n), 1))[:n].copy()
    ec = np.resize(e_c, n)
    rst = np.random.default_rng(seed).random(n) < share
    T = abi.CdrXdcTask
    col(t, T.ri_mask, np.uint32)[:] = np.where(rst, 2, 1)
    for name, c, v in (("ri_version", 0, V_LOCAL), ("ri_version", 1, V_ALT)):
        f = getattr(T, name)
        t[:, f.offset + 8 * c:f.offset + 8 * c + 8].view(np.int64)[:, 0] = v
    f = T.ri_last_event_id
    for c in (0, 1):
        t[:, f.offset + 8 * c:f.offset + 8 * c + 8].view(np.int64)[:, 0] = ec
    return np.ascontiguousarray(t), rst


class Timer:
    def __init__(self, hip):
        self.hip = hip
        hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        hip.hipEventSynchronize.argtypes = [C.c_void_p]
        hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(self.e0)) == 0 and hip.hipEventCreate(C.byref(self.e1)) == 0

    def __call__(self, launch):
        h = self.hip
        assert h.hipEventRecord(self.e0, None) == 0
        launch()
        assert h.hipEventRecord(self.e1, None) == 0 and h.hipEventSynchronize(self.e1) == 0
        ms = C.c_float()
        assert h.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return float(ms.value)


def stats(v):
    v = sorted(v)
    return {"ms_median": v[len(v) // 2], "ms_min": v[0], "ms_max": v[-1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000, help="states (workflows) on the device")
    ap.add_argument("--base", type=int, default=20_000, help="distinct histories generated on the host")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0x5EED0300 + 3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xdc_replicate.json"))
    ap.add_argument("--dry", action="store_true", help="host preparation only")
    a = ap.parse_args()
    base_n = min(a.base, a.n)
    n = a.n // base_n * base_n  # whole copies of the base histories
    t0 = time.time()
    reset, apply, base_tasks, e_c, n_ev, n_pre = build(base_n, n, a.seed)
    mixes = {name: mix_tasks(base_tasks, e_c, n, share, 7) for name, share in MIXES}
    tasks0 = (abi.CdrXdcTask * n).from_buffer(mixes["all_apply"][0])
    print(f"host: {n} states over {base_n} histories ({n_ev} events, {n_pre} before the checkpoints), "
          f"{time.time() - t0:.1f}s", flush=True)
    rec = {"workload": "config 3 (2DC builder) cut at the call boundary nearest the middle; one task per state",
           "n_states": n, "base_histories": base_n,
           "states_note": "n_states records, copies of base_histories distinct histories",
           "events_per_state": n_ev / base_n, "prefix_events_per_state": n_pre / base_n, "reps": a.reps,
           "timing": "HIP events around the call on the null stream; the state restored from a pristine copy "
                     "before every launch; mixes alternate per round; round 0 warms up and is checked",
           "mixes": {}}
    if a.dry:
        print(json.dumps(rec))
        return
    eng = engine.Engine(0)
    rounds = [(reset, apply, tasks0)]
    rep = xdc.DeviceReplicator(eng, reset, rounds, reset_tasks=False)
    print(f"device batches: {time.time() - t0:.1f}s", flush=True)
    L, dev, hip = abi.lib(), rep.dev, rep.dev.hip
    timed = Timer(hip)
    try:
        r, _, ap_plan = rep.rounds[0]
        rep.base_replay()
        tot = rep.state_plan.totals
        sizes = [("result", C.sizeof(abi.CdrWfResult) * n), ("exec", C.sizeof(abi.CdrExecInfo) * n),
                 ("repl", C.sizeof(abi.CdrReplState) * n)] + [
                     (t, C.sizeof(engine.TABLE_TYPES[t]) * max(1, getattr(tot, t))) for t in engine.TABLES]
        pristine = {name: dev.alloc(nb, zero=False) for name, nb in sizes}

        def copy_state(to_pristine):
            for name, nb in sizes:
                dst, src = (pristine[name], getattr(rep.state, name)) if to_pristine else (
                    getattr(rep.state, name), pristine[name])
                assert hip.hipMemcpy(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nb), D2D) == 0
        copy_state(True)
        st = ndc.download_out(dev, rep.state, n, rep.state_plan)
        rec["ok_states"] = int(sum(1 for w in range(0, n, max(1, n // 1000)) if st.result[w].code == abi.OK))
        rec["ok_states_note"] = "of a sample of every (n/1000)-th state"
        d_tasks = {name: dev.up(t) for name, (t, _) in mixes.items()}
        d_skip = {name: dev.up((~rst).astype(np.uint8)) for name, (_, rst) in mixes.items()}
        # the direct replays' carry: every entry onto its own state
        cy = abi.CdrCarry()
        cy.src = dev.up(np.arange(n, dtype=np.int32))
        cy.caps, cy.n_src = rep.state_caps_d, n
        cy.state = abi.CdrOut.from_buffer_copy(rep.state)
        d_cy = dev.up(cy)
        rs_db, ap_db = abi.CdrDevBatch.from_buffer_copy(r.reset), abi.CdrDevBatch.from_buffer_copy(r.apply)
        ap_db.carry = d_cy
        ap_db.cls_slab = ap_db.cls_row0 = ap_db.cls_rows = None
        ms = {name: {"admit": [], "round": [], "direct": []} for name, _ in MIXES}
        cluster = rep.cluster
        for k in range(a.reps + 1):
            for name, share in MIXES:
                r.tasks = d_tasks[name]
                rs_db.skip = d_skip[name]

                def admit():
                    rc = L.cdr_xdc_admit_async(eng.ctx, C.c_void_p(r.tasks), n, C.c_void_p(rep.state_caps_d),
                                               C.byref(rep.state), C.byref(cluster), C.c_void_p(r.dec), None)
                    assert rc == 0, rc

                def direct():
                    if share > 0:
                        rc = L.cdr_replay_sliced_async(eng.ctx, C.byref(rs_db), C.byref(r.reset_out), None)
                        assert rc == 0, rc
                    rc = L.cdr_replay_sliced_async(eng.ctx, C.byref(ap_db), C.byref(r.apply_out), None)
                    assert rc == 0, rc
                copy_state(False)
                t_admit = timed(admit)
                t_direct = timed(direct)
                copy_state(False)
                t_round = timed(lambda: rep.round(0))
                if k == 0:
                    dec = xdc.new_decisions(n)
                    dev.down(dec, r.dec)
                    d = raw(dec, abi.CdrXdcDecision, n)
                    act = np.bincount(col(d, abi.CdrXdcDecision.action, np.int32), minlength=8)
                    ran = int((col(d, abi.CdrXdcDecision.flags, np.uint32) & abi.XDD_RESET_RAN != 0).sum())
                    res = np.empty(n * C.sizeof(abi.CdrWfResult), np.uint8)
                    assert hip.hipMemcpy(C.c_void_p(res.ctypes.data), C.c_void_p(rep.state.result),
                                         C.c_size_t(res.nbytes), 2) == 0
                    codes = np.bincount(res.reshape(n, -1)[:, :4].copy().view(np.int32).ravel().clip(0, 127))
                    rec["mixes"][name] = {"reset_share": share, "resets_run": ran,
                                          "actions": {abi.XDC_ACTIONS[i]: int(c) for i, c in enumerate(act) if c},
                                          "state_codes": {abi.STATUS.get(i, str(i)): int(c)
                                                          for i, c in enumerate(codes) if c}}
                else:
                    for what, t in (("admit", t_admit), ("round", t_round), ("direct", t_direct)):
                        ms[name][what].append(t)
        for name, _ in MIXES:
            m = rec["mixes"][name]
            for what in ("admit", "round", "direct"):
                m[what] = stats(ms[name][what])
            m["round_minus_direct_ms"] = m["round"]["ms_median"] - m["direct"]["ms_median"]
            m["tasks_per_s"] = n / (m["round"]["ms_median"] * 1e-3)
            print(name, json.dumps(m), flush=True)
    finally:
        rep.close()
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
