"""Reference WorkflowMutation: a plain dict diff of two states' pending rows.

The contract (include/cdr/schema.h cdr_mutation), restated with nothing of the kernel's
method in it — no sorted merge, no ranks: per entry and table, rows are keyed in a dict and
compared as bytes.

  upsert   every OUT row whose key is absent from IN or whose record differs from IN's
  delete   the key of every IN row whose key is absent from OUT
  cond.    IN.exec.next_event_id

An entry with no stored predecessor (carry.src < 0, or carry.in_memory set) is a snapshot:
every OUT row upserted, nothing deleted, condition 0.  An entry whose replay is not OK has
no rows at all.  Lists come out in ascending key order (what the kernel promises).
"""
from cadence_amd import abi, engine

TABLES = engine.MUT_TABLES
KEY = {"act": "schedule_id", "timer": "timer_id", "child": "initiated_id", "cancel": "initiated_id",
       "signal": "initiated_id"}


def _b(row) -> bytes:
    return bytes(memoryview(row).cast("B"))


class EntryMutation:
    def __init__(self):
        self.code, self.flags, self.condition = abi.MUT_OK, 0, 0
        self.upserts = {t: [] for t in TABLES}   # row bytes, ascending key
        self.deletes = {t: [] for t in TABLES}   # keys, ascending
        # the four classes of (unchanged, changed, deleted, new) rows per table
        self.classes = {t: [0, 0, 0, 0] for t in TABLES}


def in_rows(batch, w: int, table: str):
    """The stored predecessor's rows of entry w (none for a snapshot entry)."""
    cy = batch.carry
    src = int(cy.src[w])
    if src < 0 or (cy.in_memory is not None and cy.in_memory[w]):
        return []
    return cy.state.rows(src, table)


def entry_mutation(batch, out, w: int) -> EntryMutation:
    m = EntryMutation()
    cy = batch.carry
    src = int(cy.src[w])
    snapshot = src < 0 or (cy.in_memory is not None and bool(cy.in_memory[w]))
    m.flags = abi.MUT_SNAPSHOT if snapshot else 0
    m.condition = 0 if snapshot else cy.state.exec[src].next_event_id
    if out.result[w].code != abi.OK:
        m.code = abi.MUT_NOT_OK
        return m
    for t in TABLES:
        old = {getattr(r, KEY[t]): _b(r) for r in in_rows(batch, w, t)}
        new = {getattr(r, KEY[t]): _b(r) for r in out.rows(w, t)}
        for k in sorted(new):
            if k not in old:
                m.classes[t][3] += 1
                m.upserts[t].append(new[k])
            elif old[k] != new[k]:
                m.classes[t][1] += 1
                m.upserts[t].append(new[k])
            else:
                m.classes[t][0] += 1
        for k in sorted(old):
            if k not in new:
                m.classes[t][2] += 1
                m.deletes[t].append(k)
    return m


def mutation(batch, out) -> list:
    return [entry_mutation(batch, out, w) for w in range(batch.n_wfs)]


def apply(batch, out, w: int, m: EntryMutation, table: str) -> list:
    """The stored rows of entry w after the mutation: upserts first, then deletes —
    as row bytes in ascending key order."""
    size = len(_b(engine.TABLE_TYPES[table]()))
    ty = engine.TABLE_TYPES[table]
    store = {getattr(r, KEY[table]): _b(r) for r in in_rows(batch, w, table)}
    for raw in m.upserts[table]:
        assert len(raw) == size
        store[getattr(ty.from_buffer_copy(raw), KEY[table])] = raw
    for k in m.deletes[table]:
        del store[k]  # a delete must remove exactly one row (workflowStateMaps.go:108-133)
    return [store[k] for k in sorted(store)]


def check(batch, out, mut, ref=None, fill=None, skip=()) -> list:
    """Mismatches between an engine.Mutation and the reference (of the same `out`): info,
    upsert result, upsert rows (bytes, in order), delete keys (in order); with `fill`, also
    that every byte past an entry's counts — the rest of its upsert and delete slices —
    still holds the fill byte.  Entries in `skip` are left to the caller."""
    ref = ref or mutation(batch, out)
    bad = []
    caps, cy = out.plan.caps, batch.carry
    for w in range(batch.n_wfs):
        if w in skip:
            continue
        m, info, r, ur = ref[w], mut.info[w], out.result[w], mut.upsert.result[w]
        if (info.code, info.flags, info.condition) != (m.code, m.flags, m.condition):
            bad.append(f"wf {w}: info {(info.code, info.flags, info.condition)} != {(m.code, m.flags, m.condition)}")
        want = abi.CdrWfResult.from_buffer_copy(_b(r))
        if m.code == abi.MUT_OK:
            for t in TABLES:
                setattr(want, engine.TABLE_COUNT[t], len(m.upserts[t]))
        if _b(ur) != _b(want):
            bad.append(f"wf {w}: upsert result differs")
            continue
        src = int(cy.src[w])
        for t in TABLES:
            got = [_b(x) for x in mut.upsert.rows(w, t)] if m.code == abi.MUT_OK else []
            if got != m.upserts[t]:
                bad.append(f"wf {w}: {t} upserts differ ({len(got)} rows, want {len(m.upserts[t])})")
            nd = getattr(info, "n_del_" + t)
            if nd != len(m.deletes[t]) or mut.deleted(w, t) != m.deletes[t]:
                bad.append(f"wf {w}: {t} deletes {mut.deleted(w, t) if nd < 20 else nd} != {m.deletes[t][:20]}")
            if fill is not None:
                size = len(_b(engine.TABLE_TYPES[t]()))
                off, cap = getattr(caps[w], t + "_off"), getattr(caps[w], t + "_cap")
                raw = bytes(memoryview(mut.upsert.tables[t]).cast("B")[(off + len(got)) * size:(off + cap) * size])
                if raw != bytes([fill]) * len(raw):
                    bad.append(f"wf {w}: {t} upsert slice written past its count")
                if src >= 0:
                    sc = cy.state.plan.caps[src]
                    off, cap = getattr(sc, t + "_off"), getattr(sc, t + "_cap")
                    raw = bytes(memoryview(mut.dels[t]).cast("B")[(off + nd) * 8:(off + cap) * 8])
                    if raw != bytes([fill]) * len(raw):
                        bad.append(f"wf {w}: {t} delete slice written past its count")
        if len(bad) >= 10:
            break
    return bad
