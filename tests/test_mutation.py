"""WorkflowMutation of a carry-in replay (cdr_mutation_async / cdr_mutation_batch): the
rows to upsert, the keys to delete and the condition that CloseTransactionAsMutation
(mutableStateBuilder.go:3721-3785) hands to UpdateWorkflowExecution, as the net difference
of the loaded state and the replayed one.

The reference is tests/mutation_ref.py: a dict diff of the two states' rows.  CPU: the
reference applied to the loaded rows reproduces the replayed rows, and the fixtures hold
every class of row (unchanged, changed, deleted, new), fresh and failed entries.  GPU: the
kernel equals the reference on replayed batches and on hand-made states (sizes around the
wave width, neighbours of very different sizes, keys around 2^31 and large), verifies the
key order, and its upsert view feeds the row encoders unchanged.
"""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest

from cadence_amd import abi, engine
from tests import mutation_ref as ref
from tests.states import make_state

TABLES = ref.TABLES
FILL = 0xA5


def _carry_batch(replay, cfg=None, builder=None):
    """The carry-in batches of tests/test_carry.py (test_gpu_carry_matches_oracle's configs,
    test_gpu_carry_builders' builders): prefix and suffix replayed by `replay`."""
    if builder is None:
        b = engine.synth_batch(cfg, 300, seed=0x5EED0200 + cfg, error_rate=0.1 if cfg in (0, 3) else 0.0)
        pre, cut = engine.split_batch(b, cfg + 7)
    else:
        b = engine.synth_batch(0, 300, seed=41 + builder, builder=builder, error_rate=0.2)
        pre, cut = engine.split_batch(b, builder + 3)
    sb = engine.suffix_batch(b, cut, pre, replay(pre))
    return sb, replay(sb)


@functools.lru_cache(maxsize=None)
def _oracle_batch(cfg):
    import oracle
    return _carry_batch(oracle.replay, cfg)


# ---------------------------------------------------------------- CPU
@pytest.mark.parametrize("cfg", [0, 2, 3, 4, 5])
def test_reference_applies_and_fixtures_cover(cfg):
    """IN + reference mutation == OUT, bytewise; and the fixtures hold every class, so a
    kernel that upserts everything or deletes nothing cannot pass the parity tests."""
    sb, out = _oracle_batch(cfg)
    muts = ref.mutation(sb, out)
    tot = {t: np.zeros(4, np.int64) for t in TABLES}  # unchanged, changed, deleted, new
    fresh = failed = 0
    for w, m in enumerate(muts):
        fresh += sb.carry.src[w] < 0
        if m.code != abi.MUT_OK:
            failed += 1
            assert not any(m.upserts[t] or m.deletes[t] for t in TABLES)
            continue
        for t in TABLES:
            assert ref.apply(sb, out, w, m, t) == [ref._b(r) for r in out.rows(w, t)], (w, t)
            tot[t] += m.classes[t] if sb.carry.src[w] >= 0 else [0, 0, 0, 0]
    print(cfg, {t: tot[t].tolist() for t in TABLES}, "fresh", fresh, "failed", failed)
    if cfg == 3:
        for t in ("act", "timer", "child"):
            assert (tot[t] > 0).all(), (t, tot[t])
        for t in ("cancel", "signal"):
            assert tot[t][0] > 0 and tot[t][2] > 0 and tot[t][3] > 0, (t, tot[t])
    if cfg == 5:
        for t in ("act", "timer", "child"):
            assert (tot[t] > 0).all(), (t, tot[t])
    if cfg == 2:
        assert tot["act"][2] > 0
    if cfg == 0:
        assert fresh > 0 and failed > 0
    if cfg == 4:
        assert fresh > 0
    for t in ("cancel", "signal"):  # no Replicate* method edits these rows in place
        assert tot[t][1] == 0


def test_abi_mirrors():
    L = abi.lib()
    assert C.sizeof(abi.CdrMutInfo) == 40 == L.cdr_struct_size(b"cdr_mut_info")
    assert C.sizeof(abi.CdrMutation) == C.sizeof(abi.CdrOut) + 6 * 8 == L.cdr_struct_size(b"cdr_mutation")
    assert (abi.MUT_OK, abi.MUT_NOT_OK, abi.MUT_E_ORDER, abi.MUT_SNAPSHOT) == (0, 1, 2, 1)
    assert L.cdr_mutation_async.argtypes and L.cdr_mutation_batch.argtypes
    abi.check_layouts()


# ---------------------------------------------------------------- hand-made states
def _row(table, key, salt=0):
    """A record with every byte set from (table, key, salt) and the key in its key field."""
    ty = engine.TABLE_TYPES[table]
    raw = b""
    while len(raw) < C.sizeof(ty):
        raw += hashlib.sha256(f"{table}/{key}/{salt}/{len(raw)}".encode()).digest()
    r = ty.from_buffer_copy(raw[:C.sizeof(ty)])
    setattr(r, ref.KEY[table], key)
    return r


def _last_word_changed(table, row):
    """A copy of `row` that differs only in the last byte of its last 8-byte word (never
    the key: the timer's key is the low half of that word)."""
    raw = bytearray(ref._b(row))
    raw[-1] ^= 0x80
    return engine.TABLE_TYPES[table].from_buffer_copy(bytes(raw))


def _universe(table, n):
    """n ascending unique keys straddling 2^31, the last quarter large (timer keys are
    32-bit handles: past 2^31 + 2^30, where a sign extension would sort them first)."""
    big = (1 << 30) if table == "timer" else (1 << 62)
    return [(1 << 31) - n // 2 + i + (big if i >= n - n // 4 else 0) for i in range(n)]


def _case_rows(table, case, salt):
    """(IN rows, OUT rows) of one hand-made case."""
    def rows(keys, changed=()):
        return [_row(table, k, salt + (1 if k in changed else 0)) for k in keys]
    kind = case[0]
    if kind == "sizes":  # n_in first keys and n_out last keys of a universe; every other shared key changed
        _, n_in, n_out, n_uni = case
        u = _universe(table, n_uni)
        ki, ko = u[:n_in], u[n_uni - n_out:]
        shared = [k for k in ki if k in set(ko)]
        return rows(ki), rows(ko, set(shared[::2]))
    if kind == "same":
        u = _universe(table, 1)
        return rows(u), rows(u)
    if kind == "lastword":
        r = _row(table, _universe(table, 1)[0], salt)
        return [r], [_last_word_changed(table, r)]
    if kind == "interleaved":  # 300 / 300: half the keys of each shared, half of those changed
        u = _universe(table, 450)
        ki = [k for i, k in enumerate(u) if i % 3 != 2]
        ko = [k for i, k in enumerate(u) if i % 3 != 1]
        return rows(ki), rows(ko, {k for i, k in enumerate(u) if i % 6 == 0})
    if kind == "sparse":  # (1000, 3) or (3, 1000): three keys spread over the long side, the middle one changed
        u = _universe(table, 1000)
        few = [u[0], u[500], u[999]]
        if case[1] == "in_long":
            return rows(u), rows(few, {u[500]})
        return rows(few), rows(u, {u[500]})
    raise AssertionError(case)


CASES = [("sizes", 0, 0, 1), ("sparse", "in_long"), ("sizes", 0, 1, 1), ("sizes", 63, 65, 100), ("sizes", 1, 0, 1),
         ("interleaved",), ("same",), ("sizes", 64, 64, 100), ("lastword",), ("sparse", "out_long"),
         ("sizes", 65, 63, 100), ("sizes", 129, 0, 129), ("sizes", 0, 129, 129)]


def _hand_made(entries, src=None):
    """(batch, out) of hand-made entries [(IN tables, OUT tables)]: loaded record src[w]
    (default: the records in reverse order) and entry w's replayed state."""
    n = len(entries)
    src = np.asarray(src if src is not None else [n - 1 - w for w in range(n)], np.int32)
    ins = [{t: [] for t in TABLES} for _ in range(n)]
    for w, (tin, _) in enumerate(entries):
        if src[w] >= 0:
            ins[src[w]] = tin
    _, st_in = make_state(ins, lambda w: w % 3)
    batch, st_out = make_state([tout for _, tout in entries], lambda w: (w + 1) % 4)
    batch.carry = engine.Carry(src=src, state=st_in)
    return batch, st_out


@functools.lru_cache(maxsize=None)
def _case_batch():
    entries = []
    for rep in range(3):
        for i in range(len(CASES)):
            case = CASES[(i + 5 * rep) % len(CASES)]
            pairs = {t: _case_rows(t, case, salt=10 * rep) for t in TABLES}
            entries.append(({t: pairs[t][0] for t in TABLES}, {t: pairs[t][1] for t in TABLES}))
    # a fresh builder among them: its loaded record is unused, every row an upsert
    pairs = {t: _case_rows(t, ("sizes", 0, 5, 5), 3) for t in TABLES}
    entries.append(({t: [] for t in TABLES}, {t: pairs[t][1] for t in TABLES}))
    src = [len(entries) - 1 - w for w in range(len(entries))]
    src[-1] = -1
    batch, out = _hand_made(entries, src)
    return batch, out, ref.mutation(batch, out)


def test_hand_made_reference():
    """The hand-made cases hold what they claim (CPU): the reference applies, and every
    class of row occurs in every table."""
    batch, out, muts = _case_batch()
    assert batch.n_wfs == 40
    for t in TABLES:
        assert (np.sum([m.classes[t] for m in muts], axis=0) > 0).all()
        for w, m in enumerate(muts):
            assert ref.apply(batch, out, w, m, t) == [ref._b(r) for r in out.rows(w, t)]
    assert muts[-1].flags == abi.MUT_SNAPSHOT and muts[-1].condition == 0
    assert muts[0].condition == 1000 + 7 * 39


# ---------------------------------------------------------------- GPU
def _assert_equal(batch, out, mut, **kw):
    bad = ref.check(batch, out, mut, **kw)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,builder", [(0, None), (2, None), (3, None), (4, None), (5, None),
                                         (0, abi.BUILDER_LOCAL), (0, abi.BUILDER_2DC), (0, abi.BUILDER_NDC)])
def test_gpu_mutation_matches_reference(engine_gpu, cfg, builder):
    """Prefix and suffix replayed on the GPU; the kernel's mutation == the dict diff of the
    same outputs, and nothing is written past an entry's counts or for a failed entry."""
    sb, out = _carry_batch(engine_gpu.replay, cfg, builder)
    mut = engine_gpu.mutation(sb, out, fill=FILL)
    muts = ref.mutation(sb, out)
    _assert_equal(sb, out, mut, ref=muts, fill=FILL)
    for w, m in enumerate(muts):
        assert (m.flags == abi.MUT_SNAPSHOT) == (sb.carry.src[w] < 0)
        assert (m.code == abi.MUT_NOT_OK) == (out.result[w].code != abi.OK)
    if builder is not None or cfg == 0:
        assert any(m.code == abi.MUT_NOT_OK for m in muts)
    assert any(m.code == abi.MUT_OK and sb.carry.src[w] >= 0 for w, m in enumerate(muts)) or cfg == 4


@pytest.mark.gpu
def test_gpu_hand_made_states(engine_gpu):
    batch, out, muts = _case_batch()
    mut = engine_gpu.mutation(batch, out, fill=FILL)
    _assert_equal(batch, out, mut, ref=muts, fill=FILL)


@pytest.mark.gpu
def test_gpu_order_check(engine_gpu):
    """A descending pair (OUT activities of entry 3) and a duplicate key (IN timers of
    entry 5): those entries get CDR_MUT_E_ORDER and zero counts, the others are exact."""
    entries = []
    for w in range(9):
        pairs = {t: _case_rows(t, ("sizes", 20 + 3 * w, 30 - w, 40), w) for t in TABLES}
        entries.append(({t: pairs[t][0] for t in TABLES}, {t: pairs[t][1] for t in TABLES}))
    a = entries[3][1]["act"]
    a[10], a[11] = a[11], a[10]
    tm = entries[5][0]["timer"]
    tm[7] = _row("timer", tm[6].timer_id, 99)
    batch, out = _hand_made(entries, src=list(range(9)))
    mut = engine_gpu.mutation(batch, out, fill=FILL)
    for w in (3, 5):
        info = mut.info[w]
        assert info.code == abi.MUT_E_ORDER and info.flags == 0
        assert [getattr(info, "n_del_" + t) for t in TABLES] == [0] * 5
        assert [getattr(mut.upsert.result[w], engine.TABLE_COUNT[t]) for t in TABLES] == [0] * 5
    _assert_equal(batch, out, mut, fill=FILL, skip=(3, 5))


@pytest.mark.gpu
def test_gpu_in_memory_entries_and_entry_points(engine_gpu):
    """carry.in_memory entries are snapshots; cdr_mutation_batch and cdr_mutation_async
    give the same bytes, twice."""
    sb, out = _carry_batch(engine_gpu.replay, 3)
    carried = np.nonzero(sb.carry.src >= 0)[0]
    mem = np.zeros(sb.n_wfs, np.uint8)
    mem[carried[::2]] = 1
    sb.carry.in_memory = mem
    mut = engine_gpu.mutation(sb, out, fill=FILL)
    n = 0
    for w in carried[::2]:
        if out.result[w].code != abi.OK:
            continue
        info = mut.info[w]
        assert (info.code, info.flags, info.condition) == (abi.MUT_OK, abi.MUT_SNAPSHOT, 0)
        for t in TABLES:
            assert getattr(info, "n_del_" + t) == 0
            assert [ref._b(r) for r in mut.upsert.rows(w, t)] == [ref._b(r) for r in out.rows(w, t)]
            n += len(out.rows(w, t))
    assert n > 0
    _assert_equal(sb, out, mut, fill=FILL)
    raw = mut.raw()
    assert engine_gpu.mutation(sb, out, fill=FILL, via="async").raw() == raw
    assert engine_gpu.mutation(sb, out, fill=FILL, via="async").raw() == raw
    assert engine_gpu.mutation(sb, out, fill=FILL).raw() == raw


@pytest.mark.gpu
def test_gpu_encoders_on_the_upsert_view(engine_gpu):
    """The row encoders take mut.upsert as it is: one blob per upserted row, equal to the
    blob the same row gets from the replay's own outputs (matched by key)."""
    from tests import test_encode_var as tev
    sb, out = _carry_batch(engine_gpu.replay, 3)
    mut = engine_gpu.mutation(sb, out)
    up = mut.upsert
    strs = tev._table(sb, out)

    def by_key(o, blobs, table):
        d = {}
        for w in range(sb.n_wfs):
            if o.result[w].code != abi.OK:
                continue
            off = getattr(o.plan.caps[w], table + "_off")
            for j, r in enumerate(o.rows(w, table)):
                d[(w, getattr(r, ref.KEY[table]))] = blobs[off + j]
        return d

    for table in ("timer", "cancel"):
        full = by_key(out, engine_gpu.encode_rows(sb, out, table), table)
        blobs = engine_gpu.encode_rows(sb, up, table)
        got = by_key(up, blobs, table)
        n_up = sum(getattr(up.result[w], engine.TABLE_COUNT[table]) for w in range(sb.n_wfs)
                   if up.result[w].code == abi.OK)
        assert len(blobs) == len(got) == n_up > 0
        assert all(full[k] == v for k, v in got.items())
    full_b, full_c = engine_gpu.encode_blobs(sb, out, "act", strs)
    got_b, got_c = engine_gpu.encode_blobs(sb, up, "act", strs)
    n_up = sum(up.result[w].n_activity for w in range(sb.n_wfs) if up.result[w].code == abi.OK)
    assert len(got_b) == len(got_c) == n_up > 0
    fb, fc = by_key(out, full_b, "act"), by_key(out, full_c, "act")
    assert all(fb[k] == v for k, v in by_key(up, got_b, "act").items())
    assert all(fc[k] == v for k, v in by_key(up, got_c, "act").items())


@pytest.mark.gpu
def test_gpu_argument_errors(engine_gpu):
    """A batch without loaded states has no mutation: CDR_API_EINVAL, as for null arguments."""
    L = abi.lib()
    batch, out, _ = _case_batch()
    mut = engine.Mutation(batch, out)
    db = abi.CdrDevBatch(n_wfs=batch.n_wfs)
    db.caps = C.addressof(out.plan.caps)  # never read: the call fails on its arguments
    o, m = out.cstruct(), mut.cstruct()
    assert L.cdr_mutation_async(engine_gpu.ctx, C.byref(db), C.byref(o), C.byref(m), None) == -1
    assert L.cdr_mutation_async(engine_gpu.ctx, None, C.byref(o), C.byref(m), None) == -1
    assert L.cdr_mutation_async(engine_gpu.ctx, C.byref(db), C.byref(o), None, None) == -1
    nocarry = engine.Batch(events=batch.events, wfs=batch.wfs, kvs=batch.kvs, rps=batch.rps, cluster=batch.cluster)
    pl = out.plan
    assert L.cdr_mutation_batch(engine_gpu.ctx, C.byref(nocarry.cstruct()), pl.caps, C.byref(pl.totals),
                                C.byref(o), C.byref(m), None) == -1
    assert L.cdr_mutation_batch(engine_gpu.ctx, C.byref(batch.cstruct()), pl.caps, C.byref(pl.totals), None,
                                C.byref(m), None) == -1
    with pytest.raises(RuntimeError):
        engine_gpu.mutation(nocarry, out)
