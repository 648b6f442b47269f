"""Hand-made engine states for tests: an `engine.Outputs` over a fake `engine.Batch`, built
from per-entry row lists (no replay), for the calls that take any Outputs — the mutation
kernel (tests/test_mutation.py) and the row encoders (tests/test_encode_edges.py)."""
from cadence_amd import abi, engine

PENDING = ("act", "timer", "child", "cancel", "signal")


def make_state(per_entry, slack, tables=PENDING):
    """(fake batch, Outputs) holding per_entry[w][table] rows for the tables named, entry
    w's slices slack(w) rows larger than its rows."""
    n = len(per_entry)
    caps = (abi.CdrWfCaps * n)()
    tot = abi.CdrTotals()
    for w, tabs in enumerate(per_entry):
        for t in tables:
            setattr(caps[w], t + "_off", getattr(tot, t))
            setattr(caps[w], t + "_cap", len(tabs[t]) + slack(w))
            setattr(tot, t, getattr(tot, t) + len(tabs[t]) + slack(w))
    fake = engine.Batch(events=(abi.CdrEvent * 0)(), wfs=(abi.CdrWfDesc * n)(), kvs=(abi.CdrKV * 0)(),
                        rps=(abi.CdrResetPoint * 0)(), cluster=engine.default_cluster())
    st = engine.Outputs(fake, engine.Plan(caps=caps, totals=tot))
    for w, tabs in enumerate(per_entry):
        st.exec[w].next_event_id = 1000 + 7 * w
        for t in tables:
            setattr(st.result[w], engine.TABLE_COUNT[t], len(tabs[t]))
            off = getattr(caps[w], t + "_off")
            for j, r in enumerate(tabs[t]):
                st.tables[t][off + j] = r
    return fake, st
