"""bench.py's plain run and --dump-outputs on the GPU, at a small size: the plain run times
its steps and skips every side leg, the dumped arrays are the last step's output records
(their per-entry digests equal the CPU restatement's), a second run writes the same bytes,
and a table larger than its share of the budget is a sample of its rows."""
import ctypes as C
import io
import json
import os
import sys

import numpy as np
import pytest

import bench
from cadence_amd import abi

pytestmark = pytest.mark.gpu

CFG, WFS, SEED = 3, 700, 0x5EED0003


def _run(monkeypatch, capsys, *extra):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--config", str(CFG),
                                      "--wfs", str(WFS), "--seed", str(SEED), *extra])
    bench.main()
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """(result line, arrays) of one plain run with --dump-outputs, every table whole."""
    d = tmp_path_factory.mktemp("dump")
    with pytest.MonkeyPatch.context() as mp:
        out = io.StringIO()
        mp.setattr(sys, "stdout", out)
        mp.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--config", str(CFG),
                                 "--wfs", str(WFS), "--seed", str(SEED), "--dump-outputs", str(d)])
        bench.main()
    return json.loads(out.getvalue().strip().splitlines()[-1]), _load(str(d))


def test_plain_run_times_its_steps_only(dumped):
    line, _ = dumped
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["unit"] == "events/s" and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(line["config"]["events_per_gpu"] / (line["ms_per_step"] / 1e3))
    for leg in ("cpu_baseline", "refresh", "encode", "host_path", "parity"):
        assert line[leg] is None, leg
    assert line["roofline"]["stream_copy_peak_gbs"] is None and line["parity_checked"] is False


def test_dump_holds_the_output_records(dumped):
    import oracle
    line, arrs = dumped
    assert {"result", "exec", "repl", "vh", "act", "entry_digest"} <= set(arrs) <= {
        "result", "exec", "repl", "vh", "act", "timer", "child", "cancel", "signal", "rp", "sa", "entry_digest"}
    # float64, and no table without rows is written
    assert all(a.dtype == np.float64 and a.ndim == 2 and a.size for a in arrs.values())
    want, _, hist = oracle.synth_digests(CFG, np.arange(WFS, dtype=np.uint32), SEED, threads=4)
    n = len(want)
    assert hist.get("OK", 0) == n and line["ok_workflows"] == n
    got = arrs["entry_digest"].astype(np.uint64)
    assert np.array_equal(got[:, 0] | (got[:, 1] << np.uint64(32)), want)
    assert arrs["result"].shape[0] == n and not arrs["result"][:, 0].any()  # cdr_wf_result.code == OK
    assert arrs["exec"].shape == (n, C.sizeof(abi.CdrExecInfo) // 4) and arrs["act"].shape[0] > 0


def test_dump_repeats_and_samples_large_tables(dumped, tmp_path, monkeypatch, capsys):
    _, whole = dumped
    budget = 400_000
    monkeypatch.setattr(bench, "DUMP_BUDGET", budget)
    runs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        _run(monkeypatch, capsys, "--dump-outputs", str(d))
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= budget
        runs.append(_load(str(d)))
    assert runs[0].keys() == runs[1].keys() == whole.keys()
    sampled = 0
    for name, a in runs[0].items():
        assert np.array_equal(a, runs[1][name]), name
        w = whole[name]
        assert a.shape[1:] == w.shape[1:] and len(a) <= len(w)
        if len(a) == len(w):
            assert np.array_equal(a, w), name
            continue
        # a sample: its rows are rows of the whole table, in the table's order
        sampled += 1
        at = 0
        for row in a:
            while at < len(w) and not np.array_equal(w[at], row):
                at += 1
            assert at < len(w), name
            at += 1
    assert sampled >= 2
