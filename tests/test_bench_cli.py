"""bench.py's command line: a plain run prints the headline line only, --full
adds the checks and baselines, --dump-outputs writes the last step's result."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("expected_matches", "shifted_check", "correct", "cpu_baseline", "cpu_legs")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def parse(monkeypatch, *argv):
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_and_dump_are_off_by_default(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full and a.dump_outputs == "somewhere"


def test_zero_steps_is_refused(monkeypatch):
    with pytest.raises(SystemExit):
        parse(monkeypatch, "--steps", "0")


def run_bench(*args):
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--primary", "20000", "--secondary", "300000", *args],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_count(tmp_path):
    out = run_bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "dump"))
    assert all(k in out for k in HEADLINE) and out["steps"] == 3
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(320000 / (out["ms_per_step"] * 1e-3))
    assert not any(k in out for k in FULL_ONLY)
    assert os.listdir(tmp_path / "dump") == ["matches.npy"]
    m = np.load(tmp_path / "dump" / "matches.npy")
    # every Zipf key lies in [1, |R|] and R holds each key once: the count is |S|
    assert m.dtype == np.float64 and m.tolist() == [300000.0] and out["matches"] == 300000


@pytest.mark.gpu
def test_full_run_adds_the_checks():
    out = run_bench("--steps", "2", "--warmup", "1", "--full", "--no-traffic", "--no-cpu-baseline")
    assert all(k in out for k in HEADLINE)
    assert out["correct"] is True and out["expected_matches"] == out["matches"] == 300000
    assert out["shifted_check"]["runs"] == [out["shifted_check"]["expected"]] * 4
