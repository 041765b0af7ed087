"""bench.py's --dump-outputs and --full.  CPU: the writer's size limit and its fixed sample, the options in --help.
GPU: a small plain run writes the last step's pair and the values behind it, the same in a second run, and reports
what moved behind --full as null; a --full run fills it in."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--config", "2", "--log2-cand", "12", "--steps", "3", "--warmup", "1"]


def _bench(args):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, capture_output=True, text=True,
                       timeout=240, cwd=REPO)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_dump_outputs_limit_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * 8 * 100)          # two arrays: 100 float64 each
    big = np.arange(1000, dtype=np.float64).reshape(10, 100)
    small = np.arange(7, dtype=np.int64)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), {"big": big, "small": small})
    a_big, a_small = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "small.npy")
    assert a_small.dtype == np.float64 and np.array_equal(a_small, small)
    assert a_big.dtype == np.float64 and a_big.shape == (100,)
    assert np.all(np.diff(a_big) > 0) and np.all(np.isin(a_big, big))     # distinct elements of big, in order
    assert np.array_equal(a_big, np.load(tmp_path / "b" / "big.npy"))     # the same sample in every run
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 2 * 8 * 100 + 2 * 128


def test_bench_help_names_full_and_dump_outputs():
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=240, cwd=REPO)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    """One small plain run with its outputs written: (result line, directory), shared by the tests below."""
    out = tmp_path_factory.mktemp("plain")
    return _bench(SMALL + ["--dump-outputs", str(out)]), out


@pytest.mark.gpu
def test_plain_run_line_and_outputs(plain_run):
    rec, out = plain_run
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["full"] is False
    assert abs(rec["value"] - 4096 / (rec["ms_per_step"] * 1e-3)) <= 1e-9 * rec["value"]
    for key in ("roofline", "roofline_kblock", "cpu_baseline", "reference_cpu_per_candidate", "stage_ms",
                "state_install_ms"):
        assert rec[key] is None, key
    assert sorted(os.listdir(out)) == ["acq_values.npy", "best.npy"]
    best, vals = np.load(out / "best.npy"), np.load(out / "acq_values.npy")
    assert best.dtype == np.float64 and vals.dtype == np.float64 and vals.shape == (4096,)
    # the pair of the last timed step is the arg-max (lowest index among the maxima) of the values behind it
    assert best[0] == vals.max() and int(best[1]) == int(np.argmax(vals))
    assert (best[0], int(best[1])) == (rec["best"]["value"], rec["best"]["index"])


@pytest.mark.gpu
def test_second_plain_run_writes_the_same_outputs(plain_run, tmp_path):
    _, first = plain_run
    _bench(SMALL + ["--dump-outputs", str(tmp_path)])
    for name in ("best.npy", "acq_values.npy"):
        assert np.array_equal(np.load(first / name), np.load(tmp_path / name))


@pytest.mark.gpu
def test_full_run_reports_what_moved(tmp_path):
    rec = _bench(SMALL + ["--full", "--cpu-seconds", "0.2", "--chain", "separate", "--dump-outputs", str(tmp_path)])
    assert rec["full"] is True and rec["steps"] == 3
    assert rec["roofline"]["check"] is True and rec["roofline"]["launches_timed"] == 2
    assert rec["roofline_kblock"]["ms"] > 0 and rec["state_install_ms"] > 0
    assert rec["cpu_baseline"]["value"] > 0 and rec["reference_cpu_per_candidate"] is not None
    assert sorted(os.listdir(tmp_path)) == ["acq.npy", "best.npy", "mu.npy", "var.npy"]
    acq, best = np.load(tmp_path / "acq.npy"), np.load(tmp_path / "best.npy")
    assert np.load(tmp_path / "mu.npy").shape == (2, 4096) and acq.shape == (4096,)
    assert best[0] == acq.max() and int(best[1]) == int(np.argmax(acq))
