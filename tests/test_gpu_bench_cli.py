"""bench.py's command line, at a size that takes seconds (3M c2 commits over 4,096 resources, 3 timed steps).

A plain run sets up, warms up, times `--steps` steps and prints one JSON line: no parity gate, CPU baseline, split /
PCIe leg or c3 sub-record in it.  `--full` brings those back (here without the fixed-size 1e9-row c3 sub-record).
`--dump-outputs DIR` writes the last timed step's results as float32 / float64 .npy files, at most 64 MB in all, a
fixed seeded sample of the 3M-row columns (2^21 rows: the sampling path); the generators are seeded, so the plain and
the --full run, two processes with the same arguments otherwise, must write the same files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, R, STEPS, WARMUP = 3_000_000, 4096, 3, 1


def _bench(outdir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--commits", str(N), "--resources", str(R), "--dump-outputs", str(outdir), *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.strip()][-1]  # the JSON result line
    return json.loads(line), {f[:-4]: np.load(os.path.join(outdir, f)) for f in sorted(os.listdir(outdir))}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _bench(tmp_path_factory.mktemp("plain"))


@pytest.mark.gpu
def test_plain_run_line_and_dump(plain):
    line, dump = plain
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["unit"] == "ops/s" and line["higher_is_better"] is True and line["dtype"] == "int64"
    assert line["metric"].startswith("committed ops applied/sec")
    assert line["ms_per_step"] > 0
    # value = commits of the timed steps / their time; ms_per_step = that time / --steps, rounded to 1e-4 ms in the line
    assert line["value"] == pytest.approx(N / (line["ms_per_step"] * 1e-3), rel=6e-5 / line["ms_per_step"] + 1e-6)
    assert line["config"]["commits_per_step_per_gpu"] == N and line["config"]["resident_streams"] == STEPS + WARMUP
    for k in ("parity", "cpu_baseline", "cpu_baseline_all_cores"):  # what --full measures is absent from a plain line
        assert line[k] is None, k
    for k in ("global_log_split", "end_to_end", "end_to_end_pipelined", "c3"):
        assert k not in line, k
    assert set(dump) == {"status", "value", "rows", "state_tag", "state_value", "state_current", "applied_index"}
    assert all(a.dtype in (np.float32, np.float64) for a in dump.values())
    assert sum(a.nbytes for a in dump.values()) <= 64e6
    rows = dump["rows"]
    assert len(rows) == len(dump["status"]) == len(dump["value"]) > 1 << 20
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < N  # distinct rows of the column, ascending
    assert not np.any(dump["status"] == 0xFF)  # the result prefill (no legal status): every sampled row was written
    assert len(dump["state_value"]) == R
    assert dump["applied_index"].tolist() == [float((STEPS + WARMUP) * N)]  # the last step's last log index


@pytest.mark.gpu
def test_full_run_gates_and_same_outputs(plain, tmp_path):
    line, dump = _bench(tmp_path, "--full", "--no-c3")
    assert line["steps"] == STEPS
    p = line["parity"]
    assert p["rows"] == N and p["mismatches"] == 0 and p["unwritten"] == 0 and p["state_mismatches"] == 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline_all_cores"]["value"] > 0
    assert line["global_log_split"]["round_trip_ok"] is True
    assert line["end_to_end"]["value"] > 0 and line["end_to_end_pipelined"]["value"] > 0
    assert set(dump) == set(plain[1])
    for k, a in dump.items():  # same arguments, same inputs, same results: bit for bit
        assert a.dtype == plain[1][k].dtype and np.array_equal(a, plain[1][k]), k


@pytest.mark.gpu
def test_full_run_gate_holds_when_batches_are_replayed(tmp_path):
    """More steps than resident batches (4 steps over 2 batches): batch 0 is applied again on later state, and the
    step-0 parity gate, read after the timed steps, must still see what step 0 wrote."""
    line, dump = _bench(tmp_path, "--full", "--no-c3", "--no-split", "--no-e2e", "--max-streams", "2")
    assert line["config"]["resident_streams"] == 2
    p = line["parity"]
    assert p["rows"] == N and p["mismatches"] == 0 and p["unwritten"] == 0 and p["state_mismatches"] == 0
    assert not np.any(dump["status"] == 0xFF)


def test_help_names_the_new_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs DIR" in r.stdout
