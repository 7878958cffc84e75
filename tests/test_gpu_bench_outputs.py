"""bench.py on the GPU at small sizes: a plain run prints the headline line only and
--dump-outputs writes the last timed step's result columns (checked against numpy over the
oracle's copy of the same generated rows); --full adds the per-kernel pass and the roofline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}


def run_bench(*argv):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *argv],
                         capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_plain_run_dumps_the_last_steps_groups(tmp_path):
    rows, steps, warmup = 200_003, 3, 1
    d = run_bench("--rows", str(rows), "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path))
    assert PLAIN_KEYS <= set(d) and d["steps"] == steps and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(rows / (d["ms_per_step"] * 1e-3))
    for moved in ("roofline", "kernels_ms_per_step", "order_by_limit", "cpu_baseline", "configs", "scan"):
        assert moved not in d
    # the last timed step (index warmup + steps - 1) reads input copy (index % copies): its rows
    copy = (warmup + steps - 1) % d["config"]["input_copies"]
    adv = oracle.datagen(2, rows, start=copy * rows)["AdvEngineID"].data
    keys, counts = np.unique(adv[adv != 0], return_counts=True)
    got = load(tmp_path)
    assert set(got) == {"key_AdvEngineID", "agg0_count", "n_groups"}
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["key_AdvEngineID"], keys.astype(np.float64))
    np.testing.assert_array_equal(got["agg0_count"], counts.astype(np.float64))
    assert got["n_groups"].tolist() == [len(keys)] and d["config"]["groups"] == len(keys)
    assert d["config"]["selected_rows"] == int(counts.sum())


def test_dump_of_a_high_cardinality_config(tmp_path):
    rows = 300_007
    d = run_bench("--config", "3", "--rows", str(rows), "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    uid = oracle.datagen(3, rows)["UserID"].data  # C3 runs one input copy: rows [0, rows)
    keys, counts = np.unique(uid, return_counts=True)
    got = load(tmp_path)
    assert got["n_groups"].tolist() == [len(keys)] and d["config"]["groups"] == len(keys)
    want = np.stack([keys.astype(np.float64), counts.astype(np.float64)])
    want = want[:, np.lexsort(want[::-1])]  # int64 keys that round to one float64 order by count
    np.testing.assert_array_equal(np.stack([got["key_UserID"], got["agg0_count"]]), want)


def test_full_adds_the_kernel_pass_and_the_roofline():
    d = run_bench("--rows", "200003", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert PLAIN_KEYS <= set(d)
    assert d["roofline"]["kernel_launches"] == 2 and d["roofline"]["frac"] > 0
    assert d["kernels_ms_per_step"] and d["order_by_limit"]["values_match_host_sort"]
