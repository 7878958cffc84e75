"""bench.py --dump-outputs: the writer of the result columns, on CPU tensors (no GPU), and the
option plumbing of --full / --dump-outputs."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from databend_amd import column as col  # noqa: E402
from databend_amd.device import DeviceColumn  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _columns(rng, n, perm):
    k = rng.permutation(n).astype(np.int64) * 7 - 50          # distinct keys
    cnt = rng.integers(1, 1000, n).astype(np.uint64)
    dec = [int(x) for x in rng.integers(-10**12, 10**12, n)]
    valid = rng.random(n) < 0.8
    s = [bytes(rng.integers(97, 123, rng.integers(0, 9)).astype(np.uint8)) for _ in range(n)]
    take = lambda xs: [xs[i] for i in perm]
    keys = [col.Column.from_numbers(col.Int64, k[perm]), col.Column.from_strings(take(s))]
    aggs = [col.Column.from_numbers(col.UInt64, cnt[perm]),
            col.Column.from_decimals(38, 6, take(dec), validity=valid[perm])]
    dev = lambda cs: [DeviceColumn.from_host(c, device="cpu") for c in cs]
    return dev(keys), dev(aggs), (k, cnt, np.array(dec, dtype=np.float64), valid, s)


def test_dump_is_row_order_independent_and_exact(tmp_path):
    n = 257
    rng = np.random.default_rng(1)
    keys, aggs, (k, cnt, dec, valid, s) = _columns(np.random.default_rng(7), n, np.arange(n))
    keys2, aggs2, _ = _columns(np.random.default_rng(7), n, rng.permutation(n))
    names = (["k", "s"], ["agg0_count", "agg1_sum_x"])
    bench.dump_outputs(str(tmp_path / "a"), names[0], keys, names[1], aggs, n)
    bench.dump_outputs(str(tmp_path / "b"), names[0], keys2, names[1], aggs2, n)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == {"key_k", "key_s_len", "key_s_bytesum", "key_s_wsum", "agg0_count", "agg1_sum_x",
                      "agg1_sum_x_valid", "n_groups"}
    for name in a:
        assert a[name].dtype == np.float64
        np.testing.assert_array_equal(a[name], b[name])
    o = np.argsort(k)
    np.testing.assert_array_equal(a["key_k"], k[o].astype(np.float64))
    np.testing.assert_array_equal(a["agg0_count"], cnt[o].astype(np.float64))
    np.testing.assert_array_equal(a["agg1_sum_x_valid"], valid[o].astype(np.float64))
    np.testing.assert_array_equal(a["agg1_sum_x"], np.where(valid[o], dec[o], 0.0))
    np.testing.assert_array_equal(a["key_s_len"], [len(s[i]) for i in o])
    np.testing.assert_array_equal(a["key_s_bytesum"], [sum(s[i]) for i in o])
    np.testing.assert_array_equal(a["key_s_wsum"], [sum((j + 1) * x for j, x in enumerate(s[i])) for i in o])
    assert a["n_groups"].tolist() == [n]


@pytest.mark.parametrize("string_first", [False, True])
def test_dump_sample_is_bounded_and_the_same_groups(tmp_path, string_first):
    n = 5000
    keys, aggs, (k, cnt, _, _, _) = _columns(np.random.default_rng(3), n, np.arange(n))
    keys2, aggs2, _ = _columns(np.random.default_rng(3), n, np.random.default_rng(4).permutation(n))
    kn = ["k", "s"]
    if string_first:
        keys, keys2, kn = keys[::-1], keys2[::-1], kn[::-1]
    cap = 7 * 8 * 1000  # 7 arrays of float64: at most 1000 rows
    bench.dump_outputs(str(tmp_path / "a"), kn, keys, ["c", "d"], aggs, n, cap_bytes=cap)
    bench.dump_outputs(str(tmp_path / "b"), kn, keys2, ["c", "d"], aggs2, n, cap_bytes=cap)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    total = sum(v.nbytes for v in a.values())
    assert total <= cap + 8
    m = len(a["key_k"])
    assert 0 < m <= 1000 and a["n_groups"].tolist() == [n]
    for name in a:
        np.testing.assert_array_equal(a[name], b[name])
    # the rows written are rows of the input
    count_of = dict(zip(k.tolist(), cnt.tolist()))
    assert [count_of[int(x)] for x in a["key_k"]] == a["c"].tolist()


def test_dump_outputs_refuses_several_gpus():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dump-outputs", "x", "--dry-run"],
                         capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert out.returncode == 2 and "--gpus 1" in out.stderr


def test_full_is_an_option():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--dry-run"],
                         capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
