"""bench.py's plain run and --dump-outputs: a plain run measures the headline only and can write what its last timed step
computed, on seeded reads, so that two runs (or two builds) with the same arguments can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("call", "total_kmers", "clade_hits", "hit_groups")


def _records(n, seed=3):
    rng = np.random.default_rng(seed)
    rec = np.empty((n, 4), dtype=np.uint32)
    rec[:, 0] = rng.integers(0, 2**32, n, dtype=np.uint64)  # a taxon id uses all 32 bits
    rec[:, 1:] = rng.integers(0, 1 << 18, (n, 3))
    return rec


def test_dump_writes_every_field_exactly_in_float32_or_float64(tmp_path):
    import bench
    rec = _records(1000)
    counters = np.array([1000, 37, 300000, (1 << 40) + 5], dtype=np.int64)
    bench.dump_outputs(str(tmp_path), {"results": rec, "counters": counters})
    assert sorted(os.listdir(tmp_path)) == sorted(f + ".npy" for f in FIELDS + ("counters",))
    for j, f in enumerate(FIELDS):
        a = np.load(tmp_path / (f + ".npy"))
        assert a.dtype in (np.float32, np.float64) and a.shape == (1000,), f
        assert np.array_equal(a.astype(np.uint64), rec[:, j].astype(np.uint64)), f
    c = np.load(tmp_path / "counters.npy")
    assert c.dtype == np.float64 and np.array_equal(c.astype(np.int64), counters)


def test_dump_above_the_limit_is_a_fixed_sample_with_its_positions(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 20000)
    rec = _records(5000)
    counters = np.arange(4, dtype=np.int64)
    sizes = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"results": rec, "counters": counters})
        sizes.append(sum(os.path.getsize(tmp_path / d / f) - 128 for f in os.listdir(tmp_path / d)))  # (128: .npy header)
    assert sizes[0] <= 20000
    rows = np.load(tmp_path / "a" / "row_index.npy")
    assert np.array_equal(rows, np.load(tmp_path / "b" / "row_index.npy"))
    assert len(rows) > 100 and np.all(np.diff(rows) > 0) and rows[-1] < 5000
    for j, f in enumerate(FIELDS):
        a = np.load(tmp_path / "a" / (f + ".npy"))
        assert np.array_equal(a, np.load(tmp_path / "b" / (f + ".npy")))
        assert np.array_equal(a.astype(np.uint64), rec[rows.astype(np.int64), j].astype(np.uint64)), f
    # a later dump that fits leaves no sample positions behind
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    bench.dump_outputs(str(tmp_path / "a"), {"results": rec, "counters": counters})
    assert not (tmp_path / "a" / "row_index.npy").exists()


def test_the_extra_legs_are_off_unless_full():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "/x"])
    assert a.full is True and a.dump_outputs == "/x"


@pytest.mark.gpu
def test_a_plain_run_times_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    pairs, steps = 30000, 5
    lines = []
    for d in ("a", "b"):
        env = dict(os.environ, NOHUMAN_BENCH_LOGDIR=str(tmp_path / d))
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                              "--pairs", str(pairs), "--capacity", "40000003", "--wake-ms", "10", "--dump-outputs", str(tmp_path / d)],
                             env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert out.returncode == 0, out.stderr[-3000:]
        lines.append(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]))
    d = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config", "roofline"):
        assert k in d, k
    assert d["steps"] == steps and d["unit"] == "Mreads/s" and d["higher_is_better"] is True and d["dtype"] == "u64"
    # the legs of --full are not run: no CPU baseline, no e2e, no variants, no second measurement of the same launches
    assert "cpu_baseline" not in d and "variants" not in d["roofline"] and not any(k.startswith("e2e") for k in d["config"])
    assert d["roofline"]["value_two_streams"] is None and d["roofline"]["kernel_ms_without_wake"] is None
    assert not os.path.exists(tmp_path / "a" / "bench_details.json")
    # value and ms_per_step describe the same K timed steps
    assert abs(d["value"] * 1e6 - pairs * 2 / (d["ms_per_step"] / 1e3)) / (d["value"] * 1e6) < 0.01
    counters = np.load(tmp_path / "a" / "counters.npy")
    assert counters[0] == steps * pairs and counters[2] == steps * pairs * 2 * 150
    # the reads are the same in both runs: what does not depend on the table is equal; the synthetic table's concurrent
    # inserts can place a colliding key differently, so a record's hits may differ now and then (bench.py docstring)
    cb = np.load(tmp_path / "b" / "counters.npy")
    assert counters[[0, 2, 3]].tolist() == cb[[0, 2, 3]].tolist()
    assert np.array_equal(np.load(tmp_path / "a" / "total_kmers.npy"), np.load(tmp_path / "b" / "total_kmers.npy"))
    for f in FIELDS:
        a, b = np.load(tmp_path / "a" / (f + ".npy")), np.load(tmp_path / "b" / (f + ".npy"))
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape == (pairs,), f
        assert (a != b).sum() <= 3, (f, int((a != b).sum()))
    assert np.load(tmp_path / "a" / "counters.npy").dtype == np.float64
    assert 0 < (np.load(tmp_path / "a" / "total_kmers.npy") > 0).mean()
