"""bench.py's launcher contract, checked without a GPU: `python bench.py --gpus N` started bare must itself start N
ranks (one process per GPU on real hardware) and report the communicator's size; a launcher that started a different
number of ranks than --gpus asks for is an error, not a silently smaller run."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(extra, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)


def test_bare_gpus_2_starts_two_ranks_and_reports_the_communicator_size():
    r = run_bench(["--gpus", "2", "--dry-run"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout            # rank 0 prints ONE line
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["dry_run"] is True and out["verified_bit_exact_vs_cpu"] is True
    assert out["value"] is None                 # a dry run never carries a throughput


def test_single_rank_dry_run():
    r = run_bench(["--dry-run"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["n_gpus"] == 1


def test_rank_count_that_does_not_match_gpus_is_refused():
    r = run_bench(["--gpus", "2", "--dry-run"], {"WORLD_SIZE": "3", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and "--gpus 2" in r.stderr


def test_dump_outputs_keeps_a_fixed_sample_of_aligned_rows_under_the_limit(tmp_path, monkeypatch):
    """--dump-outputs beyond the size limit: the same seeded rows of every column of a table, identical from run to run."""
    import numpy as np

    import bench

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4000)
    key = np.arange(1000, dtype=np.int64) * 3
    cols = {"key": key, "twice": key * 2, "answer": np.array([7], dtype=np.int64)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), cols)
    got = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in cols}
    assert all(v.dtype == np.float64 for v in got.values())
    assert sum(v.size for v in got.values()) * 8 <= 4000
    assert 0 < got["key"].size < 1000 and np.array_equal(got["twice"], got["key"] * 2)
    assert np.all(np.diff(got["key"]) > 0) and got["answer"].tolist() == [7.0]
    for n in cols:
        assert np.array_equal(got[n], np.load(str(tmp_path / "b" / (n + ".npy"))))


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_the_answer(tmp_path):
    """A plain run: `steps` timed steps, `ms_per_step` consistent with `value`, the last step's revenue in revenue.npy equal
    to the SQL loop over the same generated rows; nothing of --full (roofline, verification) in the line."""
    import numpy as np

    import oracle
    from mplan2vdl_amd import datagen

    rows = 600175
    r = run_bench(["--rows", str(rows), "--steps", "7", "--warmup", "2", "--jit", "off", "--dump-outputs", str(tmp_path / "out")])
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["steps"] == 7 and out["ms_per_step"] > 0
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 - rows) < 1e-6 * rows
    assert out["roofline"] is None and out["verified_bit_exact_vs_cpu"] is None and "also" not in out
    specs = [(datagen.SEED, datagen.col_id(c), datagen.LINEITEM[c].lo, datagen.LINEITEM[c].hi,
              datagen.LINEITEM[c].mul, datagen.LINEITEM[c].add) for c in datagen.Q6_COLUMNS]
    rev, cnt = oracle.sql_q6_generated(specs, 0, rows, threads=1)
    assert cnt > 0
    dumped = np.load(str(tmp_path / "out" / "revenue.npy"))
    assert dumped.dtype == np.float64 and dumped.tolist() == [float(rev)] and out["revenue"] == rev
