"""bench.py --dump-outputs: the rows of the last timed step as float64 .npy files (at most 64 MB, a seeded sample above that),
and --steps / ms_per_step on the result line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def test_dump_outputs_masks_unused_slots_and_keeps_exact_values(tmp_path):
    import bench
    ids = np.arange(40, dtype=np.uint32).reshape(4, 10)
    ids[3, 0] = 0xFFFFFFF0                                      # (u32 ids survive float64 exactly)
    cnt = np.array([0, 3, 0xFFFFFFFF, 12], dtype=np.uint32)     # no result / three / a flagged query / more than k
    sc = np.linspace(0.1, 1.0, 40).reshape(4, 10)
    bench.dump_outputs(str(tmp_path), ids, cnt, sc)
    got = {n: np.load(tmp_path / (n + ".npy")) for n in ("rows", "ids", "scores", "counts")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["rows"].tolist() == [0, 1, 2, 3]
    assert got["counts"].tolist() == [0, 3, 0xFFFFFFFF, 12]
    assert (got["ids"][0] == -1).all() and (got["scores"][0] == 0).all()
    assert got["ids"][1].tolist() == [10, 11, 12] + [-1] * 7 and got["scores"][1, :3].tolist() == sc[1, :3].tolist()
    assert got["ids"][3, 0] == 0xFFFFFFF0 and got["ids"][2].tolist() == list(range(20, 30))
    assert np.array_equal(got["scores"][2:], sc[2:])


def test_dump_outputs_samples_above_the_limit_the_same_rows_every_time(tmp_path, monkeypatch):
    import bench
    n_q, k = 1000, 10
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100 * 8 * (2 * k + 2))      # room for 100 rows
    ids = np.arange(n_q * k, dtype=np.uint32).reshape(n_q, k)
    cnt = np.full(n_q, k, dtype=np.uint32)
    sc = np.random.default_rng(5).random((n_q, k))
    rows = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), ids, cnt, sc)
        rows.append(np.load(tmp_path / d / "rows.npy"))
        total = sum(os.path.getsize(tmp_path / d / f) - 128 for f in os.listdir(tmp_path / d))     # (.npy header: 128 bytes)
        assert total <= bench.DUMP_LIMIT_BYTES
    assert np.array_equal(rows[0], rows[1]) and len(rows[0]) == 100 and np.all(np.diff(rows[0]) > 0)
    r = rows[0].astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "ids.npy"), ids[r].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "a" / "scores.npy"), sc[r])


def test_plain_run_leaves_the_extras_to_full():
    """a plain run does only what the headline figure needs; --full brings back the CPU baseline, the host-buffer legs, the live
    PMC pass and the default run's sub-configs, and its own off switches still hold there"""
    import bench
    plain = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not plain.full and plain.no_cpu_baseline and plain.no_host_rate and plain.traffic == "file"
    assert (plain.steps, plain.warmup, plain.dump_outputs) == (20, 5, None)
    full = bench.parse_args(["--full"])
    assert full.full and not full.no_cpu_baseline and not full.no_host_rate and full.traffic == "auto"
    assert plain.sub_configs == full.sub_configs == "auto"          # (main() fills `auto` in a --full run only)
    some = bench.parse_args(["--full", "--no-cpu-baseline", "--traffic", "none"])
    assert some.no_cpu_baseline and not some.no_host_rate and some.traffic == "none"
    assert bench.parse_args(["--traffic", "live"]).traffic == "live"


@pytest.mark.gpu
def test_bench_dumps_the_last_steps_rows(tmp_path):
    """a small workload through bench.py: --steps is the number of timed steps, ms_per_step is on the line, and the dumped rows
    are the oracle's for the batch the last step ran (steps rotate over the batches)"""
    import oracle
    from suggest_amd import synth
    steps, n_b, n_q, k = 7, 4, 2048, 10
    env = {kk: v for kk, v in os.environ.items() if kk not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
           "--dict-size", "100000", "--queries", str(n_q), "--batches", str(n_b), "--no-cpu-baseline", "--no-host-rate",
           "--traffic", "none", "--sub-configs", "none", "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["steps"] == steps and rec["ms_per_step"] > 0
    assert abs(rec["value"] - n_q * steps / (rec["ms_per_step"] * steps * 1e-3)) / rec["value"] < 1e-6
    got = {n: np.load(tmp_path / (n + ".npy")) for n in ("rows", "ids", "scores", "counts")}
    assert got["rows"].tolist() == list(range(n_q))
    blob, offs = synth.make_dict(100000, seed=1)
    qb, qo = synth.make_queries(n_q, blob, offs, seed=2, start=((steps - 1) % n_b) * n_q)
    ora = oracle.OracleIndex(blob=blob, offs=offs, **synth.DESCRIPTION)
    oi, os_, oc, _ = ora.suggest_batch(qb, qo, "jaccard", 0.5, k)
    assert np.array_equal(got["counts"], oc.astype(np.float64))
    valid = np.arange(k)[None, :] < np.minimum(oc, k)[:, None]
    assert np.array_equal(got["ids"][valid], oi[valid].astype(np.float64)) and (got["ids"][~valid] == -1).all()
    assert np.array_equal(got["scores"][valid].view(np.uint64), os_[valid].view(np.uint64))
    assert int(oc.sum()) > 0
