"""`bench.py --dump-outputs DIR`: the results of the last timed step as DIR/<name>.npy in float32 / float64, every value
exact, at most 64 MB in all with the same sample of PSMs on every run (CPU); and, on the GPU, a small job's files against
the CPU checker on the same seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, checker_kind

NAMES = ("best_score", "n_sig", "best_sig", "ascores", "alt_mask")


def _load(d):
    files = sorted(os.listdir(d))
    assert files == sorted(n + ".npy" for n in NAMES + ("rows",)), files
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    return got, sum(os.path.getsize(os.path.join(d, f)) for f in files)


def _masks(halves):
    """[..., 2] float64 (low, high 32 bits) -> uint64"""
    return halves[..., 0].astype(np.uint64) | (halves[..., 1].astype(np.uint64) << np.uint64(32))


def _results(n, k, seed):
    rng = np.random.default_rng(seed)
    return dict(best_score=rng.random(n, dtype=np.float32), n_sig=rng.integers(0, 2 ** 31 - 1, n).astype(np.int32),
                best_sig=rng.integers(0, 2 ** 64 - 1, n, dtype=np.uint64).view(np.int64), ascores=rng.random((n, k), dtype=np.float32),
                alt_mask=rng.integers(0, 2 ** 64 - 1, (n, k), dtype=np.uint64).view(np.int64))


def test_every_value_is_kept_exactly(tmp_path):
    import bench
    res = _results(1000, 3, 1)
    bench.dump_outputs(str(tmp_path / "d"), res)
    got, _ = _load(str(tmp_path / "d"))
    assert np.array_equal(got["rows"], np.arange(1000))
    assert got["best_score"].dtype == np.float32 and np.array_equal(got["best_score"], res["best_score"])
    assert got["ascores"].dtype == np.float32 and np.array_equal(got["ascores"], res["ascores"])
    assert np.array_equal(got["n_sig"].astype(np.int32), res["n_sig"])
    assert got["best_sig"].shape == (1000, 2) and np.array_equal(_masks(got["best_sig"]), res["best_sig"].view(np.uint64))
    assert got["alt_mask"].shape == (1000, 3, 2) and np.array_equal(_masks(got["alt_mask"]), res["alt_mask"].view(np.uint64))


def test_a_large_result_is_cut_to_the_same_sample_under_the_limit(tmp_path):
    import bench
    res = _results(1_000_000, 4, 2)                       # 108 bytes per PSM as written
    bench.dump_outputs(str(tmp_path / "a"), res)
    bench.dump_outputs(str(tmp_path / "b"), res)
    a, size = _load(str(tmp_path / "a"))
    b, _ = _load(str(tmp_path / "b"))
    assert 0.99 * 64e6 < size <= 64e6
    rows = a["rows"].astype(np.int64)
    assert len(rows) < 1_000_000 and np.all(np.diff(rows) > 0) and rows[-1] > 900_000
    assert np.array_equal(a["ascores"], res["ascores"][rows]) and np.array_equal(_masks(a["best_sig"]), res["best_sig"].view(np.uint64)[rows])
    assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
def test_dumped_outputs_are_the_checkers_results(tmp_path):
    """One small seeded job through bench.py itself: the line says `steps` as given, and the files hold what the CPU checker
    computes for the same batch."""
    from oracle import harness, orc
    from pyascore_amd import synth
    n, d = 3000, str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--blocks", "2",
                        "--config", "cfg3", "--psms", str(n), "--no-cpu-baseline", "--no-host-api", "--dump-outputs", d],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["blocks"]["n"] == 2 and line["config"]["psms_total"] == n
    got, _ = _load(d)
    desc = synth.describe("cfg3", n_psm=n, seed=1000)
    batch = synth.make_slice(desc, 0, n)
    max_k = int(desc["n_mod"].max())
    want = harness.make_scorer(orc.OracleAscore, desc["settings"], kind=checker_kind()).score_batch(batch, max_k)
    assert np.array_equal(got["rows"], np.arange(n))
    assert np.array_equal(got["best_score"], want["best_score"]) and np.array_equal(got["ascores"], want["ascores"])
    assert np.array_equal(got["n_sig"], want["n_sig"])
    assert np.array_equal(_masks(got["best_sig"]), want["best_sig"].astype(np.uint64))
    assert np.array_equal(_masks(got["alt_mask"]), want["alt_mask"].astype(np.uint64))
