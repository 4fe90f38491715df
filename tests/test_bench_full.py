"""`bench.py` with and without `--full`.  A plain run measures the headline and nothing else: no CPU baseline, no other
configs, no host-API legs, no copy-rate run, no counters.  `--full` adds each of them under its own key of the same line;
the --no-... options leave one out again.  What starts before the first GPU call is checked where there is no GPU, the
rest of the line on one."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def _ran_before_the_gpu(monkeypatch, argv):
    """bench.main() up to its first GPU call (no device is reported, so it stops there), the CPU baseline and the legs
    replaced by recorders: the names of those that were started."""
    import bench
    import torch
    ran = []
    monkeypatch.setattr(bench, "cpu_baseline", lambda *a, **k: ran.append("cpu_baseline"))
    monkeypatch.setattr(bench, "run_legs", lambda *a, **k: ran.append("other_configs") or {})
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PYA_BENCH_BACKEND"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit, match="HIP device"):
        bench.main()
    return ran


def test_a_plain_run_starts_no_baseline_and_no_legs(monkeypatch):
    assert _ran_before_the_gpu(monkeypatch, ["--gpus", "1", "--steps", "3", "--warmup", "1"]) == []
    # (the options that leave a part of --full out are no request for the rest of it)
    assert _ran_before_the_gpu(monkeypatch, ["--gpus", "1", "--no-host-api"]) == []


def test_full_starts_them_before_the_gpu(monkeypatch):
    assert _ran_before_the_gpu(monkeypatch, ["--gpus", "1", "--full"]) == ["cpu_baseline", "other_configs"]
    assert _ran_before_the_gpu(monkeypatch, ["--full", "--no-cpu-baseline"]) == ["other_configs"]
    assert _ran_before_the_gpu(monkeypatch, ["--full", "--no-other-configs"]) == ["cpu_baseline"]
    # the legs belong to the default cfg2 job only
    assert _ran_before_the_gpu(monkeypatch, ["--full", "--config", "cfg5", "--psms", "50"]) == ["cpu_baseline"]


def _line(extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", "cfg3", "--psms", "3000"] + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [r for r in p.stdout.splitlines() if r.strip()]
    assert len(rows) == 1, p.stdout
    return json.loads(rows[0])


@pytest.mark.gpu
def test_full_adds_its_keys_to_the_plain_line():
    plain, full = _line([]), _line(["--full", "--no-cpu-baseline"])
    for line in (plain, full):
        assert line["unit"] == "PSMs/s" and line["higher_is_better"] is True and line["n_gpus"] == 1
        assert line["steps"] == 3 and line["warmup"] == 1 and line["blocks"]["n"] == 5
        assert line["value"] == pytest.approx(3000 / (line["ms_per_step"] * 1e-3), rel=1e-9)
        r = line["roofline"]
        assert r["kernel"] == max(r["kernel_ms"], key=r["kernel_ms"].get) and r["achieved"] > 0
        assert "cpu_baseline" not in line and "other_configs" not in line
    assert (plain["metric"], plain["dtype"], plain["data"], plain["config"]) == (full["metric"], full["dtype"], full["data"], full["config"])
    assert plain["host_api"] is None and plain["roofline"]["achievable_peak"] is None
    assert plain["roofline"]["frac_of_achievable"] is None and "--full" in plain["roofline"]["traffic_refused"]
    assert full["host_api"]["value"] > 0 and full["host_api"]["pcie_only_ms"] > 0
    assert full["roofline"]["achievable_peak"] > 0 and full["roofline"]["frac_of_achievable"] > 0
