"""The fragment m/z recalibration, measured.  One process on one GPU:

  (a) the APPLY kernel (pya_recalibrate_spectra) over the spectra of 100 000 cfg2 PSMs and of bench.py's dense batch (about
      1 570 peaks per spectrum), with the m/z array as float64 and as float32 (the three type pairs of a run have two m/z types;
      the intensities are not read): HIP events around one in-place call on torch's stream, RUNS rounds after WARM warm-up
      rounds, median and p10..p90.  Beside it, in the same rounds: a device-to-device copy of the same m/z bytes (the floor of
      anything that reads and writes each value once) and the path the kernel replaces on a resident array (D2H, the numpy
      restatement pyascore_amd.rollup.recalibrate, H2D; wall clock around work that ends in a synchronise).  The bytes of the
      kernel and of the restatement are compared before anything is reported.
  (b) the FIT kernel (pya_mz_profile_fit) for 1, 64 and 4 096 slots of seeded tables, HIP events, against the restatement.
  (c) PyAscore.score_batch on cfg2 without and with recalibrate=, alternating, host to host.  With --batch-only nothing else
      runs and one line "rate <M PSMs/s> ..." per call is printed: --parent-lib PATH starts such a child process on another
      build of the library (PYA_LIB; the parent commit's), between two rounds of this build's, so that the plain rate of both
      commits is taken in one call of the script.

Needs a GPU: there is no fallback.

    python scripts/recalibrate_probe.py [--runs 30] [--calls 6] [--parent-lib PATH] > profiles/recalibrate/probe.txt"""
import argparse
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import harness  # noqa: E402
from pyascore_amd import PyAscore, rollup, synth  # noqa: E402
from pyascore_amd.device import DevicePlan, mz_calibration_records  # noqa: E402

KNOTS = [32.0, 28.0, 22.0, 15.0, 9.0, 4.0, 0.0, -3.0]
SLOTS = 4


def pct(v):
    return "%8.4f (%.4f..%.4f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))


def calibration():
    cal = np.zeros(SLOTS, rollup.MZ_CALIBRATION_DTYPE)
    cal["ppm"][:] = KNOTS
    cal["ppm"][1:] += np.random.default_rng(7).uniform(-5.0, 5.0, (SLOTS - 1, 8))
    return cal


def apply_rows(plan, name, batch, warm, runs):
    dev = plan.device
    cal = calibration()
    d_cal = torch.from_numpy(cal.view(np.uint8).reshape(SLOTS, -1)).to(dev)
    off = np.ascontiguousarray(batch["peak_off"], np.int64)
    n_spec = off.size - 1
    run = (np.arange(n_spec) * SLOTS // n_spec).astype(np.int32)
    d_off, d_run = torch.from_numpy(off).to(dev), torch.from_numpy(run).to(dev)
    for label, dtype in (("f64 (f64,f64 and f64,f32)", np.float64), ("f32 (f32,f32)", np.float32)):
        mz = np.ascontiguousarray(batch["mz"], dtype)
        want = rollup.recalibrate(mz, off, run, cal)
        src = torch.from_numpy(mz).to(dev)
        work, spare = src.clone(), torch.empty_like(src)
        got = plan.recalibrate(src, d_off, d_cal, run=d_run)
        assert got.cpu().numpy().tobytes() == want.tobytes(), "%s %s: the kernel and the restatement differ" % (name, label)
        t = {k: [] for k in ("kernel", "copy", "host")}
        for i in range(warm + runs):
            work.copy_(src)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            plan.recalibrate(work, d_off, d_cal, run=d_run, out=work)
            ev[1].record()
            ev[2].record()
            spare.copy_(src)                                     # (hipMemcpyAsync device to device on the same stream)
            ev[3].record()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            host = src.cpu().numpy()
            fixed = rollup.recalibrate(host, off, run, cal)
            work.copy_(torch.from_numpy(fixed))
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            if i >= warm:
                t["kernel"].append(ev[0].elapsed_time(ev[1]))
                t["copy"].append(ev[2].elapsed_time(ev[3]))
                t["host"].append(dt * 1e3)
        k, c, h = (np.array(t[x]) for x in ("kernel", "copy", "host"))
        gb = 2.0 * mz.nbytes / 1e9
        print("apply %-10s %-26s %7d spectra %9d peaks %7.1f MB  kernel ms %s = %6.0f GB/s  d2d copy ms %s  kernel/copy %5.2f  "
              "host path ms %s  host/kernel %7.0f" % (name, label, n_spec, mz.size, mz.nbytes / 2**20, pct(k), gb / (np.median(k) * 1e-3), pct(c),
                                                     np.median(k) / np.median(c), pct(h), np.median(h) / np.median(k)), flush=True)


def fit_rows(plan, warm, runs):
    dev = plan.device
    params = rollup.mz_profile_params(0.05, ppm_half_width=50.0, max_rank=9)
    rng = np.random.default_rng(17)
    for n_slots in (1, 64, 4096):
        table = np.zeros(n_slots, rollup.MZ_PROFILE_DTYPE)
        table["ppm"] = rng.poisson(5.0, (n_slots, rollup.MZP_BANDS, rollup.MZP_BINS))
        centre = rng.integers(8, 56, (n_slots, rollup.MZP_BANDS))
        for d in (-1, 0, 1):
            np.add.at(table["ppm"], (np.arange(n_slots)[:, None], np.arange(rollup.MZP_BANDS)[None, :], centre + d), 150 if d == 0 else 60)
        d_table = torch.from_numpy(table.view(np.uint8).reshape(n_slots, -1)).to(dev)
        d_cal = torch.empty((n_slots, 128), dtype=torch.uint8, device=dev)
        ms = []
        for i in range(warm + runs):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            plan.fit_mz_calibration(d_table, params, out=d_cal)
            ev[1].record()
            torch.cuda.synchronize(dev)
            if i >= warm:
                ms.append(ev[0].elapsed_time(ev[1]))
        t0 = time.perf_counter()
        want = rollup.fit_mz_calibration(table, params)
        host_ms = 1e3 * (time.perf_counter() - t0)
        assert mz_calibration_records(d_cal.cpu().numpy()).tobytes() == want.tobytes(), "fit of %d slots differs from the restatement" % n_slots
        print("fit   %5d slots  kernel ms %s  (the Python restatement, a loop per slot and band: %.1f ms)" % (n_slots, pct(np.array(ms)), host_ms),
              flush=True)


def batch_rates(scorer, batch, calls, req):
    """M PSMs/s of score_batch plain and (req not None) with recalibrate=, alternating, after one warm-up call each"""
    scorer.score_batch(batch)
    if req is not None:
        scorer.score_batch(batch, recalibrate=req)
    rates = {"plain": [], "flag": []}
    for _ in range(calls):
        t0 = time.perf_counter()
        scorer.score_batch(batch)
        rates["plain"].append(batch["n_psm"] / (time.perf_counter() - t0) / 1e6)
        if req is not None:
            t0 = time.perf_counter()
            scorer.score_batch(batch, recalibrate=req)
            rates["flag"].append(batch["n_psm"] / (time.perf_counter() - t0) / 1e6)
    return {k: np.array(v) for k, v in rates.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--dense", type=int, default=32768)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--parent-lib", default=None, help="libpyascore_hip.so of the parent commit: its plain score_batch rate in a child process")
    ap.add_argument("--batch-only", action="store_true")
    a = ap.parse_args()
    desc = synth.describe("cfg2", n_psm=a.n, seed=1000)
    cfg2 = synth.make_slice(desc)
    scorer = harness.make_scorer(PyAscore, desc["settings"])
    if a.batch_only:
        for r in batch_rates(scorer, cfg2, a.calls, None)["plain"]:
            print("rate %.4f" % r, flush=True)
        return
    print("# recalibrate_probe: seed 1000; %s; %d timed rounds after %d; %d timed score_batch calls per form and round after 1"
          % (torch.cuda.get_device_properties(scorer.device).gcnArchName, a.runs, a.warm, a.calls))
    print("# ms: median (p10..p90); kernel = HIP events around one in-place pya_recalibrate_spectra; GB/s = 2 x m/z bytes over the kernel's median; "
          "d2d copy = events around a device-to-device copy of the same bytes; host path = D2H + rollup.recalibrate + H2D, wall clock")
    plan = DevicePlan(scorer, synth.slice_batch(cfg2, 0, 2))
    apply_rows(plan, "cfg2", cfg2, a.warm, a.runs)
    dense = synth.make_slice(synth.describe("cfg2", n_psm=a.dense, seed=1000, n_noise=1500, isotopes=True))
    apply_rows(plan, "dense1570", dense, a.warm, a.runs)
    del dense
    fit_rows(plan, a.warm, a.runs)
    cal = calibration()
    req = dict(calibration=cal, run=(np.arange(a.n) * SLOTS // a.n).astype(np.int32))
    want = scorer.score_batch(dict(cfg2, mz=rollup.recalibrate(cfg2["mz"], cfg2["peak_off"], req["run"], cal)))
    got = scorer.score_batch(cfg2, recalibrate=req)
    for key in ("best_score", "best_sig", "n_sig", "ascores", "alt_mask"):
        assert got[key].tobytes() == want[key].tobytes(), "score_batch(recalibrate=) differs from corrected arrays: " + key
    first = batch_rates(scorer, cfg2, a.calls, req)
    parent = None
    if a.parent_lib:
        env = dict(os.environ, PYA_LIB=os.path.abspath(a.parent_lib), PYA_LIB_OLD="1")
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--batch-only", "--n", str(a.n), "--calls", str(2 * a.calls)], env=env,
                             check=True, capture_output=True, text=True, timeout=900).stdout
        parent = np.array([float(line.split()[1]) for line in out.splitlines() if line.startswith("rate ")])
    second = batch_rates(scorer, cfg2, a.calls, req)
    plain, flag = np.concatenate([first["plain"], second["plain"]]), np.concatenate([first["flag"], second["flag"]])
    q = lambda v: "%6.3f (%.3f..%.3f)" % (np.median(v), v.min(), v.max())  # noqa: E731
    print("score_batch cfg2 %d PSMs, M PSMs/s median (min..max): this commit plain %s; with recalibrate= %s; two rounds of this commit's plain "
          "medians %.3f and %.3f" % (a.n, q(plain), q(flag), np.median(first["plain"]), np.median(second["plain"])))
    if parent is not None:
        print("score_batch cfg2 %d PSMs, parent commit's library, plain, in a child process between the two rounds: %s" % (a.n, q(parent)))
    else:
        print("score_batch on the parent commit: not measured (no --parent-lib)")


if __name__ == "__main__":
    main()
