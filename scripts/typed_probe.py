"""Typed spectra, measured: cfg2's 100 000 PSMs (seeded) and the dense batch of bench.py (cfg2's peptides on spectra of about
1 570 peaks, 32 768 PSMs), each private and as a 5-hit shared batch, with the spectrum arrays as (float64, float64),
(float64, float32) and (float32, float32) -- the arrays ROUNDED once to float32 and widened again for the wider forms, so that
all three hold the same values and must give the same results (checked before anything is timed).  Per workload and type:

  (a) host to host: PyAscore.score_batch M PSMs/s, CALLS calls after one warm-up call, median and min..max, and the bytes
      of spectra the call uploads;
  (b) device-resident: DevicePlan.run with timing, RUNS runs after WARM warm-up runs; the median step (host clock around a
      run that ends in a stream synchronise), the p10..p90 spread, and the binning family's event time per run;
  (c) the plan's workspace bytes (a plan on a fresh scorer) and the spectrum bytes it reads from HBM.

One process; the three types alternate inside every workload, twice, so that all see the same machine state.  Needs a GPU:
there is no fallback.

    python scripts/typed_probe.py [--n 100000] [--dense 32768] [--runs 30] [--calls 6] > profiles/typed_spectra/probe.txt"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import harness  # noqa: E402
from pyascore_amd import PyAscore, synth  # noqa: E402
from pyascore_amd.device import DevicePlan  # noqa: E402
from shared_probe import shared_form, workspace_bytes  # noqa: E402

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")
TYPES = (("f64,f64", np.float64, np.float64), ("f64,f32", np.float64, np.float32), ("f32,f32", np.float32, np.float32))


def device_resident(scorer, batch, warm, runs):
    dev = torch.device("cuda", scorer.device)
    plan = DevicePlan(scorer, batch, timing=True)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    for _ in range(warm):
        plan.run(mz, it)
    plan.check()
    plan.timings_sum()
    steps = []
    for _ in range(runs):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        plan.run(mz, it)
        torch.cuda.synchronize(dev)
        steps.append(1e3 * (time.perf_counter() - t0))
    fam, n = plan.timings_sum()
    out = {k: getattr(plan, k).cpu().numpy().copy() for k in KEYS}
    plan.close()
    return np.array(steps), fam[0] / n, out


def host_to_host(scorer, batch, calls):
    scorer.score_batch(batch)
    secs = []
    for _ in range(calls):
        t0 = time.perf_counter()
        res = scorer.score_batch(batch)
        secs.append(time.perf_counter() - t0)
    return batch["n_psm"] / np.array(secs) / 1e6, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--dense", type=int, default=32768)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--calls", type=int, default=6)
    a = ap.parse_args()
    loads = []
    for name, n, opts in (("cfg2", a.n, {}), ("dense1570", a.dense, dict(n_noise=1500, isotopes=True))):
        desc = synth.describe("cfg2", n_psm=n, seed=1000, **opts)
        base = synth.make_slice(desc)
        loads.append((name, desc["settings"], base))
        loads.append((name + " 5-hit", desc["settings"], shared_form(base, 5)))
    scorer = harness.make_scorer(PyAscore, loads[0][1])
    print("# typed_probe: seed 1000; %s; %d timed runs after %d, %d timed calls after 1 per round, 2 rounds"
          % (torch.cuda.get_device_properties(scorer.device).gcnArchName, a.runs, a.warm, (a.calls + 1) // 2))
    print("# M PSMs/s = score_batch numpy to numpy (median, min..max); upload MB = spectrum bytes of that call; step = host clock around "
          "one DevicePlan.run + synchronise (median, p10..p90); bin ms = the binning family's events per run; ws MB = plan workspace")
    print("%-16s %-8s %7s %10s %9s %17s %9s %20s %8s %9s" % ("workload", "types", "PSMs", "peaks/spec", "upload MB", "M PSMs/s (min..max)", "",
                                                             "step ms (p10..p90)", "bin ms", "ws MB"))
    for name, settings, base in loads:
        forms = [(t, synth.narrow_batch(synth.widen_batch(synth.narrow_batch(base)), mz_t, it_t)) for t, mz_t, it_t in TYPES]
        rows, first = {}, None
        for t, b in forms:
            steps, bin_ms, out = device_resident(scorer, b, a.warm, a.runs)
            rows[t] = [b, steps, bin_ms, workspace_bytes(settings, b)]
            first = first or out
            for key in KEYS:
                assert np.array_equal(out[key], first[key]), "%s %s: %s differs" % (name, t, key)
        for rnd in range(2):                                  # host to host: the three types in turn, twice
            for t, b in forms:
                rate, res = host_to_host(scorer, b, (a.calls + 1) // 2)
                rows[t].append(rate)
                assert np.array_equal(res["best_score"], first["best_score"]), "%s %s: score_batch differs" % (name, t)
        for t, _ in forms:
            b, steps, bin_ms, ws, r1, r2 = rows[t]
            rate = np.concatenate([r1, r2])
            n_spec = b["peak_off"].size - 1
            print("%-16s %-8s %7d %10.0f %9.1f %9.2f %8.2f..%-8.2f %8.3f (%.3f..%.3f) %8.3f %9.1f"
                  % (name, t, b["n_psm"], b["mz"].size / n_spec, (b["mz"].nbytes + b["intensity"].nbytes) / 2**20, np.median(rate), rate.min(),
                     rate.max(), np.median(steps), np.percentile(steps, 10), np.percentile(steps, 90), bin_ms, ws / 2**20), flush=True)


if __name__ == "__main__":
    main()
