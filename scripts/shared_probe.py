"""Shared spectra, measured: cfg2's 100 000 peptides (seeded) on 100 000 / g spectra for g = 1, 2, 5, 10 -- each as a shared
batch (every spectrum once, pya_*_shared) and in its expanded form (the spectrum repeated per PSM, the entry points that
existed before).  Per g and form:

  (a) device-resident: DevicePlan.run with timing, RUNS runs after WARM warm-up runs; the median step (host clock around a
      run that ends in a stream synchronise), the p10..p90 spread, and the four kernel-family times averaged over the runs;
  (b) host to host: PyAscore.score_batch PSMs/s, CALLS calls after one warm-up call, median and spread;
  (c) the plan's workspace bytes (a plan on a fresh scorer) and the batch's spectrum bytes.

One process; shared and expanded alternate inside every g so that both see the same machine state.  The results of the two
forms are compared before anything is timed.  Needs a GPU: there is no fallback.

    python scripts/shared_probe.py [--n 100000] [--runs 30] [--calls 7] > profiles/shared_spectra/probe.txt"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import harness  # noqa: E402
from pyascore_amd import PyAscore, synth  # noqa: E402
from pyascore_amd.device import DevicePlan  # noqa: E402

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")


def shared_form(base, g):
    """PSM i of cfg2 keeps its peptide and is scored against the spectrum of PSM g * (i // g): groups of g consecutive PSMs"""
    n = base["n_psm"]
    firsts = np.arange(0, n, g)
    po = base["peak_off"]
    cnt = (po[1:] - po[:-1])[firsts]
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    idx = np.repeat(po[firsts] - off[:-1], cnt) + np.arange(off[-1], dtype=np.int64)
    return dict(base, mz=np.ascontiguousarray(base["mz"][idx]), intensity=np.ascontiguousarray(base["intensity"][idx]),
                peak_off=off, spec_of=(np.arange(n) // g).astype(np.uint32), n_spectra=int(firsts.size))


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
    return np.array(steps), tuple(f / n for f in fam), out


def workspace_bytes(settings, batch):
    """of a plan on a scorer of its own: a scorer recycles the device allocation of its previous plan, and a recycled
    allocation is reported at its own size"""
    fresh = harness.make_scorer(PyAscore, settings)
    plan = DevicePlan(fresh, batch)
    ws = plan.workspace_bytes
    plan.close()
    return ws


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
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--calls", type=int, default=7)
    a = ap.parse_args()
    desc = synth.describe("cfg2", n_psm=a.n, seed=1000)
    base = synth.make_slice(desc)
    scorer = harness.make_scorer(PyAscore, desc["settings"])
    print("# shared_probe: cfg2, %d PSMs, seed 1000; %s; %d timed runs after %d, %d timed calls after 1"
          % (a.n, torch.cuda.get_device_properties(scorer.device).gcnArchName, a.runs, a.warm, a.calls))
    print("# step = host clock around one DevicePlan.run + synchronise (median, p10..p90); families = event times per run "
          "(bin_spectra incl. the fan-out, score_signatures, score_localize, localize); M PSMs/s = score_batch host to host")
    print("%2s %-8s %8s %9s %9s %17s %9s %9s %9s %9s %12s %17s" % ("g", "form", "spectra", "spec MB", "ws MB", "step ms (p10..p90)",
                                                                   "bin ms", "score ms", "fused ms", "loc ms", "M PSMs/s", "(min..max)"))
    for g in (1, 2, 5, 10):
        shared = shared_form(base, g)
        forms = (("shared", shared), ("expanded", synth.expand_shared_batch(shared)))
        rows, outs = {}, {}
        for name, b in forms:
            steps, fam, out = device_resident(scorer, b, a.warm, a.runs)
            rows[name] = [b, steps, fam, workspace_bytes(desc["settings"], b)]
            outs[name] = out
        for key in KEYS:
            assert np.array_equal(outs["shared"][key], outs["expanded"][key]), "g = %d: %s differs" % (g, key)
        for rnd in range(2):                                  # host to host: the two forms in turn, twice
            for name, b in forms:
                rate, res = host_to_host(scorer, b, (a.calls + 1) // 2)
                rows[name].append(rate)
                assert np.array_equal(res["best_score"], outs["shared"]["best_score"]), "g = %d: score_batch differs" % g
        for name, _ in forms:
            b, steps, fam, ws, r1, r2 = rows[name]
            rate = np.concatenate([r1, r2])
            print("%2d %-8s %8d %9.1f %9.1f %7.3f (%.3f..%.3f) %9.3f %9.3f %9.3f %9.3f %12.2f %8.2f..%-8.2f"
                  % (g, name, b["peak_off"].size - 1, b["mz"].size * 16 / 2**20, ws / 2**20, np.median(steps), np.percentile(steps, 10),
                     np.percentile(steps, 90), fam[0], fam[1], fam[2], fam[3], np.median(rate), rate.min(), rate.max()), flush=True)


if __name__ == "__main__":
    main()
