"""The evidence stage, measured beside the step it follows: on a device-resident plan of cfg2, cfg3, cfg4, cfg5 and the
realistic general batch, HIP events around (a) one DevicePlan.run and (b) one DevicePlan.evidence() behind it -- RUNS pairs
after WARM warm-up pairs, median and p10..p90 of each -- and PyAscore.score_batch host to host with and without
evidence=True (CALLS calls each after one warm-up call, the two alternating, median and min..max).  The rows of the plan
are compared with those of score_batch before anything is timed.  Needs a GPU: there is no fallback.

    python scripts/evidence_probe.py [--runs 30] [--calls 5] > profiles/evidence/probe.txt"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import harness  # noqa: E402
from pyascore_amd import PyAscore, synth  # noqa: E402
from pyascore_amd.device import DevicePlan, evidence_rows  # noqa: E402

CASES = (("cfg2", 100000), ("cfg3", 100000), ("cfg4", 20000), ("cfg5", 4000), ("realistic", 20000))


def make(name, n):
    if name == "realistic":
        return synth.make_realistic(n, seed=1000, general=True)
    desc = synth.describe(name, n_psm=n, seed=1000)
    return synth.make_slice(desc), desc["settings"]


def device_resident(scorer, batch, warm, runs):
    dev = torch.device("cuda", scorer.device)
    plan = DevicePlan(scorer, batch)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    out = torch.empty((plan.n_psm, plan.max_k, 16), dtype=torch.uint8, device=dev)
    step, stage = [], []
    for r in range(warm + runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        plan.run(mz, it)
        ev[1].record()
        plan.evidence(out)
        ev[2].record()
        torch.cuda.synchronize(dev)
        if r >= warm:
            step.append(ev[0].elapsed_time(ev[1]))
            stage.append(ev[1].elapsed_time(ev[2]))
    plan.check()
    rows = evidence_rows(out.cpu().numpy()).copy()
    plan.close()
    return np.array(step), np.array(stage), rows


def host_to_host(scorer, batch, calls):
    secs = {False: [], True: []}
    for flag in (False, True):
        res = scorer.score_batch(batch, evidence=flag)
    for _ in range(calls):
        for flag in (False, True):
            t0 = time.perf_counter()
            r = scorer.score_batch(batch, evidence=flag)
            secs[flag].append(time.perf_counter() - t0)
            if flag:
                res = r
    return {f: batch["n_psm"] / np.array(s) / 1e6 for f, s in secs.items()}, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every batch size")
    a = ap.parse_args()
    print("# evidence_probe: seed 1000; %s; %d timed (run, evidence) pairs after %d, %d timed score_batch calls per form after 1"
          % (torch.cuda.get_device_properties(0).gcnArchName, a.runs, a.warm, a.calls))
    print("# step / evidence = HIP events around DevicePlan.run / DevicePlan.evidence on one stream (median, p10..p90); "
          "counted / tied = rows of that kind; M PSMs/s = score_batch host to host without and with evidence=True (median, min..max)")
    print("%-9s %7s %8s %7s %22s %22s %7s %20s %20s" % ("batch", "PSMs", "counted", "tied", "step ms (p10..p90)", "evidence ms (p10..p90)",
                                                       "ratio", "M PSMs/s plain", "M PSMs/s evidence"))
    for name, n in CASES:
        n = max(64, int(n * a.scale))
        batch, settings = make(name, n)
        scorer = harness.make_scorer(PyAscore, settings)
        step, stage, rows = device_resident(scorer, batch, a.warm, a.runs)
        rate, res = host_to_host(scorer, batch, a.calls)
        assert np.array_equal(rows.view("V16"), res["evidence"].view("V16")), "%s: plan and score_batch rows differ" % name
        p = lambda v: "%7.3f (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))  # noqa: E731
        q = lambda v: "%6.2f (%.2f..%.2f)" % (np.median(v), v.min(), v.max())  # noqa: E731
        print("%-9s %7d %8d %7d %22s %22s %7.2f %20s %20s" % (name, n, int((rows["kind"] == 1).sum()), int((rows["kind"] == 2).sum()),
                                                            p(step), p(stage), np.median(stage) / np.median(step), q(rate[False]), q(rate[True])),
              flush=True)


if __name__ == "__main__":
    main()
