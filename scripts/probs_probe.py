"""The probability stage, measured beside the step it follows and beside the site stage: on a device-resident plan, HIP
events around (a) one DevicePlan.run, (b) one DevicePlan.sites() and (c) one DevicePlan.probs() behind it on one stream --
RUNS triples after WARM warm-up triples, both stages into tensors allocated before, median and p10..p90 of each -- for cfg2, cfg4 and cfg5, with the stage's count-node
front end where the settings allow it and with the general front end forced (PYA_NO_PROB_CNT); and PyAscore.score_batch host
to host plain against probs=True (CALLS calls each after one warm-up call, the two alternating, median and min..max).  The
records of the two front ends and those of score_batch are compared bytewise before anything is reported.  The site stage
scores as the general front end does and reduces with max in place of +: probs (general) - sites is what the sequential
double sums cost over that.  Needs a GPU: there is no fallback.

    python scripts/probs_probe.py [--runs 30] [--calls 5] > profiles/probs/probe.txt"""
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

CASES = (("cfg2", 100000), ("cfg4", 20000), ("cfg5", 4000))


def device_resident(scorer, batch, warm, runs):
    dev = torch.device("cuda", scorer.device)
    plan = DevicePlan(scorer, batch)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    off = plan.site_offsets()
    out = torch.zeros((int(off[-1]), 32), dtype=torch.uint8, device=dev)
    rec = (torch.zeros((int(off[-1]), 2), dtype=torch.float64, device=dev), torch.zeros((batch["n_psm"], 16), dtype=torch.uint8, device=dev))
    step, sites, probs = [], [], []
    for r in range(warm + runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        plan.run(mz, it)
        ev[1].record()
        plan.sites(out=out)
        ev[2].record()
        plan.probs(out=rec)
        ev[3].record()
        torch.cuda.synchronize(dev)
        if r >= warm:
            step.append(ev[0].elapsed_time(ev[1]))
            sites.append(ev[1].elapsed_time(ev[2]))
            probs.append(ev[2].elapsed_time(ev[3]))
    plan.check()
    raw = rec[0].cpu().numpy().tobytes() + rec[1].cpu().numpy().tobytes()
    plan.close()
    return np.array(step), np.array(sites), np.array(probs), raw


def host_to_host(scorer, batch, calls):
    secs = {False: [], True: []}
    res = None
    for flag in (False, True):
        res = scorer.score_batch(batch, probs=flag, site_sig_cap=0)
    for _ in range(calls):
        for flag in (False, True):
            t0 = time.perf_counter()
            r = scorer.score_batch(batch, probs=flag, site_sig_cap=0)
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
    print("# probs_probe: seed 1000; %s; %d timed (run, sites, probs) triples after %d per front end, %d timed score_batch calls per form "
          "after 1" % (torch.cuda.get_device_properties(0).gcnArchName, a.runs, a.warm, a.calls))
    print("# step / sites / probs = HIP events around DevicePlan.run / .sites / .probs (no cap) on one stream (median, p10..p90); cnt = the "
          "stage as launched (count-node front end where the settings allow it: cfg2, cfg5), gen = PYA_NO_PROB_CNT; sigs = site assignments "
          "the stage scores; M PSMs/s = score_batch host to host without and with probs=True (median, min..max)")
    print("%-6s %7s %9s %10s %22s %22s %24s %24s %9s %20s %20s" % (
        "batch", "PSMs", "records", "sigs", "step ms (p10..p90)", "sites ms (p10..p90)", "probs cnt ms (p10..p90)", "probs gen ms (p10..p90)",
        "gen/cnt", "M PSMs/s plain", "M PSMs/s probs"))
    for name, n in CASES:
        n = max(64, int(n * a.scale))
        desc = synth.describe(name, n_psm=n, seed=1000)
        batch, settings = synth.make_slice(desc), desc["settings"]
        scorer = harness.make_scorer(PyAscore, settings)
        step, sites, cnt, raw_cnt = device_resident(scorer, batch, a.warm, a.runs)
        scorer.set_debug("PYA_NO_PROB_CNT", "1")
        _, _, gen, raw_gen = device_resident(scorer, batch, a.warm, a.runs)
        scorer.set_debug("PYA_NO_PROB_CNT", None)
        assert raw_cnt == raw_gen, "%s: the two front ends leave different records" % name
        rate, res = host_to_host(scorer, batch, a.calls)
        assert raw_cnt == res["site_probs"].tobytes() + res["psm_probs"].tobytes(), "%s: plan and score_batch records differ" % name
        p = lambda v: "%8.3f (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))  # noqa: E731
        q = lambda v: "%6.2f (%.2f..%.2f)" % (np.median(v), v.min(), v.max())  # noqa: E731
        print("%-6s %7d %9d %10d %22s %22s %24s %24s %9.2f %20s %20s" % (
            name, n, res["site_probs"].size, int(res["n_sig"].clip(0).sum()), p(step), p(sites), p(cnt), p(gen), np.median(gen) / np.median(cnt),
            q(rate[False]), q(rate[True])), flush=True)


if __name__ == "__main__":
    main()
