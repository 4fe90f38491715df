"""The site stage, measured beside the step it follows and beside what it replaces: on a device-resident plan, HIP events
around (a) one DevicePlan.run and (b) one DevicePlan.sites() behind it on one stream -- RUNS pairs after WARM warm-up pairs,
median and p10..p90 of each -- for cfg2, cfg4 and cfg5; PyAscore.score_batch host to host plain against sites=True (CALLS
calls each after one warm-up call, the two alternating, median and min..max); and the way without the stage: one
score_batch(keep=True), batch_pep_scores() (96 bytes per site assignment to the host) and a numpy reduction (maximum.reduceat
per residue over the CSR records), timed once after one warm-up.  The records of the plan are compared with those of
score_batch, and their scores with the host reduction, before anything is timed.  Needs a GPU: there is no fallback.

    python scripts/sites_probe.py [--runs 30] [--calls 5] > profiles/sites/probe.txt"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import harness  # noqa: E402
from pyascore_amd import PyAscore, synth  # noqa: E402
from pyascore_amd.device import DevicePlan, site_records  # noqa: E402

CASES = (("cfg2", 100000), ("cfg4", 20000), ("cfg5", 4000))


def device_resident(scorer, batch, warm, runs):
    dev = torch.device("cuda", scorer.device)
    plan = DevicePlan(scorer, batch)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    off = plan.site_offsets()
    out = torch.zeros((int(off[-1]), 32), dtype=torch.uint8, device=dev)
    step, sites = [], []
    for r in range(warm + runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        plan.run(mz, it)
        ev[1].record()
        plan.sites(out=out)
        ev[2].record()
        torch.cuda.synchronize(dev)
        if r >= warm:
            step.append(ev[0].elapsed_time(ev[1]))
            sites.append(ev[1].elapsed_time(ev[2]))
    plan.check()
    rec = site_records(out.cpu().numpy()).copy()
    plan.close()
    return np.array(step), np.array(sites), off, rec


def host_to_host(scorer, batch, calls):
    secs = {False: [], True: []}
    res = None
    for flag in (False, True):
        res = scorer.score_batch(batch, sites=flag, site_sig_cap=0)
    for _ in range(calls):
        for flag in (False, True):
            t0 = time.perf_counter()
            r = scorer.score_batch(batch, sites=flag, site_sig_cap=0)
            secs[flag].append(time.perf_counter() - t0)
            if flag:
                res = r
    return {f: batch["n_psm"] / np.array(s) / 1e6 for f, s in secs.items()}, res


def keep_and_reduce(scorer, batch, site_off):
    """(seconds, with scores, without scores): keep=True, every record to the host, maximum.reduceat per residue"""
    t0 = time.perf_counter()
    scorer.score_batch(batch, keep=True)
    ps = scorer.batch_pep_scores()
    off, bits, ws = ps["rec_off"], ps["sig_bits"], ps["weighted_score"]
    n_sites = np.diff(site_off)
    with_s, without_s = np.full(int(site_off[-1]), -1, np.float32), np.full(int(site_off[-1]), -1, np.float32)
    some = np.flatnonzero(np.diff(off) > 0)
    starts = off[:-1][some]
    for s in range(int(n_sites.max()) if n_sites.size else 0):
        has = (bits >> np.uint64(s)) & np.uint64(1) == 1
        w = np.maximum.reduceat(np.where(has, ws, np.float32(-1)), starts)
        o = np.maximum.reduceat(np.where(has, np.float32(-1), ws), starts)
        mine = n_sites[some] > s
        with_s[site_off[:-1][some][mine] + s] = w[mine]
        without_s[site_off[:-1][some][mine] + s] = o[mine]
    return time.perf_counter() - t0, with_s, without_s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every batch size")
    a = ap.parse_args()
    print("# sites_probe: seed 1000; %s; %d timed (run, sites) pairs after %d, %d timed score_batch calls per form after 1, 1 timed "
          "keep=True + host reduction after 1" % (torch.cuda.get_device_properties(0).gcnArchName, a.runs, a.warm, a.calls))
    print("# step / sites = HIP events around DevicePlan.run / .sites (no cap) on one stream (median, p10..p90); sigs = site assignments "
          "the stage scores; M PSMs/s = score_batch host to host without and with sites=True (median, min..max), and of keep=True + "
          "batch_pep_scores() + numpy maximum.reduceat (one call)")
    print("%-6s %7s %9s %10s %22s %24s %11s %20s %20s %14s" % (
        "batch", "PSMs", "records", "sigs", "step ms (p10..p90)", "sites ms (p10..p90)", "sites/step", "M PSMs/s plain", "M PSMs/s sites",
        "M PSMs/s keep"))
    for name, n in CASES:
        n = max(64, int(n * a.scale))
        desc = synth.describe(name, n_psm=n, seed=1000)
        batch, settings = synth.make_slice(desc), desc["settings"]
        scorer = harness.make_scorer(PyAscore, settings)
        step, sites, off, rec = device_resident(scorer, batch, a.warm, a.runs)
        rate, res = host_to_host(scorer, batch, a.calls)
        assert np.array_equal(off, res["site_off"]) and rec.tobytes() == res["sites"].tobytes(), "%s: plan and score_batch records differ" % name
        keep_and_reduce(scorer, batch, off)
        secs, with_s, without_s = keep_and_reduce(scorer, batch, off)
        assert with_s.tobytes() == rec["with_score"].tobytes() and without_s.tobytes() == rec["without_score"].tobytes(), \
            "%s: the stage and the host reduction differ" % name
        p = lambda v: "%8.3f (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))  # noqa: E731
        q = lambda v: "%6.2f (%.2f..%.2f)" % (np.median(v), v.min(), v.max())  # noqa: E731
        print("%-6s %7d %9d %10d %22s %24s %11.1f %20s %20s %14.3f" % (
            name, n, rec.size, int(res["n_sig"].clip(0).sum()), p(step), p(sites), np.median(sites) / np.median(step), q(rate[False]),
            q(rate[True]), n / secs / 1e6), flush=True)


if __name__ == "__main__":
    main()
