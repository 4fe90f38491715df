"""The named stage, measured beside the step it follows and beside the evidence stage: on a device-resident plan, HIP events
around (a) one DevicePlan.run, (b) one DevicePlan.evidence() and (c) one DevicePlan.named() behind it on one stream -- RUNS
triples after WARM warm-up triples, median and p10..p90 of each -- for cfg2 with one query per PSM (a random single move)
and with all k(n - k) single moves, cfg4 and cfg5 with one query; and PyAscore.score_batch host to host plain against
named= (CALLS calls each after one warm-up call, the two alternating, median and min..max).  The records of the plan are
compared with those of score_batch before anything is timed.  Needs a GPU: there is no fallback.

    python scripts/named_probe.py [--runs 30] [--calls 5] > profiles/named/probe.txt"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import harness  # noqa: E402
from pyascore_amd import PyAscore, synth  # noqa: E402
from pyascore_amd.device import DevicePlan, named_records  # noqa: E402
from pyascore_amd.named import site_residues  # noqa: E402

CASES = (("cfg2", 100000, "one"), ("cfg2", 100000, "moves"), ("cfg4", 20000, "one"), ("cfg5", 4000, "one"))


def queries(batch, settings, res, mode, rng):
    """per PSM: one random single move of the winner, or all of them"""
    off, bits = [0], []
    pep, pep_off = batch["pep"], batch["pep_off"]
    for i in range(int(batch["n_psm"])):
        best = int(res["best_sig"][i])
        ns = len(site_residues(pep[pep_off[i]:pep_off[i + 1]].tobytes(), settings["mod_group"]))
        mods = [j for j in range(ns) if best >> j & 1]
        free = [j for j in range(ns) if not best >> j & 1]
        moves = [(best & ~(1 << m)) | (1 << t) for m in mods for t in free] if res["n_sig"][i] > 0 else []
        if mode == "one" and moves:
            moves = [moves[int(rng.integers(len(moves)))]]
        bits += moves
        off.append(len(bits))
    return np.array(off, np.int64), np.array(bits, np.uint64)


def device_resident(scorer, batch, q_off, q_bits, warm, runs):
    dev = torch.device("cuda", scorer.device)
    plan = DevicePlan(scorer, batch)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    d_off, d_bits = torch.from_numpy(q_off).to(dev), torch.from_numpy(q_bits.view(np.int64)).to(dev)
    ev_out = torch.empty((plan.n_psm, plan.max_k, 16), dtype=torch.uint8, device=dev)
    step, evid, named = [], [], []
    for r in range(warm + runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        plan.run(mz, it)
        ev[1].record()
        plan.evidence(ev_out)
        ev[2].record()
        out = plan.named(d_off, d_bits)
        ev[3].record()
        torch.cuda.synchronize(dev)
        if r >= warm:
            step.append(ev[0].elapsed_time(ev[1]))
            evid.append(ev[1].elapsed_time(ev[2]))
            named.append(ev[2].elapsed_time(ev[3]))
    plan.check()
    rec = named_records(out.cpu().numpy()).copy()
    plan.close()
    return np.array(step), np.array(evid), np.array(named), rec


def host_to_host(scorer, batch, q_off, q_bits, calls):
    secs = {False: [], True: []}
    res = None
    for flag in (False, True):
        res = scorer.score_batch(batch, named=(q_off, q_bits) if flag else None)
    for _ in range(calls):
        for flag in (False, True):
            t0 = time.perf_counter()
            r = scorer.score_batch(batch, named=(q_off, q_bits) if flag else None)
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
    print("# named_probe: seed 1000; %s; %d timed (run, evidence, named) triples after %d, %d timed score_batch calls per form after 1"
          % (torch.cuda.get_device_properties(0).gcnArchName, a.runs, a.warm, a.calls))
    print("# step / evidence / named = HIP events around DevicePlan.run / .evidence / .named on one stream (median, p10..p90); queries: one = "
          "a random single move per PSM, moves = all k(n - k); counted / tied = records of that kind; M PSMs/s = score_batch host to "
          "host without and with named= (median, min..max)")
    print("%-6s %-6s %7s %8s %8s %6s %22s %22s %22s %9s %20s %20s" % (
        "batch", "query", "PSMs", "queries", "counted", "tied", "step ms (p10..p90)", "evidence ms (p10..p90)", "named ms (p10..p90)",
        "named/ev", "M PSMs/s plain", "M PSMs/s named"))
    for name, n, mode in CASES:
        n = max(64, int(n * a.scale))
        desc = synth.describe(name, n_psm=n, seed=1000)
        batch, settings = synth.make_slice(desc), desc["settings"]
        scorer = harness.make_scorer(PyAscore, settings)
        q_off, q_bits = queries(batch, settings, scorer.score_batch(batch), mode, np.random.default_rng(1000))
        step, evid, named, rec = device_resident(scorer, batch, q_off, q_bits, a.warm, a.runs)
        rate, res = host_to_host(scorer, batch, q_off, q_bits, a.calls)
        assert rec.tobytes() == res["named"].tobytes(), "%s: plan and score_batch records differ" % name
        p = lambda v: "%7.3f (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))  # noqa: E731
        q = lambda v: "%6.2f (%.2f..%.2f)" % (np.median(v), v.min(), v.max())  # noqa: E731
        print("%-6s %-6s %7d %8d %8d %6d %22s %22s %22s %9.2f %20s %20s" % (
            name, mode, n, q_bits.size, int((rec["kind"] == 4).sum()), int((rec["kind"] == 3).sum()), p(step), p(evid), p(named),
            np.median(named) / np.median(evid), q(rate[False]), q(rate[True])), flush=True)


if __name__ == "__main__":
    main()
