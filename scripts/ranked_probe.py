"""The ranked stage, measured beside the step it follows, beside the probability stage on the same plan, and beside the
keep=True + numpy sort it replaces: on a device-resident plan, HIP events around (a) one DevicePlan.run, (b) one
DevicePlan.probs() and (c) one DevicePlan.ranked(K) for each K of 2, 5, 16, 64 behind it on one stream -- RUNS rounds after
WARM warm-up rounds, every stage into tensors allocated before, median and p10..p90 of each -- for cfg2, cfg4 and cfg5; then
host to host: PyAscore.score_batch(ranked=5) against score_batch(keep=True) + batch_pep_scores() + a numpy lexsort per PSM
that makes the same rows (CALLS calls each after one warm-up call; the old way on at most --old-psms PSMs, scaled).  The rows
of the plan, of score_batch, of the general front end (PYA_NO_PROB_CNT) and of the old way are compared bytewise before
anything is reported.  Needs a GPU: there is no fallback.

    python scripts/ranked_probe.py [--runs 20] [--calls 3] [--old-psms 1000] > profiles/ranked/probe.txt"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import harness  # noqa: E402
from pyascore_amd import PyAscore, synth  # noqa: E402
from pyascore_amd.device import DevicePlan, ranked_records  # noqa: E402
from pyascore_amd.ranked import IN_BEST_TIE, RANKED_DTYPE, SCORED, TIED_PREV  # noqa: E402

CASES = (("cfg2", 100000), ("cfg4", 20000), ("cfg5", 4000))
KS = (2, 5, 16, 64)


def device_resident(scorer, batch, warm, runs):
    dev = torch.device("cuda", scorer.device)
    plan = DevicePlan(scorer, batch)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    off = plan.site_offsets()
    rec = (torch.zeros((int(off[-1]), 2), dtype=torch.float64, device=dev), torch.zeros((batch["n_psm"], 16), dtype=torch.uint8, device=dev))
    outs = {k: torch.zeros((batch["n_psm"], k, 16), dtype=torch.uint8, device=dev) for k in KS}
    step, probs, ranked = [], [], {k: [] for k in KS}
    for r in range(warm + runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3 + len(KS))]
        ev[0].record()
        plan.run(mz, it)
        ev[1].record()
        plan.probs(out=rec)
        ev[2].record()
        for j, k in enumerate(KS):
            plan.ranked(k, out=outs[k])
            ev[3 + j].record()
        torch.cuda.synchronize(dev)
        if r >= warm:
            step.append(ev[0].elapsed_time(ev[1]))
            probs.append(ev[1].elapsed_time(ev[2]))
            for j, k in enumerate(KS):
                ranked[k].append(ev[2 + j].elapsed_time(ev[3 + j]))
    plan.check()
    rows = {k: ranked_records(outs[k].cpu().numpy()).copy() for k in KS}
    plan.close()
    return np.array(step), np.array(probs), {k: np.array(v) for k, v in ranked.items()}, rows


def old_way(scorer, batch, top_k):
    """the rows from a retained batch: every record through batch_pep_scores(), a lexsort per PSM"""
    res = scorer.score_batch(batch, keep=True)
    ps = scorer.batch_pep_scores()
    n = int(batch["n_psm"])
    out = np.zeros((n, top_k), RANKED_DTYPE)
    for i in range(n):
        lo, hi = int(ps["rec_off"][i]), int(ps["rec_off"][i + 1])
        bits, ws = ps["sig_bits"][lo:hi], ps["weighted_score"][lo:hi].astype(np.float32)
        if hi == lo:
            continue
        others = np.flatnonzero(bits != res["best_sig"][i])
        order = others[np.lexsort((bits[others], -ws[others].astype(np.float64)))][:top_k - 1]
        m = 1 + order.size
        out["sig_bits"][i, :m] = np.concatenate([[res["best_sig"][i]], bits[order]])
        out["pep_score"][i, :m] = np.concatenate([[res["best_score"][i]], ws[order]])
        out["rank"][i, :m] = np.arange(m)
        out["kind"][i, :m] = SCORED
        s = out["pep_score"][i, :m]
        out["flags"][i, :m] = np.where(s == res["best_score"][i], IN_BEST_TIE, 0)
        out["flags"][i, 1:m] |= np.where(s[1:] == s[:-1], TIED_PREV, 0).astype(np.uint8)
    return out


def host_to_host(scorer, batch, calls, old_n):
    secs = {"plain": [], "ranked": [], "old": []}
    small = synth.slice_batch(batch, 0, old_n)
    res = scorer.score_batch(batch, ranked=5, site_sig_cap=0)
    scorer.score_batch(batch)
    old = old_way(scorer, small, 5)
    for _ in range(calls):
        t0 = time.perf_counter()
        scorer.score_batch(batch)
        secs["plain"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        res = scorer.score_batch(batch, ranked=5, site_sig_cap=0)
        secs["ranked"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        old = old_way(scorer, small, 5)
        secs["old"].append(time.perf_counter() - t0)
    n = {"plain": batch["n_psm"], "ranked": batch["n_psm"], "old": old_n}
    return {f: n[f] / np.array(s) / 1e6 for f, s in secs.items()}, res, old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--old-psms", type=int, default=2000, help="PSMs the keep=True + numpy way is timed on")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every batch size")
    a = ap.parse_args()
    print("# ranked_probe: seed 1000; %s; %d timed rounds (run, probs, ranked K = %s) after %d, %d timed score_batch calls per form after 1"
          % (torch.cuda.get_device_properties(0).gcnArchName, a.runs, ", ".join(map(str, KS)), a.warm, a.calls))
    print("# step / probs / K = HIP events around DevicePlan.run / .probs / .ranked(K) (no cap) on one stream, ms (median, p10..p90); "
          "gen K=5 = the same with PYA_NO_PROB_CNT (the general front end); sigs = site assignments the stage scores; M PSMs/s = "
          "score_batch host to host plain, with ranked=5, and keep=True + batch_pep_scores() + numpy lexsort on the first PSMs of the "
          "batch (median, min..max)")
    print("%-6s %7s %10s %22s %22s %s %22s %20s %20s %26s" % (
        "batch", "PSMs", "sigs", "step ms (p10..p90)", "probs ms (p10..p90)", " ".join("%22s" % ("K=%d ms (p10..p90)" % k) for k in KS),
        "gen K=5 ms (p10..p90)", "M PSMs/s plain", "M PSMs/s ranked=5", "M PSMs/s keep+numpy (n)"))
    for name, n in CASES:
        n = max(64, int(n * a.scale))
        desc = synth.describe(name, n_psm=n, seed=1000)
        batch, settings = synth.make_slice(desc), desc["settings"]
        scorer = harness.make_scorer(PyAscore, settings)
        step, probs, ranked, rows = device_resident(scorer, batch, a.warm, a.runs)
        for k in KS[:-1]:
            assert rows[k].tobytes() == np.ascontiguousarray(rows[KS[-1]][:, :k]).tobytes(), "%s: K = %d is not the prefix of K = %d" % (name, k, KS[-1])
        scorer.set_debug("PYA_NO_PROB_CNT", "1")
        _, _, gen, rows_gen = device_resident(scorer, batch, a.warm, a.runs)
        scorer.set_debug("PYA_NO_PROB_CNT", None)
        assert all(rows[k].tobytes() == rows_gen[k].tobytes() for k in KS), "%s: the two front ends leave different rows" % name
        old_n = min(n, max(64, int(a.old_psms * a.scale)))
        rate, res, old = host_to_host(scorer, batch, a.calls, old_n)
        assert rows[5].tobytes() == res["ranked"].tobytes(), "%s: plan and score_batch rows differ" % name
        assert old.tobytes() == res["ranked"][:old_n].tobytes(), "%s: the keep=True + numpy rows differ" % name
        p = lambda v: "%8.3f (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))  # noqa: E731
        q = lambda v: "%6.3f (%.3f..%.3f)" % (np.median(v), v.min(), v.max())  # noqa: E731
        print("%-6s %7d %10d %22s %22s %s %22s %20s %20s %20s (%d)" % (
            name, n, int(res["n_sig"].clip(0).sum()), p(step), p(probs), " ".join("%22s" % p(ranked[k]) for k in KS), p(gen[5]),
            q(rate["plain"]), q(rate["ranked"]), q(rate["old"]), old_n), flush=True)


if __name__ == "__main__":
    main()
