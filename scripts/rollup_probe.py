"""The roll-up stage, measured beside the step it follows, beside the probability stage on the same plan, and beside the host
way it replaces: on a device-resident plan, HIP events around (a) one DevicePlan.run, (b) one DevicePlan.probs(), (c) one
DevicePlan.rollup_clear and (d) one DevicePlan.rollup behind them on one stream -- RUNS rounds after WARM warm-up rounds, every
stage into tensors allocated before, median and p10..p90 of each -- for 100 000 cfg2 PSMs and 4 000 cfg5 PSMs keyed so that
about five PSMs share every slot; then host to host: PyAscore.score_batch with and without rollup=, and the host way on the
same plan: the residue and PSM records to the host (D2H) and a numpy reduction with np.maximum.at / np.minimum.at / np.add.at
that makes the same table.  The tables of the plan, of score_batch and of the numpy reduction are compared bytewise before
anything is reported.  Needs a GPU: there is no fallback.

    python scripts/rollup_probe.py [--runs 20] [--calls 3] > profiles/rollup/probe.txt"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import harness  # noqa: E402
from pyascore_amd import PyAscore, synth  # noqa: E402
from pyascore_amd.device import DevicePlan, psm_prob_records, rollup_records  # noqa: E402
from pyascore_amd.rollup import NO_PSM, ROLLUP_DTYPE  # noqa: E402

CASES = (("cfg2", 100000), ("cfg5", 4000))
SHARE = 5
THR = 0.75


def shared_slots(site_off, share):
    """PSM i belongs to group i mod (n / share); record r of a PSM goes to the r-th slot of its group"""
    n = site_off.size - 1
    groups = max(1, n // share)
    g = np.arange(n) % groups
    ns = np.diff(site_off)
    width = np.zeros(groups, np.int64)
    np.maximum.at(width, g, ns)
    base = np.concatenate([[0], np.cumsum(width)])
    owner = np.repeat(np.arange(n), ns)
    r = np.arange(int(site_off[-1])) - site_off[owner]
    return (base[g[owner]] + r).astype(np.int32), int(base[-1])


def numpy_way(with_prob, kind, site_off, best_sig, ascores, slot, n_slots, thr):
    n = site_off.size - 1
    owner = np.repeat(np.arange(n), np.diff(site_off))
    r = (np.arange(int(site_off[-1])) - site_off[owner]).astype(np.uint64)
    ok = (kind[owner] == 1) & (slot >= 0) & (slot < n_slots)
    s, owner, r, p = slot[ok], owner[ok], r[ok], with_prob[ok]
    bits = p.view(np.uint64)
    t = np.zeros(n_slots, ROLLUP_DTYPE)
    top = np.zeros(n_slots, np.uint64)
    np.maximum.at(top, s, bits)
    t["best_prob"] = top.view(np.float64)
    best = np.full(n_slots, NO_PSM, np.uint32)
    at = bits == top[s]
    np.minimum.at(best, s[at], owner[at].astype(np.uint32))
    t["best_psm"] = best
    np.add.at(t["n_psm"], s, 1)
    np.add.at(t["n_confident"], s[p >= thr], 1)
    sig = best_sig[owner]
    inb = (sig >> r) & np.uint64(1) != 0
    below = sig & ((np.uint64(1) << r) - np.uint64(1))
    col = np.unpackbits(below[inb].view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)
    a = ascores[owner[inb], col].view(np.uint32)
    key = np.where(a >> 31 != 0, ~a, a | np.uint32(0x80000000))
    kmax = np.zeros(n_slots, np.uint32)
    np.maximum.at(kmax, s[inb], key)
    np.add.at(t["n_in_best"], s[inb], 1)
    back = np.where(kmax >> 31 != 0, kmax & np.uint32(0x7FFFFFFF), ~kmax)
    t["best_ascore"] = np.where(t["n_in_best"] != 0, back, np.uint32(0)).astype(np.uint32).view(np.float32)
    return t


def device_resident(scorer, batch, warm, runs):
    dev = torch.device("cuda", scorer.device)
    plan = DevicePlan(scorer, batch)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    off = plan.site_offsets()
    slot, n_slots = shared_slots(off, SHARE)
    d_slot = torch.from_numpy(slot).to(dev)
    rec = (torch.zeros((int(off[-1]), 2), dtype=torch.float64, device=dev), torch.zeros((batch["n_psm"], 16), dtype=torch.uint8, device=dev))
    table = plan.rollup_clear(n_slots)
    t = {k: [] for k in ("step", "probs", "clear", "rollup", "host")}
    for i in range(warm + runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        plan.run(mz, it)
        ev[1].record()
        plan.probs(out=rec)
        ev[2].record()
        plan.rollup_clear(table=table)
        ev[3].record()
        plan.rollup(rec[0], rec[1], d_slot, table, threshold=THR)
        ev[4].record()
        torch.cuda.synchronize(dev)
        # the host way on the same records: D2H of what the reduction reads, then numpy
        t0 = time.perf_counter()
        sp = rec[0].cpu().numpy()
        pp = psm_prob_records(rec[1].cpu().numpy())
        res = dict(best_sig=plan.best_sig.cpu().numpy().view(np.uint64), ascores=plan.ascores.cpu().numpy())
        host = numpy_way(np.ascontiguousarray(sp[:, 0]), pp["kind"], off, res["best_sig"], res["ascores"], slot, n_slots, THR)
        dt = time.perf_counter() - t0
        if i >= warm:
            for j, k in enumerate(("step", "probs", "clear", "rollup")):
                t[k].append(ev[j].elapsed_time(ev[j + 1]))
            t["host"].append(dt * 1e3)
    plan.check()
    got = rollup_records(table.cpu().numpy()).copy()
    plan.close()
    return {k: np.array(v) for k, v in t.items()}, got, host, slot, n_slots


def host_to_host(scorer, batch, slot, n_slots, calls):
    secs = {"plain": [], "rollup": []}
    req = dict(slot=slot, n_slots=n_slots, threshold=THR)
    res = scorer.score_batch(batch, rollup=req, site_sig_cap=0)
    scorer.score_batch(batch)
    for _ in range(calls):
        t0 = time.perf_counter()
        scorer.score_batch(batch)
        secs["plain"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        res = scorer.score_batch(batch, rollup=req, site_sig_cap=0)
        secs["rollup"].append(time.perf_counter() - t0)
    return {f: batch["n_psm"] / np.array(s) / 1e6 for f, s in secs.items()}, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every batch size")
    a = ap.parse_args()
    print("# rollup_probe: seed 1000; %s; %d timed rounds (run, probs, clear, rollup, host way) after %d, %d timed score_batch calls per form after 1"
          % (torch.cuda.get_device_properties(0).gcnArchName, a.runs, a.warm, a.calls))
    print("# step / probs / clear / rollup = HIP events around DevicePlan.run / .probs / .rollup_clear / .rollup on one stream, ms (median, "
          "p10..p90); host ms = the way it replaces on the same records: D2H of the residue and PSM records, best_sig and ascores, "
          "then np.maximum.at / np.minimum.at / np.add.at (wall clock); records = residue records, slots = table size (about %d PSMs "
          "per slot); M PSMs/s = score_batch host to host plain and with rollup= (median, min..max)" % SHARE)
    print("%-6s %7s %9s %8s %22s %22s %22s %22s %26s %20s %20s" % (
        "batch", "PSMs", "records", "slots", "step ms (p10..p90)", "probs ms (p10..p90)", "clear ms (p10..p90)", "rollup ms (p10..p90)",
        "host ms (p10..p90)", "M PSMs/s plain", "M PSMs/s rollup="))
    for name, n in CASES:
        n = max(64, int(n * a.scale))
        desc = synth.describe(name, n_psm=n, seed=1000)
        batch, settings = synth.make_slice(desc), desc["settings"]
        scorer = harness.make_scorer(PyAscore, settings)
        t, got, host, slot, n_slots = device_resident(scorer, batch, a.warm, a.runs)
        assert got.tobytes() == host.tobytes(), "%s: the device table and the numpy reduction differ" % name
        rate, res = host_to_host(scorer, batch, slot, n_slots, a.calls)
        assert res["rollup"].tobytes() == got.tobytes(), "%s: plan and score_batch tables differ" % name
        p = lambda v: "%8.3f (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))  # noqa: E731
        q = lambda v: "%6.3f (%.3f..%.3f)" % (np.median(v), v.min(), v.max())  # noqa: E731
        print("%-6s %7d %9d %8d %22s %22s %22s %22s %26s %20s %20s" % (
            name, n, slot.size, n_slots, p(t["step"]), p(t["probs"]), p(t["clear"]), p(t["rollup"]), p(t["host"]), q(rate["plain"]),
            q(rate["rollup"])), flush=True)


if __name__ == "__main__":
    main()
