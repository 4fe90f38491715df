"""The site quantification, measured beside the roll-up stage on the same input and beside the host way it replaces: on a
device-resident plan of 100 000 cfg2 PSMs, HIP events around (a) one DevicePlan.rollup and (b) one DevicePlan.site_quant behind
one run and one probs() on one stream -- RUNS rounds after WARM warm-up rounds, every stage into tensors allocated before, the
quantification table cleared (outside the events) before every round, median and p10..p90 of each -- with 3, 18 and 64
channels, once with the slots spread by peptide (about five PSMs per slot) and once with every record folded onto 16 slots, the
hot case; then the host way on the same records, once per case: the probability records, best_sig and the matrix to the host
(D2H) and pyascore_amd.rollup.site_quant (wall clock).  The threshold is the median with_prob of the in-best records, so about
half of them contribute.  The tables of the plan and of the numpy restatement are compared bytewise before anything is reported.
Needs a GPU: there is no fallback.

    python scripts/site_quant_probe.py [--runs 30] > profiles/site_quant/probe.txt"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import harness  # noqa: E402
from pyascore_amd import PyAscore, rollup as ru, synth  # noqa: E402
from pyascore_amd.device import DevicePlan, psm_prob_records, site_quant_records  # noqa: E402
from pyascore_amd.probs import SITE_PROB_DTYPE  # noqa: E402

CHANNELS = (3, 18, 64)
SHARE = 5
HOT = 16
SCALE = 10


def spread_slots(site_off, share):
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


def matrix(n_rows, n_ch, seed=1000):
    rng = np.random.default_rng(seed + n_ch)
    v = rng.random((n_rows, n_ch)) * 1e5
    v[rng.random((n_rows, n_ch)) < 0.03] = np.nan
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--psms", type=int, default=100000)
    a = ap.parse_args()
    desc = synth.describe("cfg2", n_psm=a.psms, seed=1000)
    batch, settings = synth.make_slice(desc), desc["settings"]
    scorer = harness.make_scorer(PyAscore, settings)
    dev = torch.device("cuda", scorer.device)
    plan = DevicePlan(scorer, batch, quant=True)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    plan.run(mz, it)
    _, d_sites, d_psms = plan.probs()
    off = plan.site_offsets()
    torch.cuda.synchronize(dev)
    n, n_rec = int(batch["n_psm"]), int(off[-1])
    sp = d_sites.cpu().numpy()
    pp = psm_prob_records(d_psms.cpu().numpy())
    best_sig = plan.best_sig.cpu().numpy().view(np.uint64)
    owner = np.repeat(np.arange(n), np.diff(off))
    r = (np.arange(n_rec) - off[owner]).astype(np.uint64)
    in_best = ((best_sig[owner] >> r) & np.uint64(1) != 0) & (pp["kind"][owner] == 1)
    thr = float(np.median(sp[in_best, 0]))
    layouts = (("spread", *spread_slots(off, SHARE)), ("hot", (np.arange(n_rec) % HOT).astype(np.int32), HOT))
    print("# site_quant_probe: seed 1000; %s; cfg2, %d PSMs, %d residue records, %d in best, threshold %r (their median): %d contribute; "
          "%d timed rounds after %d" % (torch.cuda.get_device_properties(0).gcnArchName, n, n_rec, int(in_best.sum()), thr,
                                        int((in_best & (sp[:, 0] >= thr)).sum()), a.runs, a.warm))
    print("# ms: median (p10..p90); rollup / site_quant = HIP events around one DevicePlan.rollup (two launches) / one DevicePlan.site_quant "
          "(one launch) on the same records and slots, tables cleared outside the events; host = the way it replaces, once: D2H of the "
          "probability records, best_sig and the matrix, then rollup.site_quant (wall clock); spread = about %d PSMs per slot, hot = all "
          "records on %d slots" % (SHARE, HOT))
    for name, slot, n_slots in layouts:
        d_slot = torch.from_numpy(slot).to(dev)
        r_table = plan.rollup_clear(n_slots)
        for n_ch in CHANNELS:
            values = matrix(n, n_ch)
            d_values = torch.from_numpy(values).to(dev)
            p = ru.site_quant_params(threshold=thr, scale_log2=SCALE, n_channels=n_ch)
            table = plan.site_quant(d_sites, d_psms, d_slot, d_values, p, n_slots=n_slots)
            t = {"rollup": [], "quant": []}
            for i in range(a.warm + a.runs):
                plan.rollup_clear(table=r_table)
                for part in table:
                    part.zero_()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
                plan.rollup(d_sites, d_psms, d_slot, r_table, threshold=thr)
                ev[1].record()
                plan.site_quant(d_sites, d_psms, d_slot, d_values, p, table=table)
                ev[2].record()
                torch.cuda.synchronize(dev)
                if i >= a.warm:
                    t["rollup"].append(ev[0].elapsed_time(ev[1]))
                    t["quant"].append(ev[1].elapsed_time(ev[2]))
            plan.check()
            got = site_quant_records((table[0].cpu().numpy(), table[1].cpu().numpy()))
            t0 = time.perf_counter()
            h_sites, h_psms = d_sites.cpu().numpy(), psm_prob_records(d_psms.cpu().numpy())
            h_sig, h_values = plan.best_sig.cpu().numpy().view(np.uint64), d_values.cpu().numpy()
            t1 = time.perf_counter()
            want = ru.site_quant(np.ascontiguousarray(h_sites).view(SITE_PROB_DTYPE).reshape(-1), h_psms, off, h_sig, slot, n_slots, h_values,
                                 None, p)
            t2 = time.perf_counter()
            for g, w, what in zip(got, want, ("head", "cell")):
                assert g.tobytes() == w.tobytes(), "%s, %d channels: the device %s and the numpy restatement differ" % (name, n_ch, what)
            q = lambda v: "%8.4f (%.4f..%.4f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))  # noqa: E731
            print("site_quant cfg2 %-6s %2d channels  %8d slots  records summed %8d  rollup ms %s  site_quant ms %s  quant/rollup %5.2f  |  "
                  "host: D2H %7.1f ms + rollup.site_quant %8.1f ms" % (
                      name, n_ch, n_slots, int(got[0]["n_records"].sum()), q(t["rollup"]), q(t["quant"]),
                      np.median(t["quant"]) / np.median(t["rollup"]), (t1 - t0) * 1e3, (t2 - t1) * 1e3), flush=True)
    plan.close()


if __name__ == "__main__":
    main()
