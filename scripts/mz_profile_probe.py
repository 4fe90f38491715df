"""The fragment mass-error profile stage, measured beside the step it follows and beside the path it replaces: on a
device-resident plan, HIP events around (a) one DevicePlan.run and (b) one DevicePlan.mz_profile behind it on one stream -- RUNS
rounds after WARM warm-up rounds, into a table allocated before, median and p10..p90 of each -- for 100 000 cfg2, 20 000 cfg4
and 4 000 cfg5 PSMs spread over four run slots; then the replaced path on the same plan, wall clock: the ion stage (count,
scan, fill), its records and offsets to the host (D2H) and pyascore_amd.rollup.mz_profile over them; then host to host:
PyAscore.score_batch with and without mz_profile=.  The tables of the plan, of score_batch and of the numpy restatement are
compared bytewise before anything is reported.  Needs a GPU: there is no fallback.

    python scripts/mz_profile_probe.py [--runs 20] [--calls 3] > profiles/mz_profile/probe.txt"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import harness  # noqa: E402
from pyascore_amd import PyAscore, rollup, synth  # noqa: E402
from pyascore_amd.device import DevicePlan, ion_records, mz_profile_records  # noqa: E402

CASES = (("cfg2", 100000), ("cfg4", 20000), ("cfg5", 4000))
SLOTS = 4


def device_resident(scorer, batch, params, run, warm, runs):
    dev = torch.device("cuda", scorer.device)
    plan = DevicePlan(scorer, batch, mz_profile=True, ions=True)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    d_run = torch.from_numpy(run).to(dev)
    table = torch.zeros((SLOTS, rollup.MZ_PROFILE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    t = {k: [] for k in ("step", "stage", "replaced")}
    host = None
    for i in range(warm + runs):
        table.zero_()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        plan.run(mz, it)
        ev[1].record()
        plan.mz_profile(params, d_run, table=table)
        ev[2].record()
        torch.cuda.synchronize(dev)
        # the path it replaces on the same run: the ion stage, its records to the host, the numpy restatement
        t0 = time.perf_counter()
        off, rec = plan.ions()
        off, rec = off.cpu().numpy(), ion_records(rec.cpu().numpy())
        n_sig = plan.n_sig.cpu().numpy()
        host = rollup.mz_profile(off, rec[:int(off[-1])], n_sig, run, SLOTS, params)
        dt = time.perf_counter() - t0
        if i >= warm:
            t["step"].append(ev[0].elapsed_time(ev[1]))
            t["stage"].append(ev[1].elapsed_time(ev[2]))
            t["replaced"].append(dt * 1e3)
    plan.check()
    got = mz_profile_records(table.cpu().numpy()).copy()
    plan.close()
    return {k: np.array(v) for k, v in t.items()}, got, host


def host_to_host(scorer, batch, req, calls):
    secs = {"plain": [], "profile": []}
    res = scorer.score_batch(batch, mz_profile=req)
    scorer.score_batch(batch)
    for _ in range(calls):
        t0 = time.perf_counter()
        scorer.score_batch(batch)
        secs["plain"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        res = scorer.score_batch(batch, mz_profile=req)
        secs["profile"].append(time.perf_counter() - t0)
    return {f: batch["n_psm"] / np.array(s) / 1e6 for f, s in secs.items()}, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every batch size")
    a = ap.parse_args()
    print("# mz_profile_probe: seed 1000; %s; %d timed rounds (run, stage, replaced path) after %d, %d timed score_batch calls per form after 1"
          % (torch.cuda.get_device_properties(0).gcnArchName, a.runs, a.warm, a.calls))
    print("# step / stage = HIP events around DevicePlan.run / .mz_profile on one stream, ms (median, p10..p90); replaced ms = the ion "
          "stage's count + scan + fill, D2H of its records and offsets and rollup.mz_profile over them, on the same run (wall clock); "
          "ions = ions counted over the %d slots; M PSMs/s = score_batch host to host plain and with mz_profile= (median, min..max)" % SLOTS)
    print("%-6s %7s %9s %22s %22s %26s %20s %20s" % ("batch", "PSMs", "ions", "step ms (p10..p90)", "stage ms (p10..p90)",
                                                   "replaced ms (p10..p90)", "M PSMs/s plain", "M PSMs/s mz_profile="))
    for name, n in CASES:
        n = max(64, int(n * a.scale))
        desc = synth.describe(name, n_psm=n, seed=1000)
        batch, settings = synth.make_slice(desc), desc["settings"]
        scorer = harness.make_scorer(PyAscore, settings)
        params = rollup.mz_profile_params(float(np.float32(settings["mz_error"])), max_rank=settings["n_top"] - 1)
        run = (np.arange(n) * SLOTS // n).astype(np.int32)              # four files one after the other
        t, got, host = device_resident(scorer, batch, params, run, a.warm, a.runs)
        assert got.tobytes() == host.tobytes(), "%s: the device table and the numpy restatement differ" % name
        rate, res = host_to_host(scorer, batch, dict(run=run, n_slots=SLOTS), a.calls)
        assert res["mz_profile"].tobytes() == got.tobytes(), "%s: plan and score_batch tables differ" % name
        p = lambda v: "%8.3f (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))  # noqa: E731
        q = lambda v: "%6.3f (%.3f..%.3f)" % (np.median(v), v.min(), v.max())  # noqa: E731
        print("%-6s %7d %9d %22s %22s %26s %20s %20s" % (name, n, int(got["n_ions"].sum()), p(t["step"]), p(t["stage"]), p(t["replaced"]),
                                                        q(rate["plain"]), q(rate["profile"])), flush=True)


if __name__ == "__main__":
    main()
