"""The ion stage, measured beside the step it follows: on a device-resident plan of cfg2 and cfg4, HIP events around (a) one
DevicePlan.run, (b) pya_plan_ions_count behind it -- evidence rows, count pass and scan; their split per kernel comes from
a kernel trace of this script (scripts/kstat.sh) --, (c) pya_plan_ions, the fill, and (d) the copy of offsets and records
to pinned host memory -- RUNS rounds after WARM warm-up rounds, median and p10..p90 of each -- with the records and bytes
per PSM, and
PyAscore.score_batch host to host with and without ions=True (CALLS calls each after one warm-up call, the two
alternating, median and min..max).  The records of the plan are compared with those of score_batch before anything is
timed.  Needs a GPU: there is no fallback.

    python scripts/ions_probe.py [--runs 20] [--calls 3] > profiles/ions/probe.txt"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import harness  # noqa: E402
from pyascore_amd import PyAscore, synth  # noqa: E402
from pyascore_amd.device import DevicePlan  # noqa: E402

CASES = (("cfg2", 100000), ("cfg4", 20000))


def device_resident(scorer, batch, warm, runs):
    dev = torch.device("cuda", scorer.device)
    lib = scorer._lib
    plan = DevicePlan(scorer, batch, ions=True)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    plan.run(mz, it)
    off, rec = plan.ions()                                   # (sizes: the records of a run do not change from run to run)
    total = rec.shape[0]
    h_off = torch.empty(off.shape, dtype=off.dtype).pin_memory()
    h_rec = torch.empty(rec.shape, dtype=rec.dtype).pin_memory()
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = C.byref(plan._res)
    names = ("step", "count", "fill", "d2h")
    ms = {k: [] for k in names}
    for r in range(warm + runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        plan.run(mz, it)
        ev[1].record()
        assert lib.pya_plan_ions_count(plan._plan, res, stream, off.data_ptr()) == 0
        ev[2].record()
        assert lib.pya_plan_ions(plan._plan, res, stream, off.data_ptr(), rec.data_ptr(), total) == 0
        ev[3].record()
        h_off.copy_(off, non_blocking=True)
        h_rec.copy_(rec, non_blocking=True)
        ev[4].record()
        torch.cuda.synchronize(dev)
        if r >= warm:
            for i, k in enumerate(names):
                ms[k].append(ev[i].elapsed_time(ev[i + 1]))
    plan.check()
    out = h_off.numpy().copy(), h_rec.numpy().copy()
    plan.close()
    return {k: np.array(v) for k, v in ms.items()}, out


def host_to_host(scorer, batch, calls):
    secs = {False: [], True: []}
    for flag in (False, True):
        res = scorer.score_batch(batch, ions=flag)
    for _ in range(calls):
        for flag in (False, True):
            t0 = time.perf_counter()
            r = scorer.score_batch(batch, ions=flag)
            secs[flag].append(time.perf_counter() - t0)
            if flag:
                res = r
    return {f: batch["n_psm"] / np.array(s) / 1e6 for f, s in secs.items()}, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every batch size")
    a = ap.parse_args()
    print("# ions_probe: seed 1000; %s; %d timed rounds after %d, %d timed score_batch calls per form after 1"
          % (torch.cuda.get_device_properties(0).gcnArchName, a.runs, a.warm, a.calls))
    print("# ms = HIP events on one stream, median (p10..p90): step = DevicePlan.run; count = pya_plan_ions_count (evidence rows, count "
          "pass, scan); fill = pya_plan_ions; d2h = offsets and records to pinned memory; "
          "M PSMs/s = score_batch host to host without and with ions=True (median, min..max)")
    p = lambda v: "%.3f (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))  # noqa: E731
    q = lambda v: "%.2f (%.2f..%.2f)" % (np.median(v), v.min(), v.max())  # noqa: E731
    for name, n in CASES:
        n = max(64, int(n * a.scale))
        desc = synth.describe(name, n_psm=n, seed=1000)
        batch, settings = synth.make_slice(desc), desc["settings"]
        scorer = harness.make_scorer(PyAscore, settings)
        ms, (off, rec) = device_resident(scorer, batch, a.warm, a.runs)
        rate, res = host_to_host(scorer, batch, a.calls)
        assert np.array_equal(off, res["ion_off"]) and rec.tobytes() == res["ions"].tobytes(), "%s: plan and score_batch records differ" % name
        total = int(off[-1])
        first = int((res["ions"]["site"] == 255).sum())
        print("%s  %d PSMs  %d records (%d winner's, %d site-determining)  %.1f records, %.0f bytes per PSM"
              % (name, n, total, first, total - first, total / n, 16. * total / n + 8))
        for k in ("step", "count", "fill", "d2h"):
            print("    %-6s ms %s" % (k, p(ms[k])))
        print("    count + fill over step: %.1f" % ((np.median(ms["count"]) + np.median(ms["fill"])) / np.median(ms["step"])))
        print("    M PSMs/s plain %s   with ions %s" % (q(rate[False]), q(rate[True])), flush=True)


if __name__ == "__main__":
    main()
