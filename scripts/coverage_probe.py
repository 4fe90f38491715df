"""The coverage stage, measured beside the step it follows and beside the path it replaces: on a device-resident plan, HIP
events around (a) one DevicePlan.run and (b) one DevicePlan.coverage behind it on one stream -- RUNS rounds after WARM warm-up
rounds, into a tensor allocated before, median and p10..p90 of each -- for 100 000 cfg2, 20 000 cfg4 and 4 000 cfg5 PSMs; then
the replaced path on the same plan, wall clock: the ion stage (count, scan, fill), its records and offsets to the host (D2H)
and pyascore_amd.rollup.coverage over them.  The restatement is plain Python loops: it is timed on the first --restate PSMs of
the batch and scaled to the batch (the column says so); the ion stage and the copy are timed whole.  Then host to host:
PyAscore.score_batch with and without coverage=, and -- with --parent-lib, in a child process started before this one touches
the GPU -- the plain call on another build of the library (the parent commit's).  The records of the plan, of score_batch and
of the restatement (on the PSMs it covered) are compared bytewise before anything is reported.  Needs a GPU: there is no
fallback.

    python scripts/coverage_probe.py [--runs 20] [--calls 3] [--parent-lib PATH] > profiles/coverage/probe.txt"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

CASES = (("cfg2", 100000), ("cfg4", 20000), ("cfg5", 4000))


def make_case(name, n):
    from pyascore_amd import synth
    desc = synth.describe(name, n_psm=n, seed=1000)
    return synth.make_slice(desc), desc["settings"]


def plain_rates(scale, calls):
    """M PSMs/s of score_batch without the flag, per case: what a child process prints for --parent-lib"""
    from oracle import harness
    from pyascore_amd import PyAscore
    out = {}
    for name, n in CASES:
        n = max(64, int(n * scale))
        batch, settings = make_case(name, n)
        scorer = harness.make_scorer(PyAscore, settings)
        scorer.score_batch(batch)
        secs = []
        for _ in range(calls):
            t0 = time.perf_counter()
            scorer.score_batch(batch)
            secs.append(time.perf_counter() - t0)
        out[name] = [n / s / 1e6 for s in secs]
    return out


def device_resident(scorer, batch, settings, warm, runs, n_restate):
    import torch
    from pyascore_amd import rollup, synth
    from pyascore_amd.device import DevicePlan, coverage_records, ion_records
    dev = torch.device("cuda", scorer.device)
    plan = DevicePlan(scorer, batch, coverage=True, ions=True)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    out = torch.zeros((batch["n_psm"], rollup.COVERAGE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    t = {k: [] for k in ("step", "stage", "ions_d2h")}
    for i in range(warm + runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        plan.run(mz, it)
        ev[1].record()
        plan.coverage(mz, it, out=out)
        ev[2].record()
        torch.cuda.synchronize(dev)
        # the path it replaces on the same run: the ion stage and its records on the host ...
        t0 = time.perf_counter()
        off, rec = plan.ions()
        off, rec = off.cpu().numpy(), ion_records(rec.cpu().numpy())
        n_sig = plan.n_sig.cpu().numpy()
        dt = time.perf_counter() - t0
        if i >= warm:
            t["step"].append(ev[0].elapsed_time(ev[1]))
            t["stage"].append(ev[1].elapsed_time(ev[2]))
            t["ions_d2h"].append(dt * 1e3)
    plan.check()
    got = coverage_records(out.cpu().numpy()).copy()
    plan.close()
    # ... and the restatement over them, on the first n_restate PSMs, scaled to the batch
    m = min(n_restate, batch["n_psm"])
    part = synth.slice_batch(batch, 0, m)
    fwd = "".join(c for c in settings["fragment_types"] if c in "bc")
    t0 = time.perf_counter()
    host = rollup.coverage(off[:m + 1], rec, part["mz"], part["intensity"], part["peak_off"], np.diff(part["pep_off"]), fwd, n_sig[:m] > 0,
                           n_retained=got["n_retained"][:m])
    restate_ms = (time.perf_counter() - t0) * 1e3 * batch["n_psm"] / m
    return {k: np.array(v) for k, v in t.items()}, restate_ms, got, host


def host_to_host(scorer, batch, calls):
    secs = {"plain": [], "coverage": []}
    res = scorer.score_batch(batch, coverage=True)
    scorer.score_batch(batch)
    for _ in range(calls):
        t0 = time.perf_counter()
        scorer.score_batch(batch)
        secs["plain"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        res = scorer.score_batch(batch, coverage=True)
        secs["coverage"].append(time.perf_counter() - t0)
    return {f: batch["n_psm"] / np.array(s) / 1e6 for f, s in secs.items()}, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--restate", type=int, default=2000, help="PSMs the Python restatement is timed on")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every batch size")
    ap.add_argument("--parent-lib", type=str, default="", help="another build of the library: its plain score_batch rate, in a child process")
    ap.add_argument("--plain-only", action="store_true", help="print the plain score_batch rates as JSON and stop (the child of --parent-lib)")
    a = ap.parse_args()
    if a.plain_only:
        print(json.dumps(plain_rates(a.scale, a.calls)))
        return
    parent = None
    if a.parent_lib:                                        # (a fresh child process, before this one opens the GPU)
        env = dict(os.environ, PYA_LIB=os.path.abspath(a.parent_lib), PYA_LIB_OLD="1")
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--calls", str(a.calls), "--scale", str(a.scale)],
                              env=env, capture_output=True, text=True, timeout=600)
        if done.returncode != 0:
            raise SystemExit("the child with --parent-lib failed (%d):\n%s" % (done.returncode, done.stderr[-2000:]))
        parent = {k: np.array(v) for k, v in json.loads(done.stdout.strip().splitlines()[-1]).items()}
    import torch
    from oracle import harness
    from pyascore_amd import PyAscore
    print("# coverage_probe: seed 1000; %s; %d timed rounds (run, stage, ion stage + D2H) after %d, %d timed score_batch calls per form after 1"
          % (torch.cuda.get_device_properties(0).gcnArchName, a.runs, a.warm, a.calls))
    print("# step / stage = HIP events around DevicePlan.run / .coverage on one stream, ms (median, p10..p90); ions + D2H ms = the ion "
          "stage's count + scan + fill and the D2H of its records and offsets on the same run (wall clock, median, p10..p90); restate ms = "
          "rollup.coverage (Python loops) timed ONCE on the first %d PSMs and SCALED to the batch; the replaced path is the sum of the two; "
          "M PSMs/s = score_batch host to host plain, with coverage=, and plain on the parent commit's library (median, min..max; "
          "'-' without --parent-lib)" % a.restate)
    print("%-6s %7s %9s %22s %22s %26s %12s %20s %20s %20s" % ("batch", "PSMs", "fragments", "step ms (p10..p90)", "stage ms (p10..p90)",
                                                            "ions + D2H ms (p10..p90)", "restate ms", "M PSMs/s plain",
                                                            "M PSMs/s coverage=", "M PSMs/s parent"))
    for name, n in CASES:
        n = max(64, int(n * a.scale))
        batch, settings = make_case(name, n)
        scorer = harness.make_scorer(PyAscore, settings)
        t, restate_ms, got, host = device_resident(scorer, batch, settings, a.warm, a.runs, a.restate)
        assert got[:host.size].tobytes() == host.tobytes(), "%s: the device records and the restatement differ" % name
        rate, res = host_to_host(scorer, batch, a.calls)
        assert res["coverage"].tobytes() == got.tobytes(), "%s: plan and score_batch records differ" % name
        p = lambda v: "%8.3f (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))  # noqa: E731
        q = lambda v: "%6.3f (%.3f..%.3f)" % (np.median(v), v.min(), v.max())  # noqa: E731
        print("%-6s %7d %9d %22s %22s %26s %12.0f %20s %20s %20s" % (name, n, int(got["n_fragments"].sum()), p(t["step"]), p(t["stage"]),
                                                                  p(t["ions_d2h"]), restate_ms, q(rate["plain"]), q(rate["coverage"]),
                                                                  q(parent[name]) if parent is not None else "-"), flush=True)


if __name__ == "__main__":
    main()
