"""Deisotoping, measured.  One process on one GPU:

  (a) pya_deisotope_spectra (mark and count, scan, fill) over the spectra of 100 000 cfg2 PSMs and of bench.py's dense batch
      (32 768 spectra of about 1 570 peaks, two thirds of them satellites), float64 / float64: HIP events around one call on
      torch's stream, RUNS rounds after WARM warm-up rounds, median and p10..p90.  Beside it, in the same rounds: a
      device-to-device copy of the same m/z and intensity bytes (the floor of anything that reads and writes every peak once)
      and, for a few rounds, the path the kernels replace on resident arrays (D2H, the numpy restatement
      pyascore_amd.rollup.deisotope, H2D; wall clock around work that ends in a synchronise).  The bytes of the kernels and of
      the restatement are compared before anything is reported.
  (b) the resident step of the dense batch before and after filtering, for the same PSMs: DevicePlan.run on the arrays as they
      are and on the filtered ones (a plan each: the peak counts differ), HIP events around a run and the binning share from
      the plan's own timings.
  (c) PyAscore.score_batch on the dense batch's first PSMs and on cfg2 without and with deisotope=, alternating, host to host.

Needs a GPU: there is no fallback.

    python scripts/deisotope_probe.py [--runs 30] [--calls 6] > profiles/deisotope/probe.txt"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import harness  # noqa: E402
from pyascore_amd import PyAscore, device, rollup, synth  # noqa: E402

P = rollup.deisotope_params()


def pct(v):
    return "%9.4f (%.4f..%.4f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))


def kernel_rows(scorer, name, batch, warm, runs, host_rounds):
    dev = torch.device("cuda", scorer.device)
    off = np.ascontiguousarray(batch["peak_off"], np.int64)
    mz, it = np.ascontiguousarray(batch["mz"], np.float64), np.ascontiguousarray(batch["intensity"], np.float64)
    d_mz, d_it, d_off = torch.from_numpy(mz).to(dev), torch.from_numpy(it).to(dev), torch.from_numpy(off).to(dev)
    out = (torch.empty_like(d_mz), torch.empty_like(d_it))
    t0 = time.perf_counter()
    want = rollup.deisotope(mz, it, off, P)
    restatement_ms = 1e3 * (time.perf_counter() - t0)
    o_mz, o_it, d_new, d_over = device.deisotope(scorer, d_mz, d_it, d_off, P, out=out)
    new = d_new.cpu().numpy()
    kept = int(new[-1])
    assert new.tobytes() == want[2].tobytes() and o_mz.cpu().numpy()[:kept].tobytes() == want[0].tobytes() and \
        o_it.cpu().numpy()[:kept].tobytes() == want[1].tobytes(), "%s: the kernels and the restatement differ" % name
    t = {k: [] for k in ("kernel", "copy", "host")}
    for i in range(warm + runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        device.deisotope(scorer, d_mz, d_it, d_off, P, out=out)
        ev[1].record()
        ev[2].record()
        out[0].copy_(d_mz)                                       # (hipMemcpyAsync device to device on the same stream)
        out[1].copy_(d_it)
        ev[3].record()
        torch.cuda.synchronize(dev)
        if i >= warm:
            t["kernel"].append(ev[0].elapsed_time(ev[1]))
            t["copy"].append(ev[2].elapsed_time(ev[3]))
        if warm <= i < warm + host_rounds:
            t0 = time.perf_counter()
            h_mz, h_it = d_mz.cpu().numpy(), d_it.cpu().numpy()
            f = rollup.deisotope(h_mz, h_it, off, P)
            out[0][:f[0].size].copy_(torch.from_numpy(f[0]))
            out[1][:f[1].size].copy_(torch.from_numpy(f[1]))
            torch.cuda.synchronize(dev)
            t["host"].append(1e3 * (time.perf_counter() - t0))
    k, c, h = (np.array(t[x]) for x in ("kernel", "copy", "host"))
    nbytes = mz.nbytes + it.nbytes
    print("deisotope %-10s f64/f64 %7d spectra %9d peaks %7.1f MB, kept %.4f  kernels ms %s = %6.0f GB/s read  d2d copy ms %s  kernels/copy %5.2f  "
          "host path ms %s (%d rounds; the restatement alone %.0f ms)  host/kernels %7.0f"
          % (name, off.size - 1, mz.size, nbytes / 2**20, kept / max(mz.size, 1), pct(k), nbytes / 1e9 / (np.median(k) * 1e-3), pct(c),
             np.median(k) / np.median(c), pct(h), h.size, restatement_ms, np.median(h) / np.median(k)), flush=True)
    return dict(batch, mz=want[0], intensity=want[1], peak_off=want[2])


def step_rows(scorer, name, forms, warm, runs):
    dev = torch.device("cuda", scorer.device)
    for label, batch in forms:
        plan = device.DevicePlan(scorer, batch, timing=True)
        d_mz, d_it = torch.from_numpy(np.ascontiguousarray(batch["mz"])).to(dev), torch.from_numpy(np.ascontiguousarray(batch["intensity"])).to(dev)
        step, binning = [], []
        for i in range(warm + runs):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            plan.run(d_mz, d_it)
            ev[1].record()
            torch.cuda.synchronize(dev)
            if i >= warm:
                step.append(ev[0].elapsed_time(ev[1]))
                binning.append(plan.timings_ms()[0])
        plan.check()
        step, binning = np.array(step), np.array(binning)
        print("step %-10s %-9s %6d PSMs %9d peaks  resident step ms %s = %6.2f M PSMs/s  binning ms %s"
              % (name, label, batch["n_psm"], int(batch["peak_off"][-1]), pct(step), batch["n_psm"] / np.median(step) / 1e3, pct(binning)), flush=True)
        plan.close()


def batch_rows(scorer, name, batch, calls):
    want = scorer.score_batch(dict(batch, **dict(zip(("mz", "intensity", "peak_off"), rollup.deisotope(batch["mz"], batch["intensity"], batch["peak_off"], P)[:3]))))
    got = scorer.score_batch(batch, deisotope=True)
    for key in ("best_score", "best_sig", "n_sig", "ascores", "alt_mask"):
        assert got[key].tobytes() == want[key].tobytes(), "score_batch(deisotope=) differs from filtered arrays: " + key
    rates = {"plain": [], "deisotope": []}
    for _ in range(calls):
        for label, kw in (("plain", {}), ("deisotope", dict(deisotope=True))):
            t0 = time.perf_counter()
            scorer.score_batch(batch, **kw)
            rates[label].append(batch["n_psm"] / (time.perf_counter() - t0) / 1e6)
    q = lambda v: "%6.3f (%.3f..%.3f)" % (np.median(v), np.min(v), np.max(v))  # noqa: E731
    print("score_batch %-10s %6d PSMs, M PSMs/s median (min..max) of %d calls after 1: plain %s; with deisotope= %s"
          % (name, batch["n_psm"], calls, q(rates["plain"]), q(rates["deisotope"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--dense", type=int, default=32768)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--host-rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=6)
    a = ap.parse_args()
    desc = synth.describe("cfg2", n_psm=a.n, seed=1000)
    scorer = harness.make_scorer(PyAscore, desc["settings"])
    print("# deisotope_probe: seed 1000; %s; %d timed rounds after %d; tol %g, charges 1..%d, ratio %g"
          % (torch.cuda.get_device_properties(scorer.device).gcnArchName, a.runs, a.warm, P["tol"], P["max_charge"], P["ratio0"]))
    print("# ms: median (p10..p90); kernels = HIP events around one pya_deisotope_spectra (three passes); GB/s = m/z and intensity bytes read over the "
          "kernels' median; d2d copy = events around device-to-device copies of the same bytes; host path = D2H + rollup.deisotope + H2D, wall clock")
    cfg2 = synth.make_slice(desc)
    kernel_rows(scorer, "cfg2", cfg2, a.warm, a.runs, a.host_rounds)
    batch_rows(scorer, "cfg2", cfg2, a.calls)
    del cfg2
    dense = synth.make_slice(synth.describe("cfg2", n_psm=a.dense, seed=1000, n_noise=1500, isotopes=True))
    filtered = kernel_rows(scorer, "dense1570", dense, a.warm, a.runs, min(a.host_rounds, 1))
    step_rows(scorer, "dense1570", (("as it is", dense), ("filtered", filtered)), a.warm, a.runs)
    batch_rows(scorer, "dense1570", synth.slice_batch(dense, 0, min(a.dense, 8192)), a.calls)


if __name__ == "__main__":
    main()
