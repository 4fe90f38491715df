"""Precursor stripping, measured.  One process on one GPU:

  (a) pya_strip_spectra (mark and count, scan, fill) over the spectra of 100 000 cfg2 PSMs and of bench.py's dense batch
      (32 768 spectra of about 1 570 peaks), float64 / float64, with a precursor at charge 2 or 3 inside every spectrum's own
      m/z range and two rules: "cid" (the precursor, - H3PO4, - H2O, one isotope each: 3 windows) and "etd" (the same with the
      charge-reduced forms and a third loss: 8 or 12 windows).  HIP events around one call on torch's stream, RUNS rounds after
      WARM warm-up rounds, median and p10..p90.  Beside it, in the same rounds: a device-to-device copy of the same m/z and
      intensity bytes (the floor of anything that reads and writes every peak once) and pya_deisotope_spectra on the same
      input (the neighbour with the same three passes and the same fill kernel).  The bytes of the kernels and of the numpy
      restatement pyascore_amd.rollup.strip are compared before anything is reported.
  (b) PyAscore.score_batch on cfg2 and on the dense batch's first PSMs without and with strip=, alternating, host to host.

Needs a GPU: there is no fallback.

    python scripts/strip_probe.py [--runs 30] [--calls 6] > profiles/strip/probe.txt"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import harness  # noqa: E402
from pyascore_amd import PyAscore, device, rollup, synth  # noqa: E402

H3PO4, H2O, NH3 = 97.976896, 18.010565, 17.026549
RULES = {"cid": dict(tol=0.05, losses=(H3PO4, H2O), isotopes=1),
         "etd": dict(tol=0.05, losses=(H3PO4, H2O, NH3), isotopes=1, reduced=True)}
DEISO = rollup.deisotope_params()


def pct(v):
    return "%9.4f (%.4f..%.4f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))


def precursors(batch, seed=1000):
    rng = np.random.default_rng(seed)
    off = np.asarray(batch["peak_off"], np.int64)
    mz = np.asarray(batch["mz"], np.float64)
    first, last = mz[off[:-1]], mz[off[1:] - 1]                  # (the spectra are ascending and none is empty)
    return rng.uniform(first + 0.3 * (last - first), first + 0.7 * (last - first)), rng.integers(2, 4, off.size - 1).astype(np.int32)


def kernel_rows(scorer, name, batch, warm, runs):
    dev = torch.device("cuda", scorer.device)
    off = np.ascontiguousarray(batch["peak_off"], np.int64)
    mz, it = np.ascontiguousarray(batch["mz"], np.float64), np.ascontiguousarray(batch["intensity"], np.float64)
    pm, pz = precursors(batch)
    d_mz, d_it, d_off = torch.from_numpy(mz).to(dev), torch.from_numpy(it).to(dev), torch.from_numpy(off).to(dev)
    d_pm, d_pz = torch.from_numpy(pm).to(dev), torch.from_numpy(pz).to(dev)
    out = (torch.empty_like(d_mz), torch.empty_like(d_it))
    nbytes = mz.nbytes + it.nbytes
    for label, rule in RULES.items():
        p = rollup.strip_params(**rule)
        want = rollup.strip(mz, it, off, pm, pz, p)
        o_mz, o_it, d_new, d_rep, d_over = device.strip(scorer, d_mz, d_it, d_off, d_pm, d_pz, p, out=out)
        new = d_new.cpu().numpy()
        kept = int(new[-1])
        assert new.tobytes() == want[2].tobytes() and o_mz.cpu().numpy()[:kept].tobytes() == want[0].tobytes() and \
            o_it.cpu().numpy()[:kept].tobytes() == want[1].tobytes() and d_rep.cpu().numpy().tobytes() == want[3].tobytes(), \
            "%s %s: the kernels and the restatement differ" % (name, label)
        t = {k: [] for k in ("strip", "copy", "deisotope")}
        for i in range(warm + runs):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            ev[0].record()
            device.strip(scorer, d_mz, d_it, d_off, d_pm, d_pz, p, out=out)
            ev[1].record()
            ev[2].record()
            out[0].copy_(d_mz)                                   # (hipMemcpyAsync device to device on the same stream)
            out[1].copy_(d_it)
            ev[3].record()
            ev[4].record()
            device.deisotope(scorer, d_mz, d_it, d_off, DEISO, out=out)
            ev[5].record()
            torch.cuda.synchronize(dev)
            if i >= warm:
                for k, key in enumerate(("strip", "copy", "deisotope")):
                    t[key].append(ev[2 * k].elapsed_time(ev[2 * k + 1]))
        s, c, d = (np.array(t[x]) for x in ("strip", "copy", "deisotope"))
        print("strip %-10s %-3s f64/f64 %7d spectra %9d peaks %7.1f MB, windows per spectrum %4.1f, kept %.4f, spectra with a hit %.3f  "
              "kernels ms %s = %6.0f GB/s read  d2d copy ms %s  kernels/copy %5.2f  pya_deisotope_spectra ms %s  strip/deisotope %5.2f"
              % (name, label, off.size - 1, mz.size, nbytes / 2**20, float(want[3]["n_windows"].mean()), kept / max(mz.size, 1),
                 float((want[3]["hit"] != 0).mean()), pct(s), nbytes / 1e9 / (np.median(s) * 1e-3), pct(c), np.median(s) / np.median(c), pct(d),
                 np.median(s) / np.median(d)), flush=True)
    return pm, pz


def batch_rows(scorer, name, batch, pm, pz, calls):
    req = dict(RULES["cid"], precursor_mz=pm, precursor_charge=pz)
    f = rollup.strip(batch["mz"], batch["intensity"], batch["peak_off"], pm, pz, rollup.strip_params(**RULES["cid"]))
    want = scorer.score_batch(dict(batch, mz=f[0], intensity=f[1], peak_off=f[2]))
    got = scorer.score_batch(batch, strip=req)
    for key in ("best_score", "best_sig", "n_sig", "ascores", "alt_mask"):
        assert got[key].tobytes() == want[key].tobytes(), "score_batch(strip=) differs from stripped arrays: " + key
    rates = {"plain": [], "strip": []}
    for _ in range(calls):
        for label, kw in (("plain", {}), ("strip", dict(strip=req))):
            t0 = time.perf_counter()
            scorer.score_batch(batch, **kw)
            rates[label].append(batch["n_psm"] / (time.perf_counter() - t0) / 1e6)
    q = lambda v: "%6.3f (%.3f..%.3f)" % (np.median(v), np.min(v), np.max(v))  # noqa: E731
    print("score_batch %-10s %6d PSMs, M PSMs/s median (min..max) of %d calls after 1: plain %s; with strip= (cid) %s"
          % (name, batch["n_psm"], calls, q(rates["plain"]), q(rates["strip"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--dense", type=int, default=32768)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--calls", type=int, default=6)
    a = ap.parse_args()
    desc = synth.describe("cfg2", n_psm=a.n, seed=1000)
    scorer = harness.make_scorer(PyAscore, desc["settings"])
    print("# strip_probe: seed 1000; %s; %d timed rounds after %d; rules %s"
          % (torch.cuda.get_device_properties(scorer.device).gcnArchName, a.runs, a.warm, RULES))
    print("# ms: median (p10..p90); kernels = HIP events around one pya_strip_spectra (three passes); GB/s = m/z and intensity bytes read over the "
          "kernels' median; d2d copy = events around device-to-device copies of the same bytes; pya_deisotope_spectra: the same input, defaults")
    cfg2 = synth.make_slice(desc)
    print("cfg2 generated", file=sys.stderr, flush=True)
    pm, pz = kernel_rows(scorer, "cfg2", cfg2, a.warm, a.runs)
    batch_rows(scorer, "cfg2", cfg2, pm, pz, a.calls)
    del cfg2
    dense = synth.make_slice(synth.describe("cfg2", n_psm=a.dense, seed=1000, n_noise=1500, isotopes=True))
    print("dense generated", file=sys.stderr, flush=True)
    pm, pz = kernel_rows(scorer, "dense1570", dense, a.warm, a.runs)
    n = min(a.dense, 8192)
    batch_rows(scorer, "dense1570", synth.slice_batch(dense, 0, n), pm[:n], pz[:n], a.calls)


if __name__ == "__main__":
    main()
