"""The precursor-purity stage, measured beside a copy of the survey bytes, beside the marker stage on the same spectra and beside
the host way it replaces.

Part 1, QUERIES queries over SURVEYS survey scans of about 2 000 peaks and again of about 20 000 peaks (float64 m/z, float32
intensities; query q names scan q * SURVEYS // QUERIES, so a scan is re-read by QUERIES / SURVEYS consecutive queries: the
top-20 pattern); HIP events on one stream, RUNS rounds after WARM warm-up rounds, every output allocated before; median and
p10..p90: (a) a device-to-device copy of the survey m/z and intensities, (b) pya_purity_spectra, (c) pya_purity_gate over the
records and a matrix of 18 channels, in place, with select, (d) pya_marker_spectra with 3 targets on the same survey spectra
(one wavefront per SPECTRUM: the survey bytes read once); then (e) the path the stage replaces: the survey arrays to the host
(D2H) + pyascore_amd.rollup.purity, timed on the first HOST_QUERIES queries and scaled by the query count -- the scaling is
stated on the line.  The device records are compared bytewise with the restatement on those queries before anything is
reported.  What the re-reading costs shows in (b) against (a) and (d): bytes read by (b) = queries x peaks of a scan.

Part 2, PyAscore.score_batch on a cfg2 batch beside rollup= and quant=: without purity= and with it (no gate, and a gate), and
-- when --parent-lib names a build of the parent commit's library -- the same call without the key on that library, every
variant in a fresh child process, the variants alternating ROUNDS times; per variant the median over the rounds of the median
call time, and the spread (min..max over the rounds).  Without the key the rate must be the parent's, within that spread.

Needs a GPU: there is no fallback.

    python scripts/purity_probe.py [--parent-lib PATH] > profiles/purity/probe.txt"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

PEAKS = (2000, 20000)
HOST_QUERIES = 200
N_CH = 18
STEP = 1.0033548378


def survey(n_scans, n_peaks, seed=1):
    """ascending scans of n_peaks +- 5 % peaks between 350 and 1650 m/z"""
    rng = np.random.default_rng(seed + n_peaks)
    lens = rng.integers(int(n_peaks * 0.95), int(n_peaks * 1.05) + 1, size=n_scans)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    mz = rng.uniform(350.0, 1650.0, size=int(off[-1]))
    for a, b in zip(off[:-1], off[1:]):
        mz[a:b].sort()
    return mz, (rng.random(int(off[-1])) * 1e6 + 1.0).astype(np.float32), off


def queries(mz, off, n_query, seed=2):
    """query q over scan q * n_scans // n_query: the precursor is a peak of the scan, charge 2 or 3, the window +- 0.8"""
    rng = np.random.default_rng(seed)
    n_scans = off.size - 1
    sv = (np.arange(n_query, dtype=np.int64) * n_scans) // n_query
    at = off[sv] + (rng.random(n_query) * (off[sv + 1] - off[sv])).astype(np.int64)
    pm = mz[at].copy()
    return sv, pm, rng.integers(2, 4, size=n_query).astype(np.int32), pm - 0.8, pm + 0.8


def q(v):
    return "%8.4f (%.4f..%.4f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))


def kernels(a):
    import torch
    from oracle import harness
    from pyascore_amd import PyAscore, device, rollup as ru, synth
    scorer = harness.make_scorer(PyAscore, synth.describe("cfg2", 1, seed=1)["settings"])
    dev = torch.device("cuda", scorer.device)
    params = ru.purity_params()
    marks = ru.marker_params(mz=(500.0, 800.0, 1100.0), tol=0.01)
    print("# purity_probe: %s; %d queries over %d survey scans; %d timed rounds after %d; ms: median (p10..p90)" % (
        torch.cuda.get_device_properties(0).gcnArchName, a.queries, a.surveys, a.runs, a.warm))
    print("# copy = d2d copy of the survey m/z and intensities; purity = one pya_purity_spectra; gate = one pya_purity_gate over %d channels, "
          "in place, with select; markers = one pya_marker_spectra with 3 targets on the survey scans; replaced = D2H of the survey arrays + "
          "rollup.purity (timed on %d queries, scaled by queries / %d)" % (N_CH, HOST_QUERIES, HOST_QUERIES))
    for n_peaks in PEAKS:
        mz, it, off = survey(a.surveys, n_peaks)
        qs = queries(mz, off, a.queries)
        d_mz, d_it, d_off = torch.from_numpy(mz).to(dev), torch.from_numpy(it).to(dev), torch.from_numpy(off).to(dev)
        d_q = [torch.from_numpy(x).to(dev) for x in qs]
        c_mz, c_it = torch.empty_like(d_mz), torch.empty_like(d_it)
        d_rec = torch.empty((a.queries, 48), dtype=torch.uint8, device=dev)
        d_values = torch.rand((a.queries, N_CH), dtype=torch.float64, device=dev)
        d_select = torch.empty(a.queries, dtype=torch.uint8, device=dev)
        d_marks = (torch.empty((a.surveys, 3, 24), dtype=torch.uint8, device=dev), torch.empty((a.surveys, 32), dtype=torch.uint8, device=dev))
        t = {k: [] for k in ("copy", "purity", "gate", "markers")}
        for i in range(a.warm + a.runs):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            ev[0].record()
            c_mz.copy_(d_mz)
            c_it.copy_(d_it)
            ev[1].record()
            device.purity(scorer, d_mz, d_it, d_off, *d_q, params, out=d_rec)
            ev[2].record()
            device.purity_gate(scorer, d_rec, 0.7, True, d_values, out=d_values, select=d_select)
            ev[3].record()
            device.markers(scorer, d_mz, d_it, d_off, marks, out=d_marks)
            ev[4].record()
            torch.cuda.synchronize(dev)
            if i >= a.warm:
                for k, name in enumerate(("copy", "purity", "gate", "markers")):
                    t[name].append(ev[k].elapsed_time(ev[k + 1]))
        t0 = time.perf_counter()
        h_mz, h_it = d_mz.cpu().numpy(), d_it.cpu().numpy()
        t1 = time.perf_counter()
        part = tuple(x[:HOST_QUERIES] for x in qs)
        want, _ = ru.purity(h_mz, h_it, off, *part, params)
        t2 = time.perf_counter()
        got = device.purity_records(d_rec.cpu().numpy())
        assert got[:HOST_QUERIES].tobytes() == want.tobytes(), "%d peaks: the device and the numpy restatement differ" % n_peaks
        seen = float((got["flags"] == 3).mean())
        scaled = (t2 - t1) * 1e3 * a.queries / HOST_QUERIES
        survey_bytes = mz.nbytes + it.nbytes
        read_bytes = float((off[qs[0] + 1] - off[qs[0]]).sum()) * 8.0                # the m/z the purity launch asks for
        print("purity %6d peaks per scan  survey %7.1f MB, m/z asked for by the queries %8.1f MB (%.0f x the survey m/z)  copy ms %s  "
              "purity ms %s  gate ms %s  markers ms %s  |  purity/copy %6.2f  purity/markers %6.2f  purity GB/s of m/z asked for %7.1f  |  "
              "precursor seen in %.0f %%  |  replaced: D2H %7.1f ms + restatement %9.1f ms (scaled) = %9.1f ms, %.0f x the launch" % (
                  n_peaks, survey_bytes / 1e6, read_bytes / 1e6, read_bytes / mz.nbytes, q(t["copy"]), q(t["purity"]), q(t["gate"]), q(t["markers"]),
                  np.median(t["purity"]) / np.median(t["copy"]), np.median(t["purity"]) / np.median(t["markers"]),
                  read_bytes / 1e6 / np.median(t["purity"]), 100.0 * seen, (t1 - t0) * 1e3, scaled, (t1 - t0) * 1e3 + scaled,
                  ((t1 - t0) * 1e3 + scaled) / np.median(t["purity"])), flush=True)


def score_child(a):
    """one variant in this process: the median wall time of score_batch over a.steps calls after a.warm"""
    from oracle import harness
    from pyascore_amd import PyAscore, synth
    desc = synth.describe("cfg2", n_psm=a.psms, seed=1000)
    batch, settings = synth.make_slice(desc), desc["settings"]
    scorer = harness.make_scorer(PyAscore, settings)
    off = scorer.site_offsets(batch, False)
    n = int(batch["n_psm"])
    slot = (np.arange(int(off[-1])) % max(1, n // 5)).astype(np.int32)
    roll = dict(slot=slot, n_slots=max(1, n // 5))
    rng = np.random.default_rng(5)
    extra = dict(rollup=roll, quant=dict(values=rng.random((n, N_CH)) * 1e5 + 1.0, threshold=0.5, scale_log2=10))
    if a.score_child != "plain":
        mz, it, ms1_off = survey(max(1, n // 20), 2000)
        sv, pm, pz, wl, wh = queries(mz, ms1_off, n)
        extra["purity"] = dict(ms1_mz=mz, ms1_intensity=it, ms1_peak_off=ms1_off, survey=sv, precursor_mz=pm, precursor_charge=pz, window_lo=wl,
                               window_hi=wh)
        if a.score_child == "gate":
            extra["purity"]["gate"] = dict(threshold=0.7)
    times = []
    for i in range(a.warm + a.steps):
        t0 = time.perf_counter()
        scorer.score_batch(batch, **extra)
        if i >= a.warm:
            times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(median_ms=float(np.median(times)), psms=n)))


def score(a):
    variants = [("new library, quant= without purity=", "plain", None), ("new library, with purity=", "purity", None),
                ("new library, with purity= and a gate", "gate", None)]
    if a.parent_lib:
        variants.append(("parent library, quant=", "plain", a.parent_lib))
    got = {name: [] for name, _, _ in variants}
    for _ in range(a.rounds):
        for name, mode, lib in variants:
            env = dict(os.environ)
            if lib:
                env.update(PYA_LIB=os.path.abspath(lib), PYA_LIB_OLD="1")
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--score-child", mode, "--psms", str(a.psms), "--steps", str(a.steps),
                                  "--warm", str(a.warm)], env=env, check=True, capture_output=True, text=True, timeout=300).stdout
            got[name].append(json.loads(out.strip().splitlines()[-1])["median_ms"])
    print("# score_batch(rollup=, quant=) on cfg2, %d PSMs, %d channels, with purity= %d survey scans of about 2 000 peaks: per variant a fresh "
          "process per round, %d rounds alternating, in each the median wall ms of %d calls after %d; below: median over the rounds (min..max "
          "over the rounds = the spread)" % (a.psms, N_CH, max(1, a.psms // 20), a.rounds, a.steps, a.warm))
    for name, v in got.items():
        print("score_batch %-40s %9.2f ms (%.2f..%.2f)  %9.0f PSM/s" % (name, np.median(v), min(v), max(v), a.psms / np.median(v) * 1e3), flush=True)
    if not a.parent_lib:
        print("score_batch parent library: not measured (no --parent-lib)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--surveys", type=int, default=5000)
    ap.add_argument("--psms", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--score-child", default="")
    ap.add_argument("--skip-score", action="store_true")
    a = ap.parse_args()
    if a.score_child:
        return score_child(a)
    kernels(a)
    if not a.skip_score:
        score(a)


if __name__ == "__main__":
    main()
