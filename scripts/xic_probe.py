"""The precursor-XIC stage, measured beside a copy of the survey bytes, beside the purity stage on the same survey, beside its
own survey check and beside the host way it replaces.

Part 1, QUERIES queries over SURVEYS survey scans of about 2 000 peaks and again of about 20 000 peaks (float64 m/z, float32
intensities).  TRACES m/z values are in every scan, jittered by 2 ppm, with intensities that rise and fall with a period of 40
scans (maximum three times the minimum: rise 2 finds valleys); the queries name them in turn, query q seeded at scan
q * SURVEYS // QUERIES (scan order: consecutive queries share most of their window), with windows of 21 and of 64 scans.  HIP
events on one stream, RUNS rounds after WARM warm-up rounds, every output allocated before; median and p10..p90: (a) a
device-to-device copy of the survey m/z and intensities, (b) pya_purity_spectra on the same survey (one scan per query), (c)
pya_xic_survey_check, (d) pya_xic_spectra with windows of 21 scans, (e) with windows of 64 scans; then (f) the path the stage
replaces: the survey arrays to the host (D2H) + pyascore_amd.rollup.xic, timed on the first HOST_QUERIES queries of the 64-scan
windows and scaled by the query count -- the scaling is stated on the line.  The device records are compared bytewise with the
restatement on those queries before anything is reported.

Part 2, PyAscore.score_batch on a cfg2 batch beside rollup= and quant=: without xic=, with it, with it as the quant column
(values="xic_area"), and -- when --parent-lib names a build of the parent commit's library -- the call without the key on that
library, every variant in a fresh child process, the variants alternating ROUNDS times; per variant the median over the rounds
of the median call time, and the spread (min..max over the rounds).  Without the key the rate must be the parent's, within that
spread.

Not built, so not measured: a scattered query order, and a "wavefront per survey scan, lane = query" shape.

Needs a GPU: there is no fallback.

    python scripts/xic_probe.py [--parent-lib PATH] > profiles/xic/probe.txt"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

PEAKS = (2000, 20000)
WINDOWS = (21, 64)
HOST_QUERIES = 200
TRACES = 200
N_CH = 18


def survey(n_scans, n_peaks, seed=1):
    """ascending scans of n_peaks +- 5 % peaks between 350 and 1650 m/z, TRACES of them the persistent m/z values; returns
    (mz, intensity, peak_off, rt, trace m/z)"""
    rng = np.random.default_rng(seed + n_peaks)
    lens = rng.integers(int(n_peaks * 0.95), int(n_peaks * 1.05) + 1, size=n_scans)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    mz = rng.uniform(350.0, 1650.0, size=int(off[-1]))
    it = rng.random(int(off[-1])) * 1e4 + 1.0
    traces = 400.0 + 6.0 * np.arange(TRACES) + 0.123
    phase = 13 * np.arange(TRACES)
    for s, (a, b) in enumerate(zip(off[:-1], off[1:])):
        mz[a:a + TRACES] = traces * (1.0 + rng.uniform(-2e-6, 2e-6, TRACES))
        it[a:a + TRACES] = np.floor(1e5 * (2.0 + np.cos(2.0 * np.pi * (s + phase) / 40.0)))
        order = np.argsort(mz[a:b], kind="stable")
        mz[a:b], it[a:b] = mz[a:b][order], it[a:b][order]
    return mz, it.astype(np.float32), off, np.cumsum(rng.uniform(0.4, 0.6, n_scans)), traces


def queries(traces, n_scans, n_query, width):
    """query q: trace q mod TRACES at charge 2, seeded at scan q * n_scans // n_query, the window of ``width`` scans around it
    clipped to the survey"""
    seed = (np.arange(n_query, dtype=np.int64) * n_scans) // n_query
    lo = np.clip(seed - width // 2, 0, None)
    hi = np.minimum(lo + width, n_scans)
    lo = np.maximum(hi - width, 0)
    return seed, lo, hi, traces[np.arange(n_query) % TRACES].copy(), np.full(n_query, 2, np.int32)


def q(v):
    return "%8.4f (%.4f..%.4f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))


def kernels(a):
    import torch
    from oracle import harness
    from pyascore_amd import PyAscore, device, rollup as ru, synth
    scorer = harness.make_scorer(PyAscore, synth.describe("cfg2", 1, seed=1)["settings"])
    dev = torch.device("cuda", scorer.device)
    params, p_params = ru.xic_params(), ru.purity_params()
    print("# xic_probe: %s; %d queries over %d survey scans; %d timed rounds after %d; ms: median (p10..p90)" % (
        torch.cuda.get_device_properties(0).gcnArchName, a.queries, a.surveys, a.runs, a.warm))
    print("# copy = d2d copy of the survey m/z and intensities; purity = one pya_purity_spectra on the same survey; check = one "
          "pya_xic_survey_check; xic21 / xic64 = one pya_xic_spectra with windows of 21 / 64 scans (default parameters: 10 ppm, 2 isotopes, "
          "rise 2, max_gap 1); replaced = D2H of the survey arrays + rollup.xic with the 64-scan windows (timed on %d queries, scaled by "
          "queries / %d)" % (HOST_QUERIES, HOST_QUERIES))
    for n_peaks in PEAKS:
        mz, it, off, rt, traces = survey(a.surveys, n_peaks)
        qs = {w: queries(traces, a.surveys, a.queries, w) for w in WINDOWS}
        d_mz, d_it, d_off, d_rt = (torch.from_numpy(x).to(dev) for x in (mz, it, off, rt))
        d_q = {w: [torch.from_numpy(x).to(dev) for x in qs[w]] for w in WINDOWS}
        sd, _, _, pm, pz = qs[WINDOWS[0]]
        d_pq = [torch.from_numpy(x).to(dev) for x in (sd, pm, pz, pm - 0.8, pm + 0.8)]
        c_mz, c_it = torch.empty_like(d_mz), torch.empty_like(d_it)
        d_ok = torch.empty(a.surveys, dtype=torch.uint8, device=dev)
        d_rec = {w: torch.empty((a.queries, 64), dtype=torch.uint8, device=dev) for w in WINDOWS}
        d_pur = torch.empty((a.queries, 48), dtype=torch.uint8, device=dev)
        names = ("copy", "purity", "check", "xic21", "xic64")
        t = {k: [] for k in names}
        for i in range(a.warm + a.runs):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            ev[0].record()
            c_mz.copy_(d_mz)
            c_it.copy_(d_it)
            ev[1].record()
            device.purity(scorer, d_mz, d_it, d_off, *d_pq, p_params, out=d_pur)
            ev[2].record()
            device.xic_survey_check(scorer, d_mz, d_it, d_off, out=d_ok)
            ev[3].record()
            device.xic(scorer, d_mz, d_it, d_off, d_rt, d_ok, *d_q[21], params, out=d_rec[21])
            ev[4].record()
            device.xic(scorer, d_mz, d_it, d_off, d_rt, d_ok, *d_q[64], params, out=d_rec[64])
            ev[5].record()
            torch.cuda.synchronize(dev)
            if i >= a.warm:
                for k, name in enumerate(names):
                    t[name].append(ev[k].elapsed_time(ev[k + 1]))
        t0 = time.perf_counter()
        h_mz, h_it = d_mz.cpu().numpy(), d_it.cpu().numpy()
        t1 = time.perf_counter()
        part = tuple(x[:HOST_QUERIES] for x in qs[64])
        want, _ = ru.xic(h_mz, h_it, off, rt, *part, params)
        t2 = time.perf_counter()
        got = {w: device.xic_records(d_rec[w].cpu().numpy()) for w in WINDOWS}
        assert got[64][:HOST_QUERIES].tobytes() == want.tobytes(), "%d peaks: the device and the numpy restatement differ" % n_peaks
        assert d_ok.cpu().numpy().all()
        seen = float(((got[64]["flags"] & ru.XIC_SEEN) != 0).mean())
        valley = float(((got[64]["flags"] & (ru.XIC_LEFT_VALLEY | ru.XIC_RIGHT_VALLEY)) != 0).mean())
        scaled = (t2 - t1) * 1e3 * a.queries / HOST_QUERIES
        m = {k: float(np.median(v)) for k, v in t.items()}
        print("xic %6d peaks per scan  survey %7.1f MB  copy ms %s  purity ms %s  check ms %s  xic21 ms %s  xic64 ms %s  |  xic21/copy %6.2f  "
              "xic64/copy %6.2f  xic21/purity %6.2f  xic64/purity %6.2f  xic64/xic21 %5.2f  check/copy %5.2f  |  queries/s at 64 scans %.3g  |  "
              "peak found in %.0f %%, split at a valley in %.0f %% (64 scans)  |  replaced: D2H %7.1f ms + restatement %9.1f ms (scaled) = "
              "%9.1f ms, %.0f x the launch" % (
                  n_peaks, (mz.nbytes + it.nbytes) / 1e6, q(t["copy"]), q(t["purity"]), q(t["check"]), q(t["xic21"]), q(t["xic64"]),
                  m["xic21"] / m["copy"], m["xic64"] / m["copy"], m["xic21"] / m["purity"], m["xic64"] / m["purity"], m["xic64"] / m["xic21"],
                  m["check"] / m["copy"], a.queries / m["xic64"] * 1e3, 100.0 * seen, 100.0 * valley, (t1 - t0) * 1e3, scaled,
                  (t1 - t0) * 1e3 + scaled, ((t1 - t0) * 1e3 + scaled) / m["xic64"]), flush=True)
        del d_mz, d_it, c_mz, c_it


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
        n_scans = max(64, n // 20)
        mz, it, ms1_off, rt, traces = survey(n_scans, 2000)
        sd, lo, hi, pm, pz = queries(traces, n_scans, n, 21)
        extra["xic"] = dict(ms1_mz=mz, ms1_intensity=it, ms1_peak_off=ms1_off, rt=rt, seed=sd, scan_lo=lo, scan_hi=hi, precursor_mz=pm,
                            precursor_charge=pz)
        if a.score_child == "column":
            extra["quant"] = dict(values="xic_area", threshold=0.5, scale_log2=10)
    times = []
    for i in range(a.warm + a.steps):
        t0 = time.perf_counter()
        scorer.score_batch(batch, **extra)
        if i >= a.warm:
            times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(median_ms=float(np.median(times)), psms=n)))


def score(a):
    variants = [("new library, quant= without xic=", "plain", None), ("new library, with xic=", "xic", None),
                ("new library, with xic= as the quant column", "column", None)]
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
    print("# score_batch(rollup=, quant=) on cfg2, %d PSMs, %d channels (1 with the XIC column), with xic= %d survey scans of about 2 000 peaks "
          "and windows of 21 scans: per variant a fresh process per round, %d rounds alternating, in each the median wall ms of %d calls after "
          "%d; below: median over the rounds (min..max over the rounds = the spread)" % (
              a.psms, N_CH, max(64, a.psms // 20), a.rounds, a.steps, a.warm))
    for name, v in got.items():
        print("score_batch %-44s %9.2f ms (%.2f..%.2f)  %9.0f PSM/s" % (name, np.median(v), min(v), max(v), a.psms / np.median(v) * 1e3), flush=True)
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
    ap.add_argument("--skip-kernels", action="store_true")
    a = ap.parse_args()
    if a.score_child:
        return score_child(a)
    if not a.skip_kernels:
        kernels(a)
    if not a.skip_score:
        score(a)


if __name__ == "__main__":
    main()
