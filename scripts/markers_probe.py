"""The marker-ion stage, measured.  One process on one GPU (and one child for --parent-lib):

  (a) pya_marker_spectra (one launch) over the spectra of 100 000 cfg2 PSMs and of bench.py's dense batch (32 768 spectra of
      about 1 570 peaks), float64 / float64, with a precursor at charge 2 or 3 inside every spectrum's own m/z range and three
      target sets: 3 (the pY immonium ion, precursor - H3PO4, precursor - HPO3), 18 (sixteen reporter-like m/z and the two
      losses) and 64 (sixty-two fixed m/z and the two losses).  HIP events around one call on torch's stream, RUNS rounds after
      WARM warm-up rounds, median and p10..p90.  Beside it, in the same rounds: a device-to-device copy of the same m/z and
      intensity bytes (the stage reads every peak once and writes next to nothing: half of a copy's traffic) and
      pya_strip_spectra under its 3-window rule (the sibling with the same launch shape, which also writes the kept peaks).
      The route the stage replaces is timed too: the D2H copy of the spectra (wall clock, once) and pyascore_amd.rollup.markers
      on the first --restate spectra, SCALED to the batch.  The device records of those spectra and the restatement's are
      compared on bytes before anything is reported.
  (b) PyAscore.score_batch on cfg2 and on the dense batch's first PSMs without and with markers= (18 targets), alternating,
      host to host; with --parent-lib also the plain rate on another build of the library (the parent commit's), in a child
      process.

Needs a GPU: there is no fallback.

    python scripts/markers_probe.py [--runs 30] [--calls 6] [--parent-lib PATH] > profiles/markers/probe.txt"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

H3PO4, HPO3, H2O = 97.976896, 79.966331, 18.010565
LOSSES = (H3PO4, HPO3)
TARGETS = {3: dict(mz=(216.0426,), losses=LOSSES, tol=0.02),
           18: dict(mz=tuple(126.1277 + 0.5016 * k for k in range(16)), losses=LOSSES, tol=0.003, tol_ppm=10.0),
           64: dict(mz=tuple(101.07 + 2.0157 * k for k in range(62)), losses=LOSSES, tol=0.003, tol_ppm=10.0)}
STRIP_RULE = dict(tol=0.05, losses=(H3PO4, H2O), isotopes=1)


def pct(v):
    return "%9.4f (%.4f..%.4f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))


def precursors(batch, seed=1000):
    rng = np.random.default_rng(seed)
    off = np.asarray(batch["peak_off"], np.int64)
    mz = np.asarray(batch["mz"], np.float64)
    first, last = mz[off[:-1]], mz[off[1:] - 1]                  # (the spectra are ascending and none is empty)
    return rng.uniform(first + 0.3 * (last - first), first + 0.7 * (last - first)), rng.integers(2, 4, off.size - 1).astype(np.int32)


def make_batches(n, dense):
    from pyascore_amd import synth
    desc = synth.describe("cfg2", n_psm=n, seed=1000)
    yield "cfg2", desc["settings"], lambda hi=None: synth.make_slice(desc, 0, hi), n
    d = min(dense, 8192)
    dense_desc = synth.describe("cfg2", n_psm=dense, seed=1000, n_noise=1500, isotopes=True)
    yield "dense1570", desc["settings"], lambda hi=None: synth.make_slice(dense_desc, 0, hi), d


def kernel_rows(scorer, name, batch, warm, runs, restate):
    import torch
    from pyascore_amd import device, rollup
    dev = torch.device("cuda", scorer.device)
    off = np.ascontiguousarray(batch["peak_off"], np.int64)
    mz, it = np.ascontiguousarray(batch["mz"], np.float64), np.ascontiguousarray(batch["intensity"], np.float64)
    pm, pz = precursors(batch)
    d_mz, d_it, d_off = torch.from_numpy(mz).to(dev), torch.from_numpy(it).to(dev), torch.from_numpy(off).to(dev)
    d_pm, d_pz = torch.from_numpy(pm).to(dev), torch.from_numpy(pz).to(dev)
    out = (torch.empty_like(d_mz), torch.empty_like(d_it))
    nbytes = mz.nbytes + it.nbytes
    strip_p = rollup.strip_params(**STRIP_RULE)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    h_mz, h_it = d_mz.cpu(), d_it.cpu()
    d2h_ms = (time.perf_counter() - t0) * 1e3
    del h_mz, h_it
    m = min(restate, off.size - 1)
    for n_t, rule in TARGETS.items():
        p = rollup.marker_params(**rule)
        d_rec, d_spec, d_over = device.markers(scorer, d_mz, d_it, d_off, p, d_pm, d_pz)
        rec, spec = device.marker_records(d_rec.cpu().numpy()), device.marker_spectrum_records(d_spec.cpu().numpy())
        t0 = time.perf_counter()
        want = rollup.markers(mz, it, off[:m + 1], p, pm[:m], pz[:m])
        restate_ms = (time.perf_counter() - t0) * 1e3 * (off.size - 1) / m
        assert rec[:m].tobytes() == want[0].tobytes() and spec[:m].tobytes() == want[1].tobytes() and d_over.cpu().numpy().tolist() == [0, 0], \
            "%s %d targets: the kernel and the restatement differ" % (name, n_t)
        rec_out = (d_rec, d_spec)
        t = {k: [] for k in ("markers", "copy", "strip")}
        for i in range(warm + runs):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            ev[0].record()
            device.markers(scorer, d_mz, d_it, d_off, p, d_pm, d_pz, out=rec_out)
            ev[1].record()
            ev[2].record()
            out[0].copy_(d_mz)                                   # (hipMemcpyAsync device to device on the same stream)
            out[1].copy_(d_it)
            ev[3].record()
            ev[4].record()
            device.strip(scorer, d_mz, d_it, d_off, d_pm, d_pz, strip_p, out=out)
            ev[5].record()
            torch.cuda.synchronize(dev)
            if i >= warm:
                for k, key in enumerate(("markers", "copy", "strip")):
                    t[key].append(ev[2 * k].elapsed_time(ev[2 * k + 1]))
        k, c, s = (np.array(t[x]) for x in ("markers", "copy", "strip"))
        print("markers %-10s %2d targets f64/f64 %7d spectra %9d peaks %7.1f MB, active %5.2f, picked per spectrum %5.2f  kernel ms %s = %6.0f GB/s "
              "read  d2d copy ms %s  kernel/copy %5.2f  pya_strip_spectra (3 windows) ms %s  markers/strip %5.2f  |  D2H %8.1f ms + "
              "rollup.markers %10.0f ms (scaled from %d spectra)"
              % (name, n_t, off.size - 1, mz.size, nbytes / 2**20, float(spec["n_active"].mean()),
                 float(((rec["flags"] & rollup.MARKER_PICKED) != 0).sum(axis=1).mean()), pct(k), nbytes / 1e9 / (np.median(k) * 1e-3), pct(c),
                 np.median(k) / np.median(c), pct(s), np.median(k) / np.median(s), d2h_ms, restate_ms, m), flush=True)
    return pm, pz


def plain_rates(n, dense, calls):
    """M PSMs/s of plain score_batch calls on both batches (the child of --parent-lib runs only this)"""
    from oracle import harness
    from pyascore_amd import PyAscore
    rates = {}
    for name, settings, make, n_scored in make_batches(n, dense):
        batch = make(n_scored)                               # (the PSMs the parent process scores: a slice is its first PSMs)
        scorer = harness.make_scorer(PyAscore, settings)
        scorer.score_batch(batch)
        rates[name] = []
        for _ in range(calls):
            t0 = time.perf_counter()
            scorer.score_batch(batch)
            rates[name].append(batch["n_psm"] / (time.perf_counter() - t0) / 1e6)
    return rates


def batch_rows(scorer, name, batch, pm, pz, calls, parent):
    from pyascore_amd import rollup
    req = dict(TARGETS[18], precursor_mz=pm, precursor_charge=pz)
    want = scorer.score_batch(batch)
    got = scorer.score_batch(batch, markers=req)
    for key in ("best_score", "best_sig", "n_sig", "ascores", "alt_mask"):
        assert got[key].tobytes() == want[key].tobytes(), "score_batch(markers=) changes " + key
    m = min(200, int(batch["n_psm"]))
    rec, spec = rollup.markers(batch["mz"], batch["intensity"], batch["peak_off"][:m + 1], rollup.marker_params(**TARGETS[18]), pm[:m], pz[:m])
    assert got["markers"][:m].tobytes() == rec.tobytes() and got["marker_spectra"][:m].tobytes() == spec.tobytes()
    rates = {"plain": [], "markers": []}
    for _ in range(calls):
        for label, kw in (("plain", {}), ("markers", dict(markers=req))):
            t0 = time.perf_counter()
            scorer.score_batch(batch, **kw)
            rates[label].append(batch["n_psm"] / (time.perf_counter() - t0) / 1e6)
    q = lambda v: "%6.3f (%.3f..%.3f)" % (np.median(v), np.min(v), np.max(v))  # noqa: E731
    print("score_batch %-10s %6d PSMs, M PSMs/s median (min..max) of %d calls after 1: plain %s; with markers= (18 targets) %s; plain on the "
          "parent commit's library %s" % (name, batch["n_psm"], calls, q(rates["plain"]), q(rates["markers"]),
                                          q(parent[name]) if parent is not None else "-"), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--dense", type=int, default=32768)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--restate", type=int, default=200, help="spectra the Python restatement is timed on")
    ap.add_argument("--parent-lib", type=str, default="", help="another build of the library: its plain score_batch rate, in a child process")
    ap.add_argument("--plain-only", action="store_true", help="print the plain score_batch rates as JSON and stop (the child of --parent-lib)")
    a = ap.parse_args()
    if a.plain_only:
        print(json.dumps(plain_rates(a.n, a.dense, a.calls)))
        return
    parent = None
    if a.parent_lib:                                        # (a fresh child process, before this one opens the GPU)
        env = dict(os.environ, PYA_LIB=os.path.abspath(a.parent_lib), PYA_LIB_OLD="1")
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--calls", str(a.calls), "--n", str(a.n), "--dense",
                               str(a.dense)], env=env, capture_output=True, text=True, timeout=600)
        if done.returncode != 0:
            raise SystemExit("the child with --parent-lib failed (%d):\n%s" % (done.returncode, done.stderr[-2000:]))
        parent = json.loads(done.stdout.strip().splitlines()[-1])
    import torch
    from oracle import harness
    from pyascore_amd import PyAscore, synth
    print("# markers_probe: seed 1000; %s; %d timed rounds after %d; targets %s; strip rule %s"
          % (torch.cuda.get_device_properties(0).gcnArchName, a.runs, a.warm, {k: (len(v["mz"]), len(v["losses"])) for k, v in TARGETS.items()},
             STRIP_RULE))
    print("# ms: median (p10..p90); kernel = HIP events around one pya_marker_spectra (one launch); GB/s = m/z and intensity bytes read over the "
          "kernel's median; d2d copy = events around device-to-device copies of the same bytes; pya_strip_spectra: the same input, three "
          "passes; D2H = the spectra copied back once, wall clock; rollup.markers = the numpy restatement timed once on the first spectra "
          "and SCALED to the batch")
    for name, settings, make, n_scored in make_batches(a.n, a.dense):
        batch = make()
        print("%s generated" % name, file=sys.stderr, flush=True)
        scorer = harness.make_scorer(PyAscore, settings)
        pm, pz = kernel_rows(scorer, name, batch, a.warm, a.runs, a.restate)
        batch_rows(scorer, name, synth.slice_batch(batch, 0, n_scored), pm[:n_scored], pz[:n_scored], a.calls, parent)
        del batch


if __name__ == "__main__":
    main()
