"""The channel correction, measured beside a copy of the same bytes and beside the host way it replaces.

Part 1, on a device matrix of 100 000 rows x 3, 18 and 64 channels (HIP events on one stream, RUNS rounds after WARM warm-up
rounds, every output allocated before; median and p10..p90): (a) a device-to-device copy of the matrix, (b) pya_channel_correct
with the matrix, (c) with the factor alone, in place, (d) pya_channel_sums + pya_channel_factors; then (e) the whole host form
PyAscore.correct_channels (matrix and normalisation; wall clock around the call, which ends in a synchronise) and (f) the path it
replaces: the matrix to the host (D2H), pyascore_amd.rollup.correct_channels / channel_sums / channel_factors / correct_channels,
and back (H2D) -- the restatement timed on the first HOST_ROWS rows and scaled by the row count, because its explicit loops over
the channels are slow; the scaling is stated on the line.  The device results are compared bytewise with the restatement on
those rows before anything is reported.

Part 2, PyAscore.score_batch on a cfg2 batch beside rollup= and quant=: without channels= and with them, and -- when --parent-lib
names a build of the parent commit's library -- the same call without the key on that library, every variant in a fresh child
process, the variants alternating ROUNDS times; per variant the median over the rounds of the median call time, and the spread
(min..max over the rounds).  Without the key the rate must be the parent's, within that spread.

Needs a GPU: there is no fallback.

    python scripts/channel_probe.py [--parent-lib PATH] > profiles/channel_correct/probe.txt"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

CHANNELS = (3, 18, 64)
SCALE = 10
HOST_ROWS = 2000


def matrix(n_rows, n_ch, seed=1000):
    rng = np.random.default_rng(seed + n_ch)
    v = rng.random((n_rows, n_ch)) * 1e5 + 1.0
    v[rng.random((n_rows, n_ch)) < 0.03] = np.nan
    return v


def lot(n_ch, seed=7):
    from pyascore_amd import rollup as ru
    rng = np.random.default_rng(seed)
    return ru.channel_matrix(ru.channel_spill(n_ch, [(c, t, float(rng.uniform(0.01, 0.08))) for c in range(n_ch) for t in (c - 1, c + 1)
                                                     if 0 <= t < n_ch]))


def q(v):
    return "%8.4f (%.4f..%.4f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))


def kernels(a):
    import torch
    from oracle import harness
    from pyascore_amd import PyAscore, device, rollup as ru, synth
    scorer = harness.make_scorer(PyAscore, synth.describe("cfg2", 1, seed=1)["settings"])
    dev = torch.device("cuda", scorer.device)
    print("# channel_probe: %s; %d rows; %d timed rounds after %d; ms: median (p10..p90)" % (
        torch.cuda.get_device_properties(0).gcnArchName, a.rows, a.runs, a.warm))
    print("# copy = d2d copy of the matrix; matrix / factor = one pya_channel_correct (the factor pass in place); sums = pya_channel_sums + "
          "pya_channel_factors; host form = PyAscore.correct_channels(matrix, normalize) on host arrays, wall clock; replaced = D2H + "
          "the rollup restatement (timed on %d rows, scaled by rows / %d) + H2D" % (HOST_ROWS, HOST_ROWS))
    for n_ch in CHANNELS:
        values, m = matrix(a.rows, n_ch), lot(n_ch)
        d_values, d_m = torch.from_numpy(values).to(dev), torch.from_numpy(m).to(dev)
        d_out, d_copy = torch.empty_like(d_values), torch.empty_like(d_values)
        d_cell = torch.zeros((n_ch, 16), dtype=torch.uint8, device=dev)
        d_factor = torch.empty(n_ch, dtype=torch.float64, device=dev)
        t = {k: [] for k in ("copy", "matrix", "sums", "factor")}
        for i in range(a.warm + a.runs):
            d_cell.zero_()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            ev[0].record()
            d_copy.copy_(d_values)
            ev[1].record()
            device.correct_channels(scorer, d_values, matrix=d_m, out=d_out)
            ev[2].record()
            device.channel_sums(scorer, d_out, None, SCALE, out=d_cell)
            device.channel_factors(scorer, d_cell, out=d_factor)
            ev[3].record()
            device.correct_channels(scorer, d_out, factor=d_factor, out=d_out)
            ev[4].record()
            torch.cuda.synchronize(dev)
            if i >= a.warm:
                for k, name in enumerate(("copy", "matrix", "sums", "factor")):
                    t[name].append(ev[k].elapsed_time(ev[k + 1]))
        host = []
        for i in range(3 + min(a.runs, 10)):
            t0 = time.perf_counter()
            h_out, h_cell, h_factor = scorer.correct_channels(values, m, True, None, SCALE)
            if i >= 3:
                host.append((time.perf_counter() - t0) * 1e3)
        assert h_out.tobytes() == d_out.cpu().numpy().tobytes() and h_factor.tobytes() == d_factor.cpu().numpy().tobytes()
        t0 = time.perf_counter()
        back = d_values.cpu().numpy()
        t1 = time.perf_counter()
        part = back[:HOST_ROWS]
        r_mid = ru.correct_channels(part, matrix=m)
        ru.channel_factors(ru.channel_sums(r_mid, None, SCALE))
        r_out = ru.correct_channels(r_mid, factor=h_factor)
        t2 = time.perf_counter()
        d_back = torch.from_numpy(h_out).to(dev)
        torch.cuda.synchronize(dev)
        t3 = time.perf_counter()
        assert r_out.tobytes() == h_out[:HOST_ROWS].tobytes(), "%d channels: the device and the numpy restatement differ" % n_ch
        del d_back
        scaled = (t2 - t1) * 1e3 * a.rows / HOST_ROWS
        nbytes = values.nbytes
        dev_ms = np.median(t["matrix"]) + np.median(t["sums"]) + np.median(t["factor"])
        print("channel_correct %2d channels  %6.1f MB  copy ms %s  matrix ms %s  sums ms %s  factor ms %s  |  matrix/copy %5.2f  factor/copy %5.2f  "
              "sums/copy %5.2f  |  host form ms %s  |  replaced: D2H %7.1f ms + restatement %9.1f ms (scaled) + H2D %7.1f ms = %9.1f ms, "
              "%.0f x the resident chain" % (
                  n_ch, nbytes / 1e6, q(t["copy"]), q(t["matrix"]), q(t["sums"]), q(t["factor"]),
                  np.median(t["matrix"]) / np.median(t["copy"]), np.median(t["factor"]) / np.median(t["copy"]),
                  np.median(t["sums"]) / np.median(t["copy"]), q(host), (t1 - t0) * 1e3, scaled, (t3 - t2) * 1e3,
                  (t1 - t0) * 1e3 + scaled + (t3 - t2) * 1e3, ((t1 - t0) * 1e3 + scaled + (t3 - t2) * 1e3) / dev_ms), flush=True)


def score_child(a):
    """one variant in this process: the median wall time of score_batch over a.steps calls after a.warm"""
    from oracle import harness
    from pyascore_amd import PyAscore, rollup as ru, synth
    desc = synth.describe("cfg2", n_psm=a.psms, seed=1000)
    batch, settings = synth.make_slice(desc), desc["settings"]
    scorer = harness.make_scorer(PyAscore, settings)
    off = scorer.site_offsets(batch, False)
    n = int(batch["n_psm"])
    slot = (np.arange(int(off[-1])) % max(1, n // 5)).astype(np.int32)
    roll = dict(slot=slot, n_slots=max(1, n // 5))
    req = dict(values=matrix(n, 18), threshold=0.5, scale_log2=SCALE)
    if a.score_child == "channels":
        req["channels"] = dict(matrix=lot(18), normalize=True)
    times = []
    for i in range(a.warm + a.steps):
        t0 = time.perf_counter()
        scorer.score_batch(batch, rollup=roll, quant=req)
        if i >= a.warm:
            times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(median_ms=float(np.median(times)), psms=n)))


def score(a):
    variants = [("new library, quant= without channels=", "plain", None), ("new library, quant= with channels=", "channels", None)]
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
    print("# score_batch(rollup=, quant=) on cfg2, %d PSMs, 18 channels: per variant a fresh process per round, %d rounds alternating, in each "
          "the median wall ms of %d calls after %d; below: median over the rounds (min..max over the rounds = the spread)" % (
              a.psms, a.rounds, a.steps, a.warm))
    for name, v in got.items():
        print("score_batch %-40s %9.2f ms (%.2f..%.2f)  %9.0f PSM/s" % (name, np.median(v), min(v), max(v), a.psms / np.median(v) * 1e3), flush=True)
    if not a.parent_lib:
        print("score_batch parent library: not measured (no --parent-lib)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--rows", type=int, default=100000)
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
