"""Centroiding, measured.  One process on one GPU:

  (a) pya_centroid_spectra (mark, scan, place) over the spectra of N cfg2 PSMs whose every peak is rendered as a Gaussian of
      sigma 0.008 on a 0.004 m/z grid (about 16 points a peak, 5 000 a spectrum), and over LONG spectra of about 20 000 points
      each (64 distinct ones rendered from cfg2 spectra with 1 200 noise peaks, repeated), float64 / float64, half_width 8 and
      a gap of 2.5 grid steps.  HIP events around one call on torch's stream, RUNS rounds after WARM warm-up rounds, median and
      p10..p90; MARK and PLACE alone through pya_debug_centroid_passes (PLACE reads the keep words and offsets the full call
      before it left).  Beside it, in the same rounds: a device-to-device copy of the same m/z and intensity bytes (the floor
      of anything that reads every point once) and pya_deisotope_spectra on the same input (the neighbour with the same
      passes: on profile samples its rule finds nothing, it is a cost figure only).  For the first HOST spectra, once, the
      path the kernels replace on resident arrays: D2H, pyascore_amd.rollup.centroid, H2D (wall clock around work that ends in
      a synchronise).  The bytes of the kernels and of the restatement are compared on those spectra first.
  (b) the resident step (DevicePlan.run) for the same PSMs on the profile spectra as they are and on the centroided ones.

Needs a GPU: there is no fallback.

    python scripts/centroid_probe.py [--n 100000] [--long 8192] [--runs 30] > profiles/centroid/probe.txt"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import harness  # noqa: E402
from pyascore_amd import PyAscore, _lib, device, rollup, synth  # noqa: E402

SIGMA, STEP = 0.008, 0.004
RULE = rollup.centroid_params(2.5 * STEP, half_width=8)
DEISO = rollup.deisotope_params()


def pct(v):
    return "%9.4f (%.4f..%.4f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))


def render(mz, it, off, chunk=2000):
    """every peak as Gaussian samples on the grid k STEP within 4 sigma, the samples of overlapping peaks added; ``chunk``
    spectra at a time"""
    xs, ys, counts = [], [], []
    for a in range(0, off.size - 1, chunk):
        o = off[a:a + chunk + 1]
        c, h = mz[o[0]:o[-1]], it[o[0]:o[-1]]
        spec = np.repeat(np.arange(o.size - 1), np.diff(o))
        k0 = np.ceil((c - 4.0 * SIGMA) / STEP).astype(np.int64)
        cnt = np.floor((c + 4.0 * SIGMA) / STEP).astype(np.int64) - k0 + 1
        peak = np.repeat(np.arange(c.size), cnt)
        k = np.repeat(k0, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        w = h[peak] * np.exp(-((k * STEP - c[peak]) ** 2) / (2.0 * SIGMA * SIGMA))
        cells, inverse = np.unique(spec[peak] * (1 << 32) + k, return_inverse=True)
        xs.append((cells & 0xFFFFFFFF) * STEP)
        ys.append(np.bincount(inverse, weights=w, minlength=cells.size))
        counts.append(np.bincount(cells >> 32, minlength=o.size - 1))
    return np.concatenate(xs), np.concatenate(ys), np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.int64)


def timed(dev, warm, runs, jobs):
    """median-ready arrays of milliseconds, one per job, the jobs of a round one after another on the stream"""
    t = [[] for _ in jobs]
    for i in range(warm + runs):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in jobs]
        for (a, b), job in zip(ev, jobs):
            a.record()
            job()
            b.record()
        torch.cuda.synchronize(dev)
        if i >= warm:
            for k, (a, b) in enumerate(ev):
                t[k].append(a.elapsed_time(b))
    return [np.array(v) for v in t]


def kernel_rows(scorer, name, mz, it, off, warm, runs, host_spectra):
    dev = torch.device("cuda", scorer.device)
    lib = scorer._lib
    n_host = min(host_spectra, off.size - 1)
    cut = int(off[n_host])
    want = rollup.centroid(mz[:cut], it[:cut], off[:n_host + 1], RULE)
    d_mz, d_it, d_off = torch.from_numpy(mz).to(dev), torch.from_numpy(it).to(dev), torch.from_numpy(off).to(dev)
    out = (torch.empty_like(d_mz), torch.empty_like(d_it))
    # the C call with buffers that live through every round: PLACE alone reads the keep words and the offsets of the call before
    work_bytes = int(lib.pya_centroid_workspace_bytes(off.size - 1, mz.size))
    work = torch.empty(work_bytes // 8, dtype=torch.int64, device=dev)
    d_new = torch.empty(off.size, dtype=torch.int64, device=dev)
    d_over = torch.zeros(2, dtype=torch.int32, device=dev)
    t_in = _lib.TypedSpectra(d_mz.data_ptr(), d_it.data_ptr(), _lib.PYA_F64, _lib.PYA_F64)
    t_out = _lib.TypedSpectra(out[0].data_ptr(), out[1].data_ptr(), _lib.PYA_F64, _lib.PYA_F64)
    c_rule = rollup.centroid_c_params(RULE)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def passes(which):
        def job():
            lib.pya_debug_centroid_passes(which)
            rc = lib.pya_centroid_spectra(scorer._h, C.byref(t_in), d_off.data_ptr(), off.size - 1, None, C.byref(c_rule), stream, work.data_ptr(),
                                          work_bytes, C.byref(t_out), d_new.data_ptr(), d_over.data_ptr())
            lib.pya_debug_centroid_passes(7)
            assert rc == 0, lib.pya_last_error(scorer._h)
        return job

    passes(7)()
    o_mz, o_it = out
    new = d_new.cpu().numpy()
    kept, k_host = int(new[-1]), int(new[n_host])
    assert new[:n_host + 1].tobytes() == want[2].tobytes() and o_mz[:k_host].cpu().numpy().tobytes() == want[0].tobytes() and \
        o_it[:k_host].cpu().numpy().tobytes() == want[1].tobytes() and d_over.cpu().numpy().tolist() == [0, 0], \
        "%s: the kernels and the restatement differ" % name
    c_mz, c_it = o_mz[:kept].cpu().numpy(), o_it[:kept].cpu().numpy()
    nbytes = mz.nbytes + it.nbytes

    def copy():
        out[0].copy_(d_mz)                                       # (hipMemcpyAsync device to device on the same stream)
        out[1].copy_(d_it)

    # (the full call comes last in a round: MARK alone leaves unscanned counts behind, which PLACE alone must not read)
    place, mark, full, cp, deiso = timed(dev, warm, runs, [passes(4), passes(1), passes(7), copy,
                                                           lambda: device.deisotope(scorer, d_mz, d_it, d_off, DEISO, out=out)])
    t0 = time.perf_counter()
    h_mz, h_it = d_mz[:cut].cpu().numpy(), d_it[:cut].cpu().numpy()
    t1 = time.perf_counter()
    r = rollup.centroid(h_mz, h_it, off[:n_host + 1], RULE)
    t2 = time.perf_counter()
    torch.from_numpy(r[0]).to(dev), torch.from_numpy(r[1]).to(dev)
    torch.cuda.synchronize(dev)
    t3 = time.perf_counter()
    host_ms = (t3 - t0) * 1e3 * (mz.size / max(cut, 1))          # (scaled from the first spectra to all of them)
    print("centroid %-9s f64/f64 %7d spectra %10d points %8.1f MB, peaks out %9d (1 of %.1f)  three passes ms %s = %6.0f GB/s read  "
          "MARK ms %s  PLACE ms %s  d2d copy ms %s  passes/copy %5.2f  pya_deisotope_spectra ms %s  centroid/deisotope %5.2f  "
          "D2H + rollup.centroid + H2D on %d spectra, scaled to all: %.0f ms (restatement alone %.0f of %.0f ms measured) = %.0f times the passes"
          % (name, off.size - 1, mz.size, nbytes / 2**20, kept, mz.size / max(kept, 1), pct(full), nbytes / 1e9 / (np.median(full) * 1e-3),
             pct(mark), pct(place), pct(cp), np.median(full) / np.median(cp), pct(deiso), np.median(full) / np.median(deiso), n_host, host_ms,
             (t2 - t1) * 1e3, (t3 - t0) * 1e3, host_ms / np.median(full)), flush=True)
    return c_mz, c_it, new


def step_rows(scorer, name, forms, warm, runs):
    dev = torch.device("cuda", scorer.device)
    for label, batch in forms:
        plan = device.DevicePlan(scorer, batch)
        d_mz, d_it = torch.from_numpy(np.ascontiguousarray(batch["mz"])).to(dev), torch.from_numpy(np.ascontiguousarray(batch["intensity"])).to(dev)
        step, = timed(dev, warm, runs, [lambda: plan.run(d_mz, d_it)])
        plan.check()
        print("step %-9s %-10s %6d PSMs %10d peaks  resident step ms %s = %6.2f M PSMs/s  mean best_score %.1f"
              % (name, label, batch["n_psm"], int(batch["peak_off"][-1]), pct(step), batch["n_psm"] / np.median(step) / 1e3,
                 float(plan.best_score.cpu().numpy().mean())), flush=True)
        plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--long", type=int, default=8192)
    ap.add_argument("--host", type=int, default=2000)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    desc = synth.describe("cfg2", n_psm=a.n, seed=1000)
    scorer = harness.make_scorer(PyAscore, desc["settings"])
    print("# centroid_probe: seed 1000; %s; %d timed rounds after %d; sigma %g on a %g grid; rule %s"
          % (torch.cuda.get_device_properties(scorer.device).gcnArchName, a.runs, a.warm, SIGMA, STEP, RULE))
    print("# ms: median (p10..p90); HIP events on torch's stream; GB/s = m/z and intensity bytes over the three passes' median")
    cfg2 = synth.make_slice(desc)
    mz, it, off = render(np.asarray(cfg2["mz"], np.float64), np.asarray(cfg2["intensity"], np.float64), np.asarray(cfg2["peak_off"], np.int64))
    print("cfg2 rendered", file=sys.stderr, flush=True)
    c_mz, c_it, c_off = kernel_rows(scorer, "cfg2", mz, it, off, a.warm, a.runs, a.host)
    step_rows(scorer, "cfg2", (("profile", dict(cfg2, mz=mz, intensity=it, peak_off=off)), ("centroided", dict(cfg2, mz=c_mz, intensity=c_it, peak_off=c_off)),
                               ("clean", cfg2)), a.warm, a.runs)
    del cfg2, mz, it, c_mz, c_it
    few = synth.make_slice(synth.describe("cfg2", n_psm=64, seed=1000, n_noise=1200))
    mz, it, off = render(np.asarray(few["mz"], np.float64), np.asarray(few["intensity"], np.float64), np.asarray(few["peak_off"], np.int64))
    times = max(a.long // 64, 1)
    off = np.concatenate([[0], np.cumsum(np.tile(np.diff(off), times))]).astype(np.int64)
    mz, it = np.tile(mz, times), np.tile(it, times)
    print("long rendered", file=sys.stderr, flush=True)
    kernel_rows(scorer, "long", mz, it, off, a.warm, a.runs, 64)


if __name__ == "__main__":
    main()
