"""Charge deconvolution, measured.  One process on one GPU:

  (a) pya_decharge_spectra (mark, scan, place) over the spectra of 100 000 cfg2 PSMs whose peaks are 2+ or 3+ with probability
      0.6 and carry two satellites each (the generator of tests/decharge_cases.py, restated here) and over bench.py's dense batch
      (32 768 spectra of about 1 570 peaks), float64 / float64: HIP events around one call on torch's stream, RUNS rounds after
      WARM warm-up rounds, median and p10..p90; MARK and PLACE apart through pya_debug_decharge_passes (one pass a call; PLACE
      alone runs on the workspace the last full call left, same arrays, same work).  Beside them, in the same rounds:
      pya_deisotope_spectra on the same arrays and a device-to-device copy of the same m/z and intensity bytes.  The bytes of
      the kernels and of the restatement pyascore_amd.rollup.decharge are compared before anything is reported.
  (b) the payoff: for the charged cfg2 batch, the resident step (DevicePlan.run) under plain settings (b/y at 1+) on the
      decharged spectra, beside the resident step with max_fragment_charge = 3 on the deisotoped spectra -- the only answer to
      multiply charged fragments without this transform; the mean best_score of both.

Nothing here is a threshold.  Needs a GPU: there is no fallback.

    python scripts/decharge_probe.py [--runs 30] > profiles/decharge/probe.txt"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import harness  # noqa: E402
from pyascore_amd import PyAscore, device, rollup, synth  # noqa: E402

P = rollup.decharge_params()
P_ISO = rollup.deisotope_params()
S = 1.0033548378


def pct(v):
    return "%9.4f (%.4f..%.4f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))


def charged(batch, share, carrier=synth.PROTON):
    """every peak at 2+ or 3+ with probability ``share``, else 1+, with satellites at + S / z and + 2 S / z (0.5x, 0.2x)"""
    rng = np.random.default_rng(3)
    mz, it, off = np.asarray(batch["mz"], np.float64), np.asarray(batch["intensity"], np.float64), np.asarray(batch["peak_off"], np.int64)
    z = np.where(rng.random(mz.size) < share, rng.integers(2, 4, size=mz.size), 1).astype(np.float64)
    xz = (mz + (z - 1.0) * carrier) / z
    spec = np.repeat(np.arange(off.size - 1), np.diff(off))
    x = np.concatenate([xz, xz + S / z, xz + 2 * S / z])
    y = np.concatenate([it, 0.5 * it, 0.2 * it])
    order = np.lexsort((x, np.concatenate([spec, spec, spec])))
    return dict(batch, mz=x[order], intensity=y[order], peak_off=3 * off)


def kernel_rows(scorer, name, batch, warm, runs):
    dev = torch.device("cuda", scorer.device)
    off = np.ascontiguousarray(batch["peak_off"], np.int64)
    mz, it = np.ascontiguousarray(batch["mz"], np.float64), np.ascontiguousarray(batch["intensity"], np.float64)
    d_mz, d_it, d_off = torch.from_numpy(mz).to(dev), torch.from_numpy(it).to(dev), torch.from_numpy(off).to(dev)
    out = (torch.empty_like(d_mz), torch.empty_like(d_it))
    want = rollup.decharge(mz, it, off, P)
    o_mz, o_it, d_new, d_chg, _ = device.decharge(scorer, d_mz, d_it, d_off, P, out=out)
    new = d_new.cpu().numpy()
    kept = int(new[-1])
    assert new.tobytes() == want[2].tobytes() and o_mz.cpu().numpy()[:kept].tobytes() == want[0].tobytes() and \
        o_it.cpu().numpy()[:kept].tobytes() == want[1].tobytes() and d_chg.cpu().numpy()[:kept].tobytes() == want[3].tobytes(), \
        "%s: the kernels and the restatement differ" % name
    # one workspace for every call of the rounds, so that PLACE alone finds what the last full call left
    lib = scorer._lib
    work = torch.empty(int(lib.pya_decharge_workspace_bytes(off.size - 1, mz.size)) // 8, dtype=torch.int64, device=dev)
    new_off = torch.empty(off.size, dtype=torch.int64, device=dev)
    over = torch.zeros(2, dtype=torch.int32, device=dev)
    chg = torch.empty(mz.size, dtype=torch.uint8, device=dev)
    import ctypes as C
    from pyascore_amd import _lib
    c_params = rollup.decharge_c_params(P)
    t_in = _lib.TypedSpectra(d_mz.data_ptr(), d_it.data_ptr(), 0, 0)
    t_out = _lib.TypedSpectra(out[0].data_ptr(), out[1].data_ptr(), 0, 0)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(passes):
        lib.pya_debug_decharge_passes(passes)
        rc = lib.pya_decharge_spectra(scorer._h, C.byref(t_in), d_off.data_ptr(), off.size - 1, C.byref(c_params), stream, work.data_ptr(),
                                      work.numel() * 8, C.byref(t_out), new_off.data_ptr(), chg.data_ptr(), over.data_ptr())
        lib.pya_debug_decharge_passes(7)
        assert rc == 0, lib.pya_last_error(scorer._h)

    t = {k: [] for k in ("all", "mark", "place", "deiso", "copy")}
    for i in range(warm + runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(10)]
        ev[0].record()
        call(7)
        ev[1].record()
        ev[2].record()
        call(1)
        ev[3].record()
        call(2)                                                  # (the scan again: MARK left counts, PLACE needs offsets)
        ev[4].record()
        call(4)
        ev[5].record()
        ev[6].record()
        device.deisotope(scorer, d_mz, d_it, d_off, P_ISO, out=out)
        ev[7].record()
        ev[8].record()
        out[0].copy_(d_mz)                                       # (hipMemcpyAsync device to device on the same stream)
        out[1].copy_(d_it)
        ev[9].record()
        torch.cuda.synchronize(dev)
        if i >= warm:
            for key, a in (("all", 0), ("mark", 2), ("place", 4), ("deiso", 6), ("copy", 8)):
                t[key].append(ev[a].elapsed_time(ev[a + 1]))
    assert new_off.cpu().numpy().tobytes() == want[2].tobytes()
    m = {k: np.array(v) for k, v in t.items()}
    nbytes = mz.nbytes + it.nbytes
    print("decharge %-10s f64/f64 %7d spectra %9d peaks %7.1f MB, kept %.4f, moved %.4f of the kept  three passes ms %s = %6.0f GB/s read  MARK ms %s  "
          "PLACE ms %s  pya_deisotope_spectra ms %s  d2d copy ms %s  decharge/deisotope %5.2f  decharge/copy %5.2f"
          % (name, off.size - 1, mz.size, nbytes / 2**20, kept / max(mz.size, 1), float((want[3] > 1).mean()), pct(m["all"]),
             nbytes / 1e9 / (np.median(m["all"]) * 1e-3), pct(m["mark"]), pct(m["place"]), pct(m["deiso"]), pct(m["copy"]),
             np.median(m["all"]) / np.median(m["deiso"]), np.median(m["all"]) / np.median(m["copy"])), flush=True)
    return dict(batch, mz=want[0], intensity=want[1], peak_off=want[2])


def step_rows(scorer, name, forms, warm, runs):
    dev = torch.device("cuda", scorer.device)
    for label, batch in forms:
        plan = device.DevicePlan(scorer, batch)
        d_mz, d_it = torch.from_numpy(np.ascontiguousarray(batch["mz"])).to(dev), torch.from_numpy(np.ascontiguousarray(batch["intensity"])).to(dev)
        step = []
        for i in range(warm + runs):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            plan.run(d_mz, d_it)
            ev[1].record()
            torch.cuda.synchronize(dev)
            if i >= warm:
                step.append(ev[0].elapsed_time(ev[1]))
        plan.check()
        score = float(plan.best_score.cpu().numpy().mean())
        step = np.array(step)
        print("step %-10s %-44s %6d PSMs %9d peaks  resident step ms %s = %6.2f M PSMs/s  mean best_score %.1f"
              % (name, label, batch["n_psm"], int(batch["peak_off"][-1]), pct(step), batch["n_psm"] / np.median(step) / 1e3, score), flush=True)
        plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--dense", type=int, default=32768)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    a = ap.parse_args()
    desc = synth.describe("cfg2", n_psm=a.n, seed=1000)
    scorer = harness.make_scorer(PyAscore, desc["settings"])
    print("# decharge_probe: seed 1000; %s; %d timed rounds after %d; tol %g, charges 1..%d, ratio %g, carrier %g, witness %g"
          % (torch.cuda.get_device_properties(scorer.device).gcnArchName, a.runs, a.warm, P["tol"], P["max_charge"], P["ratio0"], P["carrier"],
             P["witness"]))
    print("# ms: median (p10..p90); three passes = HIP events around one pya_decharge_spectra; MARK, PLACE = events around a call that launches that "
          "pass alone; GB/s = m/z and intensity bytes read over the three passes' median; d2d copy = events around device-to-device copies of the "
          "same bytes", flush=True)
    clean = synth.make_slice(desc)
    dirty = charged(clean, 0.6)
    del clean
    decharged = kernel_rows(scorer, "charged0.6", dirty, a.warm, a.runs)
    f = rollup.deisotope(dirty["mz"], dirty["intensity"], dirty["peak_off"], P_ISO)
    deiso = dict(dirty, mz=f[0], intensity=f[1], peak_off=f[2], max_charge=np.full(a.n, 3, np.int32))
    step_rows(scorer, "charged0.6", (("decharged, plain settings (b/y at 1+)", decharged), ("deisotoped, max_fragment_charge = 3", deiso),
                                     ("deisotoped, plain settings", dict(deiso, max_charge=dirty["max_charge"]))), a.warm, a.runs)
    del dirty, decharged, deiso, f
    dense = synth.make_slice(synth.describe("cfg2", n_psm=a.dense, seed=1000, n_noise=1500, isotopes=True))
    kernel_rows(scorer, "dense1570", dense, a.warm, a.runs)


if __name__ == "__main__":
    main()
