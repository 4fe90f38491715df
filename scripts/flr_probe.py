"""The site FLR stage (pya_rollup_flr, csrc/flr.hip), measured beside the host way it replaces: for roll-up tables of 10^4,
10^5, 10^6 and 10^7 slots on the device, HIP events around the whole stage and between its phases -- the key build, each of the
nine sort passes (histogram, scan, scatter), the scans over the sorted order with the records -- through
pya_debug_rollup_flr_timed, RUNS rounds after WARM warm-up rounds into buffers allocated before, median and p10..p90; then
the host way on the same table: D2H of the table and pyascore_amd.rollup.flr (wall clock).  The tables are seeded: best_prob
from a mixture that piles up at 1.0 as real tables do (half the ranked slots exactly 1.0, a quarter within 10^-3 of it, the
rest uniform), 5 % empty slots, 10 % decoys.  The records, the order and n_ranked of the device and of the host way are
compared bytewise before anything is reported.  Needs a GPU: there is no fallback.

    python scripts/flr_probe.py [--runs 10] > profiles/flr/probe.txt"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import harness  # noqa: E402
from pyascore_amd import PyAscore, _lib, rollup as ru, synth  # noqa: E402
from pyascore_amd.device import flr_records, rollup_records  # noqa: E402

SIZES = (10 ** 4, 10 ** 5, 10 ** 6, 10 ** 7)
SEED = 1000


def make_table(n, seed=SEED):
    rng = np.random.default_rng([seed, n])
    t = ru.empty(n)
    u = rng.random(n)
    p = np.where(u < 0.5, 1.0, np.where(u < 0.75, 1.0 - 1e-3 * rng.random(n), rng.random(n)))
    covered = rng.random(n) >= 0.05
    t["best_prob"] = np.where(covered, p, 0.0)
    t["n_psm"] = np.where(covered, rng.integers(1, 6, n), 0)
    t["best_psm"] = np.where(covered, rng.integers(0, 1 << 20, n), ru.NO_PSM)
    t["n_in_best"] = np.where(covered, rng.integers(0, 3, n), 0)
    cls = (rng.random(n) < 0.10).astype(np.uint8)
    return t, cls


def measure(scorer, n, warm, runs):
    dev = torch.device("cuda", scorer.device)
    table, cls = make_table(n)
    d_table = torch.from_numpy(table.view(np.uint8).reshape(-1, 32)).to(dev)
    d_cls = torch.from_numpy(cls).to(dev)
    lib = scorer._lib
    work_bytes = int(lib.pya_flr_workspace_bytes(n))
    work = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    nr = torch.empty(2, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    phases, host = [], []
    for i in range(warm + runs):
        ms = (C.c_float * (_lib.PYA_FLR_PHASES + 1))()
        rc = lib.pya_debug_rollup_flr_timed(scorer._h, d_table.data_ptr(), n, d_cls.data_ptr(), 0, stream, work.data_ptr(), work_bytes,
                                            out.data_ptr(), order.data_ptr(), nr.data_ptr(), ms)
        if rc:
            scorer._raise(rc)
        t0 = time.perf_counter()
        h_table = rollup_records(d_table.cpu().numpy())
        h_rec, h_order, h_n = ru.flr(h_table, cls)
        dt = time.perf_counter() - t0
        if i >= warm:
            phases.append(list(ms))
            host.append(dt * 1e3)
    got = flr_records(out.cpu().numpy())
    assert got.tobytes() == h_rec.tobytes(), "%d slots: the device records and the host way differ" % n
    assert order.cpu().numpy().view(np.uint32).tobytes() == h_order.tobytes() and nr.cpu().numpy().tolist() == [h_n, 0]
    return np.array(phases), np.array(host), work_bytes, h_n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--sizes", type=str, default=",".join(str(s) for s in SIZES))
    a = ap.parse_args()
    _, settings = synth.make_batch("cfg2", n_psm=1, seed=SEED)
    scorer = harness.make_scorer(PyAscore, settings)
    print("# flr_probe: seed %d; %s; %d timed rounds after %d; tile %d slots" % (SEED, torch.cuda.get_device_properties(0).gcnArchName, a.runs,
                                                                               a.warm, _lib.PYA_FLR_TILE))
    print("# stage / keys / pass / scans = HIP events inside pya_debug_rollup_flr_timed on one stream, ms (median, p10..p90): the whole "
          "stage, the key build, ONE sort pass (median over the nine passes of a round; min..max of the per-pass medians), the scans "
          "over the sorted order with the records; host ms = the way it replaces: D2H of the table and pyascore_amd.rollup.flr (wall "
          "clock); B/slot = workspace bytes per slot")
    print("%9s %9s %7s %24s %24s %30s %24s %28s" % ("slots", "ranked", "B/slot", "stage ms (p10..p90)", "keys ms (p10..p90)",
                                                   "pass ms (min..max of 9)", "scans ms (p10..p90)", "host ms (p10..p90)"))
    p = lambda v: "%9.3f (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))  # noqa: E731
    for n in [int(s) for s in a.sizes.split(",")]:
        ph, host, work_bytes, n_ranked = measure(scorer, n, a.warm, a.runs)
        per_pass = np.median(ph[:, 1:10], axis=0)
        print("%9d %9d %7.2f %24s %24s %30s %24s %28s" % (
            n, n_ranked, work_bytes / n, p(ph[:, 11]), p(ph[:, 0]), "%9.3f (%.3f..%.3f)" % (np.median(per_pass), per_pass.min(), per_pass.max()),
            p(ph[:, 10]), p(host)), flush=True)


if __name__ == "__main__":
    main()
