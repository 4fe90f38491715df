"""The peptidoform stage (pya_plan_peptidoforms / pya_peptidoform_reduce, csrc/peptidoforms.hip), measured beside the step and
the probability stage it follows and beside the host way it replaces: on a device-resident plan, HIP events around (a) one
DevicePlan.run, (b) one DevicePlan.probs(), (c) one DevicePlan.peptidoforms() behind them on one stream, and the stage's own
events between its phases (entries, the thirteen sort passes, the segmented reduction, the finish) -- RUNS rounds after WARM
warm-up rounds, median and p10..p90 -- for 100 000 cfg2 PSMs as 20 000 groups of 5 and for 4 000 cfg5 PSMs; then the host way
on the same run: D2H of best_sig, ascores and the residue and PSM records, and numpy grouping ending in
pyascore_amd.rollup.merge_peptidoforms (wall clock).  Then the reduce alone at 10^5 and 10^6 records (DevicePlan.peptidoform_reduce
against merge_peptidoforms on the host, D2H included).  The lists of both ways are compared bytewise before anything is reported.
Needs a GPU: there is no fallback.

    python scripts/peptidoforms_probe.py [--runs 20] > profiles/peptidoforms/probe.txt"""
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
from pyascore_amd.device import DevicePlan, peptidoform_records, psm_prob_records  # noqa: E402

CASES = (("cfg2", 100000), ("cfg5", 4000))
REDUCE_SIZES = (10 ** 5, 10 ** 6)
SHARE = 5
THR = 0.75
DT = ru.PEPTIDOFORM_DTYPE


def numpy_way(with_prob, pp, site_off, best_sig, ascores, group, thr):
    """the PSMs as records (vectorised), then the host merge"""
    n = best_sig.size
    ok = (pp["kind"] == 1) & (group >= 0)
    owner = np.repeat(np.arange(n), np.diff(site_off))
    r = (np.arange(int(site_off[-1])) - site_off[owner]).astype(np.uint64)
    inb = ((best_sig[owner] >> r) & np.uint64(1)) != 0
    prob = np.full(n, np.uint64(0xFFFFFFFFFFFFFFFF))
    np.minimum.at(prob, owner[inb], with_prob.view(np.uint64)[inb])
    prob[best_sig == 0] = np.float64(1.0).view(np.uint64)
    k = np.unpackbits(best_sig.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)
    key = ru._ascore_key(ascores).reshape(ascores.shape)
    key = np.where(np.arange(ascores.shape[1])[None, :] < k[:, None], key, np.int64(1) << 40).min(axis=1)
    key[k == 0] = ru._ascore_key(np.array([np.inf], np.float32))[0]
    rec = np.zeros(n, DT)
    rec["sig_bits"], rec["group"], rec["n_psm"] = best_sig, group.astype(np.uint32), ok
    rec["best_min_prob"] = prob.view(np.float64)
    rec["n_confident"] = rec["best_min_prob"] >= thr
    rec["best_psm"] = np.arange(n)
    rec["best_z"] = pp["z"]
    rec["best_min_ascore"] = np.where(key >> 31 != 0, key - 0x80000000, 0xFFFFFFFF - key).astype(np.uint32).view(np.float32)
    return ru.merge_peptidoforms(rec)


def stage_ms(scorer):
    ms = (C.c_float * (_lib.PYA_PFORM_PHASES + 1))()
    rc = scorer._lib.pya_debug_last_peptidoform_ms(scorer._h, ms)
    if rc:
        scorer._raise(rc)
    return list(ms)


def device_resident(scorer, batch, warm, runs):
    dev = torch.device("cuda", scorer.device)
    plan = DevicePlan(scorer, batch, peptidoforms=True)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    off = plan.site_offsets()
    n = batch["n_psm"]
    group = (np.arange(n) % max(1, n // SHARE)).astype(np.int32)
    d_group = torch.from_numpy(group).to(dev)
    rec = (torch.zeros((int(off[-1]), 2), dtype=torch.float64, device=dev), torch.zeros((n, 16), dtype=torch.uint8, device=dev))
    t = {k: [] for k in ("step", "probs", "stage", "host")}
    phases = []
    scorer._lib.pya_debug_peptidoform_timing(scorer._h, 1)
    for i in range(warm + runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        plan.run(mz, it)
        ev[1].record()
        plan.probs(out=rec)
        ev[2].record()
        out, cnt = plan.peptidoforms(rec[0], rec[1], d_group, threshold=THR)
        ev[3].record()
        torch.cuda.synchronize(dev)
        ph = stage_ms(scorer)
        t0 = time.perf_counter()
        sp = rec[0].cpu().numpy()
        pp = psm_prob_records(rec[1].cpu().numpy())
        host = numpy_way(np.ascontiguousarray(sp[:, 0]), pp, off, plan.best_sig.cpu().numpy().view(np.uint64), plan.ascores.cpu().numpy(), group, THR)
        dt = time.perf_counter() - t0
        if i >= warm:
            for j, k in enumerate(("step", "probs", "stage")):
                t[k].append(ev[j].elapsed_time(ev[j + 1]))
            t["host"].append(dt * 1e3)
            phases.append(ph)
    scorer._lib.pya_debug_peptidoform_timing(scorer._h, 0)
    c = cnt.cpu().numpy()
    got = peptidoform_records(out.cpu().numpy())[:int(c[0])].copy()
    assert int(c[1]) == 0 and got.tobytes() == host.tobytes(), "the device list and the host way differ"
    plan.close()
    return {k: np.array(v) for k, v in t.items()}, np.array(phases), got.size


def reduce_alone(scorer, plan, n, warm, runs):
    dev = torch.device("cuda", scorer.device)
    rng = np.random.default_rng([1000, n])
    r = np.zeros(n, DT)
    r["group"] = rng.integers(0, max(1, n // 10), n)
    r["sig_bits"] = np.uint64(1) << rng.integers(0, 6, n).astype(np.uint64)
    r["n_psm"], r["best_psm"] = 1, np.arange(n)
    r["best_min_prob"], r["best_z"], r["best_min_ascore"] = rng.random(n), 1.0 + rng.random(n), rng.normal(10, 8, n)
    d = torch.from_numpy(r.view(np.uint8).reshape(-1, 48)).to(dev)
    t_dev, t_host, phases = [], [], []
    scorer._lib.pya_debug_peptidoform_timing(scorer._h, 1)
    for i in range(warm + runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out, cnt = plan.peptidoform_reduce(d)
        ev[1].record()
        torch.cuda.synchronize(dev)
        ph = stage_ms(scorer)
        t0 = time.perf_counter()
        host = ru.merge_peptidoforms(peptidoform_records(d.cpu().numpy()))
        dt = time.perf_counter() - t0
        if i >= warm:
            t_dev.append(ev[0].elapsed_time(ev[1]))
            t_host.append(dt * 1e3)
            phases.append(ph)
    scorer._lib.pya_debug_peptidoform_timing(scorer._h, 0)
    got = peptidoform_records(out.cpu().numpy())[:int(cnt.cpu().numpy()[0])]
    assert got.tobytes() == host.tobytes(), "%d records: the device list and the host merge differ" % n
    return np.array(t_dev), np.array(t_host), np.array(phases), got.size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every batch size")
    a = ap.parse_args()
    p = lambda v: "%8.3f (%.3f..%.3f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))  # noqa: E731
    print("# peptidoforms_probe: seed 1000; %s; %d timed rounds after %d; tile %d entries; %d bytes of workspace per entry at 10^6"
          % (torch.cuda.get_device_properties(0).gcnArchName, a.runs, a.warm, _lib.PYA_PFORM_TILE,
             _lib.load().pya_peptidoform_workspace_bytes(10 ** 6) // 10 ** 6))
    print("# step / probs / stage = HIP events around DevicePlan.run / .probs / .peptidoforms on one stream, ms (median, p10..p90); entries / "
          "sort / reduce / finish = the stage's own events between its phases (sort: thirteen passes); host ms = the way it replaces on the "
          "same run: D2H of best_sig, ascores, the residue and PSM records, numpy grouping and merge_peptidoforms (wall clock); about %d PSMs "
          "per group" % SHARE)
    head = "%-8s %8s %8s" + " %24s" * 8
    print(head % ("batch", "entries", "forms", "step ms", "probs ms", "stage ms", "entries ms", "sort ms", "reduce ms", "finish ms", "host ms"))
    scorer = None
    for name, n in CASES:
        n = max(64, int(n * a.scale))
        desc = synth.describe(name, n_psm=n, seed=1000)
        batch, settings = synth.make_slice(desc), desc["settings"]
        scorer = harness.make_scorer(PyAscore, settings)
        t, ph, forms = device_resident(scorer, batch, a.warm, a.runs)
        print(head % (name, n, forms, p(t["step"]), p(t["probs"]), p(t["stage"]), p(ph[:, 0]), p(ph[:, 1]), p(ph[:, 2]), p(ph[:, 3]), p(t["host"])),
              flush=True)
    small, _ = synth.make_batch("cfg2", n_psm=2, seed=1000)
    plan = DevicePlan(scorer, small, peptidoforms=True)
    for n in REDUCE_SIZES:
        n = max(64, int(n * a.scale))
        t_dev, t_host, ph, forms = reduce_alone(scorer, plan, n, a.warm, a.runs)
        print(head % ("reduce", n, forms, "-", "-", p(t_dev), p(ph[:, 0]), p(ph[:, 1]), p(ph[:, 2]), p(ph[:, 3]), p(t_host)), flush=True)


if __name__ == "__main__":
    main()
