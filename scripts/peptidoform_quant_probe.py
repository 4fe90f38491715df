"""The peptidoform quantification, measured beside the list stage it contains, beside the site quantification on the same batch
and beside the host way it replaces: on a device-resident plan of 100 000 cfg2 PSMs whose peptides repeat SHARE times -- the isomers split a peptide's PSMs over several
peptidoforms; the first output line says how many PSMs a peptidoform has --, HIP events around (a) one DevicePlan.peptidoform_quant -- the list and the table --, (b) one
DevicePlan.peptidoforms alone on the same PSMs -- the floor, since (a) contains it -- and (c) one DevicePlan.site_quant with the
slots keyed by peptide, all behind one run and one probs() on one stream; RUNS rounds after WARM warm-up rounds, every stage
into tensors torch's allocator has cached, median and p10..p90 of each, with 3, 18 and 64 channels.  Then the host way on the
same records, once per case: the probability records, best_sig, ascores and the matrix to the host (D2H) and
pyascore_amd.rollup.peptidoform_quant (wall clock).  Then score_batch host to host with and without peptidoform_quant=, and
with --parent-lib the plain call on another build of the library in a child process.  The quant threshold is the median
min_prob of the listed PSMs, so about half of them contribute.  The pair of the plan and of the numpy restatement are compared
bytewise before anything is reported.  Needs a GPU: there is no fallback.

    python scripts/peptidoform_quant_probe.py [--runs 30] [--parent-lib LIB] > profiles/peptidoform_quant/probe.txt"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

CHANNELS = (3, 18, 64)
SHARE = 40                  # PSMs per peptide; the isomers split them over several peptidoforms (the output says how many each)
SCALE = 10
LIST_THR = 0.75


def repeated(n, share, seed=1000):
    """n cfg2 PSMs; the peptide (and its modification count and charge) of PSM i is that of PSM i mod (n / share), the spectrum
    stays -- PSMs of one peptide lie n / share apart, scattered over the batch, which is the normal layout"""
    from pyascore_amd import synth
    desc = synth.describe("cfg2", n_psm=n, seed=seed)
    batch, settings = synth.make_slice(desc), desc["settings"]
    m = max(1, n // share)
    src = np.arange(n) % m
    lens = np.diff(batch["pep_off"])[src]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    take = np.repeat(batch["pep_off"][:-1][src] - off[:-1], lens) + np.arange(int(lens.sum()))
    assert int(batch["aux_off"][-1]) == 0, "the probe's batch has no auxiliary modifications to move"
    out = dict(batch, pep=np.ascontiguousarray(batch["pep"][take]), pep_off=off, n_of_mod=np.ascontiguousarray(batch["n_of_mod"][src]),
               max_charge=np.ascontiguousarray(batch["max_charge"][src]))
    return out, settings, src.astype(np.int32)


def matrix(n_rows, n_ch, seed=1000):
    rng = np.random.default_rng(seed + n_ch)
    v = rng.random((n_rows, n_ch)) * 1e5
    v[rng.random((n_rows, n_ch)) < 0.03] = np.nan
    return v


def plain_rates(n, calls):
    """M PSMs/s of plain score_batch calls (the child of --parent-lib runs only this)"""
    from oracle import harness
    from pyascore_amd import PyAscore
    batch, settings, _ = repeated(n, SHARE)
    scorer = harness.make_scorer(PyAscore, settings)
    scorer.score_batch(batch)
    rates = []
    for _ in range(calls):
        t0 = time.perf_counter()
        scorer.score_batch(batch)
        rates.append(n / (time.perf_counter() - t0) / 1e6)
    return rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--psms", type=int, default=100000)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--parent-lib", type=str, default="", help="another build of the library: its plain score_batch rate, in a child process")
    ap.add_argument("--plain-only", action="store_true", help="print the plain score_batch rates as JSON and stop (the child of --parent-lib)")
    a = ap.parse_args()
    if a.plain_only:
        print(json.dumps(plain_rates(a.psms, a.calls)))
        return
    parent = None
    if a.parent_lib:                                        # (a fresh child process, before this one opens the GPU)
        env = dict(os.environ, PYA_LIB=os.path.abspath(a.parent_lib), PYA_LIB_OLD="1")
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--calls", str(a.calls), "--psms", str(a.psms)], env=env,
                              capture_output=True, text=True, timeout=600)
        if done.returncode != 0:
            raise SystemExit("the child with --parent-lib failed (%d):\n%s" % (done.returncode, done.stderr[-2000:]))
        parent = json.loads(done.stdout.strip().splitlines()[-1])
    import torch
    from oracle import harness
    from pyascore_amd import PyAscore, rollup as ru
    from pyascore_amd.device import DevicePlan, peptidoform_records, psm_prob_records, site_quant_records
    from pyascore_amd.probs import SITE_PROB_DTYPE
    batch, settings, group = repeated(a.psms, SHARE)
    scorer = harness.make_scorer(PyAscore, settings)
    dev = torch.device("cuda", scorer.device)
    plan = DevicePlan(scorer, batch, peptidoform_quant=True)
    mz, it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    plan.run(mz, it)
    _, d_sites, d_psms = plan.probs()
    off = plan.site_offsets()
    torch.cuda.synchronize(dev)
    n, n_rec = int(batch["n_psm"]), int(off[-1])
    d_group = torch.from_numpy(group).to(dev)
    h_sites = np.ascontiguousarray(d_sites.cpu().numpy()).view(SITE_PROB_DTYPE).reshape(-1)
    h_psms = psm_prob_records(d_psms.cpu().numpy())
    h_sig = plan.best_sig.cpu().numpy().view(np.uint64)
    h_asc = plan.ascores.cpu().numpy()
    # the threshold: the median min_prob of the listed PSMs
    mp = ru.peptidoform_min_prob(h_sites, h_psms, off, h_sig, group)
    thr = float(np.nanmedian(mp))
    p_all = ru.site_quant_params(threshold=thr, scale_log2=SCALE, n_channels=1)
    whole = ru.peptidoform_quant(h_sites, h_psms, off, h_sig, h_asc, group, np.ones((n, 1)), None, p_all, threshold=LIST_THR)
    listed = int(whole[0]["n_psm"].sum())
    # the site quantification's slots: record r of a PSM goes to the r-th slot of its peptide
    ns = np.diff(off)
    width = np.zeros(int(group.max()) + 1, np.int64)
    np.maximum.at(width, group, ns)
    base = np.concatenate([[0], np.cumsum(width)])
    owner = np.repeat(np.arange(n), ns)
    slot = (base[group[owner]] + np.arange(n_rec) - off[owner]).astype(np.int32)
    n_slots = int(base[-1])
    d_slot = torch.from_numpy(slot).to(dev)
    print("# peptidoform_quant_probe: seed 1000; %s; cfg2, %d PSMs as %d peptides of %d PSMs, %d residue records, %d PSMs in a list of %d "
          "peptidoforms (%.2f PSMs each); quant threshold %r: about half of the listed PSMs contribute; %d timed rounds after %d"
          % (torch.cuda.get_device_properties(0).gcnArchName, n, int(group.max()) + 1, SHARE, n_rec, listed, whole[0].size,
             listed / max(1, whole[0].size), thr, a.runs, a.warm))
    print("# ms: median (p10..p90); pair = HIP events around one DevicePlan.peptidoform_quant (the list's launches and one launch of "
          "pform_quant.hip, table cleared inside); list = around one DevicePlan.peptidoforms on the same PSMs; quant part = pair - list "
          "(medians); site_quant = around one DevicePlan.site_quant, slots by peptide and residue, table cleared outside; host = the way it "
          "replaces, once: D2H of the probability records, best_sig, ascores and the matrix, then rollup.peptidoform_quant (wall clock)")
    for n_ch in CHANNELS:
        values = matrix(n, n_ch)
        d_values = torch.from_numpy(values).to(dev)
        p = ru.site_quant_params(threshold=thr, scale_log2=SCALE, n_channels=n_ch)
        sq = plan.site_quant(d_sites, d_psms, d_slot, d_values, p, n_slots=n_slots)
        t = {"pair": [], "list": [], "site": []}
        for i in range(a.warm + a.runs):
            for part in sq:
                part.zero_()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            out = plan.peptidoform_quant(d_sites, d_psms, d_group, d_values, p, threshold=LIST_THR)
            ev[1].record()
            plan.peptidoforms(d_sites, d_psms, d_group, threshold=LIST_THR)
            ev[2].record()
            plan.site_quant(d_sites, d_psms, d_slot, d_values, p, table=sq)
            ev[3].record()
            torch.cuda.synchronize(dev)
            if i >= a.warm:
                for k, key in enumerate(("pair", "list", "site")):
                    t[key].append(ev[k].elapsed_time(ev[k + 1]))
        plan.check()
        m = int(out[3].cpu()[0])
        head, cell = site_quant_records((out[1][:m].cpu().numpy(), out[2][:m].cpu().numpy()))
        got = (peptidoform_records(out[0][:m].cpu().numpy()), head, cell)
        t0 = time.perf_counter()
        r_sites = np.ascontiguousarray(d_sites.cpu().numpy()).view(SITE_PROB_DTYPE).reshape(-1)
        r_psms = psm_prob_records(d_psms.cpu().numpy())
        r_sig, r_asc, r_values = plan.best_sig.cpu().numpy().view(np.uint64), plan.ascores.cpu().numpy(), d_values.cpu().numpy()
        t1 = time.perf_counter()
        want = ru.peptidoform_quant(r_sites, r_psms, off, r_sig, r_asc, group, r_values, None, p, threshold=LIST_THR)
        t2 = time.perf_counter()
        for g, w, what in zip(got, want, ("list", "head", "cell")):
            assert g.tobytes() == w.tobytes(), "%d channels: the device %s and the numpy restatement differ" % (n_ch, what)
        q = lambda v: "%8.4f (%.4f..%.4f)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))  # noqa: E731
        part = np.median(t["pair"]) - np.median(t["list"])
        print("peptidoform_quant cfg2 %2d channels  %7d peptidoforms  PSMs summed %7d  pair ms %s  list ms %s  quant part ms %8.4f = %5.2f of "
              "the list  site_quant ms %s  |  host: D2H %7.1f ms + rollup.peptidoform_quant %8.1f ms"
              % (n_ch, m, int(head["n_records"].sum()), q(t["pair"]), q(t["list"]), part, part / np.median(t["list"]), q(t["site"]),
                 (t1 - t0) * 1e3, (t2 - t1) * 1e3), flush=True)
    plan.close()
    # score_batch host to host
    values = matrix(n, 18)
    forms = dict(group=group, threshold=LIST_THR)
    req = dict(values=values, threshold=thr, scale_log2=SCALE)
    scorer.score_batch(batch, peptidoforms=forms, peptidoform_quant=req)
    rates = {"plain": [], "list": [], "pair": []}
    for _ in range(a.calls):
        for label, kw in (("plain", {}), ("list", dict(peptidoforms=forms)), ("pair", dict(peptidoforms=forms, peptidoform_quant=req))):
            t0 = time.perf_counter()
            scorer.score_batch(batch, **kw)
            rates[label].append(n / (time.perf_counter() - t0) / 1e6)
    q = lambda v: "%6.3f (%.3f..%.3f)" % (np.median(v), np.min(v), np.max(v))  # noqa: E731
    print("score_batch cfg2 %6d PSMs, M PSMs/s median (min..max) of %d calls after 1: plain %s; with peptidoforms= %s; with peptidoforms= and "
          "peptidoform_quant= (18 channels) %s; plain on the parent commit's library %s"
          % (n, a.calls, q(rates["plain"]), q(rates["list"]), q(rates["pair"]), q(parent) if parent is not None else "-"), flush=True)


if __name__ == "__main__":
    main()
