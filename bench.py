#!/usr/bin/env python
"""bench.py -- PSMs/s of the Ascore hot path on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config cfg2] [--psms M] [--dump-outputs DIR] [--full]

A *step* is one pass of the hot path (bin_spectra -> score_signatures -> rank_and_localize)
over one batch of synthetic PSMs of the named BASELINE config whose spectra are already
resident in HBM; for N > 1 every rank scores its own batch of the same size (weak scaling)
and every step ends with the single RCCL gather of the fixed-size result records to rank 0.
The job is ONE seeded description (per-PSM shapes) cut by pyascore_amd.shard.partition into
work-balanced contiguous ranges; a rank generates and scores its own range only.  --scaling strong
keeps the job size fixed as N grows (e.g. --config cfg3 --scaling strong: 1M PSMs over N GPUs).

A plain run does what the headline needs and nothing else: it generates the job, builds the plan, warms
up, times the steps, writes --dump-outputs and prints ONE JSON line on rank 0, including
  roofline     : the dominant kernel's achieved algorithmic GB/s vs the 8 TB/s HBM peak,
                 timed with HIP events on the launch stream inside the timed region.
--full adds every measurement that takes runs of its own, each under its own key of the same line:
  roofline     : + the copy rate this device reaches (`achievable_peak`) and, per kernel family, the
                 HBM traffic and busy shares of the newest committed counters of the config;
  host_api     : host arrays in -> host results out (PyAscore.score_batch) beside what PCIe alone costs;
  other_configs: BASELINE's other single-GPU workloads and the dense-spectrum legs, a child process each;
  cpu_baseline : the reference's own C++ core (oracle/_ref, if its prebuilt library travelled;
                 otherwise this repo's CPU restatement) on the host cores, one PROCESS per core
                 (fresh children started before this program's first GPU call), on a bounded
                 sample of the same workload; one-core rate and parallel efficiency beside it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec
METRIC = "PSMs/sec (Ascore.score) at 1/2/4/8 MI355X + HBM-roofline %"


def algorithmic_bytes(batch, max_k):
    """per PSM 16*P + L + 8 + 8*n_aux + 16 + 64 (summary record)."""
    n = batch["n_psm"]
    peaks = int(batch["peak_off"][-1] - batch["peak_off"][0])
    res = int(batch["pep_off"][-1] - batch["pep_off"][0])
    aux = int(batch["aux_off"][-1] - batch["aux_off"][0])
    return 16 * peaks + res + 8 * n + 8 * aux + 16 * n + 64 * n


# the kernels between two of the plan's timing events = one family of the bench line
FAMILIES = {
    "pya_bin_spectra_kernel": ("pya_bin_spectra_kernel", "pya_bin_exact_kernel"),
    "pya_score_signatures_kernel": ("pya_score_signatures_kernel", "pya_score_nodes_kernel", "pya_score_big_kernel", "pya_score_cnt_kernel", "pya_score_cntg_kernel"),
    "pya_score_localize_kernel": ("pya_score_localize_kernel", "pya_score_localize_pack_kernel", "pya_score_localize_list_kernel",
                                  "pya_bin_score_localize_kernel"),
    "pya_localize_kernel": ("pya_localize_kernel", "pya_localize_hash_kernel", "pya_localize_ties_kernel", "pya_localize_redo_kernel",
                            "pya_localize_recount_kernel", "pya_score_big_list_kernel"),
}


def valu_costs():
    """Measured cycles a SIMD spends per vector instruction of each kernel's own instruction mix
    (profiles/r0N_isa_mix.json = scripts/isa_hist.py over the kernels' inner loops, every class priced
    from profiles/r03_valu_ceiling.csv = scripts/valu_ceiling.hip on MI355X at 6 waves per SIMD), and
    the scalar unit's measured rate (one instruction per cycle per CU)."""
    import glob
    try:
        with open(sorted(glob.glob(os.path.join(ROOT, "profiles", "*_isa_mix.json")))[-1]) as f:    # (the newest round's)
            mix = json.load(f)
    except (OSError, IndexError):
        return {}, 3.7
    cost = {k: v.get("inner_loops_cycles_per_valu") or v.get("all_cycles_per_valu") for k, v in mix.items()}
    vals = [c for c in cost.values() if c]
    return cost, (sum(vals) / len(vals) if vals else 3.7)


def profiled_counters(cfg, kern_ms, names, default_size, lib_version=None):
    """Per kernel family of the bench line, from the newest committed PMC summary of this config
    (profiles/*_rocprof_<cfg>/pmc_summary.csv, separate --pmc passes, scripts/profile.sh):
      traffic      HBM bytes per step, 2 x FETCH_SIZE + WRITE_SIZE (KB counters; gfx950's FETCH_SIZE tallies
                   128-byte requests as 64: MI355X_MICROARCH.md, HBM section);
      hbm_actual   that over the family's duration IN THE PROFILED RUN (kernel_stats.csv of the same directory:
                   counters and durations of one build on one box; `ms_profiled` beside this run's `ms_live`), GB/s;
      valu_busy    SQ_INSTS_VALU x the measured cost of a vector instruction of the kernel's own mix
                   / (1024 SIMDs x the kernel's cycles in the profiled run): the share of SIMD time its vector
                   instructions need at the measured issue rates (profiles/r03_valu_ceiling.md);
      salu_busy    SQ_INSTS_SALU / (256 CUs x cycles): the one scalar unit of a CU issues one per cycle;
      lanes_per_valu  active lanes per vector instruction, of 64 (SQ_THREAD_CYCLES_VALU / SQ_INSTS_VALU);
      lds_conflict LDS bank-conflict cycles per active LDS cycle.
    Kernel cycles = SQ_BUSY_CYCLES / 32 (the counter sums the 32 shader engines).  None when the run
    is not the profiled workload.

    REFUSED (r05 verdict item 3) unless the counters are of the kernels this run executes: scripts/profile.sh writes the
    library's source digest (pya_version: SHA-256 over csrc/ + include/) into the directory's profile_steps.json, and only
    the NEWEST *_rocprof_<cfg> directory is considered -- when its digest is missing or differs from the loaded library's,
    the line carries no traffic, no busy shares, and says why (`traffic_refused`), instead of an older build's numbers."""
    import csv
    import glob
    if not default_size:
        return None, None
    dirs = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_rocprof_" + cfg)))
    if not dirs:
        return None, None
    path = os.path.join(dirs[-1], "pmc_summary.csv")
    prof_src = None
    try:
        with open(os.path.join(dirs[-1], "profile_steps.json")) as f:
            prof_src = json.load(f).get("src")
    except (OSError, ValueError):
        pass
    if lib_version is not None:
        lib_src = lib_version.split("src=")[-1].split()[0] if "src=" in lib_version else None
        if not prof_src or prof_src != lib_src:
            why = "%s was profiled from source digest %s, this run's library is %s" % (
                os.path.relpath(dirs[-1], ROOT), (prof_src or "unrecorded")[:12], (lib_src or "unknown")[:12])
            return {"source": os.path.relpath(path, ROOT), "families": None, "whole_path_traffic": None, "refused": why}, None
    per_kernel = {}
    try:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                per_kernel.setdefault(row["kernel"], {})[row["counter"]] = float(row.get("per_step") or row["mean_value"])
    except OSError:
        return None, None
    # the profiled run's own kernel durations per step (rocprofv3 --kernel-trace --stats of the same command); the
    # number of steps that run made is written next to it by scripts/profile.sh (records older than that file: 10 + 2)
    stats_steps = 12.0
    try:
        with open(os.path.join(dirs[-1], "profile_steps.json")) as f:
            stats_steps = float(json.load(f)["stats_steps"])
    except (OSError, KeyError, ValueError):
        pass
    prof_ns = {}
    try:
        with open(os.path.join(dirs[-1], "kernel_stats.csv"), newline="") as f:
            for row in csv.DictReader(f):
                prof_ns[row["Name"].split("(")[0].replace("void ", "").strip()] = float(row["TotalDurationNs"]) / stats_steps
    except (OSError, KeyError, ValueError):
        prof_ns = {}
    cost, cost_default = valu_costs()
    fams = {}
    whole = 0.0
    for fam_name, ms in zip(names, kern_ms):
        members = FAMILIES.get(fam_name, (fam_name,))
        acc = {"traffic": 0.0, "valu_cyc": 0.0, "valu": 0.0, "salu": 0.0, "cycles": 0.0, "thread_cyc": 0.0,
               "lds_conf": 0.0, "lds_act": 0.0, "kernels": [], "ms_prof": 0.0}
        for kname, c in per_kernel.items():
            if kname.split("<")[0] not in members or "FETCH_SIZE" not in c:
                continue
            acc["kernels"].append(kname)
            acc["ms_prof"] += prof_ns.get(kname, 0.0) * 1e-6
            acc["traffic"] += (2.0 * c.get("FETCH_SIZE", 0.0) + c.get("WRITE_SIZE", 0.0)) * 1024.0
            acc["valu"] += c.get("SQ_INSTS_VALU", 0.0)
            acc["valu_cyc"] += c.get("SQ_INSTS_VALU", 0.0) * (cost.get(kname) or cost_default)
            acc["salu"] += c.get("SQ_INSTS_SALU", 0.0)
            acc["cycles"] += c.get("SQ_BUSY_CYCLES", 0.0) / 32.0
            acc["thread_cyc"] += c.get("SQ_THREAD_CYCLES_VALU", 0.0)
            acc["lds_conf"] += c.get("SQ_LDS_BANK_CONFLICT", 0.0)
            acc["lds_act"] += c.get("SQ_LDS_IDX_ACTIVE", 0.0)
        if not acc["kernels"]:
            continue
        whole += acc["traffic"]
        cyc = acc["cycles"]
        fams[fam_name] = {
            "kernels": sorted(acc["kernels"]), "traffic": acc["traffic"],
            "hbm_actual": acc["traffic"] / (acc["ms_prof"] * 1e-3) / 1e9 if acc["ms_prof"] > 0 else None,
            "ms_profiled": acc["ms_prof"] or None,
            "valu_cycles_per_inst": acc["valu_cyc"] / acc["valu"] if acc["valu"] else None,
            "valu_busy": acc["valu_cyc"] / (1024.0 * cyc) if cyc else None,
            "salu_busy": acc["salu"] / (256.0 * cyc) if cyc else None,
            "lanes_per_valu": acc["thread_cyc"] / acc["valu"] if acc["valu"] and acc["thread_cyc"] else None,
            "lds_conflict_share": acc["lds_conf"] / acc["lds_act"] if acc["lds_act"] else None,
            "ms_live": float(ms)}
    return {"source": os.path.relpath(path, ROOT), "families": fams, "whole_path_traffic": whole}, fams


def achievable_hbm_gbs(torch, dev, nbytes=1 << 30, reps=5):
    """Read + write rate of a plain device copy of 1 GiB (the "trivial kernel" of SURVEY 8(d)): the
    HBM bandwidth a streaming kernel reaches on this box, reported beside the 8 TB/s spec."""
    src = torch.empty(nbytes // 4, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        dst.copy_(src)
    t1.record()
    torch.cuda.synchronize()
    return 2.0 * nbytes * reps / (t0.elapsed_time(t1) * 1e-3) / 1e9


def effective_cores():
    """CPUs this process may really use: the affinity mask, cut to the cgroup's CPU quota when there is
    one (a container that sees 256 logical CPUs but may run 16 of them at a time gains nothing from 256
    workers).  Returns (count, how it was determined)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    why = "affinity mask"
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                txt = f.read().split()
            if path.endswith("cpu.max"):
                quota, period = txt[0], float(txt[1])
            else:
                quota = txt[0]
                with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                    period = float(f.read())
            if quota not in ("max", "-1") and float(quota) > 0:
                q = max(1, int(float(quota) / period + 0.5))
                if q < n:
                    n, why = q, "cgroup quota %s/%d" % (quota, int(period))
            break
        except (OSError, ValueError, IndexError):
            continue
    return max(1, min(n, 256)), why


def cpu_baseline(batch, settings, target_seconds=12.0):
    """The reference's C++ core (oracle/_ref; the CPU restatement if that library did not travel) on
    the host cores of this box, ONE PROCESS PER CORE (oracle/cpu_worker.py: fresh children that never
    touch the GPU; this function itself runs before bench.py's first GPU call).  Every worker scores
    a contiguous slice of a bounded sample of rank 0's batch; all start at a common wall-clock time;
    the all-core rate is the PSMs of all workers over (last end - common start).  The one-core rate is
    one such worker alone; `efficiency` = all_cores / (cores x one_core)."""
    import subprocess
    import tempfile
    from oracle import orc
    # (make says what it did about oracle/_ref: to stderr, stdout carries ONE JSON line)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "oracle", "ref"], stdout=sys.stderr)
    kind = "ref" if orc.available("ref") else "oracle"
    cores, cores_why = effective_cores()
    worker = os.path.join(ROOT, "oracle", "cpu_worker.py")
    n_avail = int(batch["n_psm"])
    tmp = tempfile.mkdtemp(prefix="pya_cpu_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    path = os.path.join(tmp, "sample.npz")
    n_sample = min(n_avail, max(cores * 64, 20000))
    from pyascore_amd.synth import slice_batch
    sample = slice_batch(batch, 0, n_sample)
    np.savez(path, settings=np.asarray(json.dumps(settings)), **{k: np.asarray(v) for k, v in sample.items()})

    def run(slices, reps):
        t_start = time.time() + 4.0 + 0.02 * len(slices)         # every worker is loaded and waiting by then
        procs = [subprocess.Popen([sys.executable, worker, path, str(lo), str(hi), str(reps), repr(t_start), kind],
                                  stdout=subprocess.PIPE, text=True) for lo, hi in slices]
        outs = [json.loads(p.communicate()[0].strip().splitlines()[-1]) for p in procs]
        late = max(o["t0"] for o in outs) - t_start
        n = sum(o["n"] for o in outs)
        return n, max(o["t1"] for o in outs) - min(o["t0"] for o in outs), late

    try:
        # one core: a probe sizes the leg at about a third of the budget
        n_probe = min(n_sample, 400)
        n, dt, _ = run([(0, n_probe)], 1)
        rate1 = n / max(dt, 1e-9)
        n1 = int(min(n_sample, max(n_probe, rate1 * target_seconds / 3)))
        reps1 = max(1, int(round(rate1 * target_seconds / 3 / n1)))
        n_one, dt_one, _ = run([(0, n1)], reps1)
        rate1 = n_one / dt_one
        # all cores: every worker a slice of the sample, repeated to fill two thirds of the budget
        cuts = [n_sample * i // cores for i in range(cores + 1)]
        slices = [(cuts[i], cuts[i + 1]) for i in range(cores) if cuts[i + 1] > cuts[i]]
        per_worker = max(1, n_sample // cores)
        # (sized from a short all-core probe, not from cores x one core: shared caches, memory bandwidth and
        # SMT siblings make the all-core rate whatever it is)
        reps_probe = max(1, int(round(rate1 * 1.0 / per_worker)))
        n_p, dt_p, _ = run(slices, reps_probe)
        reps = max(1, int(round((n_p / dt_p) * target_seconds * 2 / 3 / n_sample)))
        n_all, dt_all, late = run(slices, reps)
    finally:
        try:
            os.remove(path)
            os.rmdir(tmp)
        except OSError:
            pass
    cpu_model = "unknown CPU"
    try:
        with open("/proc/cpuinfo") as f:
            for row in f:
                if row.startswith("model name"):
                    cpu_model = row.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    rate_all = n_all / dt_all
    return {"value": rate_all, "unit": "PSMs/s", "cores": len(slices), "cores_from": cores_why,
            "logical_cpus": os.cpu_count(), "cpu": cpu_model,
            "kind": "reference" if kind == "ref" else "port",
            "sample": "%d PSMs = the first %d of rank 0's batch in %d slices x %d passes, one PROCESS per core "
                      "(oracle/cpu_worker.py), common start, %.1f s (last worker started %.2f s late)"
                      % (n_all, n_sample, len(slices), reps, dt_all, max(late, 0.0)),
            "one_core": {"value": rate1, "sample": "first %d PSMs x %d passes, one process, %.1f s" % (n1, reps1, dt_one)},
            "efficiency": rate_all / (len(slices) * rate1)}


def timed_blocks(torch, dist, dev, pipe, plan, steps, n_blocks):
    """`n_blocks` timed blocks of EXACTLY `steps` steps, each between barrier + synchronize on both sides, the steps
    enqueued back to back.  Per block: (wall seconds = the slowest rank's, own wall seconds, mean HIP-event ms of the
    four kernel families per step, seconds spent waiting for gathers).  `dist` is None without a process group."""
    blocks = []
    for _ in range(max(1, n_blocks)):
        pipe.reset_stats()
        k_ms = np.zeros(4)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        plan.timings_sum()                                 # (forget the events of the warm-up / the block before)
        n_ev = 0
        t0 = time.perf_counter()
        for s_i in range(steps):
            pipe.step()                                    # enqueued back to back: nothing waits for a step here
            if (s_i + 1) % 96 == 0:                        # (the library keeps the events of 128 runs)
                ms_, n_ = plan.timings_sum()
                k_ms += np.asarray(ms_); n_ev += n_
        pipe.drain()                                       # every gather of the timed steps has landed
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        el = time.perf_counter() - t0
        ms_, n_ = plan.timings_sum()                       # HIP events on the launch stream, read after the block
        k_ms += np.asarray(ms_); n_ev += n_
        assert n_ev == steps, (n_ev, steps)
        if dist is not None:                               # (the slowest rank's time, the same on every rank)
            t = torch.tensor([el], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el_own, el = el, float(t.item())
        else:
            el_own = el
        blocks.append((el, el_own, k_ms / max(steps, 1), pipe.gather_wait_s))
    return blocks


DUMP_LIMIT_BYTES = 64 * 10 ** 6


def dump_outputs(dirname, res):
    """--dump-outputs: `res` (name -> host array, one row per PSM: the results of the last timed step) as DIR/<name>.npy,
    so that two builds can be compared output for output on the same seeded job.  float32 stays float32 and int32 becomes
    float64; a 64-bit mask (best_sig, alt_mask: one bit per site) becomes its two 32-bit halves, low then high, as float64
    along a new last axis: every value is exact.  A result over DUMP_LIMIT_BYTES in all is cut to a sample of its PSMs, the
    same on every run (fixed seed); rows.npy names the PSMs that were kept."""
    out = {}
    for name, a in res.items():
        a = np.ascontiguousarray(a)
        if a.dtype in (np.int64, np.uint64):
            a = a.astype("<u8").view("<u4").reshape(a.shape + (2,)).astype(np.float64)
        elif a.dtype != np.float32:
            a = a.astype(np.float64)
        out[name] = a
    n = len(out["best_score"])
    rows = np.arange(n)
    row_bytes = 8 + sum(a.nbytes // max(n, 1) for a in out.values())
    keep = (DUMP_LIMIT_BYTES - 128 * (len(out) + 1)) // row_bytes          # (128 bytes: a .npy file's header)
    if n > keep:
        rows = np.sort(np.random.default_rng(0).choice(n, size=keep, replace=False))
    out = {name: a[rows] for name, a in out.items()}
    out["rows"] = rows.astype(np.float64)
    os.makedirs(dirname, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


FAMILY_NAMES = ["pya_bin_spectra_kernel", "pya_score_signatures_kernel", "pya_score_localize_kernel", "pya_localize_kernel"]


# BASELINE's other single-GPU workloads + the dense-spectrum variants of cfg2 (r05 verdict item 4): name -> (config, PSMs,
# generator options).  cfg3 is quoted on 8 GPUs: its per-GPU share is what one GPU scores here.  `dense*`: cfg2's peptides
# with ~1 500 / ~4 000 peaks per spectrum, every peak with two isotope satellites (synth._var_shape) -- what current
# instruments hand over; fewer PSMs so that the spectra (16 bytes per peak) stay in the range of the other legs.
LEGS = {
    "cfg3": ("cfg3", 125_000, {}),
    "cfg4": ("cfg4", 250_000, {}),
    "cfg5": ("cfg5", 50_000, {}),
    "dense1500": ("cfg2", 32_768, dict(n_noise=1500, isotopes=True)),
    "dense4000": ("cfg2", 16_384, dict(n_noise=4000, isotopes=True)),
}


def other_config_leg(torch, dev, local_rank, leg, steps, warmup, n_blocks, debug=()):
    """One of LEGS at its full size, timed exactly like the headline (spectra resident, plan pre-built, `n_blocks` blocks of
    `steps` steps, the median block): value, ms per step, the plan's host pre-pass, the kernel families' HIP-event times,
    the dominant family and its algorithmic GB/s against the HBM peak, and the same over the whole step."""
    from pyascore_amd import PyAscore, shard, synth
    from pyascore_amd.device import DevicePlan
    cfg, n, gen = LEGS[leg]
    t_gen = time.perf_counter()
    desc = synth.describe(cfg, n_psm=n, seed=1000, **gen)
    batch = synth.make_slice(desc, 0, n)
    t_gen = time.perf_counter() - t_gen
    st = desc["settings"]
    scorer = PyAscore(st["bin_size"], st["n_top"], st["mod_group"], st["mod_mass"], st["mz_error"], st["fragment_types"],
                      device=local_rank)
    for g, m in st["neutral_losses"]:
        scorer.add_neutral_loss(g, m)
    for kv in debug:                                         # (A/B runs of one leg: `bench.py --leg NAME --debug KEY=VALUE`)
        scorer.set_debug(*kv.split("=", 1))
    d_mz = torch.from_numpy(batch["mz"]).to(dev)
    d_int = torch.from_numpy(batch["intensity"]).to(dev)
    torch.cuda.synchronize()
    t_first = time.perf_counter()
    DevicePlan(scorer, batch, timing=True).close()           # (the scorer's first plan also builds its score and order tables)
    t_first = time.perf_counter() - t_first
    t_plan = time.perf_counter()
    plan = DevicePlan(scorer, batch, timing=True)
    t_plan = time.perf_counter() - t_plan
    pipe = shard.StepPipeline(lambda: plan.run(d_mz, d_int), None, n, n, shard.record_width(plan.max_k), dev, enabled=False)
    for _ in range(warmup):
        pipe.step()
    plan.check()
    blocks = timed_blocks(torch, None, dev, pipe, plan, steps, n_blocks)
    plan.check()
    order = sorted(range(len(blocks)), key=lambda i: blocks[i][0])
    elapsed, _, kern_ms, _ = blocks[order[len(order) // 2]]
    dom = int(np.argmax(kern_ms))
    alg = algorithmic_bytes(batch, plan.max_k)
    achieved = alg / (kern_ms[dom] * 1e-3) / 1e9 if kern_ms[dom] > 0 else 0.0
    peaks = int(batch["peak_off"][-1])
    out = {"workload": "%s: %d PSMs on 1 GPU%s" % (cfg, n, (", spectra of ~%d peaks with isotope satellites" % gen["n_noise"]) if gen else ""),
           "value": n * steps / elapsed, "unit": "PSMs/s",
           "ms_per_step": 1e3 * elapsed / max(steps, 1), "steps": steps, "warmup": warmup,
           "blocks_ms_per_step": [1e3 * b[0] / max(steps, 1) for b in blocks],
           "plan_ms": 1e3 * t_plan, "first_plan_ms": 1e3 * t_first,
           "kernel_ms": {k: float(m) for k, m in zip(FAMILY_NAMES, kern_ms)}, "kernel": FAMILY_NAMES[dom],
           "algorithmic_bytes_per_launch": alg, "achieved": achieved, "frac": achieved / HBM_PEAK_GBS,
           # (a batch of mixed shapes runs its fused family BESIDE the others, on the plan's side stream: the families' own
           # durations then add up to more than the step, and the step itself is the whole path's time)
           "whole_step_frac": alg / (min(float(kern_ms.sum()), 1e3 * elapsed / max(steps, 1)) * 1e-3) / 1e9 / HBM_PEAK_GBS if kern_ms.sum() > 0 else 0.0,
           "families_overlap": bool(float(kern_ms.sum()) > 1.001 * 1e3 * elapsed / max(steps, 1)),
           "peaks_per_spectrum": peaks / float(n),
           "bin_ns_per_peak": 1e6 * float(kern_ms[0]) / max(peaks, 1),
           "signatures_total": plan.total_signatures, "mz_error": st["mz_error"], "fragment_types": st["fragment_types"],
           "max_fragment_charge": int(batch["max_charge"].max()), "neutral_losses": st["neutral_losses"],
           "generate_s": t_gen}
    plan.close()
    del plan, d_mz, d_int, scorer
    torch.cuda.empty_cache()
    return out


def leg_child(args):
    """`bench.py --leg NAME`: one leg in a process of its own, its record as the one JSON line on stdout."""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device; there is no CPU path")
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    out = other_config_leg(torch, torch.device("cuda", local_rank), local_rank, args.leg, args.steps, args.warmup, args.other_blocks,
                           debug=args.debug)
    if args.debug:
        out["debug_switches"] = list(args.debug)
    print(json.dumps(out), flush=True)
    return 0


def run_legs(names, steps, warmup, n_blocks, timeout_s=240.0):
    """Every leg as a CHILD process (`python bench.py --leg NAME`, a fresh process each, started before this program's first
    GPU call and waited for one after the other -- the GPU is theirs alone while they run): a fault, an abort or a hang in an
    extra leg costs that leg's record, never the headline (r05 advisor).  A leg over `timeout_s` is killed with its
    process group."""
    import signal
    import subprocess
    out = {}
    for name in names:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--steps", str(steps), "--warmup", str(warmup),
               "--other-blocks", str(n_blocks)]
        t = time.perf_counter()
        try:
            p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
            try:
                so, se = p.communicate(timeout=timeout_s)
            except subprocess.TimeoutExpired:
                os.killpg(p.pid, signal.SIGKILL)
                p.communicate()
                out[name] = {"error": "timed out after %.0f s" % timeout_s}
                continue
            if p.returncode != 0:
                out[name] = {"error": "exit code %d: %s" % (p.returncode, (se or "").strip().splitlines()[-1:] or "")}
                continue
            out[name] = json.loads(so.strip().splitlines()[-1])
            out[name]["leg_wall_s"] = time.perf_counter() - t
        except Exception as e:
            out[name] = {"error": "%s: %s" % (type(e).__name__, e)}
    return out


def self_launch(n, argv):
    """Starts `python -m torch.distributed.run --nnodes=1 --nproc-per-node n ... bench.py <argv>` as a child process
    on a free port of 127.0.0.1 and returns its exit code (stdout and stderr are inherited: rank 0's JSON line is
    the only thing on stdout)."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on these hosts (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    sys.stdout.flush()
    return subprocess.call(cmd, env=env)


def launcher_dry_run(args, rank, world):
    """PYA_BENCH_BACKEND=gloo: NO scoring and NO measurement -- the launch, the rendezvous, the job's partition, the
    step loop's gathers (shard.StepPipeline over gloo, CPU tensors filled with the rank's PSM indices instead of
    results) and the shape of the line, so that the N > 1 plumbing can be run where there is no GPU
    (tests/test_bench_launch.py).  `value` is null and `data` says so: nothing here is a number."""
    import torch
    import torch.distributed as dist
    from pyascore_amd import shard, synth
    n_per_gpu = args.psms or 1000
    total = world * n_per_gpu if args.scaling == "weak" else (args.total or world * n_per_gpu)
    desc = synth.describe(args.config, n_psm=total, seed=1000)
    weights = shard.work_estimate_shapes(desc["n_sites"], desc["n_mod"], desc["L"], desc["max_charge"],
                                         n_types=len(desc["settings"]["fragment_types"]))
    ranges = shard.partition(weights, world)
    lo, hi = ranges[rank]
    job_max_k = max(1, int(desc["n_mod"].max()))
    width = shard.record_width(job_max_k)
    longest = max(h - l for l, h in ranges)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    sys.stdout.flush()
    real_stdout = os.dup(1)                                 # (the backend's banners go to stderr: one line on stdout)
    os.dup2(2, 1)
    dist.init_process_group(os.environ["PYA_BENCH_BACKEND"], rank=rank, world_size=world)
    ids = torch.arange(lo, hi, dtype=torch.int32).unsqueeze(1).expand(hi - lo, width)
    pipe = shard.StepPipeline(lambda: None, lambda out: out.copy_(ids), hi - lo, longest, width, torch.device("cpu"))
    for _ in range(args.warmup + args.steps):
        pipe.step()
    pipe.drain()
    dist.barrier()
    ok = None
    if rank == 0:
        got = pipe.gathered(ranges)
        ok = bool(got.shape == (total, width) and torch.equal(got[:, 0], torch.arange(total, dtype=torch.int32)))
        os.write(real_stdout, (json.dumps({"metric": METRIC, "value": None, "unit": "PSMs/s", "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": None, "higher_is_better": True, "scaling": args.scaling,
                          "vs_baseline": None, "dtype": "none", "data": "DRY RUN of the launcher and the gather: nothing scored",
                          "config": {"workload": "%s: %d PSMs over %d rank(s)" % (args.config, total, world),
                                     "shard_sizes": [h - l for l, h in ranges]},
                          "multi_gpu": {"rccl_ranks": dist.get_world_size(), "backend": dist.get_backend(),
                                        "gathered_in_input_order": ok, "steps_gathered": pipe.steps}}) + "\n").encode())
    dist.barrier()
    dist.destroy_process_group()
    sys.stdout.flush()
    os.dup2(real_stdout, 1)
    os.close(real_stdout)
    return 0 if ok in (None, True) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50, help="timed steps of every block (--blocks)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--psms", type=int, default=None, help="PSMs per GPU (default: the config's size)")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak: every GPU gets --psms PSMs' worth of work; strong: the job (--total) is fixed")
    ap.add_argument("--total", type=int, default=None, help="PSMs of the whole job with --scaling strong "
                    "(default: the config's size, e.g. 1M for cfg3)")
    ap.add_argument("--max-charge", type=int, default=None,
                    help="override the config's max fragment charge (real 3+/4+ precursors are scored at 2/3)")
    ap.add_argument("--blocks", type=int, default=5,
                    help="timed blocks of --steps steps each (every block bracketed by barrier + synchronize); the line "
                         "reports the MEDIAN block, and every block's ms per step beside it")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline, everything else this program measures, in runs of their own: the CPU baseline, "
                         "`other_configs`, `host_api`, the device's copy rate and the committed counters of `roofline` "
                         "(about a minute more); the --no-... options below leave one of them out again")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without `cpu_baseline`")
    ap.add_argument("--debug", action="append", default=[], metavar="KEY=VALUE",
                    help="A/B experiments: a debug switch of the scorer (include/pyascore_debug.h), e.g. --debug PYA_NO_FUSED=1; "
                         "the line then carries `debug_switches` and is not the headline")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="--full without the short timed legs of BASELINE's other configs (`other_configs` in the line, "
                         "N = 1, default cfg2 run only)")
    ap.add_argument("--other-blocks", type=int, default=2, help="timed blocks per config of `other_configs`")
    ap.add_argument("--leg", choices=sorted(LEGS), default=None,
                    help="(internal) run ONE leg of `other_configs` in this process and print its record")
    ap.add_argument("--no-host-api", action="store_true",
                    help="--full without the host-array legs (`host_api`)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, rank 0 writes the results of the LAST timed step (what the timed path hands "
                         "its caller: best_score, n_sig, best_sig, ascores, alt_mask of every PSM of the job) as DIR/<name>.npy "
                         "in float32 / float64, at most 64 MB in all; the job is seeded, so two runs with the same arguments "
                         "score the same inputs")
    args = ap.parse_args()
    if args.dump_outputs and args.steps < 1:
        ap.error("--dump-outputs needs a timed step (--steps >= 1)")

    if args.leg:
        return leg_child(args)
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` as written: this process becomes the launcher.  The ranks are CHILDREN
        # (one per GPU under torch.distributed.run), started before anything here touched the GPU; their one
        # JSON line passes through this process's stdout and their exit code is this one's.
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d (launch with torch.distributed.run)" % (args.gpus, world))
    if os.environ.get("PYA_BENCH_BACKEND", "nccl") != "nccl":
        if args.dump_outputs:
            raise SystemExit("--dump-outputs: the dry run scores nothing")
        return launcher_dry_run(args, rank, world)

    # ---- CPU only up to the marked line: the job, this rank's shard, and the CPU baseline's worker
    # processes all come before the first call that initialises the GPU ----
    from pyascore_amd import shard, synth
    # ONE job description (per-PSM shapes only) that every rank derives from the same seed; the job is
    # cut into contiguous ranges balanced by C(n,k) x (L-1) x types x charges (shard.partition) and
    # every rank generates the spectra of its own range only.
    n_per_gpu = args.psms or synth.CONFIGS[args.config]["n_psm"]
    if args.config == "cfg3" and args.psms is None:
        n_per_gpu = synth.CONFIGS["cfg3"]["n_psm"] // 8      # the config is quoted on 8 GPUs
    if args.scaling == "strong":
        total = args.total or (world * args.psms if args.psms else synth.CONFIGS[args.config]["n_psm"])
    else:
        total = world * n_per_gpu
    over = {} if args.max_charge is None else {"max_charge": args.max_charge}
    desc = synth.describe(args.config, n_psm=total, seed=1000, **over)
    settings = desc["settings"]
    weights = shard.work_estimate_shapes(desc["n_sites"], desc["n_mod"], desc["L"], desc["max_charge"],
                                         n_types=len(settings["fragment_types"]))
    ranges = shard.partition(weights, world)
    lo, hi = ranges[rank]
    batch = synth.make_slice(desc, lo, hi)
    job_max_k = max(1, int(desc["n_mod"].max()))
    longest = max(h - l for l, h in ranges)
    cpu = None
    if args.full and world == 1 and rank == 0 and not args.no_cpu_baseline:
        cpu = cpu_baseline(batch, settings)
    default_size = args.psms is None and args.max_charge is None and args.scaling == "weak" and not args.debug
    others = None
    if args.full and world == 1 and default_size and args.config == "cfg2" and not args.no_other_configs:
        # BASELINE's other workloads and the dense-spectrum legs on this GPU, so that the driver's record carries every
        # config: child processes, one after the other, BEFORE this process touches the GPU.  The headline fields are
        # cfg2's and only cfg2's.
        others = run_legs(["cfg3", "cfg4", "cfg5", "dense1500", "dense4000"], args.steps, args.warmup, args.other_blocks)
    # ---- GPU from here on ----
    import torch
    import torch.distributed as dist
    from pyascore_amd import PyAscore
    from pyascore_amd.device import DevicePlan

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device; there is no CPU path")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # PYA_BENCH_FORCE_DIST=1 runs the collective path with a world of one (the only way to exercise
    # RCCL on a single-GPU box)
    use_dist = world > 1 or bool(os.environ.get("PYA_BENCH_FORCE_DIST"))
    real_stdout = None
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        # RCCL prints a version banner through C stdio on rank 0; stdout carries ONE JSON line and nothing
        # else, so the C-level stdout is pointed at stderr while the process group lives
        sys.stdout.flush()
        real_stdout = os.dup(1)
        os.dup2(2, 1)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    scorer = PyAscore(settings["bin_size"], settings["n_top"], settings["mod_group"], settings["mod_mass"],
                      settings["mz_error"], settings["fragment_types"], device=local_rank)
    for g, m in settings["neutral_losses"]:
        scorer.add_neutral_loss(g, m)
    for kv in args.debug:
        scorer.set_debug(*kv.split("=", 1))

    d_mz = torch.from_numpy(batch["mz"]).to(dev)
    d_int = torch.from_numpy(batch["intensity"]).to(dev)
    torch.cuda.synchronize()
    t_plan = time.perf_counter()
    DevicePlan(scorer, batch, timing=True, max_k=job_max_k).close()     # the scorer's FIRST plan: + its score and order tables
    first_plan_ms = 1e3 * (time.perf_counter() - t_plan)
    t_plan = time.perf_counter()
    plan = DevicePlan(scorer, batch, timing=True, max_k=job_max_k)      # pya_plan_create: host pre-pass + arena upload
    plan_ms = 1e3 * (time.perf_counter() - t_plan)

    # the step loop lives in pyascore_amd.shard (the gloo test drives the same class on CPU): kernels of
    # this rank's shard, then the step's single RCCL gather of the packed records, asynchronous, waited
    # for one step later
    pipe = shard.StepPipeline(lambda: plan.run(d_mz, d_int), lambda out: plan.packed_summary(out=out), hi - lo, longest,
                              shard.record_width(job_max_k), dev, enabled=use_dist)

    for _ in range(args.warmup):
        pipe.step()
    pipe.drain()
    plan.check()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    # A timed block = EXACTLY --steps steps between barrier + synchronize on both sides.  One block of a 0.6 ms step is
    # 30 ms of wall time, which a clock ramp or a noisy neighbour can move by 10 %: several blocks are timed, the
    # median one is the line's value, all of them are listed.
    blocks = timed_blocks(torch, dist if use_dist else None, dev, pipe, plan, args.steps, args.blocks)
    plan.check()
    order = sorted(range(len(blocks)), key=lambda i: blocks[i][0])
    elapsed, elapsed_own, kern_ms, gather_wait_s = blocks[order[len(order) // 2]]
    block_ms = [1e3 * b[0] / max(args.steps, 1) for b in blocks]
    if args.dump_outputs and rank == 0:
        # (read before anything else runs on the device: the last block's last step, whose gather has landed)
        if use_dist:
            from pyascore_amd.device import unpack_summary
            res = unpack_summary(pipe.gathered(ranges).cpu().numpy(), job_max_k)
        else:
            res = {k: getattr(plan, k).cpu().numpy() for k in ("best_score", "n_sig", "best_sig", "ascores", "alt_mask")}
        dump_outputs(args.dump_outputs, res)

    per_rank = None
    if use_dist:
        # what every rank measured, so that the first real scaling run explains itself: per-rank kernel
        # family times, time spent waiting for gathers, own wall time, shard size and work estimate
        mine = torch.tensor(list(kern_ms) + [1e3 * gather_wait_s / max(args.steps, 1), 1e3 * elapsed_own / max(args.steps, 1),
                                             float(hi - lo), float(weights[lo:hi].sum())], dtype=torch.float64, device=dev)
        allr = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [[float(x) for x in r.tolist()] for r in allr]

    if rank == 0:
        names = FAMILY_NAMES
        dom = int(np.argmax(kern_ms))
        alg = algorithmic_bytes(batch, plan.max_k)
        achieved = alg / (kern_ms[dom] * 1e-3) / 1e9 if kern_ms[dom] > 0 else 0.0
        # host API rate (host arrays in -> host results out; PCIe and host pre-pass included)
        host = None
        if args.full and not args.no_host_api:
            scorer.score_batch(batch)                          # first call allocates the workspace (reused afterwards)
            host_s = []
            for _ in range(3):
                t = time.perf_counter()
                res = scorer.score_batch(batch)
                host_s.append(time.perf_counter() - t)
            host_rate = batch["n_psm"] / min(host_s)
            # what PCIe alone costs this entry point: the same host arrays up (16 bytes per peak, pageable
            # memory as a caller holds it) and the result arrays back, nothing else
            pcie_s = []
            d_res = {k: torch.from_numpy(v).to(dev) for k, v in res.items()}
            for _ in range(3):
                torch.cuda.synchronize()
                t = time.perf_counter()
                a = torch.from_numpy(batch["mz"]).to(dev)
                b2 = torch.from_numpy(batch["intensity"]).to(dev)
                back = [v.cpu() for v in d_res.values()]
                torch.cuda.synchronize()
                pcie_s.append(time.perf_counter() - t)
                del a, b2, back
            pcie_bytes = batch["mz"].nbytes + batch["intensity"].nbytes + sum(v.nbytes for v in res.values())
            host = {"value": host_rate, "unit": "PSMs/s", "ms": 1e3 * min(host_s),
                    "pcie_only_ms": 1e3 * min(pcie_s), "pcie_gbs": pcie_bytes / min(pcie_s) / 1e9,
                    "frac_of_pcie": min(pcie_s) / min(host_s),
                    "note": "PyAscore.score_batch: host arrays in, host results out (chunked, upload pipelined "
                            "with planning, kernels and result copies); pcie_only = the same bytes copied up "
                            "and back with nothing else"}
        # (a plain run launches nothing beside its steps and reads no counters: those keys of `roofline` are null)
        copy_gbs = achievable_hbm_gbs(torch, dev) if args.full else None
        counters, fams = (profiled_counters(args.config, kern_ms, names, default_size, scorer._lib.pya_version().decode())
                          if args.full else (None, None))
        dom_c = (fams or {}).get(names[dom], {})
        traffic_path = counters["whole_path_traffic"] if counters else None
        line = {
            "metric": METRIC, "value": total * args.steps / elapsed, "unit": "PSMs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / max(args.steps, 1), "higher_is_better": True,
            "blocks": {"n": len(block_ms), "ms_per_step": block_ms, "min": min(block_ms), "max": max(block_ms),
                       "note": "every block is exactly `steps` steps between barrier + synchronize; value / ms_per_step / "
                               "kernel_ms are the median block's"},
            # what the timed region leaves out (r05 verdict item 3): the plan's host pre-pass (letter scan, routing, tables,
            # arena upload: pya_plan_create, once per batch) -- and PCIe, which `host_api` prices
            "plan_ms": plan_ms, "first_plan_ms": first_plan_ms,
            "scaling": args.scaling, "vs_baseline": None, "dtype": "f32/f64 scalar + i32 counts",
            "data": "synthetic (SURVEY.md 8(d) generator, job seed 1000, spectra per 16k-PSM block)",
            "config": {"workload": "%s: %d PSMs over %d GPU(s), work-balanced contiguous shards" % (args.config, total, world),
                       "psms_total": total, "psms_rank0": batch["n_psm"], "shard_sizes": [h - l for l, h in ranges], "peaks_per_spectrum": float(batch["peak_off"][-1]) / batch["n_psm"],
                       "signatures_total_per_gpu": plan.total_signatures, "mz_error": settings["mz_error"],
                       "fragment_types": settings["fragment_types"],
                       "max_fragment_charge": int(batch["max_charge"].max()),
                       "neutral_losses": settings["neutral_losses"],
                       "timed_region": "spectra resident in HBM, plan pre-built (`plan_ms`, once per batch, is NOT inside), kernels only%s; "
                                       "results stay on the device (host arrays in -> host results out is `host_api`)"
                                       % (" + the step's gather of fixed-size records to rank 0" if use_dist else ""),
                       "parallelism": ("psm-shard x%d + 1 gather per step" % world) if use_dist else "1 GPU, no collective"},
            "roofline": {"bound": "hbm", "kernel": names[dom], "achieved": achieved, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": dom_c.get("traffic"),
                         # the same bytes over ALL the step's kernels (binning reads 98 % of them, not the dominant kernel)
                         # (families that overlap -- a mixed batch's fused family on the plan's side stream -- add up to more
                         # than the step: the step is then the whole path's time)
                         "whole_step_frac": (alg / (min(float(kern_ms.sum()), 1e3 * elapsed / max(args.steps, 1)) * 1e-3) / 1e9 / HBM_PEAK_GBS) if kern_ms.sum() > 0 else 0.0,
                         "families_overlap": bool(float(kern_ms.sum()) > 1.001 * 1e3 * elapsed / max(args.steps, 1)),
                         "traffic_source": counters["source"] if counters and counters.get("families") is not None else None,
                         "traffic_refused": counters.get("refused") if counters else (
                             "no committed counters for this config" if args.full else "the committed counters are read with --full"),
                         # HBM bytes the dominant kernel family really moved (counters) over its live duration
                         "hbm_actual": dom_c.get("hbm_actual"),
                         # what actually bounds the kernel: share of SIMD time its vector instructions need at the
                         # issue rates measured for its own instruction mix (profiles/r03_valu_ceiling.md)
                         "valu_busy": dom_c.get("valu_busy"), "valu_cycles_per_inst": dom_c.get("valu_cycles_per_inst"),
                         "salu_busy": dom_c.get("salu_busy"),
                         # HBM bytes of the whole path per step (every kernel) next to the algorithmic bytes
                         "traffic_whole_path": traffic_path,
                         "traffic_over_algorithmic": (traffic_path / alg) if traffic_path else None,
                         "algorithmic_bytes_per_launch": alg,
                         "achievable_peak": copy_gbs, "frac_of_achievable": achieved / copy_gbs if copy_gbs else None,
                         "whole_path_gbs": alg / (min(float(kern_ms.sum()), 1e3 * elapsed / max(args.steps, 1)) * 1e-3) / 1e9 if kern_ms.sum() > 0 else 0.0,
                         "kernel_ms": {n: float(m) for n, m in zip(names, kern_ms)},
                         "per_kernel": fams},
            "host_api": host,
            "workspace_bytes": plan.workspace_bytes,
        }
        if per_rank is not None:
            cols = names + ["gather_wait_ms", "wall_ms_per_step", "shard_psms", "work_estimate"]
            line["multi_gpu"] = {"rccl_ranks": dist.get_world_size(), "backend": dist.get_backend(),
                                 "columns": cols, "per_rank": per_rank,
                                 "record_bytes_per_step": longest * shard.record_width(job_max_k) * 4 * world,
                                 "note": "per rank: mean HIP-event ms of each kernel family per step, ms per step spent "
                                         "waiting for the previous step's gather, own wall ms per step, shard size, "
                                         "sum of the work estimate the partition balanced"}
        if args.debug:
            line["debug_switches"] = list(args.debug)
        if cpu is not None:
            line["cpu_baseline"] = cpu
        if others is not None:
            line["other_configs"] = others
        if real_stdout is not None:
            os.write(real_stdout, (json.dumps(line) + "\n").encode())
        else:
            print(json.dumps(line), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
        import ctypes
        ctypes.CDLL(None).fflush(None)                     # whatever the libraries buffered goes to stderr too
        sys.stdout.flush()
        os.dup2(real_stdout, 1)
        os.close(real_stdout)


if __name__ == "__main__":
    main()
