"""Coverage records on the GPU (pya_coverage: how much of its spectrum the reported localisation of a PSM explains).
Yardstick: pyascore_amd.rollup.coverage fed with the section-1 ion records of tests/coverage_ref.py (parts pinned to the
reference) for the winners the run reports -- every comparison is on the raw bytes of the 64-byte records."""
import ctypes as C

import numpy as np
import pytest

import coverage_ref
import strip_cases as sc
from oracle import harness
from pyascore_amd import _lib, rollup as ru, synth

pytestmark = pytest.mark.gpu

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")


def _gpu(settings):
    from pyascore_amd import PyAscore
    return harness.make_scorer(PyAscore, settings)


def _same_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == ru.COVERAGE_DTYPE and got.shape == want.shape, what
    bad = [i for i in range(got.size) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, "%s: %d records differ, first PSM %d: got %r, want %r" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])


def _want(settings, batch, res):
    """the restatement over the yardstick's section 1, for the winners of ``res``, on the arrays of ``batch``"""
    flat = synth.expand_shared_batch(batch) if batch.get("spec_of") is not None else batch
    off, ions, yard, kept = coverage_ref.batch_records(settings, flat, res, synth.unpack_psm)
    scored = res["n_sig"] > 0
    if "status" in res:
        scored = scored & (res["status"] == 0)
    fwd = "".join(c for c in settings["fragment_types"] if c in "bc")
    want = ru.coverage(off, ions, batch["mz"], batch["intensity"], batch["peak_off"], np.diff(batch["pep_off"]), fwd, scored,
                       spec_of=batch.get("spec_of"), n_retained=kept)
    _same_bytes(want, yard, "restatement against the yardstick")
    return want


def _against_yardstick(settings, batch, what, scored_all=True, **kw):
    gpu = _gpu(settings)
    plain = gpu.score_batch(batch, **kw)
    got = gpu.score_batch(batch, coverage=True, **kw)
    for key in KEYS + (("status",) if "status" in plain else ()):                # the flag changes nothing of the run
        assert got[key].tobytes() == plain[key].tobytes(), (what, key)
    want = _want(settings, batch, got)
    _same_bytes(got["coverage"], want, what)
    if scored_all:
        assert (want["kind"] == 1).all() and (want["n_fragments"] > 0).all() and (want["n_explained"] > 0).all(), what
    return got, want


@pytest.mark.parametrize("cfg,n,kw", [("cfg2", 64, {}), ("cfg4", 32, {}), ("cfg5", 8, {})])
def test_routes(cfg, n, kw):
    """plain, general (charges, a loss, four ion types) and many site assignments"""
    batch, settings = synth.make_batch(cfg, n_psm=n, seed=8100, **kw)
    got, want = _against_yardstick(settings, batch, cfg)
    if cfg == "cfg4":
        assert (want["nterm_sizes"] > 0).all() and (want["cterm_sizes"] > 0).all()


def _with_peak_count(kw, k, rng):
    """PSM ``kw`` with a spectrum of k peaks: k of its own spread over its range, or its own and noise on top"""
    mz, it = np.asarray(kw["mz_arr"], np.float64), np.asarray(kw["int_arr"], np.float64)
    if k <= mz.size:
        take = np.unique(np.round(np.linspace(0, mz.size - 1, k)).astype(np.int64))
        assert take.size == k
        mz, it = mz[take], it[take]
    else:
        extra = rng.uniform(100.0, 2000.0, size=k - mz.size)
        mz = np.concatenate([mz, extra])
        it = np.concatenate([it, rng.lognormal(4.5, 1.0, size=extra.size)])
        order = np.argsort(mz, kind="stable")
        mz, it = mz[order], it[order]
    return dict(mz=mz, intensity=it, peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=kw["max_fragment_charge"])


def test_peak_counts_at_the_lane_stride_edges():
    """1, 63, 64, 65, 128 and 129 raw peaks, and 8 193: a spectrum beyond the fast limit (the general list)"""
    base, settings = synth.make_batch("cfg2", n_psm=7, seed=8200)
    rng = np.random.default_rng(8201)
    counts = (1, 63, 64, 65, 128, 129, 8193)
    batch = synth.pack_batch([_with_peak_count(synth.unpack_psm(base, i), k, rng) for i, k in enumerate(counts)])
    assert tuple(np.diff(batch["peak_off"])) == counts
    got, want = _against_yardstick(settings, batch, "peak counts", scored_all=False, skip_invalid=True)
    assert (got["status"][1:] == 0).all() and (want["kind"][1:] == 1).all() and (want["n_explained"][1:] > 0).all()
    assert want["n_peaks"].tolist() == [k if s else 0 for k, s in zip(counts, want["kind"])]


def test_peptide_lengths():
    """two residues (one bond), 64 and 65 residues (the last of the fast route, the first of the general one)"""
    few, settings = synth.make_batch("cfg2", n_psm=1, seed=8300)
    kw = synth.unpack_psm(few, 0)
    # b1 of S + phospho (168.006), y1 of K (147.113): peaks near both, and noise
    mz = np.sort(np.concatenate([[147.113, 168.006, 88.04, 227.08], np.linspace(100.0, 400.0, 40)]))
    psms = [dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=1),
            dict(mz=mz, intensity=np.linspace(10.0, 500.0, mz.size), peptide="SK", n_of_mod=1, max_charge=1)]
    got, want = _against_yardstick(settings, synth.pack_batch(psms), "two residues")
    assert want["bonds"][1] == 1 and want["nterm_sizes"][1] == 1 and want["cterm_sizes"][1] == 1
    for L in (64, 65):
        batch, settings = synth.make_batch("cfg2", n_psm=3, seed=8301 + L, L=L, n_sites=5, n_mod=2)
        got, want = _against_yardstick(settings, batch, "%d residues" % L)
        assert (want["bonds"] > 8).all() and (want["bonds"] <= L - 1).all()


def test_a_spectrum_out_of_m_over_z_order():
    batch, settings = synth.make_batch("cfg2", n_psm=4, seed=8400)
    a, b = int(batch["peak_off"][2]), int(batch["peak_off"][3])
    mz, it = batch["mz"].copy(), batch["intensity"].copy()
    mz[a:b], it[a:b] = mz[a:b][::-1].copy(), it[a:b][::-1].copy()
    moved = dict(batch, mz=mz, intensity=it)
    got, want = _against_yardstick(settings, moved, "reversed spectrum")
    same, _ = _against_yardstick(settings, batch, "in order")
    for f in ru.COVERAGE_DTYPE.names:                                            # the order of the raw peaks moves the sums only
        if not f.endswith("_current"):
            assert np.array_equal(got["coverage"][f], same["coverage"][f]), f


@pytest.mark.parametrize("types", [(np.float64, np.float64), (np.float64, np.float32), (np.float32, np.float32)])
def test_type_pairs(types):
    base, settings = synth.make_batch("cfg2", n_psm=16, seed=8500)
    _against_yardstick(settings, synth.narrow_batch(base, *types), "%s / %s" % tuple(np.dtype(t).name for t in types))


def test_shared_spectra_in_and_out_of_order():
    base, settings = synth.make_batch("cfg2", n_psm=20, seed=8600)
    spectra, psms = [], []
    for i in range(0, 20, 5):
        kw = synth.unpack_psm(base, i)
        spectra.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"]))
        for j in range(5):
            kj = synth.unpack_psm(base, i + j)
            psms.append(dict(peptide=kj["peptide"], n_of_mod=kj["n_of_mod"], max_charge=1, aux_pos=np.zeros(0, np.uint32),
                             aux_mass=np.zeros(0, np.float32), spectrum=len(spectra) - 1))
    for order, what in ((np.arange(20), "shared"), (np.random.default_rng(3).permutation(20), "shuffled shared")):
        shared = synth.pack_shared_batch(spectra, [psms[p] for p in order])
        got, want = _against_yardstick(settings, shared, what, scored_all=False)
        assert (want["kind"] == 1).all() and want["n_explained"][np.asarray(order) % 5 == 0].all()   # (the spectrum's own peptide)


def test_psms_that_are_set_aside_have_all_zero_records():
    base, settings = synth.make_batch("cfg2", n_psm=6, seed=8700)
    psms = []
    for i in range(6):
        kw = synth.unpack_psm(base, i)
        psms.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=1))
    psms[1]["peptide"] = psms[1]["peptide"][:3] + "X" + psms[1]["peptide"][4:]   # an unknown residue
    psms[4]["n_of_mod"] = 7                                                      # more modifications than modifiable residues
    got, want = _against_yardstick(settings, synth.pack_batch(psms), "set aside", scored_all=False, skip_invalid=True)
    assert got["status"][1] != 0 and got["n_sig"][4] <= 0
    for i in (1, 4):
        assert got["coverage"][i].tobytes() == bytes(64), i
    assert (got["coverage"]["kind"][[0, 2, 3, 5]] == 1).all()


def test_chunks_by_the_workspace_budget_equal_the_uncut_call():
    big = synth.make_slice(synth.describe("cfg2", 12_000, seed=8800))
    settings = synth.describe("cfg2", 1, seed=8800)["settings"]
    gpu = _gpu(settings)
    whole = gpu.score_batch(big, coverage=True)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) == 1
    gpu.set_workspace_budget(32 << 20)
    cut = gpu.score_batch(big, coverage=True)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) >= 3
    gpu.set_workspace_budget(0)
    for key in KEYS:
        assert cut[key].tobytes() == whole[key].tobytes(), key
    _same_bytes(cut["coverage"], whole["coverage"], "chunked by the budget")
    assert (whole["coverage"]["kind"] == 1).all() and (whole["coverage"]["n_explained"] > 0).all()
    part = synth.slice_batch(big, 4_000, 4_008)                                  # ... and a few of them against the yardstick
    res = {k: whole[k][4_000:4_008] for k in KEYS}
    _same_bytes(whole["coverage"][4_000:4_008], _want(settings, part, res), "a slice of the big batch")


def test_recalibrated_and_stripped_spectra_are_what_is_covered():
    batch, settings = synth.make_batch("cfg2", n_psm=16, seed=5, mz_error=0.05)
    gpu = _gpu(settings)
    cal = np.zeros(1, ru.MZ_CALIBRATION_DTYPE)
    cal["ppm"][0] = np.linspace(30.0, -10.0, ru.MZP_BANDS)
    got = gpu.score_batch(batch, recalibrate=dict(calibration=cal), coverage=True)
    moved = dict(batch, mz=ru.recalibrate(batch["mz"], batch["peak_off"], None, cal))
    assert moved["mz"].tobytes() != batch["mz"].tobytes()
    _same_bytes(got["coverage"], _want(settings, moved, got), "recalibrated")
    dirty, prec_mz, prec_z = sc.with_precursors(batch, 0.05)
    got = gpu.score_batch(dirty, strip=dict(precursor_mz=prec_mz, precursor_charge=prec_z, tol=0.05, losses=(sc.LOSS_H3PO4, sc.LOSS_WATER),
                                            isotopes=1), coverage=True)
    clean = gpu.score_batch(batch, coverage=True)
    _same_bytes(got["coverage"], _want(settings, batch, got), "stripped")
    _same_bytes(got["coverage"], clean["coverage"], "stripped against clean")
    planted = gpu.score_batch(dirty, coverage=True)["coverage"]
    assert ru.coverage_ratios(planted)["explained"].mean() < ru.coverage_ratios(clean["coverage"])["explained"].mean()


def test_device_plan_and_refusals():
    import torch
    from pyascore_amd.device import DevicePlan, coverage_records
    batch, settings = synth.make_batch("cfg2", n_psm=40, seed=8900)
    gpu = _gpu(settings)
    lib = gpu._lib
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.zeros(40, ru.COVERAGE_DTYPE)
    assert lib.pya_last_batch_coverage(None, vp(out), 40) == _lib.PYA_ERR_ARG
    assert lib.pya_last_batch_coverage(gpu._h, vp(out), 40) == _lib.PYA_ERR_STATE and b"PYA_FLAG_COVERAGE" in lib.pya_last_error(gpu._h)
    gpu.score_batch(batch)
    assert lib.pya_last_batch_coverage(gpu._h, vp(out), 40) == _lib.PYA_ERR_STATE
    res = gpu.score_batch(batch, coverage=True)
    want = _want(settings, batch, res)
    _same_bytes(res["coverage"], want, "batch")
    assert lib.pya_last_batch_coverage(gpu._h, vp(out), 40) == 0 and out.tobytes() == want.tobytes()
    assert lib.pya_last_batch_coverage(gpu._h, vp(out), 39) == _lib.PYA_ERR_ARG
    assert lib.pya_last_batch_coverage(gpu._h, None, 40) == _lib.PYA_ERR_ARG
    dev = torch.device("cuda", 0)
    d_mz, d_it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    plan = DevicePlan(gpu, batch, coverage=True)
    guard = torch.full((40, 64), 0x5A, dtype=torch.uint8, device=dev)
    sp = _lib.TypedSpectra(d_mz.data_ptr(), d_it.data_ptr(), _lib.PYA_F64, _lib.PYA_F64)
    call = lambda pl, o, s=sp: lib.pya_plan_coverage(pl._plan, C.byref(pl._res), None if s is None else C.byref(s), None, o)  # noqa: E731
    assert call(plan, guard.data_ptr()) == _lib.PYA_ERR_STATE                   # before the first run
    plan.run(d_mz, d_it)
    assert call(plan, None) == _lib.PYA_ERR_ARG
    assert call(plan, guard.data_ptr(), None) == _lib.PYA_ERR_ARG
    assert lib.pya_plan_coverage(None, None, None, None, None) == _lib.PYA_ERR_ARG
    bad = _lib.TypedSpectra(d_mz.data_ptr(), d_it.data_ptr(), _lib.PYA_F32, _lib.PYA_F64)
    assert call(plan, guard.data_ptr(), bad) == _lib.PYA_ERR_ARG
    torch.cuda.synchronize()
    assert (guard.cpu().numpy() == 0x5A).all()                                   # nothing was launched
    first = plan.coverage(d_mz, d_it)
    second = plan.coverage(d_mz, d_it, out=guard)
    plan.check()
    _same_bytes(coverage_records(first.cpu().numpy()), want, "plan")
    _same_bytes(coverage_records(second.cpu().numpy()), want, "plan, twice")
    plan.run(d_mz, d_it)
    _same_bytes(coverage_records(plan.coverage(d_mz, d_it).cpu().numpy()), want, "plan, after a second run")
    few = synth.slice_batch(batch, 0, 5)                                         # a handful of PSMs: created with the flag
    p5 = DevicePlan(gpu, few, coverage=True)
    m5, i5 = torch.from_numpy(np.ascontiguousarray(few["mz"])).to(dev), torch.from_numpy(np.ascontiguousarray(few["intensity"])).to(dev)
    p5.run(m5, i5)
    _same_bytes(coverage_records(p5.coverage(m5, i5).cpu().numpy()), want[:5], "plan of five")
    one = synth.slice_batch(batch, 7, 8)                                         # a batch of one takes the plan's launches
    _same_bytes(gpu.score_batch(one, coverage=True)["coverage"], want[7:8], "batch of one")
    kw = synth.unpack_psm(batch, 3)                                              # ... and so does the property after score()
    gpu.score(**kw)
    assert gpu.coverage.tobytes() == want[3].tobytes()
    with pytest.raises(ValueError):
        plan.coverage(d_mz, d_it, out=guard[:-1])


def test_beside_the_other_stages():
    batch, settings = synth.make_batch("cfg3", n_psm=60, seed=8950)
    gpu = _gpu(settings)
    stages = dict(evidence=True, ions=True, sites=True, probs=True, ranked=5, mz_profile={})
    plain = gpu.score_batch(batch, **stages)
    got = gpu.score_batch(batch, coverage=True, **stages)
    for key in KEYS + ("evidence", "ion_off", "ions", "site_off", "sites", "site_probs", "psm_probs", "ranked", "mz_profile"):
        assert got[key].tobytes() == plain[key].tobytes(), key
    assert set(got) == set(plain) | {"coverage"}
    # the library's own section 1 gives the same records as the yardstick's
    fwd = "".join(c for c in settings["fragment_types"] if c in "bc")
    want = _want(settings, batch, got)
    own = ru.coverage(got["ion_off"], got["ions"], batch["mz"], batch["intensity"], batch["peak_off"], np.diff(batch["pep_off"]), fwd,
                      got["n_sig"] > 0, n_retained=want["n_retained"])
    _same_bytes(got["coverage"], want, "beside the other stages")
    _same_bytes(own, want, "from the library's ion records")


def test_command_line_file(tmp_path):
    import os
    from pyascore_amd import PyAscore, __main__ as cli, batch_cli, ingest
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ingest")
    out, cov = tmp_path / "ascores.tsv", tmp_path / "coverage.tsv"
    spec, ident = os.path.join(data, "test_spectra.mzML"), os.path.join(data, "test_psms.pep.xml")
    rows = cli.run(cli.parse_args(["--mz_error", "0.05", "--hit_depth", "2", "--coverage", str(cov), spec, ident, str(out)]), log=lambda *_: None)
    plain = cli.run(cli.parse_args(["--mz_error", "0.05", "--hit_depth", "2", spec, ident, str(tmp_path / "plain.tsv")]), log=lambda *_: None)
    assert rows == plain                                                         # the main table is unchanged
    gpu = PyAscore(100.0, 10, "STY", 79.966331, 0.05, "by")
    spectra = ingest.SpectraParser(spec, "mzML", native_precision=True).to_dict()
    psms = sorted(ingest.IdentificationParser(ident, "pepXML").to_list(), key=lambda p: p["scan"])
    picked, scans = batch_cli.select_psms(psms, spectra, "STY", 79.966331, 2, 5)
    res = gpu.score_batch(batch_cli.pack_hits(picked, scans), skip_invalid=True, coverage=True)
    ratios = ru.coverage_ratios(res["coverage"])
    lines = cov.read_text().splitlines()
    assert lines[0].split("\t") == list(batch_cli.COVERAGE_COLUMNS) and len(lines) == 1 + len(picked)
    assert (res["coverage"]["kind"] == 1).any() and (res["coverage"]["n_explained"] > 0).any()
    hit = 0
    for i, line in enumerate(lines[1:]):
        hit = hit + 1 if i and scans[i] == scans[i - 1] else 1
        want = [str(scans[i]), str(hit)] + batch_cli.coverage_fields(res["coverage"][i], {k: v[i] for k, v in ratios.items()})
        assert line.split("\t") == want, i
        assert float(want[4]) == res["coverage"]["explained_current"][i] and float(want[16]) == ratios["explained"][i]   # (repr round-trips)
