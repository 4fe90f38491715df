"""Shared spectra on the GPU: several PSMs scored against ONE uploaded, once-binned copy of a spectrum (pya_score_batch_shared /
pya_plan_create_shared; the hits of a scan in the reference's command line, `pyascore/__main__.py` groupby(psms, scan) /
hit_depth).  The binning of a spectrum depends on its peaks and the scorer's two scalars alone (cpp/Spectra.cpp:43-68), so
the yardstick everywhere is the SAME PSMs with the spectrum repeated (synth.expand_shared_batch) through the entry point
that existed before: every result must be bit-equal -- on every scoring / localize family, every binning kernel, whatever the
cut into chunks, with retained records, on a device-resident plan and through the command line's packing.  A sample of every
batch is also checked against the reference's own C++ core, as in the other GPU tests."""
import ctypes as C

import numpy as np
import pytest

import switches
from conftest import checker_kind
from oracle import orc, harness, par_check
from pyascore_amd import _lib, batch_cli, synth

pytestmark = pytest.mark.gpu

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")
ROUTE_VARS = ("PYA_NO_FUSED", "PYA_NO_CNT", "PYA_NO_BIG", "PYA_NO_LOC_HASH", "PYA_NO_PLAIN", "PYA_PLAIN_MIN", "PYA_NO_FORK",
              "PYA_DEBUG", "PYA_BIN_SELECT_MIN", "PYA_BIN_SELECT_SCAP", "PYA_CHUNK_MB", "PYA_NO_CHUNKS")


def _gpu(settings):
    from pyascore_amd import PyAscore
    return harness.make_scorer(PyAscore, settings)


def _same(got, want, what, keys=KEYS):
    for key in keys:
        assert got[key].shape == want[key].shape, "%s: %s has another shape" % (what, key)
        bad = np.flatnonzero(np.any(np.atleast_2d((got[key] != want[key]).T), axis=0))
        assert bad.size == 0, "%s: %s differs for PSMs %s" % (what, key, bad[:10])


def _psm(batch, i):
    """PSM i of a CSR batch as a pack_batch dict (peaks included)."""
    kw = synth.unpack_psm(batch, i)
    a, b = int(batch["aux_off"][i]), int(batch["aux_off"][i + 1])
    return dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=int(kw["n_of_mod"]),
                max_charge=int(batch["max_charge"][i]), aux_pos=batch["aux_pos"][a:b].copy(), aux_mass=batch["aux_mass"][a:b].copy())


def _share(base, sizes, vary=True):
    """The PSMs of `base` in order, cut into groups of the given sizes; a group is scored against the spectrum of its first
    PSM (the others are lower-ranked hits: other peptides, and -- with `vary` -- another n_of_mod, one more fragment charge, an
    n-terminal fixed modification on some of them)."""
    spectra, psms, i = [], [], 0
    for s, g in enumerate(sizes):
        first = _psm(base, i % base["n_psm"])
        spectra.append(dict(mz=first["mz"], intensity=first["intensity"]))
        for j in range(g):
            p = _psm(base, (i + j) % base["n_psm"])
            p = dict(peptide=p["peptide"], n_of_mod=p["n_of_mod"], max_charge=p["max_charge"], aux_pos=p["aux_pos"],
                     aux_mass=p["aux_mass"], spectrum=s)
            if vary and j % 3 == 2:
                p["n_of_mod"] = 1 + p["n_of_mod"] % 2
            if vary and j % 4 == 3:
                p["max_charge"] += 1
            if vary and j % 5 == 4 and not (p["aux_pos"] == 0).any():
                p["aux_pos"] = np.concatenate([[0], p["aux_pos"]]).astype(np.uint32)
                p["aux_mass"] = np.concatenate([[42.010565], p["aux_mass"]]).astype(np.float32)
            psms.append(p)
        i += g
    return synth.pack_shared_batch(spectra, psms)


def _sizes(n_spec, seed, big=200):
    rng = np.random.default_rng(seed)
    sizes = rng.choice([1, 1, 2, 3, 5, 8], size=n_spec).tolist()
    sizes[n_spec // 2] = big
    return sizes


def _check_against_reference(settings, expanded, got, n=48, keys=KEYS):
    """the first n PSMs (and the last n) of the expanded batch through the reference's own C++ core"""
    total = expanded["n_psm"]
    for lo in sorted({0, max(0, total - n)}):
        hi = min(total, lo + n)
        sub = synth.slice_batch(expanded, lo, hi)
        sub = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in sub.items()}
        k = got["ascores"].shape[1]
        want = par_check.score_batch_parallel(settings, sub, k, kind=checker_kind())
        for key in keys:
            assert np.array_equal(got[key][lo:hi], want[key]), "%s differs from the reference for PSMs %d..%d" % (key, lo, hi)


CASES = {      # the PSMs the groups are drawn from, and the number of spectra they share
    "cfg2": (lambda: synth.make_batch("cfg2", n_psm=1200, seed=501), 330),
    "cfg3": (lambda: synth.make_batch("cfg3", n_psm=900, seed=502), 220),
    "cfg4": (lambda: synth.make_batch("cfg4", n_psm=420, seed=503), 60),
    "cfg5": (lambda: synth.make_batch("cfg5", n_psm=330, seed=504), 40),
    "realistic": (lambda: synth.make_realistic(420, seed=505), 60),
    "realistic_plain": (lambda: synth.make_realistic(600, seed=506, general=False), 110),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_shared_batches_equal_the_repeated_spectrum_batches(name):
    make, n_spec = CASES[name]
    base, settings = make()
    shared = _share(base, _sizes(n_spec, seed=len(name)))
    assert shared["n_spectra"] == n_spec and shared["n_psm"] > 2 * n_spec
    expanded = synth.expand_shared_batch(shared)
    gpu = _gpu(settings)
    want = gpu.score_batch(expanded)
    got = gpu.score_batch(shared)
    _same(got, want, name)
    assert (got["n_sig"] > 0).sum() > shared["n_psm"] // 2              # (scored, not set aside)
    _check_against_reference(settings, expanded, got)


ROUTES = {
    "no_fused": ("cfg2", {"PYA_NO_FUSED": "1", "PYA_PLAIN_MIN": "0"}),
    "general_localize_lists": ("cfg2", {"PYA_NO_PLAIN": "1", "PYA_NO_LOC_HASH": "1"}),
    "no_count_nodes": ("cfg3", {"PYA_NO_CNT": "1", "PYA_PLAIN_MIN": "0"}),
    "no_count_nodes_general": ("cfg4", {"PYA_NO_CNT": "1"}),
    "no_big": ("cfg5", {"PYA_NO_BIG": "1", "PYA_PLAIN_MIN": "0"}),
    "big_records": ("cfg5", {"PYA_NO_BIG_INLINE": "1", "PYA_PLAIN_MIN": "0"}),
    "hash_off": ("cfg4", {"PYA_NO_LOC_HASH": "1"}),
    "no_fork": ("cfg3", {"PYA_NO_FORK": "1", "PYA_PLAIN_MIN": "0"}),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_kernel_family_reads_a_shared_table(route, monkeypatch):
    cfg, env = ROUTES[route]
    for v in ROUTE_VARS + ("PYA_NO_BIG_INLINE",):
        monkeypatch.delenv(v, raising=False)
    base, settings = synth.make_batch(cfg, n_psm=260, seed=600 + len(route))
    shared = _share(base, _sizes(50, seed=len(route), big=40), vary=(cfg != "cfg5"))
    expanded = synth.expand_shared_batch(shared)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gpu = _gpu(settings)                                   # (takes the switches named in the environment: conftest)
    _same(gpu.score_batch(shared), gpu.score_batch(expanded), route)
    for k in env:
        monkeypatch.delenv(k)
    plain = _gpu(settings)
    _same(gpu.score_batch(shared), plain.score_batch(expanded), route + " against the production route")


def test_general_kernel_and_long_peptides_on_shared_spectra():
    """n_top 16 sends every PSM through the general kernel; a 70-residue peptide (general kernel) shares its spectrum with a
    12-mer (fast kernels) under n_top 10."""
    base, settings = synth.make_batch("cfg2", n_psm=60, seed=77)
    shared = _share(base, [1, 4, 2, 7, 1, 3, 5, 2])
    expanded = synth.expand_shared_batch(shared)
    s16 = dict(settings, n_top=16)
    gpu = _gpu(s16)
    got = gpu.score_batch(shared)
    _same(got, gpu.score_batch(expanded), "n_top 16")
    _check_against_reference(s16, expanded, got, n=12)
    rng = np.random.default_rng(3)
    first = _psm(base, 0)
    long_pep = "".join(rng.choice(list("AGLVKEDPR"), 70))
    long_pep = long_pep[:20] + "S" + long_pep[21:40] + "T" + long_pep[41:60] + "Y" + long_pep[61:]
    spectra = [dict(mz=first["mz"], intensity=first["intensity"])]
    psms = [dict(spectrum=0, peptide="AGSLTKPEYLDR", n_of_mod=1, max_charge=1),
            dict(spectrum=0, peptide=long_pep, n_of_mod=1, max_charge=1),
            dict(spectrum=0, peptide=first["peptide"], n_of_mod=first["n_of_mod"], max_charge=2),
            dict(spectrum=0, peptide=long_pep[5:], n_of_mod=2, max_charge=1)]
    mixed = synth.pack_shared_batch(spectra, psms)
    gpu = _gpu(settings)
    got = gpu.score_batch(mixed)
    ex = synth.expand_shared_batch(mixed)
    _same(got, gpu.score_batch(ex), "long peptide beside a 12-mer")
    assert got["n_sig"].tolist() == [3, 3, got["n_sig"][2], 3]
    # (the checker's batch form packs alternative sites into residue masks: not for more than 64 residues)
    _check_against_reference(settings, ex, got, n=4, keys=("best_score", "n_sig", "ascores"))


def _dense_spectrum(rng, psm, P, mode="sorted"):
    mz = np.concatenate([psm["mz"], rng.uniform(100.0, 2500.0, P - psm["mz"].size)])
    it = np.concatenate([psm["intensity"], rng.lognormal(4.0, 1.0, P - psm["intensity"].size)])
    o = np.argsort(mz, kind="stable")
    mz, it = mz[o], it[o]
    if mode == "counts":                                   # equal intensities inside a window: the fast kernel declines
        it = np.floor(it / np.median(it) * 5.0) + 1.0
    if mode == "shuffled":                                 # peaks out of m/z order: the same
        q = rng.permutation(P)
        mz, it = mz[q], it[q]
    return dict(mz=mz, intensity=it)


def test_every_binning_kernel_bins_a_shared_spectrum(monkeypatch):
    """sparse (bin_fast), ~1 500 and ~4 000 peaks (bin_select), more than 8 192 (the global kernel, general scoring), equal
    intensities and unsorted peaks (declined, redone by the exact kernel) -- each shared by three or more PSMs; then every
    spectrum through the exact kernel (PYA_DEBUG=128), selection forced on every class, and selection with too few slots."""
    for v in ROUTE_VARS:
        monkeypatch.delenv(v, raising=False)
    rng = np.random.default_rng(41)
    base, settings = synth.make_batch("cfg2", n_psm=40, seed=41)
    kinds = [(None, "sorted"), (1500, "sorted"), (4000, "sorted"), (9000, "sorted"), (1500, "counts"), (300, "counts"),
             (400, "shuffled"), (12000, "counts"), (None, "sorted"), (4000, "counts")]
    spectra, psms = [], []
    for s, (P, mode) in enumerate(kinds):
        first = _psm(base, 4 * s)
        spectra.append(dict(mz=first["mz"], intensity=first["intensity"]) if P is None else _dense_spectrum(rng, first, max(P, first["mz"].size + 1), mode))
        for j in range(3 + s % 2):
            p = _psm(base, (4 * s + j) % base["n_psm"])
            psms.append(dict(spectrum=s, peptide=p["peptide"], n_of_mod=p["n_of_mod"], max_charge=1 + (j == 2)))
    shared = synth.pack_shared_batch(spectra, psms)
    expanded = synth.expand_shared_batch(shared)
    gpu = _gpu(settings)
    want = gpu.score_batch(expanded)
    got = gpu.score_batch(shared)
    _same(got, want, "production binning")
    assert (got["n_sig"] > 0).all()
    _check_against_reference(settings, expanded, got, n=expanded["n_psm"])
    for label, env in (("exact", {"PYA_DEBUG": "128"}), ("select_forced", {"PYA_BIN_SELECT_MIN": "0"}),
                       ("select_overflow", {"PYA_BIN_SELECT_MIN": "0", "PYA_BIN_SELECT_SCAP": "64"}),
                       ("all_pairs", {"PYA_BIN_SELECT_MIN": "1000000"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        switches.from_env(gpu)
        _same(gpu.score_batch(shared), want, label)
        for k in env:
            monkeypatch.delenv(k)
    switches.from_env(gpu)


def test_what_belongs_to_the_spectrum_hits_its_psms_and_nothing_else():
    base, settings = synth.make_batch("cfg2", n_psm=30, seed=9)
    spectra = [dict(mz=_psm(base, i)["mz"], intensity=_psm(base, i)["intensity"]) for i in range(4)]
    spectra.insert(1, dict(mz=np.array([500.0]), intensity=np.array([1.0])))                    # one multiple of 100: no windows
    spectra.insert(3, dict(mz=np.zeros(0), intensity=np.zeros(0)))                              # empty
    spectra.append(dict(mz=np.array([321.5, 400.25]), intensity=np.array([3.0, 4.0])))         # nobody refers to this one
    peps = [_psm(base, i) for i in range(12)]
    spec_of = [0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 4, 5, 5]
    psms = [dict(spectrum=s, peptide=peps[i % 12]["peptide"], n_of_mod=peps[i % 12]["n_of_mod"], max_charge=1) for i, s in enumerate(spec_of)]
    bad = 6                                                                                     # the middle PSM of spectrum 2's group
    psms[bad]["peptide"] = psms[bad]["peptide"][:3] + "X" + psms[bad]["peptide"][4:]
    shared = synth.pack_shared_batch(spectra, psms)
    assert shared["n_spectra"] == 7
    expanded = synth.expand_shared_batch(shared)
    gpu = _gpu(settings)
    want = gpu.score_batch(expanded, skip_invalid=True)
    got = gpu.score_batch(shared, skip_invalid=True)
    _same(got, want, "set-aside PSMs", KEYS + ("status",))
    assert got["status"].tolist() == [0, 0, 1, 1, 1, 0, 16, 0, 16, 16, 0, 0, 0]
    assert got["status_message"] == want["status_message"] and "PSM 6" in got["status_message"]
    assert np.all(got["best_score"][[2, 3, 4, 6, 8, 9]] == -1.0) and np.all(got["n_sig"][[5, 7]] > 0)
    for b in (shared, expanded):                                                                # without the flag both calls fail alike
        with pytest.raises(ValueError, match="PSM 6: unknown residue"):
            gpu.score_batch(b)
    # only the spectrum-side trouble left: the same PSM is named by both
    psms[bad]["peptide"] = peps[bad]["peptide"]
    shared = synth.pack_shared_batch(spectra, psms)
    messages = []
    for b in (shared, synth.expand_shared_batch(shared)):
        with pytest.raises(ValueError) as err:
            gpu.score_batch(b)
        messages.append(str(err.value))
    assert messages[0] == messages[1] and messages[0].startswith("PSM 8: empty spectrum")
    # the arguments themselves, through the C ABI: PYA_ERR_ARG and the PSM's number
    ok = synth.pack_shared_batch(spectra[:1], psms[:2])
    for spec, n_spec, who in (([1, 0], 2, 1), ([0, 2], 2, 1), ([0, 0], 0, 0)):
        with pytest.raises(ValueError, match="PSM %d" % who):
            _raw_shared(gpu, ok, np.array(spec, np.uint32), n_spec)
        assert gpu._lib.pya_error_index(gpu._h) == who


def _raw_shared(gpu, batch, spec_of, n_spectra):
    """pya_score_batch_shared as a C caller would call it (PyAscore.score_batch sorts and checks before it gets there)"""
    n = batch["n_psm"]
    peak_off = np.zeros(max(n_spectra, 2) + 1, np.int64)
    peak_off[1:] = batch["peak_off"][-1]                   # spectrum 0 has the peaks, the rest are empty: never read here
    arrs = [peak_off] + [np.ascontiguousarray(batch[k]) for k in ("pep", "pep_off", "n_of_mod", "max_charge", "aux_pos", "aux_mass", "aux_off")]
    b = _lib.Batch(n, *[a.ctypes.data_as(C.c_void_p) for a in arrs])
    out = dict(best_score=np.zeros(n, np.float32), best_sig=np.zeros(n, np.uint64), n_sig=np.zeros(n, np.int32),
               ascores=np.zeros((n, 4), np.float32), alt_mask=np.zeros((n, 4), np.uint64))
    r = _lib.Results(4, *[out[k].ctypes.data_as(C.c_void_p) for k in ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")])
    rc = gpu._lib.pya_score_batch_shared(gpu._h, C.byref(b), spec_of.ctypes.data_as(C.c_void_p), n_spectra,
                                         batch["mz"].ctypes.data_as(C.c_void_p), batch["intensity"].ctypes.data_as(C.c_void_p), 0, C.byref(r))
    assert rc in (0, _lib.PYA_ERR_ARG)
    if rc:
        gpu._raise(rc)
    return out


def test_chunked_shared_calls_equal_one_plan(monkeypatch):
    """pya_score_batch_shared cuts at spectrum groups, uploads every spectrum of a chunk once and counts it once; a group
    bigger than a chunk is cut and its spectrum travels with both parts.  Results do not depend on the cut."""
    for v in ROUTE_VARS:
        monkeypatch.delenv(v, raising=False)
    desc = synth.describe("cfg2", 9000, seed=31)
    base, settings = synth.make_slice(desc), desc["settings"]
    sizes = _sizes(9000, seed=8, big=30000)                # ~47 MB of spectra once, 55 000 PSMs on them; one group of 30 000
    rng = np.random.default_rng(5)
    pick = rng.integers(0, base["n_psm"], sum(sizes))      # (peptides drawn from the 9 000, vectorised packing)
    spec_of = np.repeat(np.arange(9000), sizes).astype(np.uint32)
    shared = synth.take_psms(dict(base, spec_of=np.arange(9000, dtype=np.uint32), n_spectra=9000), pick)
    shared["spec_of"] = spec_of
    assert shared["n_psm"] == sum(sizes) and shared["mz"].size * 16 > (32 << 20)
    gpu = _gpu(settings)
    monkeypatch.setenv("PYA_NO_CHUNKS", "1")
    switches.from_env(gpu)
    one = gpu.score_batch(shared)
    monkeypatch.delenv("PYA_NO_CHUNKS")
    switches.from_env(gpu)
    sample = np.concatenate([np.arange(0, 2000), np.flatnonzero(spec_of == 4500)[:2000], np.arange(shared["n_psm"] - 2000, shared["n_psm"])])
    ex = synth.expand_shared_batch(synth.take_psms(shared, sample))
    want = gpu.score_batch(ex)
    for key in KEYS:
        assert np.array_equal(one[key][sample], want[key]), key
    gpu.set_workspace_budget(16 << 20)                     # the group of 30 000 alone needs more: cut inside the group
    _same(gpu.score_batch(shared), one, "16 MB budget")
    gpu.set_workspace_budget(0)
    monkeypatch.setenv("PYA_CHUNK_MB", "9")                # five or six chunks by the spectra's bytes
    switches.from_env(gpu)
    _same(gpu.score_batch(shared), one, "9 MB chunks")
    bad = dict(shared, pep=shared["pep"].copy())
    where = 40_123
    bad["pep"][shared["pep_off"][where] + 1] = ord("X")
    with pytest.raises(ValueError, match="PSM %d: unknown residue" % where):
        gpu.score_batch(bad)
    got = gpu.score_batch(bad, skip_invalid=True)
    assert np.flatnonzero(got["status"]).tolist() == [where]
    keep = np.arange(shared["n_psm"]) != where
    for key in KEYS:
        assert np.array_equal(got[key][keep], one[key][keep]), key
    monkeypatch.delenv("PYA_CHUNK_MB")
    switches.from_env(gpu)


def test_a_batch_in_any_order_comes_back_in_input_order():
    base, settings = synth.make_batch("cfg3", n_psm=300, seed=12)
    shared = _share(base, _sizes(60, seed=2, big=30))
    order = np.random.default_rng(7).permutation(shared["n_psm"])
    shuffled = synth.take_psms(shared, order)
    assert np.any(np.diff(shuffled["spec_of"].astype(np.int64)) < 0)
    gpu = _gpu(settings)
    want = gpu.score_batch(synth.expand_shared_batch(shuffled))
    got = gpu.score_batch(shuffled)
    _same(got, want, "shuffled")
    in_order = gpu.score_batch(shared)
    for key in KEYS:
        assert np.array_equal(got[key], in_order[key][order]), key
    # a set-aside PSM keeps its place and its number
    bad = dict(shuffled, pep=shuffled["pep"].copy())
    bad["pep"][bad["pep_off"][17]] = ord("X")
    res = gpu.score_batch(bad, skip_invalid=True)
    assert np.flatnonzero(res["status"]).tolist() == [17] and res["status_message"].startswith("PSM 17:")
    with pytest.raises(ValueError, match="^PSM 17: unknown residue"):
        gpu.score_batch(bad)
    # with retained records such a batch is scored in its expanded form: records by the caller's PSM numbers
    kept = gpu.score_batch(shuffled, keep=True)
    _same(kept, want, "shuffled, keep")
    rec = gpu.batch_pep_scores(5, 9)
    gpu.score_batch(synth.expand_shared_batch(shuffled), keep=True)
    ref = gpu.batch_pep_scores(5, 9)
    for key in rec:
        assert np.array_equal(rec[key], ref[key]), key


def _ambiguity(gpu, psm, rec, a, b):
    """pya_calculate_ambiguity of records a and b of PSM `psm` of the retained batch (rec: its batch_pep_scores)"""
    o = int(rec["rec_off"][0])
    ra, rb = int(rec["rec_off"][-2]) - o + a, int(rec["rec_off"][-2]) - o + b
    out = C.c_float()
    sa, sb = np.ascontiguousarray(rec["scores"][ra]), np.ascontiguousarray(rec["scores"][rb])
    rc = gpu._lib.pya_calculate_ambiguity(gpu._h, psm, int(rec["sig_bits"][ra]), sa.ctypes.data_as(C.c_void_p), float(rec["weighted_score"][ra]),
                                          int(rec["sig_bits"][rb]), sb.ctypes.data_as(C.c_void_p), float(rec["weighted_score"][rb]), C.byref(out))
    if rc:
        gpu._raise(rc)
    return out.value


def test_retained_records_of_a_shared_batch():
    base, settings = synth.make_batch("cfg3", n_psm=120, seed=21)
    sizes = [1, 3, 6, 2, 1, 8, 4]
    shared = _share(base, sizes, vary=False)
    expanded = synth.expand_shared_batch(shared)
    lo, hi = 1 + 3, 1 + 3 + 6                              # the group of six
    gpu = _gpu(settings)
    plain = gpu.score_batch(expanded)
    _same(gpu.score_batch(shared, keep=True), plain, "keep")
    got = gpu.batch_pep_scores(lo, hi, batch=shared)
    assert np.diff(got["rec_off"]).min() > 1
    amb = [_ambiguity(gpu, hi - 1, got, 0, 1), _ambiguity(gpu, hi - 1, got, 1, 0)]
    whole = gpu.batch_pep_scores()
    gpu.score_batch(expanded, keep=True)
    want = gpu.batch_pep_scores(lo, hi, batch=expanded)
    for key in want:
        assert np.array_equal(got[key], want[key]), key
    assert amb == [_ambiguity(gpu, hi - 1, want, 0, 1), _ambiguity(gpu, hi - 1, want, 1, 0)] and np.isfinite(amb[0])
    whole2 = gpu.batch_pep_scores()
    for key in whole2:
        assert np.array_equal(whole[key], whole2[key]), key
    # a retained batch beyond the budget: scored shared, its records re-scored on demand in expanded form
    gpu.set_workspace_budget(16 << 20)
    big, _ = synth.make_batch("cfg3", n_psm=4000, seed=22)
    shared = _share(big, [8] * 500, vary=False)
    res = gpu.score_batch(shared, keep=True)
    assert gpu._lazy_batch is not None and "spec_of" not in gpu._lazy_batch
    lazy = gpu.batch_pep_scores(1000, 1040)
    gpu.set_workspace_budget(0)
    gpu.score_batch(synth.expand_shared_batch(shared), keep=True)
    full = gpu.batch_pep_scores(1000, 1040)
    for key in full:
        assert np.array_equal(lazy[key], full[key]), key
    assert res["n_sig"][1000:1040].sum() == int(lazy["rec_off"][-1])


def test_device_resident_plan_on_shared_spectra():
    import torch
    from pyascore_amd.device import DevicePlan
    base, settings = synth.make_batch("cfg2", n_psm=4000, seed=61)
    shared = _share(base, [4] * 1000, vary=False)
    expanded = synth.expand_shared_batch(shared)
    gpu = _gpu(settings)
    dev = torch.device("cuda", gpu.device)
    results = {}
    for name, b in (("shared", shared), ("expanded", expanded)):
        plan = DevicePlan(_gpu(settings), b, timing=True)      # (a scorer of its own: no recycled allocation behind workspace_bytes)
        mz, it = torch.from_numpy(b["mz"]).to(dev), torch.from_numpy(b["intensity"]).to(dev)
        runs = []
        for _ in range(2):                                 # back to back: the second run sees the first one's workspace
            plan.run(mz, it)
            plan.check()
            runs.append({k: getattr(plan, k).cpu().numpy().copy() for k in KEYS})
        for key in KEYS:
            assert np.array_equal(runs[0][key], runs[1][key]), (name, key)
        ms = plan.timings_ms()
        assert ms[0] > 0.0 and all(t >= 0.0 for t in ms)
        results[name] = (runs[1], plan.workspace_bytes)
        plan.close()
    for key in KEYS:
        assert np.array_equal(results["shared"][0][key], results["expanded"][0][key]), key
    saved = results["expanded"][1] - results["shared"][1]
    tables = 8 * (expanded["mz"].size - shared["mz"].size)              # 8 bytes per retained-table slot not held
    assert saved >= tables * 0.9, (saved, tables)
    host = gpu.score_batch(expanded)
    assert np.array_equal(results["shared"][0]["best_score"], host["best_score"])
    assert np.array_equal(results["shared"][0]["best_sig"].view(np.uint64), host["best_sig"])


def test_the_command_line_packs_the_hits_of_a_scan_on_one_spectrum():
    """batch_cli.localize(hit_depth=2): the rows of the per-PSM loop over the checker (the construction of
    tests/test_batch_cli.py), from a batch that holds every scan's peaks once."""
    from test_batch_cli import PHOSPHO, _toy_inputs
    from pyascore_amd import PyAscore
    spectra, psms = _toy_inputs()
    picked, scans = batch_cli.select_psms(psms, spectra, "STY", PHOSPHO, 2, 3)
    packed = batch_cli.pack_hits(picked, scans)
    assert packed["n_spectra"] == len(set(scans)) < packed["n_psm"] == len(picked)
    assert packed["mz"].size == sum(spectra[s]["mz_values"].size for s in sorted(set(scans)))
    gpu = PyAscore(100.0, 10, "STY", PHOSPHO, 0.05, "by")
    rows = batch_cli.localize(gpu, psms, spectra, "STY", PHOSPHO, hit_depth=2, max_fragment_charge=3)
    chk = orc.OracleAscore(100.0, 10, "STY", PHOSPHO, 0.05, "by", kind=checker_kind())
    want = []
    for match in psms:
        spectrum = spectra[match["scan"]]
        cpos, cmass, nvar = batch_cli.process_mods("STY", PHOSPHO, match["peptide"], match["mod_positions"], match["mod_masses"])
        if nvar > 0:
            chk.score(spectrum["mz_values"], spectrum["intensity_values"], match["peptide"], nvar,
                      min(3, batch_cli.psm_charge(match, spectrum) - 1), cpos, cmass)
            want.append([match["scan"], chk.best_sequence, chk.best_score, ";".join(str(s) for s in chk.ascores),
                         ";".join(",".join(str(s) for s in alt) for alt in chk.alt_sites)])
    assert rows == want
    unshared = gpu.score_batch(synth.pack_batch(picked), skip_invalid=True)
    _same(gpu.score_batch(packed, skip_invalid=True), unshared, "pack_hits", KEYS + ("status",))
