"""Inputs for the peptidoform quantification tests (host and GPU): seeded channel matrices, record sets made directly,
synthetic pairs for the reduce calls, batches whose peptides repeat, and the coverage conditions every test asserts of its
own input -- checked with the yardsticks (tests/peptidoforms_ref.py, tests/peptidoform_quant_ref.py) alone."""
import struct

import numpy as np

import peptidoform_lists as pl
import peptidoforms_ref
import probs_ref
from pyascore_amd import _lib, synth

NAN, INF = float("nan"), float("inf")
SCORED, NONE, OVER = _lib.PYA_SITE_SCORED, _lib.PYA_SITE_NONE, _lib.PYA_SITE_OVER
HEAD, CELL = np.dtype(_lib.SITE_QUANT_HEAD_DTYPE), np.dtype(_lib.SITE_QUANT_DTYPE)
SCALE = 10


def same(got, want, what):
    """list, head and cell of two pairs as raw bytes"""
    for g, w, name in zip(got, want, ("list", "head", "cell")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            at = tuple(bad[0]) if len(bad) else ()
            raise AssertionError("%s: %d %s records differ, first %s: got %s, want %s" % (what, len(bad), name, at, g[at], w[at]))


def matrix(seed, n_rows, n_ch, wide=False):
    """a seeded matrix with NaNs, zeros and negatives among its readings, a few rows without a gap; wide: readings that
    saturate as well"""
    rng = np.random.default_rng(seed)
    v = rng.random((n_rows, n_ch)) * 10.0 ** rng.integers(0, 7, (n_rows, n_ch))
    kind = rng.random((n_rows, n_ch))
    kind[rng.random(n_rows) < 0.3] = 1.0
    v[kind < 0.06] = NAN
    v[(kind >= 0.06) & (kind < 0.11)] = 0.0
    v[(kind >= 0.11) & (kind < 0.13)] = -1.0
    if wide:
        v[(kind >= 0.13) & (kind < 0.15)] = INF
        v[(kind >= 0.15) & (kind < 0.17)] = 1e300
        v[(kind >= 0.17) & (kind < 0.19)] = -0.0
    return v


def repeats(batch, share=3):
    """the batch with the peptides of its first n / share PSMs repeated against the spectra of the others"""
    n = int(batch["n_psm"])
    m = max(1, n // share)
    kws = [synth.unpack_psm(batch, i) for i in range(n)]
    psms = [dict(mz=kws[i]["mz_arr"], intensity=kws[i]["int_arr"], peptide=kws[i % m]["peptide"], n_of_mod=kws[i % m]["n_of_mod"],
                 max_charge=kws[i % m]["max_fragment_charge"]) for i in range(n)]
    return synth.pack_batch(psms), [p["peptide"] for p in psms]


def peptides(batch):
    return [synth.unpack_psm(batch, i)["peptide"] for i in range(int(batch["n_psm"]))]


def records(seed, n_psm, n_groups=40, max_k=3):
    """a random record set made directly, with everything the rule names: unscored PSMs, negative groups, best_sig 0, equal
    keys in many PSMs, probabilities on and beside a threshold of 0.5"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 7, n_psm)
    site_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n_rec = int(site_off[-1])
    psm_probs = np.zeros(n_psm, probs_ref.PSM_DTYPE)
    psm_probs["kind"] = rng.choice([SCORED, SCORED, SCORED, SCORED, SCORED, NONE, OVER], n_psm)
    psm_probs["z"] = 1.0 + rng.integers(0, 16, n_psm) / 8.0
    site_probs = np.zeros(n_rec, probs_ref.SITE_DTYPE)
    site_probs["with_prob"] = rng.choice([0.0, 1.0, 0.5, np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0)], n_rec)
    mix = rng.random(n_rec) < 0.7
    site_probs["with_prob"][mix] = rng.random(int(mix.sum()))
    group = rng.integers(-1, n_groups, n_psm).astype(np.int32)
    best_sig = np.zeros(n_psm, np.uint64)
    for i in range(n_psm):                                     # few site assignments per group, so that keys repeat
        c = int(counts[i])
        if c:
            k = int(min(c, max_k, 1 + (int(group[i]) + i) % 2))
            first = (int(group[i]) * 7 + int(rng.integers(0, 2))) % c
            best_sig[i] = sum(1 << ((first + j) % c) for j in range(k))
    ascores = (rng.random((n_psm, max_k)) * 60.0 - 5.0).astype(np.float32)
    ascores[rng.random((n_psm, max_k)) < 0.05] = np.inf
    return dict(site_probs=site_probs, psm_probs=psm_probs, site_off=site_off, best_sig=best_sig, ascores=ascores, group=group)


def take(r, psms):
    """the record set of the PSMs `psms`, in that order"""
    psms = np.asarray(psms, np.int64)
    n_rec = np.diff(r["site_off"])[psms]
    off = np.concatenate([[0], np.cumsum(n_rec)]).astype(np.int64)
    at = np.repeat(r["site_off"][:-1][psms] - off[:-1], n_rec) + np.arange(int(n_rec.sum()))
    return dict(site_probs=r["site_probs"][at], psm_probs=r["psm_probs"][psms], site_off=off, best_sig=r["best_sig"][psms],
                ascores=r["ascores"][psms], group=r["group"][psms])


def min_probs(r, group):
    """(PSM, min_prob) of the PSMs that contribute to the list, by the list's yardstick"""
    n = len(r["best_sig"])
    entries = peptidoforms_ref.psm_entries(r["best_sig"], r["ascores"], r["site_off"], r["site_probs"], r["psm_probs"], group, 0.0,
                                           psm_id=list(range(n)))
    return [(e[4], struct.unpack("<d", struct.pack("<Q", e[5]))[0], (e[0], e[1])) for e in entries]


def threshold(r, group, row=None, n_rows=None):
    """The quant threshold of a test: the median min_prob of the PSMs that contribute to the list.  Asserts the coverage
    conditions: between a quarter and three quarters of them are at or above it, at least one key has three or more PSMs that
    contribute to the table, at least one group has two isomers."""
    mp = min_probs(r, group)
    assert mp, "no PSM contributes to the list"
    thr = float(np.median([p for _, p, _ in mp]))
    share = sum(1 for _, p, _ in mp if p >= thr) / len(mp)
    assert 0.25 <= share <= 0.75, "%.3f of the list's PSMs contribute at the median %r" % (share, thr)
    per_key, isomers = {}, {}
    for i, p, key in mp:
        isomers.setdefault(key[0], set()).add(key[1])
        rw = i if row is None else int(row[i])
        if p >= thr and rw >= 0 and (n_rows is None or rw < n_rows):
            per_key[key] = per_key.get(key, 0) + 1
    assert max(per_key.values()) >= 3, "no key has three contributing PSMs"
    assert max(len(s) for s in isomers.values()) >= 2, "no group has two isomers"
    return thr


def synthetic_pair(n, kind, n_ch, seed=0, table=True):
    """a pair made directly for the reduce calls: peptidoform_lists' records (any order, repeated keys, n_psm == 0 among them)
    and a random table row-aligned with them"""
    records = pl.make(n, kind, seed)
    if not table:
        return records, None, None
    rng = np.random.default_rng([seed, n, n_ch, 77])
    head, cell = np.zeros(n, HEAD), np.zeros((n, n_ch), CELL)
    head["n_records"] = rng.integers(0, 9, n)
    head["n_complete"] = rng.integers(0, 9, n) % (head["n_records"] + 1)
    cell["n"] = rng.integers(0, 9, (n, n_ch))
    cell["n_saturated"] = rng.integers(0, 3, (n, n_ch)) % (cell["n"] + 1)
    cell["sum"] = rng.integers(0, 1 << 50, (n, n_ch)).astype(np.uint64) * (cell["n"] != 0)
    return records, head, cell


# ---- the inputs of tests/test_gpu_peptidoform_quant.py that assert the coverage conditions; tests/test_peptidoform_quant_host.py
# confirms the conditions for every one of them on the CPU through the reference core ----
GOLDEN_SHARE = 4
# the edge goldens hold 13 PSMs; repeated with GOLDEN_SHARE every one of their listed PSMs has min_prob exactly 1.0 (a spectrum
# that decides its sites completely), so the median is 1.0, everything is at or above it and "a quarter to three quarters"
# cannot hold; edge_nKc is the one whose probabilities spread
EDGE_WITHOUT_SPREAD = ("edge_Zc", "edge_default", "edge_err05", "edge_highres", "edge_nl", "edge_yb")


def shared_inputs(tol=0.05):
    """20 planted cfg2 spectra (seed 9850) with three PSMs each, the peptides of the first twelve PSMs in turn: (settings, spectra,
    psms, precursor m/z, precursor charge) for synth.pack_shared_batch"""
    import markers_cases as mc
    base, settings = synth.make_batch("cfg2", n_psm=60, seed=9850)
    planted, pm, pz, _ = mc.with_markers(base, tol)
    spectra, psms = [], []
    for i in range(0, 60, 3):
        kw = synth.unpack_psm(planted, i)
        spectra.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"]))
        for j in range(3):
            kj = synth.unpack_psm(planted, (i + j) % 12)
            psms.append(dict(peptide=kj["peptide"], n_of_mod=kj["n_of_mod"], max_charge=1, aux_pos=np.zeros(0, np.uint32),
                             aux_mass=np.zeros(0, np.float32), spectrum=len(spectra) - 1))
    return settings, spectra, psms, pm[::3].copy(), pz[::3].copy()


SHARED_ORDERS = (("shared", np.arange(60)), ("shuffled shared", np.random.default_rng(3).permutation(60)))
CHUNKED_ROWS = 2000


def chunked_inputs():
    """7 000 cfg2 PSMs (seed 9860; 34 MiB of spectra, the smallest batch the library cuts into chunks), every peptide five
    times: (settings, batch, peptides, row) with fewer rows than PSMs and some PSMs without one"""
    big = synth.make_slice(synth.describe("cfg2", 7000, seed=9860))
    settings = synth.describe("cfg2", 1, seed=9860)["settings"]
    big, names = repeats(big, share=5)
    return settings, big, names, (np.arange(7000) % (CHUNKED_ROWS + 1) - 1).astype(np.int32)
