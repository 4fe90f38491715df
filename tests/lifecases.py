"""One scorer's life: a pool of SMALL batches under one settings dict, and sequences of calls drawn from it.

Almost every GPU test makes a fresh scorer, does one thing with it and drops it; a caller keeps one handle for a whole job.
The handle is stateful -- its device tables grow and MOVE (the score table in ``ensure_lut``, the signature order tables in
``shape_offset`` / ``upload_shared_tables``), its workspaces, pinned blocks, retained batch and report words are reused from
call to call -- and the tests of tests/test_gpu_scorer_life.py drive that state on purpose.  This module holds what they share
and what tests/test_scorer_life_host.py checks about it without a GPU: the pool (every entry says what it is for), the
sequences of steps, and ``expected_growth``: whether a call must make the handle's tables grow, by arithmetic from the
constants of csrc/common.h and csrc/host_tables.cpp, not from the library.

The settings are cfg2's (b/y, 0.05, STY, no neutral loss); cfg3 and cfg5 generate under the same ones.
"""
import math

import numpy as np

from pyascore_amd import synth
from pyascore_amd.shard import count_sites

LUT_FLOOR = 128                 # host_tables.cpp ensure_lut: std::max<uint32_t>(n_max, 128)
NODE_SHAPE_MAX = 64             # host_tables.cpp shape_offset: shapes of at most 64 signatures carry a shared-node table
N_TYPES, N_UNIQ = 2, 1          # b and y; no neutral loss: one loss sum (0)
CHUNK_MIN_BYTES = 32 << 20      # host_batch.cpp kChunkMin: spectra bytes below which a batch call is never cut into chunks
SMALL_BUDGET = 16 << 20         # the smallest budget pya_set_workspace_budget takes
LOSS = ("STY", 97.9769)         # the settings change of the refusal tests
FLAGS = ("evidence", "ions", "sites", "probs", "ranked", "coverage", "keep", "skip_invalid")
SEEDS, N_STEPS = (0, 1, 2), 40

_, SETTINGS = synth.make_batch("cfg2", n_psm=1, seed=0)


def _psms(batch):
    """the PSMs of a private CSR batch as the dicts ``synth.pack_batch`` takes"""
    out = []
    for i in range(int(batch["n_psm"])):
        kw = synth.unpack_psm(batch, i)
        out.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"],
                        max_charge=kw["max_fragment_charge"]))
    return out


def _fixed(seed, n, **shape):
    batch, settings = synth.make_batch("cfg2", n_psm=n, seed=seed, **shape)
    assert settings == SETTINGS
    return batch


def shapes(batch):
    """the (n_sites, n_of_mod) of every PSM, as a list of pairs"""
    return list(zip(count_sites(batch, SETTINGS["mod_group"]).tolist(), np.asarray(batch["n_of_mod"]).tolist()))


def _a_small():
    return _fixed(7100, 64)                                    # cfg2's own shape: 20-mers, 6 sites, 3 mods, charge 1


def _b_shapes():
    cfg3, settings = synth.make_batch("cfg3", n_psm=130, seed=7101)
    assert settings == SETTINGS
    psms = [p for p, sh in zip(_psms(cfg3), shapes(cfg3)) if sh != (6, 3)]
    cfg5, settings = synth.make_batch("cfg5", n_psm=3, seed=7102)          # 15 choose 5 = 3 003 order entries at once
    assert settings == SETTINGS
    return synth.pack_batch(psms + _psms(cfg5))


def _b_lut():
    # The score table is built on the host in time cubic in its rows (score_table.cpp: 0.8 s for 944 rows, 7 s for 2 000,
    # 54 s for the 4 032 of a PSM at the top of the table, as tests/test_gpu_parity.py builds one -- measured on one core).
    # Every fresh scorer of the sequence test that meets this entry builds it again, so the PSM that makes the growth LARGE
    # stops at 50 x 6 x 2 = 600 rows: 0.2 s, 7 MB against the 0.07 MB of the 128-row floor, a new allocation a hundred times
    # the old one.
    return synth.pack_batch(_psms(_fixed(7103, 4, L=40, n_sites=5, n_mod=2, max_charge=3)) +
                            _psms(_fixed(7104, 1, L=51, n_sites=4, n_mod=2, max_charge=6)))


def _general():
    long_pep = _psms(_fixed(7105, 1, L=70, n_sites=4, n_mod=2))           # more than PYA_FAST_PEPTIDE_LEN residues
    dense = _psms(_fixed(7106, 1))[0]                                       # more than PYA_FAST_PEAKS peaks
    rng = np.random.default_rng(7107)
    mz = np.concatenate([dense["mz"], rng.uniform(100.0, 2000.0, 9000 - dense["mz"].size)])
    it = np.concatenate([dense["intensity"], rng.lognormal(4.5, 1.0, mz.size - dense["mz"].size)])
    order = np.argsort(mz, kind="stable")
    return synth.pack_batch(long_pep + [dict(dense, mz=mz[order], intensity=it[order])])


def _invalid():
    psms = _psms(_fixed(7108, 12))
    bad = psms[3]["peptide"]
    psms[3] = dict(psms[3], peptide=bad[:5] + "X" + bad[6:])              # unknown residue
    psms[8] = dict(psms[8], mz=np.zeros(0), intensity=np.zeros(0))         # empty spectrum
    return synth.pack_batch(psms)


INVALID_PSMS = (3, 8)


def _shared():
    base = _fixed(7109, 8)
    spectra = [dict(mz=p["mz"], intensity=p["intensity"]) for p in _psms(base)]
    hits = _psms(_fixed(7110, 40))                                          # five hits per spectrum: other peptides, same shape
    return synth.pack_shared_batch(spectra, [dict(peptide=h["peptide"], n_of_mod=h["n_of_mod"], max_charge=1, spectrum=i // 5)
                                             for i, h in enumerate(hits)])


def _empty():
    return synth.pack_batch([])


def _wide():
    batch, settings = synth.make_batch("cfg3", n_psm=300, seed=7111)       # fused and count-node PSMs mixed
    assert settings == SETTINGS
    return batch


def _chunked():
    # Beyond the ten entries of the small pool: no batch under 32 MiB of spectra is ever cut into chunks, whatever the budget
    # (host_batch.cpp kChunkMin), so "the chunked and unchunked paths alternate on one handle" needs ONE entry above it:
    # 7 000 cfg2 PSMs, 36 MB of float64 spectra, milliseconds on the device.
    return _fixed(7112, 7000)


# name -> (builder, what it is for)
_BUILDERS = {
    "a_small": (_a_small, "64 cfg2 PSMs of one shape (6 sites, 3 mods), 20-mers at charge 1: score-table need 19*1*1*2 = 38, under the floor"),
    "b_shapes": (_b_shapes, "about 120 cfg3-style PSMs whose shapes are all absent from a_small, one of them cfg5's (15, 5): the order table must grow"),
    "b_lut": (_b_lut, "40-mers at charge 3 (need 39*3*2 = 234 > 128) and one 51-mer at charge 6 (600): the score table must be extended and moved"),
    "general": (_general, "a 70-residue peptide and a 9 000-peak spectrum: the general route"),
    "one": (lambda: _fixed(7113, 1), "a single PSM: the one-launch kernel, the one-PSM staging"),
    "empty": (_empty, "n_psm = 0"),
    "invalid": (_invalid, "cfg2 PSMs with two invalid ones among them (unknown residue, empty spectrum): skip_invalid=True"),
    "shared": (_shared, "cfg2 PSMs as 5 hits per spectrum: the shared entry points"),
    "f32": (lambda: synth.narrow_batch(_a_small()), "a_small with float32 arrays: the typed entry points"),
    "wide": (_wide, "300 cfg3 PSMs, fused and count-node PSMs mixed: the largest of the small entries"),
    "chunked": (_chunked, "7 000 cfg2 PSMs, 36 MB of spectra: the one entry a 16 MiB budget cuts into chunks"),
}
NAMES = tuple(_BUILDERS)
PURPOSE = {k: v[1] for k, v in _BUILDERS.items()}
MUST_SKIP_INVALID = ("invalid",)                 # without the flag the call raises, and no step may raise
SCOREABLE = ("a_small", "b_shapes", "b_lut", "general", "one", "wide")     # private float64 entries: PyAscore.score takes their PSMs
_pool = {}


def entry(name):
    """the batch of a pool entry (built once, never modified)"""
    if name not in _pool:
        _pool[name] = _BUILDERS[name][0]()
    return _pool[name]


def checker_batch(name):
    """the VALID PSMs of the entry as the reference checker takes them: private spectra, float64 arrays holding the same
    values (the reference aborts on an unknown residue and reads past an empty spectrum: the invalid PSMs never reach it)"""
    batch = entry(name)
    if batch.get("spec_of") is not None:
        batch = synth.expand_shared_batch(batch)
    batch = synth.widen_batch(batch)
    ok = valid(name)
    return batch if ok.all() else synth.pack_batch([p for p, good in zip(_psms(batch), ok) if good])


_answers = {}


def answer(name, kind, with_loss=False):
    """best_score, best_sig, n_sig, ascores, alt_mask of the entry's valid PSMs from the CPU checker ``kind`` ("ref": the
    reference's own core), under SETTINGS or under SETTINGS with LOSS added; computed once"""
    from oracle import harness, orc
    key = (name, kind, with_loss)
    if key not in _answers:
        settings = dict(SETTINGS, neutral_losses=[list(LOSS)]) if with_loss else SETTINGS
        batch = checker_batch(name)
        max_k = max(1, int(np.max(entry(name)["n_of_mod"]))) if int(entry(name)["n_psm"]) else 1
        _answers[key] = harness.make_scorer(orc.OracleAscore, settings, kind=kind).score_batch(batch, max_k)
    return _answers[key]


def concat(*names):
    """the PSMs of several private float64 entries as one batch"""
    return synth.pack_batch([p for n in names for p in _psms(entry(n))])


def valid(name):
    """which PSMs of the entry are valid"""
    ok = np.ones(int(entry(name)["n_psm"]), bool)
    if name == "invalid":
        ok[list(INVALID_PSMS)] = False
    return ok


# ---- what a call must make the handle's tables do ----------------------------------------------------------------------------
def lut_need(batch, ok=None):
    """the largest trial count of a PSM: (L - 1) x charges x loss sums x ion types (host_plan.cpp: lut_need)"""
    n = int(batch["n_psm"])
    if n == 0:
        return 0
    need = (np.diff(batch["pep_off"]) - 1) * np.asarray(batch["max_charge"], np.int64) * N_UNIQ * N_TYPES
    return int(need[np.ones(n, bool) if ok is None else ok].max())


def lut_rows(need, rows_before=0):
    """rows of the score table on the device after a call with this need (host_tables.cpp: ensure_lut)"""
    return rows_before if rows_before > need else max(need, LUT_FLOOR) + 1


def order_entries(shape_set):
    """entries of the order table the shapes take: C(n, k) signatures each and, for a shape of at most 64, its shared-node
    table behind them -- 2 (n + 1) words of own bits and 2 (n + 1) ceil(C / 8) words of group ranks (host_tables.cpp:
    shape_offset)"""
    total = 0
    for n, k in shape_set:
        c = math.comb(n, k) if 0 <= k <= n else 0
        total += c
        if 1 <= c <= NODE_SHAPE_MAX:
            total += 2 * (n + 1) * (1 + (c + 7) // 8)
    return total


def _state_after(names):
    need, seen = 0, set()
    for name in names:
        ok = valid(name)
        need = max(need, lut_need(entry(name), ok))
        seen |= {sh for sh, good in zip(shapes(entry(name)), ok) if good and 0 <= sh[1] <= sh[0]}
    return need, seen


def expected_growth(before, after):
    """What scoring (or planning) the entries ``after`` does to a handle that has seen the entries ``before`` and nothing else:
    dict(lut=must the score table grow, lut_rows=(before, after), order=must the order table grow, order_entries=(before,
    after)).  Entry names or lists of them."""
    before = [before] if isinstance(before, str) else list(before)
    after = [after] if isinstance(after, str) else list(after)
    need0, shapes0 = _state_after(before)
    need1, shapes1 = _state_after(before + after)
    rows0 = lut_rows(need0) if before else 0
    rows1 = lut_rows(need1, rows0)
    return dict(lut=rows1 > rows0, lut_rows=(rows0, rows1), order=bool(shapes1 - shapes0),
                order_entries=(order_entries(shapes0), order_entries(shapes1)))


# ---- sequences of calls --------------------------------------------------------------------------------------------------------
def sequence(seed, n_steps=N_STEPS):
    """A list of steps for ONE scorer.  A step is ("batch", entry, flags, budget) -- ``score_batch(entry, **flags)`` with
    ``flags`` a random subset of FLAGS (ranked -> ranked=5) under a workspace budget of ``budget`` bytes (0: the default) -- or
    ("score", entry, psm, read_records): ``score()`` of one PSM of a scoreable entry, then (or not) a read of ``pep_scores``.
    A quarter of the steps are score steps.  The batch steps go round the pool in shuffled rounds, so that every entry comes
    up in every sequence of at least 2 x len(NAMES) steps; a quarter of them run under SMALL_BUDGET -- except the steps of
    ``chunked``, the one entry a budget can cut, which take turns (small budget first), so that chunked and unchunked calls of
    the same batch alternate on the handle."""
    rng = np.random.default_rng(1000 + seed)
    steps, rounds, n_chunked = [], [], 0
    for _ in range(n_steps):
        if rng.random() < 0.25:
            name = SCOREABLE[int(rng.integers(len(SCOREABLE)))]
            steps.append(("score", name, int(rng.integers(int(entry(name)["n_psm"]))), bool(rng.random() < 0.5)))
            continue
        if not rounds:
            rounds = [NAMES[i] for i in rng.permutation(len(NAMES))]
        name = rounds.pop()
        flags = {f: True for f in FLAGS if rng.random() < 0.5}
        if "ranked" in flags:
            flags["ranked"] = 5
        if name in MUST_SKIP_INVALID:
            flags["skip_invalid"] = True
        small = bool(rng.random() < 0.25)
        if name == "chunked":
            small = n_chunked % 2 == 0
            n_chunked += 1
        steps.append(("batch", name, flags, SMALL_BUDGET if small else 0))
    return steps


def step_key(step):
    """a hashable name of a step: two steps with the same key are the same call"""
    if step[0] == "batch":
        return (step[0], step[1], tuple(sorted(step[2].items())), step[3])
    return step
