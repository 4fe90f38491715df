"""Channel correction on the host (include/pyascore_hip.h: channel correction): the numpy restatement
pyascore_amd.rollup.correct_channels / channel_sums / channel_factors against the plain-Python yardstick tests/channel_ref.py, byte
for byte; the clamp; the sums as one row of the site quantification's table; planted intensities recovered through a lot-sheet-like
spill and unequal loading; and the planted reporters of the site quantification's cfg2 batch recovered per site.  No GPU."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import channel_ref as ref
import markers_cases as mc
import probs_ref
import site_quant_ref
from conftest import ROOT, checker_kind
from oracle import harness, orc
from pyascore_amd import _lib, rollup as ru, synth

NAN, INF = float("nan"), float("inf")
CHANNELS = [1, 2, 18, 63, 64]


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), "%s differs at %s" % (what, np.argwhere(got.view(np.uint8) != want.view(np.uint8))[:4].tolist())


@pytest.mark.parametrize("n_ch", CHANNELS)
def test_restatement_equals_the_yardstick(n_ch):
    rng = np.random.default_rng(500 + n_ch)
    n_rows = 37
    v = ref.special_matrix(rng, n_rows, n_ch)
    assert np.isnan(v).any() and np.isinf(v).any() and (v < 0).any() and (v == 0).any() and np.signbit(v[v == 0]).any()
    assert ((v > 0) & (v < 2.3e-308)).any() and (v == 1e300).any()
    m = ref.mixing_matrix(rng, n_ch)
    f = rng.uniform(0.5, 2.0, n_ch)
    f[0] = 0.0 if n_ch > 1 else f[0]                                                 # (a factor that clamps)
    for name, kw in (("matrix", dict(matrix=m)), ("factor", dict(factor=f)), ("both", dict(matrix=m, factor=f))):
        got, want = ru.correct_channels(v, **kw), ref.apply(v, **kw)
        _same(got, want, "%d channels, %s" % (n_ch, name))
        keep = ~((v == v) & (v > 0.0))
        assert got[keep].tobytes() == v[keep].tobytes()                             # what is no reading stays, bits and all
        assert not np.isnan(got[~keep]).any() and (got[~keep] >= 0.0).all() and not np.signbit(got[~keep]).any()
    for scale in (-3, 10):
        select = (rng.random(n_rows) < 0.6).astype(np.uint8)
        for sel in (None, select, np.zeros(n_rows, np.uint8)):
            _same(ru.channel_sums(v, sel, scale), ref.sums(v, sel, scale), "sums")
    cell = ru.channel_sums(v, None, 10)
    assert cell["n_saturated"].any() or n_ch < 18
    _same(ru.channel_factors(cell), ref.factors(cell), "factors")
    with pytest.raises(ValueError):
        ru.correct_channels(v)
    for bad in (dict(matrix=np.eye(n_ch + 1)), dict(factor=np.ones(n_ch + 1)), dict(matrix=np.ones(n_ch))):
        with pytest.raises(ValueError):
            ru.correct_channels(v, **bad)


def test_identity_gives_the_input_back():
    rng = np.random.default_rng(1)
    v = ref.special_matrix(rng, 50, 18)
    _same(ru.correct_channels(v, factor=np.ones(18)), v, "unit factor")
    # a +inf reading times the zeros of the identity is a NaN in every other channel's chain: the usable readings of its row are
    # clamped to +0.0 (the rule says so), the others stay
    with_inf = (v == INF).any(axis=1)
    assert with_inf.any() and not with_inf.all()
    got = ru.correct_channels(v, matrix=np.eye(18))
    _same(got[~with_inf], v[~with_inf], "identity matrix")
    was, rest = (v[with_inf] > 0) & (v[with_inf] < INF), ~(v[with_inf] > 0)
    assert was.any() and (got[with_inf][was] == 0.0).all() and got[with_inf][rest].tobytes() == v[with_inf][rest].tobytes()
    _same(ru.correct_channels(v, matrix=np.eye(18), factor=np.ones(18)), got, "both")


def test_negative_entries_clamp():
    """a reading smaller than what its neighbours spill into it comes out at or below zero: it is clamped to +0.0"""
    m = ru.channel_matrix(ru.channel_spill(3, [(0, 1, 0.08), (1, 0, 0.05), (1, 2, 0.07), (2, 1, 0.04)]))
    assert (m < 0).any()
    v = np.array([[1000.0, 10.0, 1000.0], [1000.0, 500.0, 1.0], [200.0, 300.0, 400.0], [NAN, 1.0, 1e6]])
    got = ru.correct_channels(v, matrix=m)
    _same(got, ref.apply(v, matrix=m), "clamped")
    clamped = (got == 0.0) & (v > 0.0)
    assert clamped.sum() == 3 and clamped[0, 1] and clamped[1, 2] and clamped[3, 1] and not np.signbit(got[clamped]).any()
    assert np.isnan(got[3, 0]) and (got[2] > 0).all()
    cell = ru.channel_sums(got, None, 10)
    assert cell["n"].tolist() == [3, 2, 3]                                          # a clamped reading is "no reading" to the sums


def test_sums_are_one_row_of_the_site_quantification():
    """every row contributes once to one slot: the cell row of tests/site_quant_ref.py is the row of channel_sums"""
    rng = np.random.default_rng(9)
    n_rows, n_ch = 60, 18
    v = ref.special_matrix(rng, n_rows, n_ch)
    site_probs = np.zeros(n_rows, probs_ref.SITE_DTYPE)
    site_probs["with_prob"] = 1.0
    psm_probs = np.zeros(n_rows, probs_ref.PSM_DTYPE)
    psm_probs["kind"] = _lib.PYA_SITE_SCORED
    head, cell = site_quant_ref.table(site_probs, psm_probs, np.arange(n_rows + 1, dtype=np.int64), np.ones(n_rows, np.uint64),
                                      np.zeros(n_rows, np.int32), 1, v, None, 0.5, 10)
    assert head["n_records"][0] == n_rows
    whole = ru.channel_sums(v, None, 10)
    _same(whole, cell[0], "one slot")
    first = ru.channel_sums(v[:25], None, 10)
    _same(ru.channel_sums(v[25:], None, 10, into=first), whole, "two calls with into=")
    assert first.tobytes() != whole.tobytes()                                       # (into= is copied, not written)
    _same(ref.sums(v[25:], None, 10, into=ref.sums(v[:25], None, 10)), whole, "the yardstick, two calls")
    select = np.zeros(n_rows, np.uint8)
    select[:25] = 1
    _same(ru.channel_sums(v, select, 10), first, "select")
    with pytest.raises(ValueError):
        ru.channel_sums(v, None, 10, into=np.zeros(17, ru.SITE_QUANT_DTYPE))
    with pytest.raises(ValueError):
        ru.channel_sums(v, select[:-1], 10)
    with pytest.raises(ValueError):
        ru.channel_sums(v, None, 65)


def test_factors_of_large_and_empty_sums():
    cell = np.zeros(5, ru.SITE_QUANT_DTYPE)
    cell["sum"] = [(1 << 63) + 1025, (1 << 53) + 1, 0, 3, (1 << 63) + 1025]
    f = ru.channel_factors(cell)
    _same(f, ref.factors(cell), "factors")
    top = float((1 << 63) + 1025)
    assert top == 2.0 ** 63 + 2048.0                                                # (to nearest: 1025 of 2048 rounds up)
    assert f.tolist() == [1.0, top / float(1 << 53), 1.0, top / 3.0, 1.0]
    want = Fraction(int(top)) / Fraction(3)
    assert abs(Fraction(f[3]) - want) <= Fraction(np.spacing(f[3])) / 2             # one correctly rounded division
    assert ru.channel_factors(np.zeros(3, ru.SITE_QUANT_DTYPE)).tolist() == [1.0, 1.0, 1.0]
    for bad in (np.zeros(0, ru.SITE_QUANT_DTYPE), np.zeros((2, 2), ru.SITE_QUANT_DTYPE), np.zeros(65, ru.SITE_QUANT_DTYPE)):
        with pytest.raises(ValueError):
            ru.channel_factors(bad)


def _lot_sheet(rng, n_ch):
    """a spill as a reagent lot's sheet has it: 1 to 8 % of every channel to each of its neighbours, a little out of the plex"""
    entries = []
    for c in range(n_ch):
        for to in (c - 1, c + 1):
            if 0 <= to < n_ch:
                entries.append((c, to, float(rng.uniform(0.01, 0.08))))
        entries.append((c, -1, float(rng.uniform(0.0, 0.01))))
    return ru.channel_spill(n_ch, entries)


def _observed(spill, true):
    """rows of S true, formed in long double and rounded once"""
    return np.ascontiguousarray((true.astype(np.longdouble) @ spill.astype(np.longdouble).T).astype(np.float64))


def test_planted_intensities_are_recovered():
    rng = np.random.default_rng(2024)
    n_rows, n_ch, scale = 200, 18, 10
    T = rng.uniform(1e3, 1e6, (n_rows, n_ch))
    T = T * (T.sum(axis=0).max() / T.sum(axis=0))[None, :]                           # equal column totals
    assert T.min() >= 1e3 and np.ptp(T.sum(axis=0)) <= 1e-12 * T.sum(axis=0).max()
    S = _lot_sheet(rng, n_ch)
    g = rng.uniform(0.5, 2.0, n_ch)
    assert np.linalg.cond(S) < 10
    loaded = T.astype(np.longdouble) * g.astype(np.longdouble)[None, :]
    observed = _observed(S, loaded)
    M = ru.channel_matrix(S)
    exact = observed.astype(np.longdouble) @ M.astype(np.longdouble).T
    assert (exact > 0).all() and (M < 0).any()                                       # exact arithmetic clamps nothing
    corrected = ru.correct_channels(observed, matrix=M)
    assert (corrected > 0).all()
    cell = ru.channel_sums(corrected, None, scale)
    f = ru.channel_factors(cell)
    out = ru.correct_channels(corrected, factor=f)
    _same(out, ref.apply(ref.apply(observed, matrix=M), factor=ref.factors(ref.sums(corrected, None, scale))), "the chain")
    assert f.min() == 1.0 and f.max() > 1.5
    # the chain of C products and sums is off by at most C 2^-52 cond(S) relative: the first term is five orders above it;
    # a column total is short by less than one quantum per row: the second
    assert n_ch * 2.0 ** -52 * np.linalg.cond(S) < 1e-14
    tol = 1e-9 + 2.0 * n_rows / float(cell["sum"].min())
    assert tol < 1e-6
    got, want = out / out[:, :1], T / T[:, :1]
    assert (np.abs(got - want) <= tol * want).all(), float((np.abs(got - want) / want).max())
    raw = observed / observed[:, :1]
    assert not (np.abs(raw - want) <= tol * want).all()                              # (without the correction they are not)


def test_channel_matrix_and_spill_refusals():
    S = ru.channel_spill(3, [(0, 1, 0.05), (1, 2, 0.02), (2, -1, 0.03)])
    assert S.tolist() == [[0.95, 0.0, 0.0], [0.05, 0.98, 0.0], [0.0, 0.02, 0.97]]
    M = ru.channel_matrix(S)
    assert M.dtype == np.float64 and M.flags["C_CONTIGUOUS"] and np.allclose(M @ S, np.eye(3), atol=1e-15)
    _same(ru.channel_matrix(np.eye(4)), np.eye(4), "identity")
    for bad in (np.ones((2, 3)), np.ones(4), [[1.0, NAN], [0.0, 1.0]], [[1.0, INF], [0.0, 1.0]], np.zeros((2, 2)), [[1.0, 1.0], [1.0, 1.0]],
                [[1.0, 1.0], [1.0, 1.0 + 1e-9]], np.eye(65), np.zeros((0, 0)), "x"):
        with pytest.raises(ValueError):
            ru.channel_matrix(bad)
    for n, entries in ((0, []), (65, []), (2.5, []), (3, [(0, 3, 0.1)]), (3, [(3, 0, 0.1)]), (3, [(0, -2, 0.1)]), (3, [(1, 1, 0.1)]),
                       (3, [(0, 1, -0.1)]), (3, [(0, 1, NAN)]), (3, [(0, 1, 0.1), (0, 1, 0.1)]), (3, [(0, 1, 0.6), (0, 2, 0.4)]), (3, [(0, 1)]),
                       (3, [("a", 1, 0.1)])):
        with pytest.raises(ValueError):
            ru.channel_spill(n, entries)


def test_header_and_bindings_declare_the_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert re.search(r"#define\s+PYA_CHANNEL_TILE\s+%du" % _lib.PYA_CHANNEL_TILE, text)
    assert re.search(r"#define\s+PYA_CHANNEL_NORMALIZE\s+%du" % _lib.PYA_CHANNEL_NORMALIZE, text)
    assert "THE STAGE HAS ONE DEFINED ORDER OF ARITHMETIC" in text and ru.CHANNEL_TILE == _lib.PYA_CHANNEL_TILE
    from pyascore_amd import build
    build.build()
    lib = _lib.load()
    for name in ("pya_channel_correct", "pya_channel_sums", "pya_channel_factors", "pya_channel_correct_host"):
        assert re.search(r"int\s+%s\s*\(" % name, text) and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.pya_channel_correct(None, None, 0, 1, None, None, None, None) == _lib.PYA_ERR_ARG            # no handle, no call
    assert lib.pya_channel_sums(None, None, 0, 1, None, 10, None, None) == _lib.PYA_ERR_ARG
    assert lib.pya_channel_factors(None, None, 1, None, None) == _lib.PYA_ERR_ARG
    assert lib.pya_channel_correct_host(None, None, 0, 1, None, None, 10, 0, None, None, None) == _lib.PYA_ERR_ARG


def test_score_batch_request_is_checked_before_anything_runs():
    from pyascore_amd.ascore import _channels_request
    values = np.arange(12.0).reshape(4, 3)
    req = _channels_request("quant", dict(values=values, channels=dict(matrix=np.eye(3), normalize=True, select=[1, 0, 1, 1])))
    assert req["normalize"] is True and req["matrix"].shape == (3, 3) and req["select"].dtype == np.uint8
    assert _channels_request("quant", dict(values=values)) is None and _channels_request("quant", dict(values=values, channels=None)) is None
    assert _channels_request("quant", dict(values=None, channels=dict(normalize=True)))["matrix"] is None
    marks = dict(mz=(126.1, 127.1, 128.1), losses=(98.0,))
    assert _channels_request("quant", dict(values=None, channels=dict(matrix=np.eye(3))), marks)["matrix"].shape == (3, 3)
    with pytest.raises(ValueError, match="matrix has shape"):                        # (before the marker stage runs)
        _channels_request("quant", dict(values=None, channels=dict(matrix=np.eye(4))), marks)
    for bad in (3, dict(), dict(matrix=None), dict(normalize=False), dict(matrix=np.eye(3), window=1), dict(matrix=np.eye(4)), dict(matrix=np.ones(3)),
                dict(matrix="x"), dict(normalize=1), dict(normalize=True, select=[1, 0]), dict(normalize=True, select=[[1, 0, 1, 1]]),
                dict(matrix=np.eye(3), select=[1, 0, 1, 1])):
        with pytest.raises(ValueError):
            _channels_request("quant", dict(values=values, channels=bad))


def test_planted_reporters_recovered_per_site_through_the_reference_core():
    """The 120 cfg2 PSMs of the site quantification's planting (tests/test_site_quant_host.py): the planted reporter matrix is the
    TRUTH, what the instrument would have seen is S truth; the site sums over the corrected matrix are the exact sums of the
    truth to one quantum per record and the rounding of the chain, the sums over the observed matrix are not."""
    base, settings = synth.make_batch("cfg2", 120, seed=3)
    tol, n, m, scale = 0.05, 120, 30, 10
    planted, pm, pz, want = mc.with_markers(base, tol)
    kws = [synth.unpack_psm(planted, i) for i in range(n)]
    psms = [dict(mz=kws[i]["mz_arr"], intensity=kws[i]["int_arr"], peptide=kws[i % m]["peptide"], n_of_mod=kws[i % m]["n_of_mod"],
                 max_charge=kws[i % m]["max_fragment_charge"]) for i in range(n)]
    batch = synth.pack_batch(psms)
    chk = harness.make_scorer(orc.OracleAscore, settings, kind=checker_kind())
    exp = harness.collect(chk, batch, synth.unpack_psm)
    site_off, site_probs, psm_probs = probs_ref.batch_records(settings, batch, exp, exp, synth.unpack_psm)
    slot, n_slots, keys = ru.peptide_slots([p["peptide"] for p in psms], site_off, residues=settings["mod_group"])
    truth = np.ascontiguousarray(want[:, :10])
    assert (truth > 0).all()
    S = _lot_sheet(np.random.default_rng(5), 10)
    assert np.linalg.cond(S) < 10
    observed = _observed(S, truth)
    M = ru.channel_matrix(S)
    assert (observed.astype(np.longdouble) @ M.astype(np.longdouble).T > 0).all()
    corrected = ru.correct_channels(observed, matrix=M)
    in_best = np.array([(int(exp["best_sig"][i]) >> r) & 1 for i in range(n) for r in range(int(site_off[i + 1] - site_off[i]))], bool)
    thr = float(np.median(site_probs["with_prob"][in_best]))
    p = ru.site_quant_params(threshold=thr, scale_log2=scale, n_channels=10)
    head, cell = ru.site_quant(site_probs, psm_probs, site_off, exp["best_sig"], slot, n_slots, corrected, None, p)
    _, cell_raw = ru.site_quant(site_probs, psm_probs, site_off, exp["best_sig"], slot, n_slots, observed, None, p)
    owner = np.repeat(np.arange(n), np.diff(site_off))
    contributes = in_best & (site_probs["with_prob"] >= thr)
    assert 0.25 * in_best.sum() <= contributes.sum() <= 0.75 * in_best.sum() + 1
    rel = Fraction(1e-9)
    checked = off = 0
    for s in np.flatnonzero(head["n_records"]):
        who = owner[contributes & (slot == s)]
        k = int(head["n_records"][s])
        assert who.size == k and (cell["n"][s] == k).all()
        for c in range(10):
            exact = sum(Fraction(float(truth[i, c])) for i in who)
            room = Fraction(k, 1 << scale) + rel * exact
            assert abs(Fraction(int(cell["sum"][s, c]), 1 << scale) - exact) <= room, (keys[s], c)
            off += abs(Fraction(int(cell_raw["sum"][s, c]), 1 << scale) - exact) > room
        checked += 1
    assert checked >= 10 and off >= 5 * checked
