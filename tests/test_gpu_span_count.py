"""The span count of the fused score-localize body (csrc/span_guard.h; csrc/fused_core.hip.h, `no_cross`): for a PSM whose
residue masses cannot bring a span ion of the winner within mz_error of any ion of a competitor, a round counts the
site-determining ions from the recorded ranks instead of building and comparing fragment m/z lists.

Every case is scored four times -- batch kernel (PYA_NO_TINY) and single-launch kernel (its first 64 PSMs), each with the
span count and with PYA_DEBUG bit 0x04000000 ("no span count") -- and compared byte for byte in best_score, best_sig, n_sig,
ascores and alt_mask with each other and with the reference's own core.  Which side of the guard a PSM lies on is invisible in
the results, so every case also asserts what the host restatement of the guard (pya_debug_span_guard) says about its PSMs.

The batches are made here (positions of the sites, alphabets and modification masses are what the cases are about);
spectra: the fragments of a true assignment with phospho-sized shifts, 60 % kept, and 60 noise peaks."""
import ctypes as C

import numpy as np
import pytest

from conftest import checker_kind
from oracle import harness, orc
from pyascore_amd import synth
from test_gpu_general_edges import _same_results

pytestmark = pytest.mark.gpu

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")
NO_SPAN_COUNT = 0x04000000
ERR = float(np.float32(0.05))               # mz_error as the library holds it
ASN = np.float32(114.04293)                  # N; G + G = 114.04292
NO_G = "ACDEFHIKLMNPQRVW"                    # (synth.BASE_ALPHABET without G: no two-residue run near N)


def _settings(types="by", err=0.05, mod=synth.PHOSPHO, group="STY"):
    return dict(bin_size=100.0, n_top=10, mod_group=group, mod_mass=float(mod), mz_error=err, fragment_types=types, neutral_losses=[])


def _batch(n, L, n_mod, seed, sites=None, n_sites=None, alphabet=synth.BASE_ALPHABET, every_other=None, err=0.05):
    """n PSMs of length L; `sites`: the positions of the S/T/Y residues of every PSM, or n_sites random ones per PSM;
    `every_other`: this letter on every second residue that is not a site."""
    rng = np.random.default_rng(seed)
    base = np.frombuffer(alphabet.encode(), np.uint8)
    pep = base[rng.integers(0, len(base), size=(n, L))]
    if every_other:
        pep[:, 1::2] = ord(every_other)
    if sites is None:
        pos = np.sort(np.argsort(rng.random((n, L)), axis=1)[:, :n_sites], axis=1)
    else:
        pos = np.tile(np.asarray(sites, np.int64), (n, 1))
    ns = pos.shape[1]
    rows = np.arange(n)[:, None]
    pep[rows, pos] = np.frombuffer(b"STY", np.uint8)[rng.choice(3, size=(n, ns), p=(0.5, 0.35, 0.15))]
    truth = np.argsort(rng.random((n, ns)), axis=1)[:, :n_mod]
    mass = synth._MASS_LUT[pep]
    np.add.at(mass, (np.repeat(np.arange(n), n_mod), pos[rows, truth].ravel()), synth.PHOSPHO)
    fwd, rev = np.cumsum(mass, axis=1)[:, :L - 1], np.cumsum(mass[:, ::-1], axis=1)[:, :L - 1]
    sig = np.concatenate([fwd + synth.PROTON, rev + synth.WATER + synth.PROTON], axis=1)
    keep = rng.random(sig.shape) < 0.6
    sig = sig + rng.uniform(-0.4 * err, 0.4 * err, size=sig.shape)
    mz = np.concatenate([np.where(keep, sig, np.inf), rng.uniform(100.0, 100.0 + 110.0 * L, size=(n, 60))], axis=1)
    inten = np.concatenate([rng.lognormal(6.0, 1.2, size=sig.shape), rng.lognormal(4.5, 1.0, size=(n, 60))], axis=1)
    order = np.argsort(mz, axis=1, kind="stable")
    mz, inten = np.take_along_axis(mz, order, axis=1), np.take_along_axis(inten, order, axis=1)
    counts = keep.sum(axis=1) + 60
    valid = np.arange(mz.shape[1])[None, :] < counts[:, None]
    return dict(n_psm=n, mz=mz[valid], intensity=inten[valid], peak_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                pep=pep.ravel().copy(), pep_off=(np.arange(n + 1) * L).astype(np.int64), n_of_mod=np.full(n, n_mod, np.int32),
                max_charge=np.ones(n, np.int32), aux_pos=np.zeros(0, np.uint32), aux_mass=np.zeros(0, np.float32),
                aux_off=np.zeros(n + 1, np.int64))


def _checker(settings, batch):
    return harness.make_scorer(orc.OracleAscore, settings, kind=checker_kind()).score_batch(batch, int(batch["n_of_mod"].max()))


def _guard(gpu, batch):
    """the host restatement for every PSM: (counted 0 / 1, E)"""
    side, E = np.zeros(batch["n_psm"], np.int64), np.zeros(batch["n_psm"])
    out = (C.c_double * 3)()
    for i in range(batch["n_psm"]):
        a, b = int(batch["pep_off"][i]), int(batch["pep_off"][i + 1])
        e, f = int(batch["aux_off"][i]), int(batch["aux_off"][i + 1])
        pos = np.ascontiguousarray(batch["aux_pos"][e:f], np.uint32)
        am = np.ascontiguousarray(batch["aux_mass"][e:f], np.float32)
        side[i] = gpu._lib.pya_debug_span_guard(gpu._h, bytes(batch["pep"][a:b]), b - a, pos.ctypes.data, am.ctypes.data, f - e, out)
        E[i] = out[0]
    return side, E


def _check(settings, batch, what, counted, want=None):
    """-> (the checker's results, E of the PSMs)"""
    from pyascore_amd import PyAscore
    want = _checker(settings, batch) if want is None else want
    gpu = harness.make_scorer(PyAscore, settings)
    side, E = _guard(gpu, batch)
    assert np.all(side == (1 if counted else 0)), "%s: the guard's restatement says %s, expected %d for every PSM" % (what, side.tolist(), counted)
    head = synth.slice_batch(batch, 0, min(64, int(batch["n_psm"])))
    keys = KEYS if int(np.diff(batch["pep_off"]).max()) <= 64 else tuple(k for k in KEYS if k != "alt_mask")
    for tiny, b, w in ((False, batch, want), (True, head, {k: want[k][:head["n_psm"]] for k in KEYS})):
        res = []
        for debug in (0, NO_SPAN_COUNT):
            gpu.reload_env()                                 # (every switch at its production default)
            if not tiny:
                gpu.set_debug("PYA_NO_TINY", "1")
            if debug:
                gpu.set_debug("PYA_DEBUG", str(debug))
            res.append(gpu.score_batch(b))
        where = what + (" (single launch)" if tiny else " (batch kernel)")
        _same_results(res[0], w, keys, where + " against the checker")
        _same_results(res[1], w, keys, where + ", no span count, against the checker")
        _same_results(res[0], res[1], KEYS, where + " against no span count")
    return want, E


def test_identity_on_the_flagship_shape():
    """256 PSMs of cfg2's shape: L = 20, 6 sites, 3 modifications, b/y, 0.05 Da"""
    batch, settings = synth.make_batch("cfg2", n_psm=256, seed=4100)
    want, E = _check(settings, batch, "cfg2", True)
    assert np.any(want["ascores"] != 0.0)
    assert set(E.tolist()) <= {ERR + 22 * 2.0 ** -11, ERR + 22 * 2.0 ** -12}   # (L + 2) ulp_f32 of a bound in [2048, 8192)


# name -> (L, sites or number of sites, n_mod, fragment types, PSMs)
SHAPES = {}
for _L in range(2, 8):                                       # L - 1 = 1 .. 6 (6: the first that splits its walk)
    SHAPES["L%d" % _L] = (_L, min(_L, 3), 1, "by", 16)
SHAPES["adjacent_2"] = (12, (5, 6), 1, "by", 64)             # span length 1; ties (below)
SHAPES["adjacent_in_4"] = (12, (3, 4, 5, 9), 2, "by", 32)
SHAPES["termini_2"] = (12, (0, 11), 1, "by", 32)
SHAPES["termini_3"] = (12, (0, 5, 11), 2, "by", 32)
SHAPES["n_2"] = (20, 2, 1, "by", 24)                         # site assignments: 2, 21 (the last split walk), 22, 32 (plain walk)
SHAPES["n_21"] = (20, 7, 2, "by", 24)
SHAPES["n_22"] = (22, 22, 1, "by", 24)
SHAPES["n_32"] = (32, 32, 1, "by", 24)
SHAPES["wide_35"] = (40, 35, 1, "by", 24)                    # 33 .. 64: the launch that walks its directions one after the other
SHAPES["wide_36"] = (20, 9, 2, "by", 24)
SHAPES["wide_63"] = (64, 63, 1, "by", 16)                   # (63 modifiable residues: the most a PSM may have)
SHAPES["b_only"] = (20, 6, 3, "b", 32)                       # the one-direction instantiation
SHAPES["y_only"] = (20, 6, 3, "y", 32)
SHAPES["b_only_36"] = (20, 9, 2, "b", 24)
SHAPES["rounds_4"] = (20, 6, 4, "by", 32)                    # up to four / five pushed competitors: two rounds
SHAPES["rounds_5"] = (20, 6, 5, "by", 32)


@pytest.mark.parametrize("name", list(SHAPES))
def test_small_and_awkward_shapes(name):
    L, sites, k, types, n = SHAPES[name]
    kw = dict(n_sites=sites) if isinstance(sites, int) else dict(sites=sites)
    batch = _batch(n, L, k, 4200 + list(SHAPES).index(name), **kw)
    want, _ = _check(_settings(types), batch, name, True)
    assert np.any(want["ascores"] != 0.0), "%s: no PSM with a non-zero Ascore" % name
    if name == "adjacent_2":
        # both fragments that tell the two sites apart are missing from four spectra in twenty-five: the assignments tie
        assert np.any((want["ascores"][:, 0] == 0.0) & (want["alt_mask"][:, 0] != 0)), "no PSM whose best score ties"
    if name.startswith("rounds"):
        assert np.any((want["ascores"] != 0.0).sum(axis=1) > 3), "no PSM with more than three pushed competitors"


def _edge_batch(seed=4300, alphabet=NO_G):
    """L = 12, 4 sites, 2 modifications; N on every second residue that is not a site: in and next to every span"""
    return _batch(32, 12, 2, seed, n_sites=4, alphabet=alphabet, every_other="N")


def _edge_E():
    """E of the edge batch's PSMs around mod_mass = N (one value: the bound on the fragment m/z stays inside one binade)"""
    from pyascore_amd import PyAscore
    _, E = _guard(harness.make_scorer(PyAscore, _settings(mod=ASN)), _edge_batch())
    assert np.all(E == E[0]) and E[0] == ERR + 14 * 2.0 ** -12
    return float(E[0])


def _f32_near(x, up):
    """the float32 next to float32(x) on the far side of x: above x (up) or below it"""
    v = np.float32(x)
    return np.nextafter(v, np.float32(np.inf if up else -np.inf))


@pytest.mark.parametrize("name", ["equal", "above_outside", "above_inside", "below_outside", "below_inside"])
def test_mod_mass_around_a_residue_mass(name):
    E = _edge_E()
    mod, counted = {"equal": (ASN, False),
                    "above_outside": (_f32_near(float(ASN) + E, True), True),       # N + E + one float32 ulp
                    "above_inside": (_f32_near(float(ASN) + E, False), False),
                    "below_outside": (_f32_near(float(ASN) - E, False), True),      # N - E - one float32 ulp
                    "below_inside": (_f32_near(float(ASN) - E, True), False)}[name]
    assert (abs(float(mod) - float(ASN)) > E) == counted
    _, got_E = _check(_settings(mod=mod), _edge_batch(), "mod_mass %r (%s)" % (float(mod), name), counted)
    assert np.all(got_E == E)


def test_fixed_modification_moves_a_residue_onto_the_delta():
    batch = _edge_batch(4310)
    batch["pep"].reshape(32, 12)[:, 0] = ord("A")            # A + 8.929221 = 79.96633: a residue that weighs a phosphate
    batch["aux_off"] = np.arange(33, dtype=np.int64)
    batch["aux_pos"] = np.ones(32, np.uint32)
    batch["aux_mass"] = np.full(32, synth.PHOSPHO - synth.RESIDUE_MASS["A"], np.float32)
    _check(_settings(), batch, "fixed modification onto the delta", False)
    batch["aux_mass"] = np.full(32, 57.021465, np.float32)   # (and one that moves it elsewhere)
    _check(_settings(), batch, "fixed modification off the delta", True)


@pytest.mark.parametrize("mod", [-synth.PHOSPHO, 0.03, -0.03])
def test_negative_and_tiny_mod_mass(mod):
    _check(_settings(mod=mod), _edge_batch(4320), "mod_mass %r" % mod, False)


def test_two_residue_run_equal_to_the_delta():
    batch = _batch(32, 12, 2, 4330, n_sites=4, alphabet=NO_G.replace("N", ""), every_other="G")   # G G = 114.04292, no N
    _check(_settings(mod=ASN), batch, "G G against 114.043", False)
    batch = _batch(32, 12, 2, 4330, n_sites=4, alphabet=NO_G.replace("N", ""), every_other="A")   # (the same without G)
    _check(_settings(mod=ASN), batch, "A A against 114.043", True)


def test_long_peptide_has_its_own_margin():
    batch = _batch(24, 60, 2, 4340, n_sites=4)
    assert float(batch["mz"].max()) > 4096.0
    want, E = _check(_settings(), batch, "60 residues", True)
    assert np.any(want["ascores"] != 0.0)
    assert np.all(E == ERR + 62 * 2.0 ** -10)               # five and a half times cfg2's margin
