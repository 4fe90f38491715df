"""tests/faroffsets.py on the CPU: the arithmetic of the layouts at all four marks (offsets only, nothing allocated), the
layout materialised at the HARNESS mark and scored by the reference core, the conditions on the real PSMs that keep "equal
bytes" from being an accident of degenerate inputs, and the rules that make the filler transparent to the transforms."""
import numpy as np
import pytest

import faroffsets as fo
from conftest import checker_kind
from oracle import harness, orc
from pyascore_amd import rollup as ru, synth

KEYS = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")
#: which GPU tests run at which mark (tests/test_gpu_far_offsets.py)
RUNS = {"HARNESS": ("plan", "stages", "far_input", "recalibrate", "recalibrate_in_place", "far_output"),
        "M1": ("plan", "stages", "far_input", "recalibrate", "recalibrate_in_place", "far_output"),
        "M2": ("plan", "stages", "far_input", "recalibrate", "recalibrate_in_place", "far_output"),
        "M3": ("far_input", "recalibrate_in_place")}


def _ref(name):
    return harness.make_scorer(orc.OracleAscore, fo.SETTINGS[name], kind=checker_kind())


def _score(name, batch):
    wide = synth.widen_batch(batch)
    wide = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in wide.items()}
    return _ref(name).score_batch(wide, 3)


def _rows_differ(a, b):
    """per PSM: some of the five result arrays differ"""
    out = np.zeros(a["n_sig"].size, bool)
    for key in KEYS:
        out |= np.any(np.atleast_2d((a[key].view(np.uint8).reshape(a[key].shape[0], -1) !=
                                     b[key].view(np.uint8).reshape(b[key].shape[0], -1)).T), axis=0)
    return out


@pytest.mark.parametrize("name", list(fo.MARKS))
def test_layout_arithmetic(name):
    lay = fo.layout(name)
    off, mark = lay.peak_off, lay.mark
    sizes = np.diff(off)
    assert off[0] == 0 and (sizes > 0).all()
    assert sizes.max() <= fo.MAX_PEAKS
    s = lay.straddler
    assert off[s] + 64 <= mark and mark + 64 <= off[s + 1]
    # a 64-peak stride of the straddler's wavefront crosses the mark as well
    assert (mark - off[s]) % 64 != 0
    assert all(off[f] >= mark for f in lay.far) and off[lay.far[0]] == off[s + 1]
    assert lay.n_filler <= 2 ** 32 - 2 and lay.n_spectra <= 2 ** 32 - 2
    assert (sizes[lay.filler[0]:lay.filler[-1]] == fo.W).all() and sizes[lay.filler[-1]] == lay.last_len
    assert 512 <= lay.last_len <= fo.W                                  # (a short last filler that still has windows to bin)
    assert lay.filler_end - lay.filler_begin == (lay.n_filler - 1) * fo.W + lay.last_len
    assert lay.total == off[-1] > mark
    assert lay.total * lay.mz_dtype.itemsize > {"HARNESS": 0, "M1": 2 ** 32, "M2": 2 ** 33, "M3": 2 ** 34}[name]
    assert [int(lay.real_of[f]) for f in lay.far] == [int(lay.real_of[n]) for n in lay.near] == list(range(fo.N_NEAR))
    # the real spectra: one above PYA_FAST_PEAKS, one of a single peak
    real = np.diff(lay.real["peak_off"])
    assert (real > fo.W).sum() == 1 and (real == 1).sum() == 1 and real.size == fo.N_NEAR + 1
    b = lay.batch()
    assert b["pep_off"][-1] == b["pep"].size and (b["pep"] != 0).all() and b["n_psm"] == lay.n_spectra
    assert bytes(b["pep"][b["pep_off"][lay.filler[0]]:b["pep_off"][lay.filler[0] + 1]]) == b"SAK"
    # the device bytes of every GPU test at this mark, the plan's workspace apart
    for test in RUNS[name]:
        need = lay.device_bytes(test)
        assert 0 < need <= fo.CAP_BYTES, (name, test, need)
    if name == "M3":
        # left out at M3, as tests/test_gpu_far_offsets.py says: they do not fit the cap
        # (a plan keeps an 8-byte retained entry per raw peak: 34.4 GB beside the 34.4 GB of the two arrays)
        for test in ("plan", "stages", "far_output", "recalibrate"):
            assert lay.device_bytes(test) > fo.CAP_BYTES, test


@pytest.fixture(scope="module")
def harness_layout():
    lay = fo.layout("HARNESS")
    mz, it = fo.materialise(lay)
    for a in (mz, it):
        a.setflags(write=False)
    return lay, mz, it


def test_materialised_layout_is_what_the_offsets_say(harness_layout):
    lay, mz, it = harness_layout
    off, r = lay.peak_off, lay.real
    for s in lay.real_spectra():
        i = int(lay.real_of[s])
        a, b = int(r["peak_off"][i]), int(r["peak_off"][i + 1])
        assert mz[off[s]:off[s + 1]].tobytes() == r["mz"][a:b].tobytes()
        assert it[off[s]:off[s + 1]].tobytes() == r["intensity"][a:b].tobytes()
    for j, s in enumerate(lay.filler):
        fm, fi = fo.filler_spectrum(lay.mz_dtype, lay.it_dtype, j, int(off[s + 1] - off[s]))
        assert mz[off[s]:off[s + 1]].tobytes() == fm.tobytes() and it[off[s]:off[s + 1]].tobytes() == fi.tobytes()


@pytest.mark.parametrize("setting", ["cfg2", "cfg4"])
def test_reference_scores_the_layout_as_it_scores_the_psms_alone(harness_layout, setting):
    """the builder and the comparisons, where everything fits a host: the whole HARNESS layout through the reference core
    gives every real PSM the rows it has alone, and every filler the rows of its pattern"""
    lay, mz, it = harness_layout
    whole = _score(setting, dict(lay.batch(), mz=mz, intensity=it))
    real = lay.real_spectra()
    alone = _score(setting, lay.alone(real))
    for key in KEYS:
        assert np.array_equal(whole[key][real], alone[key]), key
    pats = _score(setting, lay.filler_alone())
    fill = np.arange(lay.n_filler)
    idx = np.where(fill == lay.n_filler - 1, 4, fill % 4)
    for key in KEYS:
        assert np.array_equal(whole[key][lay.filler[0]:lay.filler[-1] + 1], pats[key][idx]), key


@pytest.mark.parametrize("dtypes", ["f64", "f32"])
@pytest.mark.parametrize("setting", ["cfg2", "cfg4"])
def test_real_psms_are_not_degenerate(setting, dtypes):
    """At least three quarters of the real PSMs have more than one site assignment and a positive best score, AND score
    differently on their neighbour's spectrum: a kernel that reads the wrong spectrum cannot give the right bytes."""
    t = np.float64 if dtypes == "f64" else np.float32
    lay = fo.layout(fo.HARNESS, t, t)
    n = fo.N_NEAR + 1
    own = _score(setting, lay.alone(lay.real_spectra()[:n]))
    r = synth.widen_batch(lay.real)
    nxt = [(i + 1) % n for i in range(n)]
    psms = []
    for i in range(n):
        kw, sp = synth.unpack_psm(r, i), synth.unpack_psm(r, nxt[i])
        psms.append(dict(mz=sp["mz_arr"], intensity=sp["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"],
                         max_charge=kw["max_fragment_charge"]))
    other = _score(setting, synth.pack_batch(psms))
    scored = (own["n_sig"] > 1) & (own["best_score"] > 0)
    moved = _rows_differ(own, other)
    good = scored & moved
    print("%s %s: %d of %d PSMs scored, %d differ on the neighbour's spectrum, %d both" % (setting, dtypes, scored.sum(), n, moved.sum(),
                                                                                         good.sum()))
    assert good.sum() * 4 >= 3 * n


@pytest.mark.parametrize("dtypes", ["f64", "f32"])
def test_filler_passes_the_transforms_unchanged(dtypes):
    """deisotope, decharge, strip (unusable precursor) and centroid return every filler byte for byte under the parameters the
    GPU tests use: new_off == peak_off across the filler"""
    t = np.float64 if dtypes == "f64" else np.float32
    specs = [fo.filler_spectrum(t, t, j) for j in range(4)] + [fo.filler_spectrum(t, t, 2, 700), fo.filler_spectrum(t, t, 1, 513)]
    mz, it = np.concatenate([s[0] for s in specs]), np.concatenate([s[1] for s in specs])
    off = np.concatenate([[0], np.cumsum([s[0].size for s in specs])]).astype(np.int64)
    assert mz.dtype == t and it.dtype == t
    outs = {
        "deisotope": ru.deisotope(mz, it, off, fo.DEISOTOPE)[:3],
        "decharge": ru.decharge(mz, it, off, fo.DECHARGE)[:3],
        "strip": ru.strip(mz, it, off, np.zeros(len(specs)), np.zeros(len(specs), np.int32), fo.STRIP)[:3],
        "centroid": ru.centroid(mz, it, off, fo.CENTROID)[:3],
    }
    for name, (o_mz, o_it, new_off) in outs.items():
        assert np.array_equal(new_off, off), name
        assert o_mz.tobytes() == mz.tobytes() and o_it.tobytes() == it.tobytes(), name
    assert (ru.decharge(mz, it, off, fo.DECHARGE)[3] == 1).all()
    assert not ru.centroid(mz, it, off, fo.CENTROID)[3].any()
    assert (ru.strip(mz, it, off, np.zeros(len(specs)), np.zeros(len(specs), np.int32), fo.STRIP)[3]["n_windows"] == 0).all()


@pytest.mark.parametrize("dtypes", ["f64", "f32"])
def test_transforms_change_the_real_spectra(dtypes):
    """... while they do remove or merge peaks of the real spectra: the far tests compare something"""
    t = np.float64 if dtypes == "f64" else np.float32
    lay = fo.layout(fo.HARNESS, t, t)
    r = lay.real
    pm, pz = lay.precursors(lay.real_spectra()[:fo.N_NEAR + 1])
    n = int(r["peak_off"][-1])
    assert ru.deisotope(r["mz"], r["intensity"], r["peak_off"], fo.DEISOTOPE)[2][-1] < n
    assert ru.strip(r["mz"], r["intensity"], r["peak_off"], pm, pz, fo.STRIP)[2][-1] < n
    assert ru.centroid(r["mz"], r["intensity"], r["peak_off"], fo.CENTROID)[2][-1] < n
    assert (ru.decharge(r["mz"], r["intensity"], r["peak_off"], fo.DECHARGE)[3] > 1).any()
    rec, _ = ru.markers(r["mz"], r["intensity"], r["peak_off"], fo.MARKERS, pm, pz)
    picked = (rec["flags"] & ru.MARKER_PICKED) != 0
    assert picked.any(axis=1).sum() >= fo.N_NEAR // 2 and picked[:, 3].any()          # (column 3: the loss target)


@pytest.mark.parametrize("dtypes", ["f64", "f32"])
@pytest.mark.parametrize("setting", ["cfg2", "cfg4"])
def test_filler_psms_are_valid(setting, dtypes):
    """each of the four fillers and the short last one of every mark, paired with "SAK", scores under both settings"""
    t = np.float64 if dtypes == "f64" else np.float32
    for name, (mark, mt, _) in fo.MARKS.items():
        if np.dtype(mt) != np.dtype(t):
            continue
        got = _score(setting, fo.layout(name).filler_alone())
        assert (got["n_sig"] == 1).all() and np.isfinite(got["best_score"]).all() and (got["best_score"] >= 0).all(), name
