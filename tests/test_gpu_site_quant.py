"""Site quantification on the GPU (pya_site_quant: channel intensities summed per roll-up slot over the confidently localised
records).  Yardstick: tests/site_quant_ref.py fed with the arrays score_batch(probs=True) returns for the same batch -- every
comparison is on the raw bytes of the head and cell records; every field is an integer sum.  In every test the threshold is the
median with_prob of the in-best records of the plain run, so between a quarter and three quarters of them contribute, which
each test asserts.  Slots are keyed by peptide, and the batches repeat their peptides so that many PSMs share a slot."""
import ctypes as C
import os

import numpy as np
import pytest

import markers_cases as mc
import site_quant_ref as ref
import switches
from conftest import GOLDEN, golden_cases
from oracle import harness
from pyascore_amd import _lib, rollup as ru, synth

pytestmark = pytest.mark.gpu

SCALE = 10
NAN = float("nan")


def _gpu(settings, **debug):
    from pyascore_amd import PyAscore
    gpu = harness.make_scorer(PyAscore, settings)
    for k, v in debug.items():
        gpu.set_debug(k, v)
    return gpu


def _same(got, want, what):
    for g, w, name in zip(got, want, ("head", "cell")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            at = tuple(bad[0])
            raise AssertionError("%s: %d %s records differ, first %s: got %s, want %s" % (what, len(bad), name, at, g[at], w[at]))


def _repeats(batch, share=3):
    """the batch with the peptides of its first n / share PSMs repeated against the spectra of the others"""
    n = int(batch["n_psm"])
    m = max(1, n // share)
    kws = [synth.unpack_psm(batch, i) for i in range(n)]
    psms = [dict(mz=kws[i]["mz_arr"], intensity=kws[i]["int_arr"], peptide=kws[i % m]["peptide"], n_of_mod=kws[i % m]["n_of_mod"],
                 max_charge=kws[i % m]["max_fragment_charge"]) for i in range(n)]
    return synth.pack_batch(psms), [p["peptide"] for p in psms]


def _peptides(batch):
    return [synth.unpack_psm(batch, i)["peptide"] for i in range(int(batch["n_psm"]))]


def _matrix(seed, n_rows, n_ch):
    """a seeded matrix with NaNs, zeros and negatives among its readings, a few rows without a gap"""
    rng = np.random.default_rng(seed)
    v = rng.random((n_rows, n_ch)) * 10.0 ** rng.integers(0, 7, (n_rows, n_ch))
    kind = rng.random((n_rows, n_ch))
    kind[rng.random(n_rows) < 0.3] = 1.0
    v[kind < 0.06] = NAN
    v[(kind >= 0.06) & (kind < 0.11)] = 0.0
    v[(kind >= 0.11) & (kind < 0.13)] = -1.0
    return v


def _in_best(res):
    """one boolean per residue record: the record of a scored PSM whose residue best_sig modifies"""
    off = res["site_off"]
    owner = np.repeat(np.arange(off.size - 1), np.diff(off))
    r = (np.arange(int(off[-1])) - off[owner]).astype(np.uint64)
    return ((res["best_sig"][owner] >> r) & np.uint64(1) != 0) & (res["psm_probs"]["kind"][owner] == _lib.PYA_SITE_SCORED)


def _threshold(res):
    """the median with_prob of the in-best records, and the check that a quarter to three quarters of them are at or above it"""
    p = res["site_probs"]["with_prob"][_in_best(res)]
    assert p.size, "no in-best record"
    thr = float(np.median(p))
    share = float((p >= thr).mean())
    assert 0.25 <= share <= 0.75, "%.3f of the in-best records contribute at the median %r" % (share, thr)
    return thr


def _ref(res, slot, n_slots, values, row, thr, complete_only=False, into=None, scale=SCALE):
    return ref.table(res["site_probs"], res["psm_probs"], res["site_off"], res["best_sig"], slot, n_slots, values, row, thr, scale,
                     complete_only, into=into)


def _table(res):
    return res["quant_head"], res["quant"]


def _against_yardstick(settings, batch, peptides, what, channels=(1, 18, 64), skip_invalid=False, rows="psm", **debug):
    gpu = _gpu(settings, **debug)
    first = gpu.score_batch(batch, skip_invalid=skip_invalid, probs=True)
    slot, n_slots, keys = ru.peptide_slots(peptides, first["site_off"], residues=settings["mod_group"])
    roll = dict(slot=slot, n_slots=n_slots)
    plain = gpu.score_batch(batch, skip_invalid=skip_invalid, probs=True, rollup=roll)           # the unflagged call
    thr = _threshold(plain)
    n = int(batch["n_psm"])
    general = _gpu(settings, PYA_NO_PROB_CNT="1", **debug)
    seen = 0
    for n_ch in channels:
        if rows == "psm":
            values, row = _matrix(n_ch + n, n, n_ch), None
        else:                                                                                    # fewer rows than PSMs, some PSMs without
            values = _matrix(n_ch + n, max(1, n // 2), n_ch)
            row = (np.arange(n) % (values.shape[0] + 1) - 1).astype(np.int32)
        req = dict(values=values, row=row, threshold=thr, scale_log2=SCALE)
        got = gpu.score_batch(batch, skip_invalid=skip_invalid, probs=True, rollup=roll, quant=req)
        for key in plain:                                                                        # nothing of the run moves
            if key != "status_message":
                assert got[key].tobytes() == plain[key].tobytes(), (what, n_ch, key)
        assert set(got) - set(plain) == {"quant_head", "quant", "quant_params"}
        assert got["quant_params"] == ru.site_quant_params(threshold=thr, scale_log2=SCALE, n_channels=n_ch)
        want = _ref(plain, slot, n_slots, values, row, thr)
        _same(_table(got), want, "%s, %d channels" % (what, n_ch))
        _same(ru.site_quant(plain["site_probs"], plain["psm_probs"], plain["site_off"], plain["best_sig"], slot, n_slots, values, row,
                            got["quant_params"]), want, "%s, %d channels: the numpy restatement" % (what, n_ch))
        alone = gpu.score_batch(batch, skip_invalid=skip_invalid, rollup=roll, quant=dict(req, complete_only=True))
        assert "site_probs" not in alone and alone["rollup"].tobytes() == plain["rollup"].tobytes()
        _same(_table(alone), _ref(plain, slot, n_slots, values, row, thr, complete_only=True), "%s, %d channels, complete only" % (what, n_ch))
        other = general.score_batch(batch, skip_invalid=skip_invalid, rollup=roll, quant=req)
        _same(_table(other), want, "%s, %d channels (general front end)" % (what, n_ch))
        seen += int(want[0]["n_records"].sum())
    assert seen
    return gpu, plain, (slot, n_slots, keys), thr


@pytest.mark.parametrize("case", [c for c in golden_cases() if c.startswith(("velos_", "ties_", "edge_"))])
def test_golden_cases_equal_the_yardstick(case):
    settings, batch, _ = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    _against_yardstick(settings, batch, _peptides(batch), case)


@pytest.mark.parametrize("cfg,n", [("cfg1", 300), ("cfg2", 300), ("cfg3", 300), ("cfg4", 60), ("cfg5", 24)])
def test_seeded_batches_equal_the_yardstick(cfg, n):
    batch, settings = synth.make_batch(cfg, n_psm=n, seed=9710)
    batch, peptides = _repeats(batch)
    _against_yardstick(settings, batch, peptides, cfg, rows="psm" if cfg != "cfg2" else "fewer")


@pytest.mark.parametrize("general", [False, True])
def test_realistic_batches_equal_the_yardstick(general):
    batch, settings = synth.make_realistic(60, seed=9720 + general, general=general)
    batch, peptides = _repeats(batch, share=2)
    _against_yardstick(settings, batch, peptides, "realistic general=%s" % general)


def _with_records(n_rec):
    """a cfg2 batch with exactly n_rec residue records: PSMs of four modifiable residues and one of the remainder (2 .. 5)"""
    k = (n_rec - 2) // 4
    a, settings = synth.make_batch("cfg2", n_psm=k, seed=9730, n_sites=4, n_mod=1)
    b, _ = synth.make_batch("cfg2", n_psm=1, seed=9731, n_sites=n_rec - 4 * k, n_mod=1)
    psms = []
    for src in (a, b):
        for i in range(int(src["n_psm"])):
            kw = synth.unpack_psm(src, i)
            psms.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=1))
    return synth.pack_batch(psms), settings


@pytest.mark.parametrize("n_rec", [63, 64, 65, 257])
def test_boundary_shapes(n_rec):
    """residue records that straddle a wavefront and a workgroup; all on one slot, all distinct, two of one PSM on one slot; all
    PSMs on row 0; 1, 63 and 64 channels"""
    batch, settings = _with_records(n_rec)
    gpu = _gpu(settings)
    plain = gpu.score_batch(batch, probs=True)
    assert int(plain["site_off"][-1]) == n_rec
    thr = _threshold(plain)
    n = int(batch["n_psm"])
    pair = np.arange(n_rec, dtype=np.int32)
    pair[plain["site_off"][:-1] + 1] = pair[plain["site_off"][:-1]]                  # the first two records of every PSM on one slot
    slots = dict(one=(np.zeros(n_rec, np.int32), 1), distinct=(np.arange(n_rec, dtype=np.int32), n_rec), pair=(pair, n_rec),
                 few=((np.arange(n_rec) % 5).astype(np.int32), 5))
    total = 0
    for n_ch in (1, 63, 64):
        values = _matrix(n_rec + n_ch, n, n_ch)
        for name, (slot, n_slots) in slots.items():
            for row in (None, np.zeros(n, np.int32)):
                got = gpu.score_batch(batch, rollup=dict(slot=slot, n_slots=n_slots), quant=dict(values=values, row=row, threshold=thr,
                                                                                                  scale_log2=SCALE))
                want = _ref(plain, slot, n_slots, values, row, thr)
                _same(_table(got), want, "%d records, %d channels, %s, row %s" % (n_rec, n_ch, name, "0" if row is not None else "i"))
                total += int(want[0]["n_records"].sum())
                if name == "one":
                    assert want[0]["n_records"][0] == int((_in_best(plain) & (plain["site_probs"]["with_prob"] >= thr)).sum())
    assert total


def test_rows_of_a_shared_batch_and_the_marker_chain():
    """spec_of as the rows, in and out of spectrum order; markers= with values=None against the explicit matrix; marker_values"""
    import torch
    from pyascore_amd import device
    base, settings = synth.make_batch("cfg2", n_psm=60, seed=9740)
    tol = 0.05
    planted, pm, pz, _ = mc.with_markers(base, tol)
    spectra, psms = [], []
    for i in range(0, 60, 3):
        kw = synth.unpack_psm(planted, i)
        spectra.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"]))
        for j in range(3):
            kj = synth.unpack_psm(planted, (i + j) % 12)
            psms.append(dict(peptide=kj["peptide"], n_of_mod=kj["n_of_mod"], max_charge=1, aux_pos=np.zeros(0, np.uint32),
                             aux_mass=np.zeros(0, np.float32), spectrum=len(spectra) - 1))
    pm, pz = pm[::3].copy(), pz[::3].copy()
    gpu = _gpu(settings)
    marks = dict(mz=mc.REPORTERS, losses=(mc.LOSS_H3PO4,), tol=tol, precursor_mz=pm, precursor_charge=pz)
    for order, what in ((np.arange(60), "shared"), (np.random.default_rng(3).permutation(60), "shuffled shared")):
        mine = [psms[p] for p in order]
        shared = synth.pack_shared_batch(spectra, mine)
        flat = gpu.score_batch(synth.expand_shared_batch(shared), probs=True)
        thr = _threshold(flat)
        slot, n_slots, _ = ru.peptide_slots([p["peptide"] for p in mine], flat["site_off"], residues=settings["mod_group"])
        roll = dict(slot=slot, n_slots=n_slots)
        values = _matrix(5, len(spectra), 18)
        spec_of = np.asarray(shared["spec_of"]).astype(np.int32)
        want = _ref(flat, slot, n_slots, values, spec_of, thr)
        assert (want[0]["n_records"] >= 3).any()
        got = gpu.score_batch(shared, rollup=roll, quant=dict(values=values, row=spec_of, threshold=thr, scale_log2=SCALE))
        _same(_table(got), want, what)
        # the chain: the fixed targets of markers= are the channels, spec_of the rows
        with_m = gpu.score_batch(shared, rollup=roll, markers=marks)
        matrix = np.ascontiguousarray(ru.marker_matrix(with_m["markers"])[:, :10])
        assert (matrix > 0).all()
        chained = gpu.score_batch(shared, rollup=roll, markers=marks, quant=dict(values=None, threshold=thr, scale_log2=SCALE))
        explicit = gpu.score_batch(shared, rollup=roll, markers=marks, quant=dict(values=matrix, row=spec_of, threshold=thr, scale_log2=SCALE))
        _same(_table(chained), _table(explicit), what + ": values=None beside markers=")
        _same(_table(chained), _ref(flat, slot, n_slots, matrix, spec_of, thr), what + ": the chain against the yardstick")
        for key in with_m:                                                           # nothing of the run, the roll-up or the markers moves
            if key != "status_message":
                assert chained[key].tobytes() == with_m[key].tobytes(), (what, key)
        assert chained["quant_params"]["n_channels"] == 10 and (chained["quant_head"]["n_complete"] == chained["quant_head"]["n_records"]).all()
    # marker records to a matrix on the device: the columns of marker_matrix the mask names
    dev = torch.device("cuda", 0)
    rec = with_m["markers"]
    rec["flags"][::7, 3] &= ~np.uint32(ru.MARKER_PICKED)                             # (a target that picked nothing)
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(rec.shape[0], rec.shape[1], 24).copy()).to(dev)
    full = ru.marker_matrix(rec)
    for mask in (None, 0x3FF, 0b10000001000, 1 << 10, 1):
        cols = [t for t in range(11) if mask is None or (mask >> t) & 1]
        got = device.marker_values(gpu, d_rec, mask).cpu().numpy()
        assert got.shape == (rec.shape[0], len(cols)) and got.tobytes() == np.ascontiguousarray(full[:, cols]).tobytes(), mask
    assert np.isnan(device.marker_values(gpu, d_rec, 1 << 3).cpu().numpy()[::7]).all()
    for bad in (0, 1 << 11):
        with pytest.raises(ValueError):
            device.marker_values(gpu, d_rec, bad)
    assert gpu._lib.pya_marker_values(gpu._h, d_rec.data_ptr(), rec.shape[0], 11, 1 << 11, None, d_rec.data_ptr()) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_marker_values(gpu._h, d_rec.data_ptr(), rec.shape[0], 65, 1, None, d_rec.data_ptr()) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_marker_values(gpu._h, None, rec.shape[0], 11, 1, None, d_rec.data_ptr()) == _lib.PYA_ERR_ARG


def test_bytes_do_not_depend_on_chunk_cuts(monkeypatch):
    big = synth.make_slice(synth.describe("cfg2", 12_000, seed=9750))
    settings = synth.describe("cfg2", 1, seed=9750)["settings"]
    big, peptides = _repeats(big, share=5)
    gpu = _gpu(settings)
    monkeypatch.setenv("PYA_NO_CHUNKS", "1")
    switches.from_env(gpu)
    plain = gpu.score_batch(big, probs=True)
    thr = _threshold(plain)
    slot, n_slots, _ = ru.peptide_slots(peptides, plain["site_off"], residues=settings["mod_group"])
    roll = dict(slot=slot, n_slots=n_slots)
    values = _matrix(11, 4000, 3)
    row = (np.arange(12_000) % 4001 - 1).astype(np.int32)
    req = dict(values=values, row=row, threshold=thr, scale_log2=SCALE)
    uncut = gpu.score_batch(big, rollup=roll, quant=req)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) == 1
    monkeypatch.delenv("PYA_NO_CHUNKS")
    monkeypatch.setenv("PYA_CHUNK_MB", "2")
    switches.from_env(gpu)
    cut = gpu.score_batch(big, rollup=roll, quant=req, evidence=True)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) > 8
    none = gpu.score_batch(big, rollup=roll, quant=dict(req, row=None, values=_matrix(12, 12_000, 3)))
    monkeypatch.delenv("PYA_CHUNK_MB")
    switches.from_env(gpu)
    want = _ref(plain, slot, n_slots, values, row, thr)
    assert (want[0]["n_records"] >= 5).any()
    _same(_table(uncut), want, "uncut")
    _same(_table(cut), want, "chunked")
    _same(_table(none), _ref(plain, slot, n_slots, _matrix(12, 12_000, 3), None, thr), "chunked, row None: the PSM's place in the batch")
    assert cut["rollup"].tobytes() == uncut["rollup"].tobytes()


def _hip():
    """the HIP runtime the process already holds"""
    with open("/proc/self/maps") as maps:
        path = next(line.split()[-1] for line in maps if "libamdhip64" in line)
    return C.CDLL(path)


def _plan(gpu, batch, dev):
    import torch
    from pyascore_amd.device import DevicePlan
    plan = DevicePlan(gpu, batch, quant=True)
    plan.run(torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev))
    return plan


def test_accumulation_over_plans_equals_one_call():
    import torch
    from pyascore_amd.device import site_quant_records
    batch, settings = synth.make_batch("cfg3", n_psm=600, seed=9760)
    batch, peptides = _repeats(batch, share=4)
    gpu = _gpu(settings)
    res = gpu.score_batch(batch, probs=True, site_sig_cap=0)
    thr = _threshold(res)
    slot, n_slots, _ = ru.peptide_slots(peptides, res["site_off"], residues=settings["mod_group"])
    values = _matrix(13, 600, 18)
    p = ru.site_quant_params(threshold=thr, scale_log2=SCALE, n_channels=18)
    whole = _table(gpu.score_batch(batch, rollup=dict(slot=slot, n_slots=n_slots), site_sig_cap=0,
                                   quant=dict(values=values, threshold=thr, scale_log2=SCALE)))
    _same(whole, _ref(res, slot, n_slots, values, None, thr), "one call")
    dev = torch.device("cuda", 0)
    d_values = torch.from_numpy(values).to(dev)
    cut, rec = 250, int(res["site_off"][250])
    halves = [(synth.slice_batch(batch, 0, cut), slot[:rec], 0), (synth.slice_batch(batch, cut, 600), slot[rec:], cut)]
    host = lambda t: site_quant_records((t[0].cpu().numpy(), t[1].cpu().numpy()))   # noqa: E731
    for order in ((0, 1), (1, 0)):
        plans = [_plan(gpu, halves[h][0], dev) for h in order]
        table, parts = None, []
        for plan, h in zip(plans, order):
            _, sp, pp = plan.probs()
            d_slot = torch.from_numpy(halves[h][1]).to(dev)
            table = plan.site_quant(sp, pp, d_slot, d_values, p, n_slots=n_slots, row_base=halves[h][2], table=table)
            d_row = torch.arange(halves[h][2], halves[h][2] + plan.n_psm, dtype=torch.int32, device=dev)
            parts.append(plan.site_quant(sp, pp, d_slot, d_values, p, n_slots=n_slots, row=d_row))     # the same plan again, a table of its own
            plan.check()
        _same(host(table), whole, "two plans into one table, order %s" % (order,))
        _same(ru.merge_site_quant(*[host(t) for t in parts]), whole, "a table per plan, merged on the host")
        stream = torch.cuda.current_stream(dev).cuda_stream
        for t in table:                                                              # cleared by hipMemsetAsync: the empty table again
            assert _hip().hipMemsetAsync(C.c_void_p(t.data_ptr()), 0, C.c_size_t(t.numel()), C.c_void_p(stream)) == 0
        _same(host(table), ru.empty_site_quant(n_slots, 18), "the cleared table")
        again = plans[0].site_quant(*plans[0].probs()[1:], torch.from_numpy(halves[order[0]][1]).to(dev), d_values, p, row_base=halves[order[0]][2],
                                    table=table)
        _same(host(again), host(parts[0]), "a cleared table takes a plan as a new one does")


def test_limits_and_guards():
    import torch
    from pyascore_amd.device import DevicePlan, site_quant_records
    batch, settings = synth.make_batch("cfg2", n_psm=200, seed=9770)
    batch, peptides = _repeats(batch)
    gpu = _gpu(settings)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    head, cell = ru.empty_site_quant(4, 3)
    assert gpu._lib.pya_last_batch_site_quant(gpu._h, vp(head), vp(cell), 4, 3) == _lib.PYA_ERR_STATE      # no batch with the flag yet
    assert b"PYA_FLAG_QUANT" in gpu._lib.pya_last_error(gpu._h)
    res = gpu.score_batch(batch, probs=True)
    thr = _threshold(res)
    slot, n_slots, _ = ru.peptide_slots(peptides, res["site_off"], residues=settings["mod_group"])
    roll = dict(slot=slot, n_slots=n_slots)
    values = _matrix(17, 200, 3)
    req = dict(values=values, threshold=thr, scale_log2=SCALE)
    with pytest.raises(ValueError, match="rollup="):                                 # quant= needs rollup=
        gpu.score_batch(batch, quant=req)
    want = _ref(res, slot, n_slots, values, None, thr)
    got = gpu.score_batch(batch, rollup=roll, quant=req)
    _same(_table(got), want, "one call")
    back = ru.empty_site_quant(n_slots, 3)
    assert gpu._lib.pya_last_batch_site_quant(gpu._h, vp(back[0]), vp(back[1]), n_slots, 3) == 0
    _same(back, want, "pya_last_batch_site_quant")
    assert gpu._lib.pya_last_batch_site_quant(gpu._h, vp(back[0]), vp(back[1]), n_slots - 1, 3) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_last_batch_site_quant(gpu._h, vp(back[0]), vp(back[1]), n_slots, 4) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_last_batch_site_quant(gpu._h, None, vp(back[1]), n_slots, 3) == _lib.PYA_ERR_ARG
    gpu.score_batch(batch, rollup=roll)
    assert gpu._lib.pya_last_batch_site_quant(gpu._h, vp(back[0]), vp(back[1]), n_slots, 3) == _lib.PYA_ERR_STATE
    # the C ABI: the flag without the roll-up's flag, the flag without a loan, the refusals of pya_set_site_quant
    r = gpu.score_batch(batch)
    arrs = [np.ascontiguousarray(batch[k], t) for k, t in (("peak_off", np.int64), ("pep", np.uint8), ("pep_off", np.int64), ("n_of_mod", np.int32),
                                                           ("max_charge", np.int32), ("aux_pos", np.uint32), ("aux_mass", np.float32),
                                                           ("aux_off", np.int64))]
    b = _lib.Batch(200, *[vp(a) for a in arrs])
    keys = ("best_score", "best_sig", "n_sig", "ascores", "alt_mask")
    outs = [np.zeros_like(r[k]) for k in keys]
    rs = _lib.Results(r["ascores"].shape[1], *[vp(a) for a in outs])
    mz, it = np.ascontiguousarray(batch["mz"], np.float64), np.ascontiguousarray(batch["intensity"], np.float64)
    c_params = ru.site_quant_c_params(ru.site_quant_params(threshold=thr, n_channels=3))
    assert gpu._lib.pya_set_site_quant(gpu._h, vp(values), 200, None, 200, C.byref(c_params)) == 0
    assert gpu._lib.pya_score_batch(gpu._h, C.byref(b), vp(mz), vp(it), _lib.PYA_FLAG_QUANT, C.byref(rs)) == _lib.PYA_ERR_ARG
    assert b"PYA_FLAG_ROLLUP" in gpu._lib.pya_last_error(gpu._h)
    assert gpu._lib.pya_set_rollup(gpu._h, vp(slot), slot.size, n_slots, 0.75, None) == 0
    assert gpu._lib.pya_score_batch(gpu._h, C.byref(b), vp(mz), vp(it), _lib.PYA_FLAG_QUANT | _lib.PYA_FLAG_ROLLUP, C.byref(rs)) == _lib.PYA_ERR_ARG
    assert b"pya_set_site_quant" in gpu._lib.pya_last_error(gpu._h)                  # (the loan ended with the refused call)
    assert gpu._lib.pya_set_site_quant(gpu._h, vp(values), 200, None, 199, C.byref(c_params)) == 0
    assert gpu._lib.pya_set_rollup(gpu._h, vp(slot), slot.size, n_slots, 0.75, None) == 0
    assert gpu._lib.pya_score_batch(gpu._h, C.byref(b), vp(mz), vp(it), _lib.PYA_FLAG_QUANT | _lib.PYA_FLAG_ROLLUP, C.byref(rs)) == _lib.PYA_ERR_ARG
    assert b"199 PSMs" in gpu._lib.pya_last_error(gpu._h)
    for change in (dict(scale_log2=65), dict(scale_log2=-65), dict(n_channels=0), dict(n_channels=65), dict(flags=2), dict(reserved=1),
                   dict(threshold=NAN)):
        bad = ru.site_quant_c_params(ru.site_quant_params(threshold=thr, n_channels=3))
        for k, v in change.items():
            setattr(bad, k, v)
        assert gpu._lib.pya_set_site_quant(gpu._h, vp(values), 200, None, 200, C.byref(bad)) == _lib.PYA_ERR_ARG, change
    assert gpu._lib.pya_set_site_quant(gpu._h, None, 200, None, 200, C.byref(c_params)) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_set_site_quant(gpu._h, vp(values), 1 << 31, None, 200, C.byref(c_params)) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_set_site_quant(gpu._h, vp(values), 200, None, 1 << 31, C.byref(c_params)) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_set_site_quant(gpu._h, vp(values), 200, None, 200, None) == _lib.PYA_ERR_ARG
    # a slot at or above n_slots, a row at or above n_rows: the limit error
    with pytest.raises(ValueError, match="n_slots"):
        gpu.score_batch(batch, rollup=dict(slot=slot, n_slots=n_slots - 3), quant=req)
    with pytest.raises(ValueError, match="n_rows"):
        gpu.score_batch(batch, rollup=roll, quant=dict(req, values=values[:150]))
    _same(_table(gpu.score_batch(batch, rollup=roll, quant=req)), want, "after the refused calls")
    dev = torch.device("cuda", 0)
    plan = _plan(gpu, batch, dev)
    _, sp, pp = plan.probs()
    p = ru.site_quant_params(threshold=thr, scale_log2=SCALE, n_channels=3)
    d_slot, d_values = torch.from_numpy(slot).to(dev), torch.from_numpy(values).to(dev)
    table = plan.site_quant(sp, pp, d_slot, d_values, p, n_slots=n_slots)
    plan.check()
    host = lambda t: site_quant_records((t[0].cpu().numpy(), t[1].cpu().numpy()))   # noqa: E731
    _same(host(table), want, "plan")
    # every slot outside: nothing is written, the bytes stay, check() reports; the same for the rows
    plan.site_quant(sp, pp, torch.full_like(d_slot, n_slots), d_values, p, table=table)
    with pytest.raises(ValueError, match="n_slots"):
        plan.check()
    assert gpu._lib.pya_plan_check(plan._plan) == _lib.PYA_ERR_LIMIT
    _same(host(table), want, "a call whose slots are all outside")
    plan.site_quant(sp, pp, d_slot, d_values, p, table=table, row_base=200)
    with pytest.raises(ValueError, match="n_rows"):
        plan.check()
    _same(host(table), want, "a call whose rows are all outside")
    plan.site_quant(sp, pp, torch.full_like(d_slot, -1), d_values, p, table=table)  # negative: silently nothing, and the report is gone
    plan.check()
    plan.site_quant(sp, pp, d_slot, d_values, p, table=table, row=torch.full((200,), -1, dtype=torch.int32, device=dev))
    plan.check()
    _same(host(table), want, "negative slots and rows")
    # a table smaller than the slots, guard bytes behind it: the slots inside are what they are in the full table
    small = n_slots - 3
    g_head = torch.full((n_slots + 5, 8), 0x5A, dtype=torch.uint8, device=dev)
    g_cell = torch.full((n_slots + 5, 3, 16), 0x5A, dtype=torch.uint8, device=dev)
    g_head[:small].zero_()
    g_cell[:small].zero_()
    args = (plan._plan, C.byref(plan._res), None, sp.data_ptr(), pp.data_ptr(), d_slot.data_ptr())
    c_p = ru.site_quant_c_params(p)
    assert gpu._lib.pya_plan_site_quant(*args, small, d_values.data_ptr(), 200, None, 0, C.byref(c_p), g_head.data_ptr(), g_cell.data_ptr()) == 0
    assert gpu._lib.pya_plan_check(plan._plan) == _lib.PYA_ERR_LIMIT
    h_host, c_host = g_head.cpu().numpy(), g_cell.cpu().numpy()
    assert (h_host[small:] == 0x5A).all() and (c_host[small:] == 0x5A).all()
    _same(site_quant_records((h_host[:small], c_host[:small])), (want[0][:small], want[1][:small]), "the slots inside a smaller table")
    for bad in (dict(scale_log2=65), dict(n_channels=0), dict(n_channels=65), dict(flags=2), dict(reserved=1), dict(threshold=NAN)):
        c_bad = ru.site_quant_c_params(p)
        for k, v in bad.items():
            setattr(c_bad, k, v)
        assert gpu._lib.pya_plan_site_quant(*args, n_slots, d_values.data_ptr(), 200, None, 0, C.byref(c_bad), table[0].data_ptr(),
                                            table[1].data_ptr()) == _lib.PYA_ERR_ARG, bad
    for n_s, n_r, vals, hd in ((1 << 31, 200, d_values.data_ptr(), table[0].data_ptr()), (n_slots, 1 << 31, d_values.data_ptr(), table[0].data_ptr()),
                               (n_slots, 200, None, table[0].data_ptr()), (n_slots, 200, d_values.data_ptr(), None)):
        assert gpu._lib.pya_plan_site_quant(*args, n_s, vals, n_r, None, 0, C.byref(c_p), hd, table[1].data_ptr()) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_plan_site_quant(*args, n_slots, d_values.data_ptr(), 200, None, 0, None, table[0].data_ptr(), table[1].data_ptr()) == _lib.PYA_ERR_ARG
    _same(host(table), want, "after the refused calls")
    fresh = DevicePlan(gpu, batch, quant=True)
    assert gpu._lib.pya_plan_site_quant(fresh._plan, *args[1:], n_slots, d_values.data_ptr(), 200, None, 0, C.byref(c_p), table[0].data_ptr(),
                                        table[1].data_ptr()) == _lib.PYA_ERR_STATE
    with pytest.raises(ValueError):
        plan.site_quant(sp, pp, d_slot[:-1], d_values, p, table=table)
    with pytest.raises(ValueError):
        plan.site_quant(sp, pp, d_slot, d_values[:, :2], p, table=table)
    # pya_score_one refuses the flag
    kw = synth.unpack_psm(batch, 0)
    m, i = np.ascontiguousarray(kw["mz_arr"], np.float64), np.ascontiguousarray(kw["int_arr"], np.float64)
    pep = np.frombuffer(kw["peptide"].encode(), np.uint8)
    one = (np.zeros(1, np.float32), np.zeros(1, np.uint64), np.zeros(1, np.int32), np.zeros((1, 4), np.float32), np.zeros((1, 4), np.uint64))
    r1 = _lib.Results(4, *[vp(x) for x in one])
    rc = gpu._lib.pya_score_one(gpu._h, vp(m), vp(i), m.size, vp(pep), pep.size, int(kw["n_of_mod"]), int(kw["max_fragment_charge"]), None, None, 0,
                                _lib.PYA_FLAG_QUANT, C.byref(r1))
    assert rc == _lib.PYA_ERR_ARG and b"PYA_FLAG_QUANT" in gpu._lib.pya_last_error(gpu._h)


def test_two_reports_in_one_run_and_none_after_it():
    """the 200-PSM plan above: a roll-up call and a site-quantification call of one run both have something to report, and
    check() names the roll-up, the first in its order; the reports belong to their run -- after the next run, with no stage
    asked, check() passes --, and a good call behind that run gives the yardstick's table"""
    import torch
    from pyascore_amd.device import DevicePlan, rollup_records, site_quant_records
    batch, settings = synth.make_batch("cfg2", n_psm=200, seed=9770)
    batch, peptides = _repeats(batch)
    gpu = _gpu(settings)
    res = gpu.score_batch(batch, probs=True)
    thr = _threshold(res)
    slot, n_slots, _ = ru.peptide_slots(peptides, res["site_off"], residues=settings["mod_group"])
    values = _matrix(17, 200, 3)
    want = _ref(res, slot, n_slots, values, None, thr)
    dev = torch.device("cuda", 0)
    d_mz, d_in = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    plan = DevicePlan(gpu, batch, quant=True)
    plan.run(d_mz, d_in)
    _, sp, pp = plan.probs()
    p = ru.site_quant_params(threshold=thr, scale_log2=SCALE, n_channels=3)
    d_slot, d_values = torch.from_numpy(slot).to(dev), torch.from_numpy(values).to(dev)
    host = lambda t: site_quant_records((t[0].cpu().numpy(), t[1].cpu().numpy()))   # noqa: E731
    rolled = plan.rollup_clear(n_slots)
    plan.rollup(sp, pp, torch.full_like(d_slot, n_slots), rolled)                   # every slot outside
    table = plan.site_quant(sp, pp, d_slot, d_values, p, n_slots=n_slots, row_base=200)   # every row outside
    with pytest.raises(ValueError, match="pya_plan_rollup"):
        plan.check()
    assert rollup_records(rolled.cpu().numpy()).tobytes() == ru.empty(n_slots).tobytes()
    _same(host(table), ru.empty_site_quant(n_slots, 3), "a call whose rows are all outside")
    plan.run(d_mz, d_in)                                                             # the next run: nothing of it has been asked
    plan.check()
    _, sp, pp = plan.probs()
    plan.site_quant(sp, pp, d_slot, d_values, p, table=table)
    plan.check()
    _same(host(table), want, "a good call behind the second run")


def test_set_aside_and_unscored_psms():
    good, settings = synth.make_batch("cfg2", n_psm=12, seed=9930)
    psms = []
    for i in range(good["n_psm"]):
        kw = synth.unpack_psm(good, i)
        psms.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"], max_charge=1))
    for i in range(6, 12):                                                     # every peptide twice
        psms[i] = dict(psms[i], peptide=psms[i - 6]["peptide"], n_of_mod=psms[i - 6]["n_of_mod"])
    psms[0] = dict(psms[0], peptide="ASGTPEYIDEK", n_of_mod=3)                 # as many modifications as sites
    psms[1] = dict(psms[1], peptide="PEPTXIDESK")                              # unknown residue: set aside, no records
    psms[2] = dict(psms[2], peptide="AGSPEPIDEK", n_of_mod=2)                  # more modifications than sites: not scored
    psms[3] = dict(psms[3], mz=np.zeros(0), intensity=np.zeros(0))             # empty spectrum: set aside
    psms[5] = dict(psms[5], peptide="ASGTPEYIDEK", n_of_mod=0)                 # no modification: covers, reports nothing
    batch = synth.pack_batch(psms)
    peptides = [p["peptide"] for p in psms]
    gpu, plain, (slot, n_slots, keys), thr = _against_yardstick(settings, batch, peptides, "mixed batch", channels=(18,), skip_invalid=True)
    assert plain["status"][[1, 3]].all() and np.diff(plain["site_off"])[[1, 3]].tolist() == [0, 0]
    values = _matrix(3, 12, 18)
    got = gpu.score_batch(batch, skip_invalid=True, rollup=dict(slot=slot, n_slots=n_slots), quant=dict(values=values, threshold=0.999,
                                                                                                         scale_log2=SCALE))
    first = keys.index(("ASGTPEYIDEK", 2))                                     # PSM 0 reports it with probability 1, PSM 5 reports nothing
    assert got["quant_head"]["n_records"][first] == 1 and got["rollup"]["n_psm"][first] == 2
    unscored = keys.index(("AGSPEPIDEK", 3))
    assert not got["quant_head"][unscored].tobytes().strip(b"\0") and not got["quant"][unscored].tobytes().strip(b"\0")
    with pytest.raises(ValueError):                                            # without skip_invalid the call fails as before
        gpu.score_batch(batch, rollup=dict(slot=slot, n_slots=n_slots), quant=dict(values=values))


def test_a_handful_and_a_batch_of_none():
    batch, settings = synth.make_batch("cfg2", n_psm=300, seed=9780)
    batch, peptides = _repeats(batch)
    gpu = _gpu(settings)
    res = gpu.score_batch(batch, probs=True)
    thr = _threshold(res)
    slot, n_slots, _ = ru.peptide_slots(peptides, res["site_off"], residues=settings["mod_group"])
    values = _matrix(19, 300, 18)
    for lo, hi in ((0, 1), (7, 8), (10, 15)):
        r0, r1 = int(res["site_off"][lo]), int(res["site_off"][hi])
        part = gpu.score_batch(synth.slice_batch(batch, lo, hi), probs=True, rollup=dict(slot=slot[r0:r1], n_slots=n_slots),
                               quant=dict(values=values, row=np.arange(lo, hi, dtype=np.int32), threshold=thr, scale_log2=SCALE))
        _same(_table(part), _ref(part, slot[r0:r1], n_slots, values, np.arange(lo, hi), thr), "PSMs %d..%d" % (lo, hi))
    empty = gpu.score_batch(synth.slice_batch(batch, 0, 0), rollup=dict(slot=np.zeros(0, np.int32), n_slots=3), quant=dict(values=values))
    _same(_table(empty), ru.empty_site_quant(3, 18), "no PSM")
