"""Channel correction on the GPU (include/pyascore_hip.h: channel correction; csrc/channel_correct.hip): pya_channel_correct,
pya_channel_sums and pya_channel_factors against the numpy restatement pyascore_amd.rollup.correct_channels / channel_sums /
channel_factors (which tests/test_channel_correct_host.py holds against the plain-Python yardstick), the resident chain from marker
records to a site table, score_batch(quant=dict(channels=...)), the host form and the refusals.  Every comparison is on raw
bytes.  The row counts straddle a wavefront's stride and PYA_CHANNEL_TILE; the channel counts give 64, 32, 3, 1 and 1 rows per
stride, with idle lanes at 18 and 63."""
import ctypes as C

import numpy as np
import pytest

import channel_ref as ref
import markers_cases as mc
from oracle import harness
from pyascore_amd import _lib, rollup as ru, synth

pytestmark = pytest.mark.gpu

TILE = _lib.PYA_CHANNEL_TILE
ROWS = sorted({0, 1, 63, 64, 65, 257, TILE - 1, TILE, TILE + 1})
CHANNELS = [1, 2, 18, 63, 64]
SCALE = 10
CANARY = 0x5A

_cache = {}


def _gpu():
    if "gpu" not in _cache:
        from pyascore_amd import PyAscore
        _cache["settings"] = synth.describe("cfg2", 1, seed=1)["settings"]
        _cache["gpu"] = harness.make_scorer(PyAscore, _cache["settings"])
    return _cache["gpu"]


def _dev():
    import torch
    return torch.device("cuda", _gpu().device)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(np.frombuffer(got.tobytes(), np.uint8) != np.frombuffer(want.tobytes(), np.uint8)) // want.dtype.itemsize
        raise AssertionError("%s: %d elements differ, first at flat index %d" % (what, len(set(bad.tolist())), int(bad[0])))


def _cell(t):
    from pyascore_amd.device import channel_sum_records
    return channel_sum_records(t.cpu().numpy())


def _case(n_rows, n_ch):
    """values, matrix, factor and a mixed select of one shape; seeded by the shape; never changed"""
    key = ("case", n_rows, n_ch)
    if key not in _cache:
        rng = np.random.default_rng(1000 * n_ch + n_rows)
        f = rng.uniform(0.5, 2.0, n_ch)
        if n_ch > 1:
            f[n_ch // 2] = 0.0                                                       # (a factor that clamps)
        _cache[key] = (ref.special_matrix(rng, n_rows, n_ch), ref.mixing_matrix(rng, n_ch), f, (rng.random(n_rows) < 0.6).astype(np.uint8))
    return _cache[key]


@pytest.mark.parametrize("n_ch", CHANNELS)
def test_entry_points_equal_the_restatement(n_ch):
    import torch
    from pyascore_amd import device
    gpu = _gpu()
    seen = clamped = 0
    for n_rows in ROWS:
        v, m, f, select = _case(n_rows, n_ch)
        d_v, d_m, d_f = _up(v), _up(m), _up(f)
        corrected = None
        for name, kw, d_kw in (("matrix", dict(matrix=m), dict(matrix=d_m)), ("factor", dict(factor=f), dict(factor=d_f)),
                               ("both", dict(matrix=m, factor=f), dict(matrix=d_m, factor=d_f))):
            what = "%d rows, %d channels, %s" % (n_rows, n_ch, name)
            want = ru.correct_channels(v, **kw)
            # out of place, between guard rows
            room = torch.full((n_rows + 2, n_ch), float("nan"), dtype=torch.float64, device=_dev())
            room.view(torch.uint8).fill_(CANARY)
            device.correct_channels(gpu, d_v, out=room[1:n_rows + 1], **d_kw)
            host = room.cpu().numpy()
            _same(host[1:n_rows + 1], want, what)
            assert (host[[0, -1]].view(np.uint8) == CANARY).all(), what
            assert d_v.cpu().numpy().tobytes() == v.tobytes()                       # the input is only read
            # exactly in place
            d_w = d_v.clone()
            assert device.correct_channels(gpu, d_w, out=d_w, **d_kw) is d_w
            _same(d_w.cpu().numpy(), want, what + ", in place")
            seen += int(((v == v) & (v > 0)).sum())
            clamped += int(((want == 0.0) & (v > 0)).sum())
            if name == "matrix":
                corrected = want
        # host arrays for matrix and factor are uploaded
        _same(device.correct_channels(gpu, d_v, matrix=m, factor=f).cpu().numpy(), ru.correct_channels(v, matrix=m, factor=f), "host operands")
        for sel_name, sel in (("all", None), ("none", np.zeros(n_rows, np.uint8)), ("mixed", select)):
            d_cell = device.channel_sums(gpu, d_v, None if sel is None else _up(sel), SCALE)
            want = ru.channel_sums(v, sel, SCALE)
            _same(_cell(d_cell), want, "%d rows, %d channels, sums over %s" % (n_rows, n_ch, sel_name))
            _same(device.channel_factors(gpu, d_cell).cpu().numpy(), ru.channel_factors(want), "factors over %s" % sel_name)
        d_cell = device.channel_sums(gpu, _up(corrected), None, -3)
        _same(_cell(d_cell), ru.channel_sums(corrected, None, -3), "sums of the corrected matrix, scale 2^-3")
    assert seen and (clamped or n_ch == 1)


def test_sums_accumulate_count_saturation_and_stride_the_grid():
    from pyascore_amd import device
    gpu = _gpu()
    v, _, _, select = _case(TILE + 1, 18)
    whole = ru.channel_sums(v, select, SCALE)
    assert whole["n_saturated"].any() and (whole["n_saturated"] < whole["n"]).all()   # +inf and 1e300 saturate, and are counted
    d_cell = device.channel_sums(gpu, _up(v[:100]), _up(select[:100]), SCALE)
    first = _cell(d_cell).copy()
    assert device.channel_sums(gpu, _up(v[100:]), _up(select[100:]), SCALE, out=d_cell) is d_cell
    _same(_cell(d_cell), whole, "two calls into one row")
    _same(first, ru.channel_sums(v[:100], select[:100], SCALE), "the first call")
    _same(_cell(device.channel_sums(gpu, _up(v), _up(select), SCALE)), whole, "one call")
    # sums above 2^53 and an empty column through the factors
    cell = np.zeros(4, ru.SITE_QUANT_DTYPE)
    cell["sum"] = [(1 << 63) + 1025, (1 << 53) + 1, 0, 3]
    d_f = device.channel_factors(gpu, _up(cell.view(np.uint8).reshape(4, 16)))
    _same(d_f.cpu().numpy(), ru.channel_factors(cell), "factors of large sums")
    # more strides than wavefronts: the sums kernel walks them by a grid stride (256 workgroups of eight: 2048 strides at a time)
    for n_big, n_ch in ((3000, 64), (7000, 18)):
        wide, _, _, _ = _case(n_big, n_ch)
        some = (np.arange(n_big) % 3 != 0).astype(np.uint8)
        _same(_cell(device.channel_sums(gpu, _up(wide), _up(some), SCALE)), ru.channel_sums(wide, some, SCALE), "%d rows of %d" % (n_big, n_ch))


def _planted(n=60):
    """n cfg2 PSMs with ten planted reporters, the peptides of the first third repeated so that PSMs share slots"""
    if "planted" not in _cache:
        base, settings = synth.make_batch("cfg2", n_psm=n, seed=9740)
        tol = 0.05
        planted, pm, pz, _ = mc.with_markers(base, tol)
        kws = [synth.unpack_psm(planted, i) for i in range(n)]
        m = n // 3
        psms = [dict(mz=kws[i]["mz_arr"], intensity=kws[i]["int_arr"], peptide=kws[i % m]["peptide"], n_of_mod=kws[i % m]["n_of_mod"],
                     max_charge=kws[i % m]["max_fragment_charge"]) for i in range(n)]
        from pyascore_amd import PyAscore
        gpu = harness.make_scorer(PyAscore, settings)
        batch = synth.pack_batch(psms)
        plain = gpu.score_batch(batch, probs=True)
        in_best = _in_best(plain)
        p = plain["site_probs"]["with_prob"][in_best]
        thr = float(np.median(p))
        assert 0.25 <= float((p >= thr).mean()) <= 0.75                              # a quarter to three quarters contribute
        peptides = [q["peptide"] for q in psms]
        slot, n_slots, _ = ru.peptide_slots(peptides, plain["site_off"], residues=settings["mod_group"])
        rng = np.random.default_rng(4)
        spill = ru.channel_spill(10, [(c, t, float(rng.uniform(0.01, 0.08))) for c in range(10) for t in (c - 1, c + 1) if 0 <= t < 10])
        _cache["planted"] = dict(gpu=gpu, settings=settings, batch=batch, plain=plain, thr=thr, slot=slot, n_slots=n_slots, peptides=peptides,
                                 tol=tol, pm=pm, pz=pz, matrix=ru.channel_matrix(spill))
    return _cache["planted"]


def _in_best(res):
    off = res["site_off"]
    owner = np.repeat(np.arange(off.size - 1), np.diff(off))
    r = (np.arange(int(off[-1])) - off[owner]).astype(np.uint64)
    return ((res["best_sig"][owner] >> r) & np.uint64(1) != 0) & (res["psm_probs"]["kind"][owner] == _lib.PYA_SITE_SCORED)


def _restated_chain(values, matrix, select=None):
    corrected = ru.correct_channels(values, matrix=matrix)
    cell = ru.channel_sums(corrected, select, SCALE)
    factors = ru.channel_factors(cell)
    return ru.correct_channels(corrected, factor=factors), cell, factors


def test_resident_chain_equals_the_restatement_chain():
    """marker records -> channel matrix -> impurity matrix -> sums -> factors -> factor -> site table, nothing read in between"""
    import torch
    from pyascore_amd import device
    from pyascore_amd.device import DevicePlan, site_quant_records
    c = _planted()
    gpu, batch, plain = c["gpu"], c["batch"], c["plain"]
    dev = torch.device("cuda", gpu.device)
    params = mc.planted_params(c["tol"])
    d_mz, d_it = torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev)
    plan = DevicePlan(gpu, batch, quant=True)
    plan.run(d_mz, d_it)
    _, sp, pp = plan.probs()
    p = ru.site_quant_params(threshold=c["thr"], scale_log2=SCALE, n_channels=10)
    d_slot = torch.from_numpy(c["slot"]).to(dev)
    d_matrix = torch.from_numpy(c["matrix"]).to(dev)
    d_rec, _, _ = device.markers(gpu, d_mz, d_it, batch["peak_off"], params, c["pm"], c["pz"])
    d_values = device.marker_values(gpu, d_rec, 0x3FF)
    device.correct_channels(gpu, d_values, matrix=d_matrix, out=d_values)
    d_cell = device.channel_sums(gpu, d_values, None, SCALE)
    d_factor = device.channel_factors(gpu, d_cell)
    device.correct_channels(gpu, d_values, factor=d_factor, out=d_values)
    table = plan.site_quant(sp, pp, d_slot, d_values, p, n_slots=c["n_slots"])
    plan.check()
    rec, _ = ru.markers(batch["mz"], batch["intensity"], batch["peak_off"], params, c["pm"], c["pz"])
    raw = np.ascontiguousarray(ru.marker_matrix(rec)[:, :10])
    assert (raw > 0).all()
    values, cell, factors = _restated_chain(raw, c["matrix"])
    assert factors.max() > 1.0 and factors.min() == 1.0
    _same(d_values.cpu().numpy(), values, "the corrected matrix")
    _same(_cell(d_cell), cell, "the column sums")
    _same(d_factor.cpu().numpy(), factors, "the factors")
    want = ru.site_quant(plain["site_probs"], plain["psm_probs"], plain["site_off"], plain["best_sig"], c["slot"], c["n_slots"], values, None, p)
    got = site_quant_records((table[0].cpu().numpy(), table[1].cpu().numpy()))
    assert want[0]["n_records"].sum() > 10 and (want[0]["n_records"] >= 2).any()
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    uncorrected = ru.site_quant(plain["site_probs"], plain["psm_probs"], plain["site_off"], plain["best_sig"], c["slot"], c["n_slots"], raw, None, p)
    assert uncorrected[1].tobytes() != want[1].tobytes()


def _equal_but(got, plain, extra, what):
    for key in plain:
        if key not in extra and key != "status_message":
            g, w = got[key], plain[key]
            assert (g.tobytes() == w.tobytes()) if isinstance(w, np.ndarray) else (g == w), (what, key)
    assert set(got) - set(plain) == set(extra) - set(plain), (what, sorted(set(got) ^ set(plain)))


@pytest.mark.parametrize("option", ["quant", "peptidoform_quant"])
def test_score_batch_with_channels(option):
    c = _planted()
    gpu, batch, thr = c["gpu"], c["batch"], c["thr"]
    n = int(batch["n_psm"])
    rng = np.random.default_rng(31)
    V = rng.uniform(1e2, 1e5, (n, 10)) * rng.uniform(0.5, 2.0, 10)[None, :]
    V[rng.random((n, 10)) < 0.05] = float("nan")
    V[3, 4], V[5, 5] = 0.0, 0.5                                                      # (0.5 beside large neighbours: clamped by the matrix)
    select = (rng.random(n) < 0.7).astype(bool)
    if option == "quant":
        base = dict(rollup=dict(slot=c["slot"], n_slots=c["n_slots"]))
        tables = ("quant_head", "quant", "quant_params")
    else:
        group, _, _ = ru.peptide_groups(c["peptides"])
        base = dict(peptidoforms=dict(group=group, threshold=0.75))
        tables = ("peptidoform_quant_head", "peptidoform_quant", "peptidoform_quant_params")
    extra = (option + "_channel_sums", option + "_channel_factors")
    req = dict(values=V, threshold=thr, scale_log2=SCALE)
    without = gpu.score_batch(batch, probs=True, **base, **{option: req})
    for what, ch in (("matrix", dict(matrix=c["matrix"])), ("normalize", dict(normalize=True, select=select)),
                     ("both", dict(matrix=c["matrix"], normalize=True))):
        got = gpu.score_batch(batch, probs=True, **base, **{option: dict(req, channels=ch)})
        corrected = ru.correct_channels(V, matrix=ch["matrix"]) if "matrix" in ch else V
        cell = ru.channel_sums(corrected, ch.get("select"), SCALE)
        factors = None
        if ch.get("normalize"):
            factors = ru.channel_factors(cell)
            corrected = ru.correct_channels(corrected, factor=factors)
        want = gpu.score_batch(batch, probs=True, **base, **{option: dict(req, values=corrected)})
        for key in tables[:2]:
            assert got[key].tobytes() == want[key].tobytes(), (what, key)
        assert got[tables[2]] == want[tables[2]]
        assert got[tables[1]].tobytes() != without[tables[1]].tobytes(), what       # (the correction moved the sums)
        _equal_but(got, without, tables + extra, what)                               # nothing else of the run moves
        _same(got[extra[0]], cell, what + ": channel sums")
        if factors is None:
            assert got[extra[1]] is None
        else:
            _same(got[extra[1]], factors, what + ": channel factors")
    for bad in (dict(matrix=np.eye(9)), dict(matrix=c["matrix"], window=1), dict(), dict(normalize=True, select=select[:-1]), 3):
        with pytest.raises(ValueError):
            gpu.score_batch(batch, **base, **{option: dict(req, channels=bad)})


def test_score_batch_with_channels_beside_markers():
    c = _planted()
    gpu, batch, thr = c["gpu"], c["batch"], c["thr"]
    marks = dict(mz=mc.REPORTERS, losses=(mc.LOSS_H3PO4,), tol=c["tol"], precursor_mz=c["pm"], precursor_charge=c["pz"])
    roll = dict(slot=c["slot"], n_slots=c["n_slots"])
    group, _, _ = ru.peptide_groups(c["peptides"])
    forms = dict(group=group, threshold=0.75)
    req = dict(values=None, threshold=thr, scale_log2=SCALE)
    ch = dict(matrix=c["matrix"], normalize=True)
    without = gpu.score_batch(batch, rollup=roll, peptidoforms=forms, markers=marks, quant=req, peptidoform_quant=req)
    got = gpu.score_batch(batch, rollup=roll, peptidoforms=forms, markers=marks, quant=dict(req, channels=ch), peptidoform_quant=dict(req, channels=ch))
    raw = np.ascontiguousarray(ru.marker_matrix(without["markers"])[:, :10])
    values, cell, factors = _restated_chain(raw, c["matrix"])
    want = gpu.score_batch(batch, rollup=roll, peptidoforms=forms, quant=dict(req, values=values), peptidoform_quant=dict(req, values=values))
    tables = ("quant_head", "quant", "peptidoform_quant_head", "peptidoform_quant")
    for key in tables:
        assert got[key].tobytes() == want[key].tobytes(), key
    assert got["quant"].tobytes() != without["quant"].tobytes()
    extra = ("quant_channel_sums", "quant_channel_factors", "peptidoform_quant_channel_sums", "peptidoform_quant_channel_factors")
    _equal_but(got, without, tables + extra, "beside markers=")
    for key in extra:
        _same(got[key], cell if key.endswith("sums") else factors, key)
    with pytest.raises(ValueError, match="matrix has shape"):                        # ten fixed targets: refused before the marker stage
        gpu.score_batch(batch, rollup=roll, markers=marks, quant=dict(req, channels=dict(matrix=np.eye(9))))
    with pytest.raises(ValueError):                                                  # no markers=: there is no matrix to correct
        gpu.score_batch(batch, rollup=roll, quant=dict(req, channels=ch))


@pytest.mark.parametrize("n_rows,n_ch", [(0, 3), (1, 1), (TILE + 1, 18), (65, 64)])
def test_host_form_equals_the_device_chain(n_rows, n_ch):
    from pyascore_amd import device
    gpu = _gpu()
    v, m, _, select = _case(n_rows, n_ch)
    before = v.copy()
    for what, kw in (("matrix", dict(matrix=m)), ("normalize", dict(normalize=True)), ("both", dict(matrix=m, normalize=True)),
                     ("both, select", dict(matrix=m, normalize=True, select=select)), ("both, scale", dict(matrix=m, normalize=True, scale_log2=-3))):
        out, cell, factors = gpu.correct_channels(v, **kw)
        scale = kw.get("scale_log2", SCALE)
        d = _up(v)
        if "matrix" in kw:
            device.correct_channels(gpu, d, matrix=m, out=d)
        d_cell = device.channel_sums(gpu, d, kw.get("select"), scale)
        _same(cell, _cell(d_cell), what + ": cell")
        if kw.get("normalize"):
            d_f = device.channel_factors(gpu, d_cell)
            device.correct_channels(gpu, d, factor=d_f, out=d)
            _same(factors, d_f.cpu().numpy(), what + ": factors")
        else:
            assert factors is None
        _same(out, d.cpu().numpy(), what)
        # ... and the restatement: clamp(clamp(M u) f), two applications of the rule
        want = ru.correct_channels(v, matrix=m) if "matrix" in kw else v
        _same(cell, ru.channel_sums(want, kw.get("select"), scale), what + ": restated cell")
        if kw.get("normalize"):
            want = ru.correct_channels(want, factor=ru.channel_factors(cell))
        _same(out, want, what + ": restated")
    assert v.tobytes() == before.tobytes()
    for bad in (dict(), dict(matrix=np.eye(n_ch + 1)), dict(normalize=1), dict(matrix=m, select=select[:-1] if n_rows else [1]), dict(matrix=m, scale_log2=65)):
        with pytest.raises(ValueError):
            gpu.correct_channels(v, **bad)
    with pytest.raises(ValueError):
        gpu.correct_channels(v.reshape(-1), matrix=m)


def test_refusals_leave_the_output_untouched():
    import torch
    gpu = _gpu()
    lib, h, ARG = gpu._lib, gpu._h, _lib.PYA_ERR_ARG
    dev = _dev()
    n_rows, n_ch = 70, 3
    v, m, f, select = _case(n_rows, n_ch)
    d_v, d_m, d_f, d_sel = _up(v), _up(m), _up(f), _up(select)
    out = torch.empty((n_rows, n_ch), dtype=torch.float64, device=dev)
    cell = torch.empty((n_ch, 16), dtype=torch.uint8, device=dev)
    fac = torch.empty(n_ch + 1, dtype=torch.float64, device=dev)
    for t in (out, cell, fac):
        t.view(torch.uint8).fill_(CANARY)
    V, M, F, O, S, CELL, FAC = (t.data_ptr() for t in (d_v, d_m, d_f, out, d_sel, cell, fac))
    for args in ((V, n_rows, 0, M, F, None, O), (V, n_rows, 65, M, F, None, O), (V, n_rows, n_ch, None, None, None, O),
                 (None, n_rows, n_ch, M, F, None, O), (V, n_rows, n_ch, M, F, None, None), (V + 4, n_rows, n_ch, M, F, None, O),
                 (V, n_rows, n_ch, M + 4, F, None, O), (V, n_rows, n_ch, M, F + 4, None, O), (V, n_rows, n_ch, M, F, None, O + 4),
                 (V, 0xFFFFFFFF, n_ch, M, F, None, O), (V, 1 << 40, n_ch, M, F, None, O)):
        assert lib.pya_channel_correct(h, *args) == ARG, args
    assert b"pya_channel_correct" in lib.pya_last_error(h)
    for args in ((V, n_rows, 0, S, SCALE, None, CELL), (V, n_rows, 65, S, SCALE, None, CELL), (V, n_rows, n_ch, S, 65, None, CELL),
                 (V, n_rows, n_ch, S, -65, None, CELL), (None, n_rows, n_ch, S, SCALE, None, CELL), (V, n_rows, n_ch, S, SCALE, None, None),
                 (V + 4, n_rows, n_ch, S, SCALE, None, CELL), (V, n_rows, n_ch, S, SCALE, None, CELL + 4), (V, 0xFFFFFFFF, n_ch, S, SCALE, None, CELL)):
        assert lib.pya_channel_sums(h, *args) == ARG, args
    for args in ((CELL, 0, None, FAC), (CELL, 65, None, FAC), (None, n_ch, None, FAC), (CELL, n_ch, None, None), (CELL + 4, n_ch, None, FAC),
                 (CELL, n_ch, None, FAC + 4)):
        assert lib.pya_channel_factors(h, *args) == ARG, args
    torch.cuda.synchronize(dev)
    for t in (out, cell, fac):
        assert (t.view(torch.uint8).cpu().numpy() == CANARY).all()
    assert d_v.cpu().numpy().tobytes() == v.tobytes()
    # the host form: the same, on host arrays
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    h_out = np.full((n_rows, n_ch), np.nan)
    h_out.view(np.uint8)[:] = CANARY
    h_cell = np.zeros(n_ch, ru.SITE_QUANT_DTYPE)
    h_cell.view(np.uint8)[:] = CANARY
    h_fac = np.zeros(n_ch)
    h_fac.view(np.uint8)[:] = CANARY
    NORM = _lib.PYA_CHANNEL_NORMALIZE
    for args in ((vp(v), n_rows, 0, vp(m), None, SCALE, NORM, vp(h_out), vp(h_cell), vp(h_fac)),
                 (vp(v), n_rows, 65, vp(m), None, SCALE, NORM, vp(h_out), vp(h_cell), vp(h_fac)),
                 (vp(v), n_rows, n_ch, None, None, SCALE, 0, vp(h_out), vp(h_cell), vp(h_fac)),
                 (vp(v), n_rows, n_ch, vp(m), None, 65, NORM, vp(h_out), vp(h_cell), vp(h_fac)),
                 (vp(v), n_rows, n_ch, vp(m), None, SCALE, 2, vp(h_out), vp(h_cell), vp(h_fac)),
                 (None, n_rows, n_ch, vp(m), None, SCALE, NORM, vp(h_out), vp(h_cell), vp(h_fac)),
                 (vp(v), n_rows, n_ch, vp(m), None, SCALE, NORM, None, vp(h_cell), vp(h_fac)),
                 (vp(v), n_rows, n_ch, vp(m), None, SCALE, NORM, vp(h_out), None, vp(h_fac)),
                 (vp(v), n_rows, n_ch, vp(m), None, SCALE, NORM, vp(h_out), vp(h_cell), None),
                 (vp(v), 0xFFFFFFFF, n_ch, vp(m), None, SCALE, NORM, vp(h_out), vp(h_cell), vp(h_fac))):
        assert lib.pya_channel_correct_host(h, *args) == ARG, args
    for a in (h_out, h_cell, h_fac):
        assert (a.view(np.uint8) == CANARY).all()
    # n_rows == 0 writes nothing; a good call after the refused ones gives the restatement
    assert lib.pya_channel_correct(h, None, 0, n_ch, M, None, None, None) == 0
    assert lib.pya_channel_sums(h, None, 0, n_ch, None, SCALE, None, CELL) == 0
    torch.cuda.synchronize(dev)
    assert (cell.cpu().numpy() == CANARY).all()
    assert lib.pya_channel_correct(h, V, n_rows, n_ch, M, F, torch.cuda.current_stream(dev).cuda_stream, O) == 0
    _same(out.cpu().numpy(), ru.correct_channels(v, matrix=m, factor=f), "after the refused calls")
