"""The binning stage observed directly: the retained-peak table the kernels leave in the workspace
(include/pyascore_debug.h: pya_debug_retained_table / pya_debug_plan_retained_table) against the reference's own
BinnedSpectra (oracle/_ref), entry by entry, on the spectrum families of tests/binedges.py -- peaks on and next to every
window border, bin sizes whose FLOAT window count is one below the exact one, extremes on multiples of 100, 1 .. 65 535
windows, every peak order, the intensity regimes of test_gpu_parity.py.

Three copies of the window arithmetic produce that table (bin_fast and bin_exact of csrc/bin_core.hip.h, bin_select of
csrc/bin_select.hip.h), reached by seven kernels in three element-type instantiations each.  Every copy is driven here:

  tiny            a float64 batch of at most PYA_TINY_MAX PSMs under production switches (pya_tiny_batch_kernel)
  fast            PYA_NO_TINY: pya_bin_spectra_kernel / pya_bin_select_kernel by peak class, as a big batch is binned (typed
                  batches take this route under production switches)
  all_pairs       PYA_BIN_SELECT_MIN huge: bin_fast for every class
  select_forced   PYA_BIN_SELECT_MIN=0: bin_select for every class
  select_overflow ... with 64 survivor slots: nearly everything is handed over to the exact kernel
  exact           PYA_DEBUG=128: every spectrum through pya_bin_exact_kernel
  score()         pya_one_kernel (float64 only); a shared batch; a device.DevicePlan run; more than 8 192 peaks
                  (pya_bin_global_kernel)

each with float64, float64 m/z + float32 intensity, and float32 spectra (synth.narrow_batch; the reference gets the widened
arrays).  The same batches go through score_batch against the checker, so the stages behind the binning are seen to cope with
one window and with 65 535."""
import ctypes as C

import numpy as np
import pytest

import binedges
import switches
from conftest import checker_kind
from oracle import harness, orc
from pyascore_amd import synth

pytestmark = pytest.mark.gpu

KEYS = ("n_sig", "best_sig", "best_score", "alt_mask", "ascores")
TYPES = {"f64_f64": (np.float64, np.float64), "f64_f32": (np.float64, np.float32), "f32_f32": (np.float32, np.float32)}
NO_TINY = {"PYA_NO_TINY": "1"}
ROUTES = {"tiny": {}, "fast": NO_TINY, "all_pairs": dict(NO_TINY, PYA_BIN_SELECT_MIN="1000000"),
          "select_forced": dict(NO_TINY, PYA_BIN_SELECT_MIN="0"),
          "select_overflow": dict(NO_TINY, PYA_BIN_SELECT_MIN="0", PYA_BIN_SELECT_SCAP="64"), "exact": dict(NO_TINY, PYA_DEBUG="128")}
ROUTE_VARS = ("PYA_NO_TINY", "PYA_BIN_SELECT_MIN", "PYA_BIN_SELECT_SCAP", "PYA_DEBUG")


def _gpu(settings):
    from pyascore_amd import PyAscore
    return harness.make_scorer(PyAscore, settings)


def _route(gpu, monkeypatch, route):
    for name in ROUTE_VARS:
        monkeypatch.delenv(name, raising=False)
    for name, v in ROUTES[route].items():
        monkeypatch.setenv(name, v)
    switches.from_env(gpu)
    for name in ROUTES[route]:
        monkeypatch.delenv(name, raising=False)


def _table(gpu, index, room, plan=None):
    """(m/z, rank, status) of entry `index` of the scorer's retained plan, or of a DevicePlan"""
    mz, rank = np.full(room + 2, np.nan, np.float32), np.zeros(room + 2, np.uint32)
    n, st = C.c_uint64(), C.c_int32(-1)
    if plan is None:
        rc = gpu._lib.pya_debug_retained_table(gpu._h, index, mz.ctypes.data, rank.ctypes.data, room, C.byref(n), C.byref(st))
    else:
        rc = gpu._lib.pya_debug_plan_retained_table(plan._plan, index, mz.ctypes.data, rank.ctypes.data, room, C.byref(n), C.byref(st))
    assert rc == 0, gpu._lib.pya_last_error(gpu._h)
    return mz[: n.value], rank[: n.value], st.value


def _expected(settings, psms, types):
    """per PSM: the reference's table of the arrays as the device gets them (narrowed, then widened), or the status it must get"""
    out = []
    for p in psms:
        mz = np.asarray(p["mz"], types[0]).astype(np.float64)
        if binedges.expected_status(settings, mz):
            out.append(binedges.expected_status(settings, mz))
            continue
        it = np.asarray(p["intensity"], types[1]).astype(np.float64)
        out.append(binedges.expected_table(binedges.reference_binned(settings, mz, it, kind=checker_kind())))
    return out


def _check_table(got, want, what):
    mz, rank, status = got
    if isinstance(want, int):
        assert status == want and mz.size == 0, "%s: status %d with %d entries, expected status %d" % (what, status, mz.size, want)
        return
    assert status == 0, "%s: binning status %d" % (what, status)
    assert mz.size == want[0].size, "%s: %d retained peaks, the reference has %d" % (what, mz.size, want[0].size)
    assert np.all(mz[1:] >= mz[:-1]), "%s: the table is not in m/z order" % what
    o = np.lexsort((rank, mz))
    bad = np.flatnonzero((mz[o] != want[0]) | (rank[o] != want[1]))
    assert bad.size == 0, "%s: entry %d is (%r, %d), the reference has (%r, %d); %d entries differ" % (
        what, bad[0], mz[o][bad[0]], rank[o][bad[0]], want[0][bad[0]], want[1][bad[0]], bad.size)


def _check_tables(gpu, psms, want, what, index=None, plan=None):
    for i, p in enumerate(psms):
        _check_table(_table(gpu, i if index is None else index[i], len(p["mz"]), plan), want[i], "%s, PSM %d" % (what, i))


def _check_scores(got, want, good, what):
    for key in KEYS:
        bad = np.flatnonzero(np.any(np.atleast_2d((got[key][good] != want[key]).T), axis=0))
        assert bad.size == 0, "%s: %s differs from the checker for PSMs %s" % (what, key, good[bad][:10])


def _case(monkeypatch, cid, settings, psms, note, routes=tuple(ROUTES), types=tuple(TYPES), extras=True):
    """one batch of a family: every route x element type, tables against the reference, results against the checker"""
    gpu = _gpu(settings)
    chk = harness.make_scorer(orc.OracleAscore, settings, kind=checker_kind())
    batch = synth.pack_batch(psms)
    max_k = int(batch["n_of_mod"].max())
    for t in types:
        nb = synth.narrow_batch(batch, *TYPES[t])
        want_tab = _expected(settings, psms, TYPES[t])
        codes = np.asarray([w if isinstance(w, int) else 0 for w in want_tab], np.int32)
        if t == "f64_f64":
            assert np.array_equal(codes, [p.get("expect_status", 0) for p in psms]), cid
        good = np.flatnonzero(codes == 0)
        alone = synth.pack_batch([psms[i] for i in good])
        want = chk.score_batch(synth.widen_batch(synth.narrow_batch(alone, *TYPES[t])), max_k)
        for route in routes:
            if route == "tiny" and t != "f64_f64":
                continue                                   # (typed batches never take the tiny kernel: "fast" is their production route)
            what = "%s (%s) %s / %s" % (cid, note, t, route)
            _route(gpu, monkeypatch, route)
            if codes.any():
                with pytest.raises(ValueError):
                    gpu.score_batch(nb, keep=True)
            got = gpu.score_batch(nb, keep=True, skip_invalid=bool(codes.any()))
            if codes.any():
                assert np.array_equal(got["status"], codes), "%s: status %s" % (what, got["status"])
                assert np.all(got["n_sig"][codes != 0] == -1) and np.all(got["best_score"][codes != 0] == -1.0), what
            _check_tables(gpu, psms, want_tab, what)
            _check_scores(got, want, good, what)
        if not extras:
            continue
        _route(gpu, monkeypatch, "tiny")                   # (production switches)
        # a shared batch: two hits per spectrum, tables by spectrum number; every hit of a bad spectrum gets its code
        hits = [dict(spectrum=i // 2, peptide=psms[i // 2]["peptide"] if i % 2 == 0 else binedges.PEPTIDES[(i // 2 + 1) % 4],
                     n_of_mod=1, max_charge=1 + i % 2) for i in range(2 * len(psms))]
        spectra = [dict(mz=np.asarray(p["mz"], TYPES[t][0]), intensity=np.asarray(p["intensity"], TYPES[t][1])) for p in psms]
        shared = synth.pack_shared_batch(spectra, hits)
        got = gpu.score_batch(shared, keep=True, skip_invalid=bool(codes.any()))
        if codes.any():
            assert np.array_equal(got["status"], np.repeat(codes, 2)), "%s %s shared: status %s" % (cid, t, got["status"])
        _check_tables(gpu, psms, want_tab, "%s (%s) %s / shared" % (cid, note, t))
        sgood = np.flatnonzero(np.repeat(codes, 2) == 0)
        exp = synth.widen_batch(synth.expand_shared_batch(synth.take_psms(shared, sgood)))
        _check_scores(got, chk.score_batch(exp, 1), sgood, "%s %s shared" % (cid, t))
        # a device-resident plan
        import torch
        from pyascore_amd.device import DevicePlan
        dev = torch.device("cuda", gpu.device)
        plan = DevicePlan(gpu, nb)
        plan.run(torch.from_numpy(nb["mz"]).to(dev), torch.from_numpy(nb["intensity"]).to(dev))
        _check_tables(gpu, psms, want_tab, "%s (%s) %s / DevicePlan" % (cid, note, t), plan=plan)
        if codes.any():
            with pytest.raises(ValueError):
                plan.check()
        else:
            plan.check()
            _check_scores({k: getattr(plan, k).cpu().numpy().view(want[k].dtype) for k in KEYS}, want, good, "%s %s DevicePlan" % (cid, t))
        plan.close()
    if not extras:
        return
    # PyAscore.score(): the one-PSM kernel bins with four wavefronts and stores its table like the batch kernels do.  A scorer
    # of its own per call: it retains nothing, so the read-back answers from the workspace of that one call.
    want_tab = _expected(settings, psms, TYPES["f64_f64"])
    codes = np.asarray([p.get("expect_status", 0) for p in psms], np.int32)
    good = np.flatnonzero(codes == 0)
    want = chk.score_batch(synth.pack_batch([psms[i] for i in good]), max_k)
    for i in list(range(len(psms)))[:: max(1, len(psms) // 6)]:
        p = psms[i]
        one = _gpu(settings)
        args = (p["mz"], p["intensity"], p["peptide"], int(p["n_of_mod"]), int(p["max_charge"]))
        if codes[i]:
            with pytest.raises(ValueError):
                one.score(*args)
        else:
            one.score(*args)
            assert np.float32(one.best_score) == want["best_score"][int(np.flatnonzero(good == i)[0])], (cid, i)
        _check_table(_table(one, 0, len(p["mz"])), want_tab[i], "%s (%s) score() of PSM %d" % (cid, note, i))


@pytest.mark.parametrize("family", list(binedges.FAMILIES))
def test_retained_tables_equal_the_reference(family, monkeypatch):
    for cid, settings, psms, note in binedges.cases(family):
        _case(monkeypatch, cid, settings, psms, note)


def test_retained_tables_with_thousands_of_windows(monkeypatch):
    """4 096 .. 65 535 windows: the composite keys have room for 64, so everything here is handed over to the exact body; the
    scoring and localisation behind it see tables that span 65 535 windows"""
    for cid, settings, psms, note in binedges.cases("window_counts_large"):
        _case(monkeypatch, cid, settings, psms, note)


def test_too_many_windows_is_a_status(monkeypatch):
    """65 536 windows and more: PYA_PSM_TOO_MANY_WINDOWS on every binning route, a ValueError without skip_invalid, every hit of
    a shared spectrum; the siblings in the batch are binned and scored as they are alone"""
    for cid, settings, psms, note in binedges.cases("too_many_windows"):
        _case(monkeypatch, cid, settings, psms, note)


def test_read_back_refuses_what_it_cannot_answer():
    settings, psms, _ = binedges.borders()[0]
    gpu = _gpu(settings)
    lib = gpu._lib
    n, st = C.c_uint64(), C.c_int32()
    buf = np.zeros(4096, np.float32), np.zeros(4096, np.uint32)
    call = lambda index, cap: lib.pya_debug_retained_table(gpu._h, index, buf[0].ctypes.data, buf[1].ctypes.data, cap, C.byref(n), C.byref(st))
    assert call(0, 4096) == -1                             # nothing retained, no score() yet
    gpu.score_batch(synth.pack_batch(psms), keep=True)
    assert call(len(psms), 4096) == -1                     # index out of range
    assert call(0, 3) == -1 and n.value > 3                # too little room: *n says how much is needed
    full = n.value
    assert call(0, full) == 0 and n.value == full
    assert lib.pya_debug_plan_retained_table(None, 0, None, None, 0, C.byref(n), C.byref(st)) == -1
    # a PSM the host pre-pass set aside was never binned: refused, with its code
    bad = dict(psms[1], peptide="AAXBZ")
    gpu.score_batch(synth.pack_batch([psms[0], bad]), keep=True, skip_invalid=True)
    assert call(0, 4096) == 0 and call(1, 4096) == -1 and st.value == 16


def test_more_than_8192_peaks(monkeypatch):
    """pya_bin_global_kernel (arrays in the workspace instead of LDS): borders, a cut-off stretch, shuffled peaks"""
    a = binedges.dense(7001, 400, 1200, 100.0, per_window=1100)
    b = binedges.dense(7002, 400, 1200, 100.0, per_window=1100, first_bright=False, narrow=True)
    rng = np.random.default_rng(7003)
    o = rng.permutation(a[0].size)
    psms = [binedges.psm(*a, 0), binedges.psm(*b, 1), binedges.psm(a[0][o], a[1][o], 2), binedges.psm(*binedges.dense(7004, 400, 1200, 100.0), 3)]
    assert all(len(p["mz"]) > 8192 for p in psms[:3])
    _case(monkeypatch, "global/0", binedges._settings(100.0), psms, "8 windows", routes=("fast", "exact"), extras=False)
    bs = np.float32(100 / 3)
    c = binedges.dense(7005, 400, 500, bs, per_window=2300)
    d = binedges.dense(7006, 400, 500, bs, per_window=2300, tie=True)
    psms = [binedges.psm(*c, 0), binedges.psm(*d, 1)]
    assert all(len(p["mz"]) > 8192 for p in psms)
    _case(monkeypatch, "global/1", binedges._settings(bs), psms, "3 windows in float, 4 exactly", routes=("fast",), extras=False)
