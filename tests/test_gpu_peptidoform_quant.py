"""Peptidoform quantification on the GPU (include/pyascore_hip.h; csrc/pform_quant.hip): the pair -- the peptidoform list and
the table row-aligned with it -- against tests/peptidoform_quant_ref.py fed with the arrays score_batch(probs=True) returns
for the same batch.  Every comparison is on the raw bytes of list, head and cell.  In every test on scored batches the quant
threshold is the median min_prob of the PSMs that contribute to the list, and peptidoform_quant_cases.threshold asserts the
coverage conditions (a quarter to three quarters contribute, a key with three contributing PSMs, a group with two isomers); the
batches repeat their peptides against other spectra.  The conditions are NOT asserted, and the threshold is the plain median, in
four places, each for a reason that lies in the input: six of the seven edge goldens (peptidoform_quant_cases.EDGE_WITHOUT_SPREAD:
every min_prob is 1.0), the 16 planted 63-site PSMs of tests/manysites.py (the same), test_wavefront_edges (it needs an exact
number of contributing PSMs on distinct keys, which rules out "a key with three") and the 200-PSM slice of the refusal test
(its subject is what is refused; the whole 400-PSM batch it is cut from meets the conditions in the plan test)."""
import ctypes as C
import os

import numpy as np
import pytest

import manysites as ms
import markers_cases as mc
import peptidoform_quant_cases as pc
import peptidoform_quant_ref as ref
import switches
from conftest import GOLDEN, golden_cases
from oracle import harness
from pyascore_amd import _lib, rollup as ru, synth

pytestmark = pytest.mark.gpu

SCALE = pc.SCALE
LIST_THR = 0.75
T = _lib.PYA_PFORM_TILE
NAN = float("nan")


def _gpu(settings, **debug):
    from pyascore_amd import PyAscore
    gpu = harness.make_scorer(PyAscore, settings)
    for k, v in debug.items():
        gpu.set_debug(k, v)
    return gpu


def _pair(res):
    return res["peptidoforms"], res["peptidoform_quant_head"], res["peptidoform_quant"]


def _ref(res, group, values, row, thr, complete_only=False, psm_id=None, psm_base=0, prev=None, cap=None, scale=SCALE):
    return ref.pair(res["best_sig"], res["ascores"], res["site_off"], res["site_probs"], res["psm_probs"], group, values, row, LIST_THR, thr,
                    scale, complete_only, psm_id=psm_id, psm_base=psm_base, prev=prev, cap=cap)


def _restated(res, group, values, row, p, **kw):
    return ru.peptidoform_quant(res["site_probs"], res["psm_probs"], res["site_off"], res["best_sig"], res["ascores"], group, values, row, p,
                                threshold=LIST_THR, **kw)


def _median(res, group):
    """the threshold where the coverage conditions cannot hold: the median, with something at or above it"""
    mp = [q for _, q, _ in pc.min_probs(res, group)]
    assert mp
    return float(np.median(mp))


def _against_yardstick(settings, batch, group, what, channels=(1, 18, 63, 64), coverage=True, skip_invalid=False, rows="psm", **debug):
    gpu = _gpu(settings, **debug)
    forms = dict(group=group, threshold=LIST_THR)
    plain = gpu.score_batch(batch, skip_invalid=skip_invalid, probs=True, peptidoforms=forms)    # the unflagged call
    n = int(batch["n_psm"])
    general = _gpu(settings, PYA_NO_PROB_CNT="1", **debug)
    seen = 0
    for n_ch in channels:
        if rows == "psm":
            values, row = pc.matrix(n_ch + n, n, n_ch), None
        else:                                                                                    # fewer rows than PSMs, some PSMs without
            values = pc.matrix(n_ch + n, max(1, n // 2), n_ch)
            row = (np.arange(n) % (values.shape[0] + 1) - 1).astype(np.int32)
        thr = pc.threshold(plain, group, row, values.shape[0]) if coverage else _median(plain, group)
        req = dict(values=values, row=row, threshold=thr, scale_log2=SCALE)
        got = gpu.score_batch(batch, skip_invalid=skip_invalid, probs=True, peptidoforms=forms, peptidoform_quant=req)
        for key in plain:                                                                        # nothing of the run or the list moves
            if key != "status_message":
                assert got[key].tobytes() == plain[key].tobytes(), (what, n_ch, key)
        assert set(got) - set(plain) == {"peptidoform_quant_head", "peptidoform_quant", "peptidoform_quant_params"}
        assert got["peptidoform_quant_params"] == ru.site_quant_params(threshold=thr, scale_log2=SCALE, n_channels=n_ch)
        want = _ref(plain, group, values, row, thr)
        pc.same(_pair(got), want, "%s, %d channels" % (what, n_ch))
        pc.same(_restated(plain, group, values, row, got["peptidoform_quant_params"]), want, "%s, %d channels: the numpy restatement" % (what, n_ch))
        alone = gpu.score_batch(batch, skip_invalid=skip_invalid, peptidoforms=forms, peptidoform_quant=dict(req, complete_only=True))
        assert "site_probs" not in alone
        pc.same(_pair(alone), _ref(plain, group, values, row, thr, complete_only=True), "%s, %d channels, complete only" % (what, n_ch))
        other = general.score_batch(batch, skip_invalid=skip_invalid, peptidoforms=forms, peptidoform_quant=req)
        pc.same(_pair(other), want, "%s, %d channels (general front end)" % (what, n_ch))
        seen += int(want[1]["n_records"].sum())
    assert seen
    return gpu, plain


@pytest.mark.parametrize("case", [c for c in golden_cases() if c.startswith(("velos_", "ties_", "edge_"))])
def test_golden_cases_equal_the_yardstick(case):
    settings, batch, _ = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    batch, peptides = pc.repeats(batch, share=pc.GOLDEN_SHARE)
    group, _, _ = ru.peptide_groups(peptides)
    _against_yardstick(settings, batch, group, case, channels=(1, 18, 64), coverage=case not in pc.EDGE_WITHOUT_SPREAD)


@pytest.mark.parametrize("seed,rows", [(9810, "psm"), (9811, "fewer")])
def test_seeded_cfg2_batches_equal_the_yardstick(seed, rows):
    batch, settings = synth.make_batch("cfg2", n_psm=300, seed=seed)
    batch, peptides = pc.repeats(batch, share=5)
    group, _, _ = ru.peptide_groups(peptides)
    _against_yardstick(settings, batch, group, "cfg2 seed %d" % seed, rows=rows)


def _flat(n):
    """n cfg2 PSMs scored once, as the arrays of score_batch(probs=True); the module keeps them and never changes them"""
    if n not in _flat.kept:
        batch, settings = synth.make_batch("cfg2", n_psm=n, seed=9820)
        gpu = _gpu(settings)
        _flat.kept[n] = (batch, settings, gpu, gpu.score_batch(batch, probs=True))
    return _flat.kept[n]


_flat.kept = {}


@pytest.mark.parametrize("n_want", [63, 64, 65, 257])
def test_wavefront_edges(n_want):
    """exactly 63 / 64 / 65 / 257 contributing PSMs -- the first so many with min_prob at or above the median; the others are
    kept out by a negative row --: all on distinct peptidoforms (a group per PSM), and the PSMs of one group interleaved with
    others so that no two are adjacent in PSM order.  (All on ONE peptidoform is the next test.)"""
    batch, settings, gpu, res = _flat(900)
    n, n_ch = 900, 18
    mp = pc.min_probs(res, np.zeros(n, np.int32))
    thr = float(np.median([q for _, q, _ in mp]))
    who = [i for i, q, _ in mp if q >= thr][:n_want]
    assert len(who) == n_want
    values = pc.matrix(n_want, n, n_ch)
    row = np.full(n, -1, np.int32)
    row[who] = np.asarray(who, np.int32)
    inter = np.arange(n, dtype=np.int32) + 1000                                       # even places of the contributing PSMs share group 5
    inter[who[::2]] = 5
    assert all(b - a > 1 for a, b in zip(who[::2], who[2::2]))
    for name, group in (("distinct", np.arange(n, dtype=np.int32)), ("interleaved", inter)):
        want = _ref(res, group, values, row, thr)
        assert int(want[1]["n_records"].sum()) == n_want, name
        assert (want[1]["n_records"] <= 1).all() if name == "distinct" else (want[1]["n_records"] >= 3).any()
        got = gpu.score_batch(batch, peptidoforms=dict(group=group, threshold=LIST_THR),
                              peptidoform_quant=dict(values=values, row=row, threshold=thr, scale_log2=SCALE))
        pc.same(_pair(got), want, "%d contributing PSMs, %s" % (n_want, name))


def test_all_psms_on_one_peptidoform():
    """ONE key for certain: a peptide with as many modifications as sites has one assignment, against 63 / 64 / 65 / 257
    spectra -- the first so many of 300 against which it is scored, so that exactly that many PSMs contribute"""
    src, settings = synth.make_batch("cfg2", n_psm=300, seed=9830)
    one, _ = synth.make_batch("cfg2", n_psm=1, seed=9831, n_sites=2, n_mod=2)
    kw1 = synth.unpack_psm(one, 0)
    gpu = _gpu(settings)
    psms = []
    for i in range(300):
        kw = synth.unpack_psm(src, i)
        psms.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw1["peptide"], n_of_mod=2, max_charge=1))
    every = gpu.score_batch(synth.pack_batch(psms), probs=True)
    scored = np.flatnonzero(every["psm_probs"]["kind"] == pc.SCORED)
    assert scored.size >= 257
    for n in (63, 64, 65, 257):
        batch = synth.pack_batch([psms[i] for i in scored[:n]])
        group = np.zeros(n, np.int32)
        res = gpu.score_batch(batch, probs=True)
        assert (res["psm_probs"]["kind"] == pc.SCORED).all()
        values = pc.matrix(n, n, 64)
        want = _ref(res, group, values, None, 0.5)
        assert want[0].size == 1 and int(want[0]["n_psm"][0]) == n and int(want[1]["n_records"][0]) == n   # (one assignment: min_prob is 1.0)
        got = gpu.score_batch(batch, peptidoforms=dict(group=group, threshold=LIST_THR),
                              peptidoform_quant=dict(values=values, threshold=0.5, scale_log2=SCALE))
        pc.same(_pair(got), want, "%d PSMs on one peptidoform" % n)


def test_psms_and_an_earlier_record_share_one_group():
    """8 PSMs on one peptidoform (built as above), 3 channels; the plan's call without an earlier pair, then the same call with
    the first call's pair as prev.  Wavefront 0 of the second launch holds 8 PSM lanes and 1 record lane on one list position:
    ONE group of 9 that mixes both kinds of entry, walked four at a time with a tail of 1.  The merge of the yardstick: 16
    records behind the one list record, every sum doubled."""
    import torch
    src, settings = synth.make_batch("cfg2", n_psm=24, seed=9830)
    one, _ = synth.make_batch("cfg2", n_psm=1, seed=9831, n_sites=2, n_mod=2)
    kw1 = synth.unpack_psm(one, 0)
    gpu = _gpu(settings)
    psms = []
    for i in range(24):
        kw = synth.unpack_psm(src, i)
        psms.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw1["peptide"], n_of_mod=2, max_charge=1))
    every = gpu.score_batch(synth.pack_batch(psms), probs=True)
    scored = np.flatnonzero(every["psm_probs"]["kind"] == pc.SCORED)
    assert scored.size >= 8
    n, n_ch = 8, 3
    batch = synth.pack_batch([psms[i] for i in scored[:n]])
    res = gpu.score_batch(batch, probs=True)
    assert (res["psm_probs"]["kind"] == pc.SCORED).all()
    group = np.zeros(n, np.int32)
    values = pc.matrix(n, n, n_ch)
    p = ru.site_quant_params(threshold=0.5, scale_log2=SCALE, n_channels=n_ch)
    dev = torch.device("cuda", 0)
    plan = _run_plan(gpu, batch, dev)
    _, sp, pp = plan.probs()
    d_group, d_values = torch.from_numpy(group).to(dev), torch.from_numpy(values).to(dev)
    first = plan.peptidoform_quant(sp, pp, d_group, d_values, p, threshold=LIST_THR)
    plan.check()
    f_pair, f_n = _down(*first)
    assert f_n == 1 and f_pair[0].size == 1                                           # the list has exactly one record
    once = _ref(res, group, values, None, 0.5)
    assert int(once[1]["n_records"][0]) == n and once[2]["sum"].any()
    pc.same(f_pair, once, "8 PSMs on one peptidoform, no earlier pair")
    d_first = tuple(t[:f_n].contiguous() for t in first[:3])
    got, count = _down(*plan.peptidoform_quant(sp, pp, d_group, d_values, p, threshold=LIST_THR, prev=d_first))
    plan.check()
    twice = _ref(res, group, values, None, 0.5, prev=f_pair)
    assert count == 1 and twice[0].size == 1 and int(twice[1]["n_records"][0]) == 2 * n
    for field in ("sum", "n", "n_saturated"):
        assert (twice[2][field] == 2 * once[2][field]).all(), field
    pc.same(got, twice, "8 PSMs and their own earlier record in one group")


# ---- the reduce calls on synthetic pairs ----
@pytest.fixture(scope="module")
def ctx():
    import torch
    from pyascore_amd.device import DevicePlan
    batch, settings = synth.make_batch("cfg2", n_psm=2, seed=9100)
    gpu = _gpu(settings)
    return gpu, DevicePlan(gpu, batch, peptidoforms=True, peptidoform_quant=True), torch.device("cuda", 0)


def _up(dev, pair):
    import torch
    records, head, cell = pair
    d = [torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(-1, 48).copy()).to(dev)]
    if head is None:
        return d[0], None, None
    d.append(torch.from_numpy(np.ascontiguousarray(head).view(np.uint8).reshape(-1, 8).copy()).to(dev))
    d.append(torch.from_numpy(np.ascontiguousarray(cell).view(np.uint8).reshape(cell.shape[0], cell.shape[1], 16).copy()).to(dev))
    return tuple(d)


def _down(records, head, cell, n):
    """the pair a device call returned, cut to its length; the rows behind the list must be zero bytes"""
    from pyascore_amd.device import peptidoform_records, site_quant_records
    n = n.cpu().numpy()
    assert int(n[1]) == 0
    m = min(int(n[0]), records.shape[0])
    h, c = site_quant_records((head.cpu().numpy(), cell.cpu().numpy()))
    assert not h[m:].tobytes().strip(b"\0") and not c[m:].tobytes().strip(b"\0"), "rows behind the list are not zero"
    return (peptidoform_records(records.cpu().numpy())[:m], h[:m], c[:m]), int(n[0])


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T + 1])
def test_reduce_over_synthetic_pairs(ctx, n):
    """PYA_PFORM_TILE edges; keys of a absent from b and the reverse; records with n_psm == 0; large groups with bit 31 clear;
    sig_bits with bit 63 set; the host form and the device form against the yardstick and the numpy merge"""
    gpu, plan, dev = ctx
    for kind, n_ch in (("zeros", 3), ("group_ends", 18), ("sig_top", 64), ("group_byte3", 1), ("distinct", 18), ("runs", 3)):
        cut = n // 3
        a = pc.synthetic_pair(cut, kind, n_ch, seed=1)
        b = pc.synthetic_pair(n - cut, kind, n_ch, seed=2)
        keys_a, keys_b = (set(zip(x[0]["group"][x[0]["n_psm"] != 0].tolist(), x[0]["sig_bits"][x[0]["n_psm"] != 0].tolist())) for x in (a, b))
        if kind == "distinct":                                  # keys of a absent from b and the reverse
            assert keys_a - keys_b and keys_b - keys_a
        if kind == "zeros":                                     # ... beside keys that both hold
            assert keys_a & keys_b
        if kind == "zeros":
            assert (a[0]["n_psm"] == 0).any() and (b[0]["n_psm"] == 0).any()
        if kind == "group_ends":
            assert (a[0]["group"] == 0x7FFFFFFF).any() and (a[0]["sig_bits"] >> np.uint64(63)).any()
        want = ref.reduce(a, b, n_ch)
        what = "%d entries, %s, %d channels" % (n, kind, n_ch)
        pc.same(ru.merge_peptidoform_quant(a, b), want, what + ": numpy merge")
        pc.same(gpu.peptidoform_quant_reduce(a, b), want, what + ": host form")
        d_a, d_b = _up(dev, a), _up(dev, b)
        got, count = _down(*plan.peptidoform_quant_reduce(d_a, d_b))
        assert count == want[0].size
        pc.same(got, want, what + ": device form")
        for d, h in ((d_a, a), (d_b, b)):                       # the inputs are only read
            assert d[0].cpu().numpy().tobytes() == h[0].tobytes() and d[2].cpu().numpy().tobytes() == h[2].tobytes()
        # a side without a table counts as all zero
        bare = (b[0], None, None)
        zero = (b[0], np.zeros_like(b[1]), np.zeros_like(b[2]))
        got_bare, _ = _down(*plan.peptidoform_quant_reduce(d_a, (d_b[0], None, None)))
        pc.same(got_bare, ref.reduce(a, zero, n_ch), what + ": b without a table")
        pc.same(gpu.peptidoform_quant_reduce(a, bare), got_bare, what + ": b without a table, host form")
        # the cap prefix
        m = want[0].size
        for cap in (0, 1, m // 2, m - 1, m + 3):
            got_cap, count = _down(*plan.peptidoform_quant_reduce(d_a, d_b, cap=cap))
            assert count == m
            pc.same(got_cap, tuple(x[:cap] for x in want), what + ": cap %d" % cap)


# ---- plans ----
def _run_plan(gpu, batch, dev):
    import torch
    from pyascore_amd.device import DevicePlan
    plan = DevicePlan(gpu, batch, peptidoform_quant=True)
    plan.run(torch.from_numpy(batch["mz"]).to(dev), torch.from_numpy(batch["intensity"]).to(dev))
    return plan


def _chain_inputs():
    batch, settings = synth.make_batch("cfg2", n_psm=400, seed=9840)
    batch, peptides = pc.repeats(batch, share=5)
    group, _, _ = ru.peptide_groups(peptides)
    return batch, settings, group


def test_prev_semantics_and_cap_on_a_plan():
    import torch
    batch, settings, group = _chain_inputs()
    gpu = _gpu(settings)
    res = gpu.score_batch(batch, probs=True)
    n, n_ch, cut = 400, 18, 170
    values = pc.matrix(21, n, n_ch)
    thr = pc.threshold(res, group)
    p = ru.site_quant_params(threshold=thr, scale_log2=SCALE, n_channels=n_ch)
    whole = _ref(res, group, values, None, thr)
    pc.same(_pair(gpu.score_batch(batch, peptidoforms=dict(group=group, threshold=LIST_THR),
                                  peptidoform_quant=dict(values=values, threshold=thr, scale_log2=SCALE))), whole, "one call")
    dev = torch.device("cuda", 0)
    d_values = torch.from_numpy(values).to(dev)
    halves = [(synth.slice_batch(batch, 0, cut), group[:cut], 0), (synth.slice_batch(batch, cut, n), group[cut:], cut)]
    plans = [_run_plan(gpu, h[0], dev) for h in halves]
    stage = []
    for plan, h in zip(plans, halves):
        _, sp, pp = plan.probs()
        stage.append((plan, sp, pp, torch.from_numpy(np.ascontiguousarray(h[1], np.int32)).to(dev), h[2]))

    def call(k, prev=None, cap=None, row=None, values=d_values):
        plan, sp, pp, d_group, base = stage[k]
        out = plan.peptidoform_quant(sp, pp, d_group, values, p, threshold=LIST_THR, psm_base=base, row=row, row_base=base, prev=prev, cap=cap)
        plan.check()
        return out

    for order in ((0, 1), (1, 0)):
        first = call(order[0])
        (f_pair, f_n) = _down(*first)
        d_first = tuple(t[:f_n].contiguous() for t in first[:3])
        got, _ = _down(*call(order[1], prev=d_first))
        pc.same(got, whole, "two plans chained, order %s" % (order,))
        # a NULL earlier table equals an all-zero one
        bare, _ = _down(*call(order[1], prev=(d_first[0], None, None)))
        zero, _ = _down(*call(order[1], prev=(d_first[0], torch.zeros_like(d_first[1]), torch.zeros_like(d_first[2]))))
        pc.same(bare, zero, "a NULL earlier table, order %s" % (order,))
        assert bare[0].tobytes() == whole[0].tobytes() and bare[1].tobytes() != whole[1].tobytes()
        # two pairs merged by the reduce call
        second = call(order[1])
        (_, s_n) = _down(*second)
        merged, _ = _down(*plans[0].peptidoform_quant_reduce(d_first, tuple(t[:s_n].contiguous() for t in second[:3])))
        pc.same(merged, whole, "two plans merged, order %s" % (order,))
        # the list equals pya_plan_peptidoforms' byte for byte
        plan, sp, pp, d_group, base = stage[order[0]]
        rec, cnt = plan.peptidoforms(sp, pp, d_group, threshold=LIST_THR, psm_base=base)
        assert rec[:f_n].cpu().numpy().tobytes() == first[0][:f_n].cpu().numpy().tobytes() and int(cnt.cpu()[0]) == f_n
    # the cap prefix on the device, with and without an earlier pair; rows behind the list are zero bytes
    first = call(0)
    (_, f_n) = _down(*first)
    d_first = tuple(t[:f_n].contiguous() for t in first[:3])
    m = whole[0].size
    for cap in (0, 1, m // 2, m - 1, m, m + 7):
        got, count = _down(*call(1, prev=d_first, cap=cap))
        assert count == m
        pc.same(got, tuple(x[:cap] for x in whole), "cap %d" % cap)
    # a row out of range: PYA_ERR_LIMIT through check(), the table untouched for that PSM, the list as it was
    plan, sp, pp, d_group, base = stage[0]
    short = d_values[:cut - 40].contiguous()
    out = plan.peptidoform_quant(sp, pp, d_group, short, p, threshold=LIST_THR)
    with pytest.raises(ValueError, match="n_rows"):
        plan.check()
    assert gpu._lib.pya_plan_check(plan._plan) == _lib.PYA_ERR_LIMIT
    got, _ = _down(*out)
    row = np.arange(cut, dtype=np.int32)
    row[cut - 40:] = -1                                                               # (what the library left out, said with negative rows)
    part = {k: v for k, v in gpu.score_batch(halves[0][0], probs=True).items()}
    pc.same(got, _ref(part, halves[0][1], values, row, thr), "rows outside write nothing")
    call(0, row=torch.full((cut,), -1, dtype=torch.int32, device=dev))                # negative: silently nothing, and the report is gone
    # refusals of the plan call
    c_p = ru.site_quant_c_params(p)
    work_bytes = int(gpu._lib.pya_peptidoform_quant_workspace_bytes(cut + f_n, n_ch))
    assert work_bytes >= int(gpu._lib.pya_peptidoform_workspace_bytes(cut + f_n))
    work = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
    o_rec = torch.empty((cut + f_n, 48), dtype=torch.uint8, device=dev)
    o_head = torch.empty((cut + f_n, 8), dtype=torch.uint8, device=dev)
    o_cell = torch.empty((cut + f_n, n_ch, 16), dtype=torch.uint8, device=dev)
    o_n = torch.empty(2, dtype=torch.int32, device=dev)

    def raw(prev_head=d_first[1].data_ptr(), prev_cell=d_first[2].data_ptr(), params=c_p, wb=work_bytes, head=o_head.data_ptr()):
        return gpu._lib.pya_plan_peptidoform_quant(plan._plan, C.byref(plan._res), None, sp.data_ptr(), pp.data_ptr(), d_group.data_ptr(), LIST_THR,
                                                   None, 0, d_first[0].data_ptr(), prev_head, prev_cell, f_n, d_values.data_ptr(), n, None, 0,
                                                   C.byref(params), work.data_ptr(), wb, o_rec.data_ptr(), head, o_cell.data_ptr(), cut + f_n,
                                                   o_n.data_ptr())
    assert raw() == 0
    assert raw(prev_head=None) == _lib.PYA_ERR_ARG and raw(prev_cell=None) == _lib.PYA_ERR_ARG      # exactly one NULL earlier-table pointer
    assert raw(wb=work_bytes - 1) == _lib.PYA_ERR_ARG                                               # a workspace one byte short
    assert raw(head=None) == _lib.PYA_ERR_ARG
    for bad in (dict(n_channels=0), dict(n_channels=65), dict(threshold=NAN), dict(scale_log2=65), dict(flags=2), dict(reserved=1)):
        c_bad = ru.site_quant_c_params(p)
        for k, v in bad.items():
            setattr(c_bad, k, v)
        assert raw(params=c_bad) == _lib.PYA_ERR_ARG, bad
    assert raw() == 0
    torch.cuda.synchronize()
    plan.check()


def test_chunked_shared_and_marker_chain(monkeypatch):
    """chunk cuts forced small against the uncut call; a shared batch in and out of spectrum order with spec_of as the rows;
    values=None beside markers=; together with rollup= / quant= in one call"""
    tol = 0.05
    settings, spectra, psms, pm, pz = pc.shared_inputs(tol)
    gpu = _gpu(settings)
    marks = dict(mz=mc.REPORTERS, losses=(mc.LOSS_H3PO4,), tol=tol, precursor_mz=pm, precursor_charge=pz)
    for what, order in pc.SHARED_ORDERS:
        mine = [psms[q] for q in order]
        shared = synth.pack_shared_batch(spectra, mine)
        flat = gpu.score_batch(synth.expand_shared_batch(shared), probs=True)
        group, _, _ = ru.peptide_groups([q["peptide"] for q in mine])
        thr = pc.threshold(flat, group)
        forms = dict(group=group, threshold=LIST_THR)
        values = pc.matrix(5, len(spectra), 18)
        spec_of = np.asarray(shared["spec_of"]).astype(np.int32)
        want = _ref(flat, group, values, spec_of, thr)
        got = gpu.score_batch(shared, peptidoforms=forms, peptidoform_quant=dict(values=values, row=spec_of, threshold=thr, scale_log2=SCALE))
        pc.same(_pair(got), want, what)
        with_m = gpu.score_batch(shared, peptidoforms=forms, markers=marks)
        matrix = np.ascontiguousarray(ru.marker_matrix(with_m["markers"])[:, :10])
        chained = gpu.score_batch(shared, peptidoforms=forms, markers=marks, peptidoform_quant=dict(values=None, threshold=thr, scale_log2=SCALE))
        pc.same(_pair(chained), _ref(flat, group, matrix, spec_of, thr), what + ": values=None beside markers=")
        assert chained["peptidoform_quant_params"]["n_channels"] == 10
        # together with rollup= / quant= in one call: neither table moves
        slot, n_slots, _ = ru.peptide_slots([q["peptide"] for q in mine], flat["site_off"], residues=settings["mod_group"])
        roll = dict(slot=slot, n_slots=n_slots)
        sq = dict(values=values, row=spec_of, threshold=thr, scale_log2=SCALE)
        sites = gpu.score_batch(shared, rollup=roll, quant=sq)
        both = gpu.score_batch(shared, rollup=roll, quant=sq, peptidoforms=forms, peptidoform_quant=sq)
        pc.same(_pair(both), want, what + ": beside rollup= and quant=")
        for key in ("rollup", "quant_head", "quant"):
            assert both[key].tobytes() == sites[key].tobytes(), (what, key)
    # chunk cuts
    # (the library pipelines a call from 32 MiB of spectra on: 7 000 cfg2 PSMs are 34 MiB, the smallest batch it cuts)
    settings, big, peptides, row = pc.chunked_inputs()
    group, _, _ = ru.peptide_groups(peptides)
    gpu = _gpu(settings)
    monkeypatch.setenv("PYA_NO_CHUNKS", "1")
    switches.from_env(gpu)
    plain = gpu.score_batch(big, probs=True)
    thr = pc.threshold(plain, group, row, pc.CHUNKED_ROWS)
    forms = dict(group=group, threshold=LIST_THR)
    values = pc.matrix(11, pc.CHUNKED_ROWS, 3)
    req = dict(values=values, row=row, threshold=thr, scale_log2=SCALE)
    uncut = gpu.score_batch(big, peptidoforms=forms, peptidoform_quant=req)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) == 1
    monkeypatch.delenv("PYA_NO_CHUNKS")
    monkeypatch.setenv("PYA_CHUNK_MB", "2")
    switches.from_env(gpu)
    cut = gpu.score_batch(big, peptidoforms=forms, peptidoform_quant=req, evidence=True)
    assert gpu._lib.pya_debug_last_chunks(gpu._h) > 8
    none = gpu.score_batch(big, peptidoforms=forms, peptidoform_quant=dict(req, row=None, values=pc.matrix(12, 7000, 3)))
    listed = gpu.score_batch(big, peptidoforms=forms)
    monkeypatch.delenv("PYA_CHUNK_MB")
    switches.from_env(gpu)
    want = _ref(plain, group, values, row, thr)
    pc.same(_pair(uncut), want, "uncut")
    pc.same(_pair(cut), want, "chunked")
    pc.same(_pair(none), _ref(plain, group, pc.matrix(12, 7000, 3), None, thr), "chunked, row None: the PSM's place in the batch")
    assert listed["peptidoforms"].tobytes() == want[0].tobytes()


def test_batch_refusals_and_the_c_abi():
    batch, settings, group = _chain_inputs()
    batch, group = synth.slice_batch(batch, 0, 200), group[:200]
    gpu = _gpu(settings)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    head, cell = ru.empty_site_quant(4, 3)
    assert gpu._lib.pya_last_batch_peptidoform_quant(gpu._h, vp(head), vp(cell), 4, 3) == _lib.PYA_ERR_STATE
    assert b"PYA_FLAG_PFORM_QUANT" in gpu._lib.pya_last_error(gpu._h)
    res = gpu.score_batch(batch, probs=True)
    thr = _median(res, group)
    values = pc.matrix(17, 200, 3)
    forms = dict(group=group, threshold=LIST_THR)
    req = dict(values=values, threshold=thr, scale_log2=SCALE)
    with pytest.raises(ValueError, match="peptidoforms="):                           # the keyword without peptidoforms=
        gpu.score_batch(batch, peptidoform_quant=req)
    want = _ref(res, group, values, None, thr)
    got = gpu.score_batch(batch, peptidoforms=forms, peptidoform_quant=req)
    pc.same(_pair(got), want, "one call")
    m = want[0].size
    back = ru.empty_site_quant(m, 3)
    assert gpu._lib.pya_last_batch_peptidoform_quant(gpu._h, vp(back[0]), vp(back[1]), m, 3) == 0
    pc.same((want[0],) + back, want, "pya_last_batch_peptidoform_quant")
    assert gpu._lib.pya_last_batch_peptidoform_quant(gpu._h, vp(back[0]), vp(back[1]), m - 1, 3) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_last_batch_peptidoform_quant(gpu._h, vp(back[0]), vp(back[1]), m, 4) == _lib.PYA_ERR_ARG
    gpu.score_batch(batch, peptidoforms=forms)
    assert gpu._lib.pya_last_batch_peptidoform_quant(gpu._h, vp(back[0]), vp(back[1]), m, 3) == _lib.PYA_ERR_STATE
    # the C ABI: the flag without the list's flag, the flag without a loan, the refusals of the loan
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
    flag, pf = _lib.PYA_FLAG_PFORM_QUANT, _lib.PYA_FLAG_PEPTIDOFORMS
    assert gpu._lib.pya_set_peptidoform_quant(gpu._h, vp(values), 200, None, 200, C.byref(c_params)) == 0
    assert gpu._lib.pya_score_batch(gpu._h, C.byref(b), vp(mz), vp(it), flag, C.byref(rs)) == _lib.PYA_ERR_ARG
    assert b"PYA_FLAG_PEPTIDOFORMS" in gpu._lib.pya_last_error(gpu._h)
    assert gpu._lib.pya_set_peptidoforms(gpu._h, vp(group), 200, LIST_THR, None) == 0
    assert gpu._lib.pya_score_batch(gpu._h, C.byref(b), vp(mz), vp(it), flag | pf, C.byref(rs)) == _lib.PYA_ERR_ARG
    assert b"pya_set_peptidoform_quant" in gpu._lib.pya_last_error(gpu._h)           # (the loan ended with the refused call)
    assert gpu._lib.pya_set_peptidoform_quant(gpu._h, vp(values), 200, None, 199, C.byref(c_params)) == 0
    assert gpu._lib.pya_set_peptidoforms(gpu._h, vp(group), 200, LIST_THR, None) == 0
    assert gpu._lib.pya_score_batch(gpu._h, C.byref(b), vp(mz), vp(it), flag | pf, C.byref(rs)) == _lib.PYA_ERR_ARG
    assert b"199 PSMs" in gpu._lib.pya_last_error(gpu._h)
    for change in (dict(scale_log2=65), dict(n_channels=0), dict(n_channels=65), dict(flags=2), dict(reserved=1), dict(threshold=NAN)):
        bad = ru.site_quant_c_params(ru.site_quant_params(threshold=thr, n_channels=3))
        for k, v in change.items():
            setattr(bad, k, v)
        assert gpu._lib.pya_set_peptidoform_quant(gpu._h, vp(values), 200, None, 200, C.byref(bad)) == _lib.PYA_ERR_ARG, change
    assert gpu._lib.pya_set_peptidoform_quant(gpu._h, None, 200, None, 200, C.byref(c_params)) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_set_peptidoform_quant(gpu._h, vp(values), 200, None, 200, None) == _lib.PYA_ERR_ARG
    # a row at or above n_rows: the limit error; the next call is as before
    with pytest.raises(ValueError, match="n_rows"):
        gpu.score_batch(batch, peptidoforms=forms, peptidoform_quant=dict(req, values=values[:150]))
    pc.same(_pair(gpu.score_batch(batch, peptidoforms=forms, peptidoform_quant=req)), want, "after the refused calls")
    # the reduce calls' refusals
    a = pc.synthetic_pair(10, "distinct", 3)
    for bad in ((a, (a[0], a[1], None)), ((a[0], None, None), (a[0], None, None))):
        with pytest.raises(ValueError):
            gpu.peptidoform_quant_reduce(*bad)
    out = (np.zeros(20, ref.DTYPE),) + ru.empty_site_quant(20, 3)
    cnt = C.c_uint64(0)
    args = (gpu._h, vp(a[0]), vp(a[1]), vp(a[2]), 10, vp(a[0]), vp(a[1]), vp(a[2]), 10)
    tail = (vp(out[0]), vp(out[1]), vp(out[2]), 20, C.byref(cnt))
    assert gpu._lib.pya_peptidoform_quant_reduce_host(*args, 3, *tail) == 0 and cnt.value == 10
    assert gpu._lib.pya_peptidoform_quant_reduce_host(*args, 0, *tail) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_peptidoform_quant_reduce_host(*args, 65, *tail) == _lib.PYA_ERR_ARG
    assert gpu._lib.pya_peptidoform_quant_reduce_host(gpu._h, vp(a[0]), vp(a[1]), None, 10, None, None, None, 0, 3, *tail) == _lib.PYA_ERR_ARG
    # pya_score_one refuses the flag
    kw = synth.unpack_psm(batch, 0)
    m1, i1 = np.ascontiguousarray(kw["mz_arr"], np.float64), np.ascontiguousarray(kw["int_arr"], np.float64)
    pep = np.frombuffer(kw["peptide"].encode(), np.uint8)
    one = (np.zeros(1, np.float32), np.zeros(1, np.uint64), np.zeros(1, np.int32), np.zeros((1, 4), np.float32), np.zeros((1, 4), np.uint64))
    r1 = _lib.Results(4, *[vp(x) for x in one])
    rc = gpu._lib.pya_score_one(gpu._h, vp(m1), vp(i1), m1.size, vp(pep), pep.size, int(kw["n_of_mod"]), int(kw["max_fragment_charge"]), None, None, 0,
                                flag, C.byref(r1))
    assert rc == _lib.PYA_ERR_ARG and b"PYA_FLAG_PFORM_QUANT" in gpu._lib.pya_last_error(gpu._h)
    # a batch of none
    empty = gpu.score_batch(synth.slice_batch(batch, 0, 0), peptidoforms=dict(group=np.zeros(0, np.int32)), peptidoform_quant=dict(values=values))
    assert empty["peptidoforms"].size == 0 and empty["peptidoform_quant_head"].shape == (0,) and empty["peptidoform_quant"].shape == (0, 3)


def test_psms_with_31_to_63_modifiable_residues():
    """a best_sig above bit 31 reaches the search key: the high-word isomers of tests/manysites.py, every peptide against four
    spectra, two of them on one key"""
    batch, group, _ = ms.isomer_batch()
    settings = ms.BASE_SETTINGS
    gpu = _gpu(settings)
    res = gpu.score_batch(batch, probs=True)
    assert (res["best_sig"] >> np.uint64(32)).any()
    n = int(batch["n_psm"])
    values = pc.matrix(3, n, 18)
    thr = _median(res, group)                                                         # (16 planted PSMs: min_prob is 1.0 nearly throughout)
    want = _ref(res, group, values, None, thr)
    assert (want[0]["sig_bits"] >> np.uint64(32)).any() and (want[1]["n_records"] >= 2).any() and (want[0]["n_isomers"] >= 2).any()
    got = gpu.score_batch(batch, peptidoforms=dict(group=group, threshold=LIST_THR),
                          peptidoform_quant=dict(values=values, threshold=thr, scale_log2=SCALE))
    pc.same(_pair(got), want, "high-word isomers")
    pc.same(_restated(res, group, values, None, got["peptidoform_quant_params"]), want, "high-word isomers: the numpy restatement")


def test_command_line_driver_end_to_end(tmp_path):
    """batch_cli.localize(peptidoform_quant=...) and write_peptidoform_quant_tsv on a toy run: three peptides against five scans
    each, one PSM per scan; every scan carries two planted reporter peaks, 2^(12 + k) and twice that for scan k, so the sum of a
    row's first channel names the scans behind it.  With a threshold below every probability all listed PSMs contribute: every
    row's scans must be exactly the PSMs of that peptide that the main table reports with ONE localisation."""
    from pyascore_amd import PyAscore, batch_cli
    phospho, targets = 79.966331, (126.5, 127.5)
    rng = np.random.default_rng(11)
    spectra, psms = {}, []
    for k in range(15):
        pep = ("ASTLGYKR", "KSTAYSGLSTR", "MSTYLKAGSR")[k % 3]
        mz = np.sort(np.concatenate([targets, rng.uniform(130.0, 1500.0, 180)]))
        it = rng.lognormal(5, 1, mz.size)
        it[:2] = 2.0 ** (12 + k), 2.0 ** (13 + k)
        spectra[100 + k] = dict(mz_values=mz, intensity_values=it, precursor_charge=2)
        site = [i + 1 for i, c in enumerate(pep) if c in "STY"][0]
        psms.append(dict(scan=100 + k, charge_state=2, peptide=pep, mod_positions=np.array([site], np.int32), mod_masses=np.array([phospho])))
    gpu = PyAscore(100.0, 10, "STY", phospho, 0.05, "by")
    table, quant_rows, marker_rows = [], [], []
    rows = batch_cli.localize(gpu, psms, spectra, "STY", phospho, hit_depth=1, max_fragment_charge=1, peptidoform_table=table,
                              markers=dict(mz=targets), marker_rows=marker_rows, peptidoform_quant=dict(threshold=-1.0, scale_log2=0),
                              peptidoform_quant_rows=quant_rows)
    assert len(rows) == 15 and len(quant_rows) == len(table) >= 3
    width = len(batch_cli.PEPTIDOFORM_TABLE_COLUMNS)
    reported = {}                                                                     # (peptide, localisation) -> scans, from the main table
    for row in rows:
        k = int(row[0]) - 100
        reported.setdefault((psms[k]["peptide"], row[1]), set()).add(k)
    seen = set()
    for row, plain in zip(quant_rows, table):
        assert row[:width] == plain and len(row) == width + 4                          # the columns of --peptidoform_table first, row-aligned
        records, complete, first, second = int(row[width]), int(row[width + 1]), float(row[width + 2]), float(row[width + 3])
        assert records == complete == int(row[2]) and second == 2.0 * first and first == int(first)
        scans = {k for k in range(15) if (int(first) >> (12 + k)) & 1}
        assert int(first) == sum(1 << (12 + k) for k in scans) and len(scans) == records
        assert {psms[k]["peptide"] for k in scans} == {row[0]}
        assert scans in [v for (pep, _), v in reported.items() if pep == row[0]], "a row's scans are not those of one reported localisation"
        assert not scans & seen
        seen |= scans
    assert seen == set(range(15))
    out = tmp_path / "pq.tsv"
    batch_cli.write_peptidoform_quant_tsv(quant_rows, str(out), mz=targets)
    lines = out.read_text().splitlines()
    assert lines[0].split("\t") == list(batch_cli.peptidoform_quant_columns(targets)) and len(lines) == len(quant_rows) + 1
    assert lines[1].split("\t") == [str(f) for f in quant_rows[0]]
