"""Site FLR on the GPU (pya_site_flr: a roll-up table sorted by best_prob, scanned into false-localisation rates).
Yardstick: tests/flr_ref.py on the same table -- records, order and n_ranked are compared byte for byte, through the host
form (PyAscore.rollup_flr) and the device form (DevicePlan.rollup_flr).  The tables are built as records (tests/flr_tables.py)."""
import ctypes as C

import numpy as np
import pytest

import flr_ref
import flr_tables
from oracle import harness
from pyascore_amd import _lib, rollup as ru, synth

pytestmark = pytest.mark.gpu

T = _lib.PYA_FLR_TILE
GUARD = 256


@pytest.fixture(scope="module")
def ctx():
    import torch
    from pyascore_amd import PyAscore
    from pyascore_amd.device import DevicePlan
    batch, settings = synth.make_batch("cfg2", n_psm=2, seed=9100)
    gpu = harness.make_scorer(PyAscore, settings)
    return gpu, DevicePlan(gpu, batch, rollup=True), torch.device("cuda", 0)


_wanted = {}


def _want(n, kind):
    """the table and the yardstick's answer, computed once per case and never changed"""
    if (n, kind) not in _wanted:
        table, cls, flag = flr_tables.make(n, kind)
        want = flr_ref.flr(table, cls, flag)
        for a in (table, want[0], want[1]) + (() if cls is None else (cls,)):
            a.setflags(write=False)
        _wanted[(n, kind)] = (table, cls, flag, want)
    return _wanted[(n, kind)]


def _same(got, want, what):
    rec, order, n_ranked = got
    assert int(n_ranked) == want[2], what
    assert rec.dtype.itemsize == 32 and rec.shape == want[0].shape, what
    bad = np.flatnonzero(np.asarray(rec).view("V32") != want[0].view("V32"))
    assert bad.size == 0, "%s: %d records differ, first slot %d: got %s, want %s" % (what, bad.size, bad[0], rec[bad[0]], want[0][bad[0]])
    bad = np.flatnonzero(np.asarray(order) != want[1])
    assert bad.size == 0, "%s: order differs at %d positions, first %d: got %d, want %d" % (what, bad.size, bad[0], order[bad[0]], want[1][bad[0]])


def _device(ctx, table, cls, flag):
    import torch
    from pyascore_amd.device import flr_records
    gpu, plan, dev = ctx
    d_table = torch.from_numpy(np.ascontiguousarray(table).view(np.uint8).reshape(-1, 32).copy()).to(dev)
    d_cls = None if cls is None else torch.from_numpy(np.array(cls)).to(dev)
    rec, order, nr = plan.rollup_flr(d_table, d_cls, reported_only=flag)
    nr = nr.cpu().numpy()
    assert d_table.cpu().numpy().tobytes() == table.tobytes(), "the stage wrote into the table"
    return (flr_records(rec.cpu().numpy()), order.cpu().numpy().view(np.uint32), nr[0]), int(nr[1])


def _both(ctx, n, kind):
    table, cls, flag, want = _want(n, kind)
    _same(ctx[0].rollup_flr(table, cls, reported_only=flag), want, "host form, %d slots, %s" % (n, kind))
    got, errors = _device(ctx, table, cls, flag)
    assert errors == 0
    _same(got, want, "device form, %d slots, %s" % (n, kind))
    return want


@pytest.mark.parametrize("n", [n for n in flr_tables.SIZES if n < 64])
def test_small_tables(ctx, n):
    for kind in ("same", "distinct", "special"):
        _both(ctx, n, kind)


@pytest.mark.parametrize("kind", flr_tables.KINDS)
@pytest.mark.parametrize("n", [n for n in flr_tables.SIZES if n >= 64])
def test_tables_equal_the_yardstick(ctx, n, kind):
    rec, order, n_ranked = _both(ctx, n, kind)
    ranked = order[:n_ranked].astype(np.int64)
    assert (np.diff(rec["flr"][ranked]) >= 0).all() and (np.diff(rec["decoy_q"][ranked]) >= 0).all()
    assert (rec["rank"][order[n_ranked:].astype(np.int64)] == 0).all()


def test_every_slot_unranked(ctx):
    table, _, _ = flr_tables.make(2 * T + 1, "eight")
    table = table.copy()
    table["n_psm"] = 0
    for cls in (None, np.full(table.size, 2, np.uint8)):
        t = table.copy()
        if cls is not None:
            t["n_psm"] = 1
        want = flr_ref.flr(t, cls)
        assert want[2] == 0 and want[0].tobytes() == bytes(32 * t.size) and want[1].tolist() == list(range(t.size))
        _same(ctx[0].rollup_flr(t, cls), want, "host form")
        _same(_device(ctx, t, cls, False)[0], want, "device form")


def test_no_decoy_means_no_q_value(ctx):
    table, _, _ = flr_tables.make(T + 1, "distinct")
    cls = np.zeros(table.size, np.uint8)
    cls[::7] = 2
    rec, order, n_ranked = ctx[0].rollup_flr(table, cls)
    _same((rec, order, n_ranked), flr_ref.flr(table, cls), "no decoy")
    assert n_ranked and not rec["decoy_q"].any() and not rec["n_decoy"].any()


def test_permuting_the_slots_permutes_the_records(ctx):
    for kind in ("eight", "special", "byte3"):
        table, cls, flag, want = _want(2 * T + 1, kind)
        perm = np.random.default_rng(77).permutation(table.size)
        rec, order, n_ranked = ctx[0].rollup_flr(table[perm], None if cls is None else cls[perm], reported_only=flag)
        assert n_ranked == want[2]
        assert rec.tobytes() == want[0][perm].tobytes(), kind
        got, _ = _device(ctx, table[perm], None if cls is None else cls[perm], flag)
        assert got[0].tobytes() == want[0][perm].tobytes(), kind


def _repeats(batch, share=3):
    """the batch with the peptides of its first n / share PSMs repeated against the spectra of the others"""
    n = int(batch["n_psm"])
    m = max(1, n // share)
    kws = [synth.unpack_psm(batch, i) for i in range(n)]
    psms = [dict(mz=kws[i]["mz_arr"], intensity=kws[i]["int_arr"], peptide=kws[i % m]["peptide"], n_of_mod=kws[i % m]["n_of_mod"],
                 max_charge=kws[i % m]["max_fragment_charge"]) for i in range(n)]
    return synth.pack_batch(psms), [p["peptide"] for p in psms]


def test_end_to_end_from_a_scored_batch():
    import torch
    from pyascore_amd import PyAscore
    from pyascore_amd.device import DevicePlan, flr_records
    batch, settings = synth.make_batch("cfg2", n_psm=300, seed=9110)
    batch, peptides = _repeats(batch)
    gpu = harness.make_scorer(PyAscore, settings)
    res = gpu.score_batch(batch, probs=True)
    slot, n_slots, keys = ru.peptide_slots(peptides, res["site_off"], residues=settings["mod_group"])
    table = gpu.score_batch(batch, rollup=dict(slot=slot, n_slots=n_slots))["rollup"]
    cls = ru.decoy_classes(keys, decoys="S")                 # (no decoy residues in the group: serines stand in)
    assert (cls == 1).any() and (cls == 0).any()
    want = flr_ref.flr(table, cls)
    got = gpu.rollup_flr(table, cls)
    _same(got, want, "one call")
    assert want[2] == int((table["n_psm"] != 0).sum()) > 50
    dev = torch.device("cuda", 0)
    cut, rec = 130, int(res["site_off"][130])
    halves = [(synth.slice_batch(batch, 0, cut), slot[:rec], 0), (synth.slice_batch(batch, cut, 300), slot[rec:], cut)]
    d_table = None
    for part, part_slot, base in halves:
        plan = DevicePlan(gpu, part, rollup=True)
        plan.run(torch.from_numpy(part["mz"]).to(dev), torch.from_numpy(part["intensity"]).to(dev))
        if d_table is None:
            d_table = plan.rollup_clear(n_slots)
        _, sp, pp = plan.probs()
        plan.rollup(sp, pp, torch.from_numpy(part_slot).to(dev), d_table, psm_base=base)
        plan.check()
    d_rec, d_order, d_nr = plan.rollup_flr(d_table, torch.from_numpy(cls).to(dev))
    assert flr_records(d_rec.cpu().numpy()).tobytes() == got[0].tobytes()
    assert d_order.cpu().numpy().view(np.uint32).tobytes() == got[1].tobytes() and d_nr.cpu().numpy().tolist() == [got[2], 0]
    rows = ru.table(table, keys, flr=got)
    assert [r["rank"] for r in rows] == sorted(r["rank"] for r in rows) and len(rows) == want[2]
    assert len(ru.cut(*got, flr=0.05)) == int((got[0]["rank"] != 0).sum() and (got[0]["flr"][got[0]["rank"] != 0] <= 0.05).sum())


def _raw_call(ctx, n_slots, table_n, flags=0, short=0, cls=None):
    """pya_rollup_flr on guarded buffers: (rc, the three buffers, their payload sizes)"""
    import torch
    gpu, plan, dev = ctx
    table, _, _ = flr_tables.make(table_n, "eight")
    d_table = torch.from_numpy(table.view(np.uint8).reshape(-1, 32).copy()).to(dev)
    work_bytes = int(gpu._lib.pya_flr_workspace_bytes(table_n))
    sizes = (table_n * 32, table_n * 4, work_bytes)
    out, order, work = (torch.full((s + GUARD,), 0xA5, dtype=torch.uint8, device=dev) for s in sizes)
    nr = torch.full((2,), 77, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = gpu._lib.pya_rollup_flr(gpu._h, d_table.data_ptr(), n_slots, None if cls is None else cls.data_ptr(), flags, stream, work.data_ptr(),
                                 work_bytes - short, out.data_ptr(), order.data_ptr(), nr.data_ptr())
    torch.cuda.synchronize(dev)
    return rc, table, (out.cpu().numpy(), order.cpu().numpy(), work.cpu().numpy()), sizes, nr.cpu().numpy()


def test_guard_regions_keep_their_fill(ctx):
    for n in (T + 1, 2 * T + 1):
        rc, table, bufs, sizes, nr = _raw_call(ctx, n, n)
        assert rc == 0
        for buf, size, name in zip(bufs, sizes, ("d_out", "d_order", "workspace")):
            assert (buf[size:] == 0xA5).all(), "%s: written past its end" % name
        want = flr_ref.flr(table)
        assert bufs[0][:sizes[0]].tobytes() == want[0].tobytes() and bufs[1][:sizes[1]].tobytes() == want[1].tobytes()
        assert nr.tolist() == [want[2], 0]


def test_refusals_launch_nothing(ctx):
    gpu = ctx[0]
    n = T + 1
    for kw in (dict(short=1), dict(flags=2), dict(flags=0x80000001)):
        rc, _, bufs, _, nr = _raw_call(ctx, n, n, **kw)
        assert rc == _lib.PYA_ERR_ARG, kw
        assert all((b == 0xA5).all() for b in bufs) and nr.tolist() == [77, 77], kw
    rc, _, bufs, _, nr = _raw_call(ctx, 2 ** 31, n)
    assert rc == _lib.PYA_ERR_ARG and all((b == 0xA5).all() for b in bufs) and nr.tolist() == [77, 77]
    assert gpu._lib.pya_flr_workspace_bytes(0) == 0
    table, _, _ = flr_tables.make(100, "eight")
    cls = np.zeros(100, np.uint8)
    cls[41] = 3
    with pytest.raises(Exception, match="class byte"):
        gpu.rollup_flr(table, cls)
    assert gpu._lib.pya_error_index(gpu._h) == 41
    with pytest.raises(Exception):
        gpu.rollup_flr(table, cls[:50])


def test_an_unknown_class_on_the_device_is_left_out_and_counted(ctx):
    table, _, _ = flr_tables.make(T + 1, "distinct")
    cls = np.zeros(table.size, np.uint8)
    cls[[5, 900]] = (3, 255)
    as_left_out = np.where(cls > 2, 2, cls).astype(np.uint8)
    got, errors = _device(ctx, table, cls, False)
    assert errors == 2
    _same(got, flr_ref.flr(table, as_left_out), "unknown classes")
