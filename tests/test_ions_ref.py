"""The ion yardstick (tests/ions_ref.py) held to the golden vectors, and the public surface of the ion records: header,
bindings, record size, command line.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import evidence_ref
import ions_ref
from conftest import GOLDEN, golden_cases
from oracle import harness
from pyascore_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", golden_cases())
def test_yardstick_adds_up_to_the_golden_counts(case):
    """Section 1 cumulates, by rank, to the winner's golden count row at every depth; section 2 has ref_possible /
    ref_matched / comp_possible / comp_matched records of the right kind for every counted evidence row, none for the
    others; a PSM without a result has no records."""
    settings, batch, exp = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    res = dict(best_sig=exp["best_sig"], alt_mask=exp["alt_mask"], ascores=exp["ascores"], n_sig=exp["n_sig"])
    ev, _ = evidence_ref.batch_rows(settings, batch, res, exp, synth.unpack_psm)
    off, rec = ions_ref.batch_records(settings, batch, res, ev, synth.unpack_psm)
    assert rec.dtype.itemsize == 16 and off[-1] == rec.size
    n_top, counted_rows = settings["n_top"], 0
    for i in range(batch["n_psm"]):
        r = rec[off[i]:off[i + 1]]
        if exp["n_sig"][i] <= 0:
            assert r.size == 0, i
            continue
        L = int(batch["pep_off"][i + 1] - batch["pep_off"][i])
        assert (r["reserved"] == 0).all() and (r["size"] >= 1).all() and (r["size"] <= L - 1).all(), i
        assert set(chr(t) for t in r["type"]) <= set(settings["fragment_types"]), i
        assert (r["charge"] >= 1).all() and (r["charge"] <= batch["max_charge"][i]).all(), i
        lo, hi = int(exp["ps_off"][i]), int(exp["ps_off"][i + 1])
        winner = lo + list(exp["ps_bits"][lo:hi]).index(exp["best_sig"][i])
        s1 = r[r["site"] == ions_ref.WINNER]
        assert (s1["rank"] < n_top).all() and (s1["peak_mz"] > 0).all() and not (s1["flags"] & (0xff ^ ions_ref.LOSS)).any(), i
        assert (np.abs(s1["peak_mz"] - s1["theo_mz"]) < np.float32(settings["mz_error"]) + 1e-3).all(), i
        assert np.array_equal(np.cumsum(np.bincount(s1["rank"], minlength=n_top)), exp["ps_counts"][winner]), (i, "section 1")
        for a in range(ev.shape[1]):
            s2 = r[r["site"] == a]
            if ev[i, a]["kind"] != evidence_ref.COUNTED:
                assert s2.size == 0, (i, a)
                continue
            counted_rows += 1
            comp, hit = (s2["flags"] & ions_ref.COMP) != 0, (s2["flags"] & ions_ref.COUNTED) != 0
            got = (int((~comp).sum()), int((~comp & hit).sum()), int(comp.sum()), int((comp & hit).sum()))
            assert got == tuple(int(ev[i, a][f]) for f in ("ref_possible", "ref_matched", "comp_possible", "comp_matched")), (i, a)
            assert (hit == (s2["rank"] <= ev[i, a]["depth"])).all() and ((s2["rank"] == ions_ref.NO_MATCH) == (s2["peak_mz"] == 0)).all()
    assert counted_rows


def test_canonical_order_is_byte_order():
    rec = np.zeros(4, ions_ref.DTYPE)
    rec["theo_mz"] = [3., 1., 2., 1.]
    rec["size"] = [1, 9, 1, 2]
    got = ions_ref.canonical(rec)
    assert [bytes(x.tobytes()) for x in got] == sorted(bytes(x.tobytes()) for x in rec)
    both = ions_ref.canonical_batch(np.array([0, 2, 4]), rec)
    assert both[:2].tobytes() == ions_ref.canonical(rec[:2]).tobytes() and both[2:].tobytes() == ions_ref.canonical(rec[2:]).tobytes()


def test_header_declares_the_ion_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert re.search(r"#define\s+PYA_FLAG_IONS\s+16u", text)
    assert re.search(r"int\s+pya_plan_ions_count\s*\(\s*pya_plan\s*\*", text)
    assert re.search(r"int\s+pya_plan_ions\s*\(\s*pya_plan\s*\*", text)
    assert re.search(r"int\s+pya_last_batch_ions\s*\(\s*pya_handle\s*\*", text)
    for name in ("PYA_ION_WINNER 255", "PYA_ION_LOSS 1", "PYA_ION_COMP 2", "PYA_ION_COUNTED 4"):
        assert "#define " + name in text
    assert "typedef struct pya_ion" in text


def test_bindings_and_record_size():
    from pyascore_amd import _lib, ascore, device
    lib = _lib.load()
    assert _lib.PYA_FLAG_IONS == 16
    for name in ("pya_plan_ions_count", "pya_plan_ions", "pya_last_batch_ions"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(_lib.Ion) == 16
    assert ascore.ION_DTYPE.itemsize == 16 and device.ION_DTYPE == ascore.ION_DTYPE == ions_ref.DTYPE
    assert [f[0] for f in _lib.Ion._fields_] == list(ascore.ION_DTYPE.names)
    for name, _ in _lib.Ion._fields_:
        assert getattr(_lib.Ion, name).offset == ascore.ION_DTYPE.fields[name][1], name
    raw = np.arange(3 * 16, dtype=np.uint8).reshape(3, 16)
    rec = device.ion_records(raw)
    assert rec.shape == (3,) and rec.base is not None and rec["size"][0] == 8 + 9 * 256 and rec["rank"][2] == 44 and rec["flags"][1] == 30


def test_command_line_lists_the_option():
    out = subprocess.run([sys.executable, "-m", "pyascore_amd", "--help"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert "--ions" in out


def test_ion_fields_of_the_tsv():
    from pyascore_amd import batch_cli
    rec = np.zeros(3, ions_ref.DTYPE)
    rec[0] = (np.float32(512.25), np.float32(512.5), 7, ord("y"), 2, 3, ions_ref.WINNER, ions_ref.LOSS, 0)
    rec[1] = (np.float32(300.5), np.float32(300.5), 4, ord("b"), 1, 0, 1, ions_ref.COUNTED, 0)
    rec[2] = (np.float32(310.5), np.float32(0.), 4, ord("b"), 1, 255, 1, ions_ref.COMP, 0)
    assert batch_cli.ion_fields(rec[0]) == ["winner", "", "winner", "y7++*", "512.25", "512.5", "4", "0"]
    assert batch_cli.ion_fields(rec[1]) == ["site", "2", "winner", "b4+", "300.5", "300.5", "1", "1"]
    assert batch_cli.ion_fields(rec[2]) == ["site", "2", "competitor", "b4+", "310.5", "", "", "0"]
    assert batch_cli.ION_COLUMNS == ("Scan", "Hit", "Section", "Site", "Side", "Ion", "TheoMz", "PeakMz", "Rank", "Counted")
    assert len(batch_cli.ION_COLUMNS) == 2 + len(batch_cli.ion_fields(rec[0]))
