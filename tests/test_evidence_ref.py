"""The evidence yardstick (tests/evidence_ref.py) held to the golden vectors, and the public surface of the evidence
records: header, bindings, record size, command line.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import evidence_ref
from conftest import GOLDEN, golden_cases
from oracle import harness
from pyascore_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", golden_cases())
def test_yardstick_reproduces_golden_ascores(case):
    """score(depth, ref_possible, ref_matched) - score(depth, comp_possible, comp_matched) of every counted row IS the
    golden Ascore, bit for bit; a tied row stands for an Ascore of 0; comp_score is the competitor's golden PepScore."""
    settings, batch, exp = harness.load_case(os.path.join(GOLDEN, case + ".npz"))
    res = dict(best_sig=exp["best_sig"], alt_mask=exp["alt_mask"], ascores=exp["ascores"], n_sig=exp["n_sig"])
    ev, values = evidence_ref.batch_rows(settings, batch, res, exp, synth.unpack_psm)
    assert ev.dtype.itemsize == 16
    kinds = set()
    for i in range(batch["n_psm"]):
        kw = synth.unpack_psm(batch, i)
        k = kw["n_of_mod"]
        sites = evidence_ref.modifiable_positions(kw["peptide"], settings["mod_group"])
        cont = evidence_ref.containers_of(exp, int(exp["ps_off"][i]), int(exp["ps_off"][i + 1])) if exp["n_sig"][i] > 0 else {}
        for a in range(ev.shape[1]):
            row, want = ev[i, a], exp["ascores"][i, a] if a < k else None
            kinds.add(int(row["kind"]))
            if a >= k or exp["n_sig"][i] <= 0 or np.isinf(want):
                assert row.tobytes() == b"\0" * 16, (i, a)
                continue
            assert row["kind"] in (evidence_ref.COUNTED, evidence_ref.TIED), (i, a)
            assert int(row["comp_pos"]) in evidence_ref.alt_positions(exp["alt_mask"][i, a], kw["peptide"], sites)
            mod = [j for j in range(len(sites)) if (int(exp["best_sig"][i]) >> j) & 1][a]
            comp = (int(exp["best_sig"][i]) & ~(1 << mod)) | (1 << sites.index(int(row["comp_pos"]) - 1))
            assert np.float32(row["comp_score"]).tobytes() == np.float32(cont[comp][1]).tobytes(), (i, a)
            if row["kind"] == evidence_ref.TIED:
                assert want == 0. and row["depth"] == 0 and row["ref_possible"] == 0 and row["comp_possible"] == 0, (i, a)
                continue
            got = evidence_ref.score(settings, int(row["depth"]), row["ref_possible"], row["ref_matched"]) - \
                evidence_ref.score(settings, int(row["depth"]), row["comp_possible"], row["comp_matched"])
            assert np.float32(got).tobytes() == np.float32(want).tobytes(), (i, a, got, want)
            assert np.float32(values[i][a]).tobytes() == np.float32(want).tobytes(), (i, a)
    assert evidence_ref.COUNTED in kinds


def test_ties_golden_has_tied_rows():
    settings, batch, exp = harness.load_case(os.path.join(GOLDEN, "ties_cfg2.npz"))
    res = dict(best_sig=exp["best_sig"], alt_mask=exp["alt_mask"], ascores=exp["ascores"], n_sig=exp["n_sig"])
    ev, _ = evidence_ref.batch_rows(settings, batch, res, exp, synth.unpack_psm)
    tied = ev["kind"] == evidence_ref.TIED
    assert tied.any()
    assert (exp["ascores"][tied] == 0.).all() and (ev["depth"][tied] == 0).all()


def test_header_declares_the_evidence_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert re.search(r"#define\s+PYA_FLAG_EVIDENCE\s+8u", text)
    assert re.search(r"int\s+pya_plan_evidence\s*\(\s*pya_plan\s*\*", text)
    assert re.search(r"int\s+pya_last_batch_evidence\s*\(\s*pya_handle\s*\*", text)
    for name in ("PYA_EV_NONE 0", "PYA_EV_COUNTED 1", "PYA_EV_TIED 2"):
        assert "#define " + name in text
    assert "typedef struct pya_evidence" in text


def test_bindings_and_record_size():
    from pyascore_amd import _lib, ascore, device
    lib = _lib.load()
    assert _lib.PYA_FLAG_EVIDENCE == 8
    for name in ("pya_plan_evidence", "pya_last_batch_evidence"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(_lib.Evidence) == 16
    assert ascore.EVIDENCE_DTYPE.itemsize == 16 and device.EVIDENCE_DTYPE == ascore.EVIDENCE_DTYPE
    assert [f[0] for f in _lib.Evidence._fields_] == list(ascore.EVIDENCE_DTYPE.names)
    for name, _ in _lib.Evidence._fields_:
        assert getattr(_lib.Evidence, name).offset == ascore.EVIDENCE_DTYPE.fields[name][1], name
    raw = np.arange(2 * 3 * 16, dtype=np.uint8).reshape(2, 3, 16)
    rows = device.evidence_rows(raw)
    assert rows.shape == (2, 3) and rows.base is not None and rows["kind"][0, 0] == 7 and rows["depth"][1, 2] == 86


def test_command_line_lists_the_option():
    out = subprocess.run([sys.executable, "-m", "pyascore_amd", "--help"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert "--evidence" in out


def test_evidence_fields_of_the_tsv():
    from pyascore_amd import batch_cli
    ev = np.zeros(3, evidence_ref.DTYPE)
    ev[0] = (np.float32(12.5), 7, 3, evidence_ref.COUNTED, 2, 4, 0, 4)
    ev[1] = (np.float32(40.25), 9, 0, evidence_ref.TIED, 0, 0, 0, 0)
    assert batch_cli.evidence_fields(ev) == ["4;;", "2/4|0/4;tie;", "12.5;40.25;"]
    assert batch_cli.COLUMNS == ("Scan", "LocalizedSequence", "PepScore", "Ascores", "AltSites")
