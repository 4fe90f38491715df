"""The public surface of the named-localisation records without a GPU: header, bindings, record layout, the pure-Python
signature helpers, the command line's reported columns."""
import ctypes
import os
import re

import numpy as np
import pytest

from pyascore_amd import batch_cli, ingest, named as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "ingest")
PHOSPHO = 79.966331
OFFSETS = dict(sig_bits=0, pep_score=8, ambiguity=12, total_fragments=16, kind=20, depth=21, n_moved=22, reserved=23,
               ref_matched=24, ref_possible=26, comp_matched=28, comp_possible=30)


def test_header_declares_the_named_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert re.search(r"#define\s+PYA_FLAG_NAMED\s+32u", text)
    assert re.search(r"int\s+pya_plan_named\s*\(\s*pya_plan\s*\*", text)
    assert re.search(r"int\s+pya_score_batch_named\s*\(\s*pya_handle\s*\*", text)
    for name in ("PYA_NAMED_NONE 0", "PYA_NAMED_INVALID 1", "PYA_NAMED_WINNER 2", "PYA_NAMED_TIED 3", "PYA_NAMED_COUNTED 4"):
        assert re.search(r"#define\s+" + name.replace(" ", r"\s+"), text), name
    assert "typedef struct pya_named" in text
    host = open(os.path.join(ROOT, "pyascore_amd", "csrc", "host_internal.h")).read()
    assert re.search(r"static_assert\(sizeof\(pya_named\) == 32", host)          # the C side of the layout below
    for field, off in OFFSETS.items():
        if field != "sig_bits":
            assert "offsetof(pya_named, %s) == %d" % (field, off) in host, field


def test_bindings_and_record_layout():
    from pyascore_amd import _lib, ascore, device
    lib = _lib.load()
    assert _lib.PYA_FLAG_NAMED == 32
    assert (_lib.PYA_NAMED_NONE, _lib.PYA_NAMED_INVALID, _lib.PYA_NAMED_WINNER, _lib.PYA_NAMED_TIED, _lib.PYA_NAMED_COUNTED) == (0, 1, 2, 3, 4)
    for name in ("pya_plan_named", "pya_score_batch_named"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(_lib.Named) == 32
    dt = np.dtype(_lib.NAMED_DTYPE)
    assert dt.itemsize == 32 and ascore.NAMED_DTYPE == dt and device.NAMED_DTYPE == dt and nm.NAMED_DTYPE == dt
    for field, off in OFFSETS.items():
        assert getattr(_lib.Named, field).offset == off and dt.fields[field][1] == off, field
    raw = np.zeros((3, 32), np.uint8)
    raw[1, 20] = 4
    assert device.named_records(raw)["kind"].tolist() == [0, 4, 0]
    with pytest.raises(ValueError):
        device.named_records(np.zeros((3, 16), np.uint8))


def test_sig_bits_of():
    assert nm.sig_bits_of("ASTYK", [2], "STY") == 1 and nm.sig_bits_of("ASTYK", [4, 2], "STY") == 0b101
    assert nm.sig_bits_of("ASTYK", [], "STY") == 0
    assert nm.sig_bits_of("ASTYK", [1], "STY") == 0                            # not a modifiable residue
    assert nm.sig_bits_of("ASTYK", [2, 2], "STY") == 0                         # repeated
    assert nm.sig_bits_of("ASTYK", [6], "STY") == 0 and nm.sig_bits_of("ASTYK", [-1], "STY") == 0
    # termini: 'n' makes the first residue a site (position 0 or 1), 'c' the last one
    assert nm.sig_bits_of("ASTYK", [0], "STY") == 0
    assert nm.sig_bits_of("ASTYK", [0], "nSTY") == 1 and nm.sig_bits_of("ASTYK", [1], "nSTY") == 1
    assert nm.sig_bits_of("ASTYK", [0, 1], "nSTY") == 0                        # both name the first residue
    assert nm.sig_bits_of("ASTYK", [0, 3], "nSTY") == 0b101
    assert nm.sig_bits_of("ASTYK", [5], "STYc") == 0b1000 and nm.sig_bits_of("ASTYK", [5], "STY") == 0
    assert nm.sig_bits_of("STYK", [1], "nSTY") == 1 and nm.site_residues("STYK", "nSTYc") == [0, 1, 2, 3]
    assert nm.sig_bits_of(b"ASTYK", [3], "STY") == 0b10                        # bytes as a batch holds them
    # above 64 residues the bits still count modifiable residues, not positions
    long = "A" * 70 + "S" + "G" * 10 + "T" + "K"
    assert nm.sig_bits_of(long, [82], "STY") == 0b10 and nm.sig_bits_of(long, [71, 82], "STY") == 0b11
    many = "S" * 70
    assert nm.sig_bits_of(many, [64], "STY") == 1 << 63 and nm.sig_bits_of(many, [65], "STY") == 0
    assert nm.sig_bits_batch(["ASTYK", "ASTYK"], [[2], [1]], "STY").tolist() == [1, 0]
    assert nm.sig_bits_batch(["ASTYK"], [[4, 3]], "STY").dtype == np.uint64


def test_query_csr_forms():
    off, bits = nm.query_csr([[1, 2], [], [5]], 3)
    assert off.tolist() == [0, 2, 2, 3] and bits.tolist() == [1, 2, 5] and off.dtype == np.int64 and bits.dtype == np.uint64
    off2, bits2 = nm.query_csr((off, bits), 3)
    assert off2.tolist() == off.tolist() and bits2.tolist() == bits.tolist()
    assert nm.query_csr([3, 4], 2)[0].tolist() == [0, 1, 2]                    # one signature per PSM
    with pytest.raises(ValueError):
        nm.query_csr([[1]], 2)
    with pytest.raises(ValueError):
        nm.query_csr((np.array([0, 1]), bits), 3)
    with pytest.raises(ValueError):
        nm.query_csr((np.array([0, 2, 2, 9]), bits), 3)
    new_off, new_bits, src = nm.take_queries(off, bits, np.array([2, 0, 1]))
    assert new_off.tolist() == [0, 1, 3, 3] and new_bits.tolist() == [5, 1, 2] and src.tolist() == [2, 0, 1]


@pytest.mark.parametrize("name,kind", [("test_psms.pep.xml", "pepXML"), ("test_psms.mzid", "mzIdentML")])
def test_reported_positions_are_what_process_mods_counts(name, kind):
    psms = ingest.IdentificationParser(os.path.join(DATA, name), kind).to_list()
    assert psms
    seen = 0
    for residues in ("STY", "nSTY", "M"):
        for mass in (PHOSPHO, 15.994915):
            for m in psms:
                const_pos, const_mass, n_var = batch_cli.process_mods(residues, mass, m["peptide"], m["mod_positions"], m["mod_masses"])
                pos = batch_cli.reported_positions(residues, mass, m["peptide"], m["mod_positions"], m["mod_masses"])
                assert len(pos) == n_var
                assert sorted(pos + const_pos.tolist()) == sorted(int(p) for p in m["mod_positions"])
                if n_var:
                    seen += 1
                    bits = nm.sig_bits_of(m["peptide"], pos, residues)
                    if len(set(max(p, 1) for p in pos)) == n_var:
                        assert bin(bits).count("1") == n_var, (m["peptide"], pos)
                zb = batch_cli.reported_positions(residues, mass, m["peptide"], [p - 1 for p in m["mod_positions"]], m["mod_masses"],
                                                  zero_based=True)
                assert zb == pos
    assert seen > 0


def test_reported_fields_for_every_kind():
    rec = np.zeros(5, nm.NAMED_DTYPE)
    rec["kind"] = [0, 1, 2, 3, 4]
    rec["pep_score"] = [0, 0, 41.5, 41.5, 12.25]
    rec["ambiguity"] = [0, 0, 0, 0, np.float32(17.3)]
    assert batch_cli.reported_fields(rec[0], "") == ["", "", ""]
    assert batch_cli.reported_fields(rec[1], "") == ["", "", ""]
    assert batch_cli.reported_fields(rec[2], "AS[80]K") == ["AS[80]K", "41.5", "0"]
    assert batch_cli.reported_fields(rec[3], "AS[80]K") == ["AS[80]K", "41.5", "tie"]
    assert batch_cli.reported_fields(rec[4], "AT[80]K") == ["AT[80]K", "12.25", str(np.float32(17.3))]
    assert batch_cli.REPORTED_COLUMNS == ("ReportedSequence", "ReportedPepScore", "ReportedAscore")


def test_default_tsv_is_unchanged(tmp_path):
    rows = [[100, "AS[80]TK", 41.5, "17.3", "3"], [101, "", float("nan"), "", ""]]
    plain, wide = tmp_path / "a.tsv", tmp_path / "b.tsv"
    batch_cli.write_tsv(rows, str(plain))
    assert plain.read_text() == "Scan\tLocalizedSequence\tPepScore\tAscores\tAltSites\n100\tAS[80]TK\t41.5\t17.3\t3\n101\t\tnan\t\t\n"
    batch_cli.write_tsv([rows[0] + ["AST[80]K", "12.25", "17.3"], rows[1] + ["", "", ""]], str(wide), reported=True)
    lines = wide.read_text().split("\n")
    assert lines[0].split("\t") == list(batch_cli.COLUMNS + batch_cli.REPORTED_COLUMNS)
    assert lines[1].split("\t")[5:] == ["AST[80]K", "12.25", "17.3"] and lines[2].split("\t")[5:] == ["", "", ""]
    from pyascore_amd.__main__ import build_parser
    args = build_parser().parse_args(["a", "b", "c"])
    assert args.reported is False and build_parser().parse_args(["--reported", "a", "b", "c"]).reported is True
