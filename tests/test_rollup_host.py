"""The host side of the site roll-up without a device: pyascore_amd.rollup (slot builders, merge, table), the record
layout against the header, the wrapper's argument checks and the command line's site-table writer on canned records."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from pyascore_amd import _lib, batch_cli, rollup as ru


def test_record_layout_matches_the_header():
    dt = np.dtype(_lib.ROLLUP_DTYPE)
    assert dt.itemsize == 32
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    body = re.search(r"typedef struct pya_site_rollup \{(.*?)\} pya_site_rollup;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(double|uint32_t|float)\s+(\w+);", body)
    size = {"double": 8, "uint32_t": 4, "float": 4}
    kind = {"double": "<f8", "uint32_t": "<u4", "float": "<f4"}
    off = 0
    for ctype, name in fields:
        assert dt.fields[name][1] == off and dt.fields[name][0] == np.dtype(kind[ctype]), name
        off += size[ctype]
    assert off == 32 and [n for _, n in fields] == list(dt.names)
    assert dt.names == ("best_prob", "best_psm", "n_psm", "n_confident", "n_in_best", "best_ascore", "reserved")
    import ctypes as C
    for name, _ in _lib.SiteRollup._fields_:
        assert getattr(_lib.SiteRollup, name).offset == dt.fields[name][1], name
    assert C.sizeof(_lib.SiteRollup) == 32
    assert re.search(r"#define PYA_FLAG_ROLLUP 512u", text) and _lib.PYA_FLAG_ROLLUP == 512
    flags = [int(v) for v in re.findall(r"#define PYA_FLAG_[A-Z_]+ (\d+)u", text)]
    assert len(flags) == len(set(flags)) and 512 in flags                      # the bit was free
    assert "pya_plan_rollup" in _lib.SYMBOLS and "pya_set_rollup" in _lib.SYMBOLS and "pya_rollup_clear" in _lib.SYMBOLS


def test_peptide_slots():
    peps = ["ASPTK", "MSTK", b"ASPTK", "AAAK", "MSTK"]
    off, pos = ru.site_offsets(peps, "STY")
    assert off.tolist() == [0, 2, 4, 6, 6, 8] and pos.tolist() == [2, 4, 2, 3, 2, 4, 2, 3]
    slot, n, keys = ru.peptide_slots(peps, off, residues="STY")
    assert slot.dtype == np.int32 and slot.tolist() == [0, 1, 2, 3, 0, 1, 2, 3] and n == 4
    assert keys == [("ASPTK", 2), ("ASPTK", 4), ("MSTK", 2), ("MSTK", 3)]          # in order of first appearance
    slot2, n2, keys2 = ru.peptide_slots(peps, off, positions=pos)
    assert slot2.tolist() == slot.tolist() and keys2 == keys
    # a PSM that was set aside has no records
    off_b = np.array([0, 2, 2, 4, 4, 6])
    slot3, n3, keys3 = ru.peptide_slots(peps, off_b, residues="STY")
    assert slot3.tolist() == [0, 1, 0, 1, 2, 3] and n3 == 4 and keys3 == keys
    # a terminus in the group: the first residue whatever its letter
    off_n, pos_n = ru.site_offsets(["ASPTK"], "nSTY")
    assert off_n.tolist() == [0, 3] and pos_n.tolist() == [1, 2, 4]
    with pytest.raises(ValueError):
        ru.peptide_slots(peps, off)
    with pytest.raises(ValueError):
        ru.peptide_slots(peps, off, positions=pos[:-1])
    with pytest.raises(ValueError):
        ru.peptide_slots(peps, off[:-1], residues="STY")


def test_protein_slots_overlap():
    # ASPTK at 10 and PTKS at 12 of protein P1 share T (13); the third PSM has no protein
    off = np.array([0, 2, 4, 5])
    pos = np.array([2, 4, 2, 4, 1])
    slot, n, keys = ru.protein_slots(["P1", "P1", None], [10, 12, 1], off, pos)
    assert slot.tolist() == [0, 1, 1, 2, -1] and n == 3
    assert keys == [("P1", 11), ("P1", 13), ("P1", 15)]
    with pytest.raises(ValueError):
        ru.protein_slots(["P1"], [1, 2], off, pos)


def _canned():
    t = ru.empty(4)
    t[0] = (0.98, 1, 3, 2, 2, np.float32(19.5), 0)
    t[1] = (0.5, 0, 3, 0, 1, np.float32(np.inf), 0)
    t[3] = (0.02, 2, 1, 0, 0, np.float32(0), 0)
    return t, [("ASPTK", 2), ("ASPTK", 4), ("MSTK", 2), ("MSTK", 3)]


def test_table_and_empty():
    t, keys = _canned()
    assert ru.empty(2)["best_psm"].tolist() == [ru.NO_PSM] * 2 and not ru.empty(2)["n_psm"].any()
    rows = ru.table(t, keys)
    assert [r["key"] for r in rows] == [keys[0], keys[1], keys[3]]                  # the slot nobody covers has no row
    assert rows[0] == dict(key=("ASPTK", 2), best_prob=0.98, best_psm=1, n_psm=3, n_confident=2, n_in_best=2, best_ascore=19.5)
    assert rows[1]["best_ascore"] == float("inf") and rows[2]["best_ascore"] is None
    with pytest.raises(ValueError):
        ru.table(t, keys[:-1])


def test_merge_is_max_min_and_sum():
    a, _ = _canned()
    b = ru.empty(4)
    b[0] = (0.98, 0, 2, 2, 1, np.float32(25.0), 0)          # ties the probability: the smaller id; the larger Ascore
    b[1] = (0.75, 7, 1, 1, 0, np.float32(0), 0)             # a larger probability; reports nothing: the Ascore stays
    b[2] = (0.0, 5, 1, 0, 1, np.float32(-4.0), 0)           # into an empty slot
    m = ru.merge(a, b)
    assert m[0].tolist() == (0.98, 0, 5, 4, 3, 25.0, 0)
    assert m[1].tolist() == (0.75, 7, 4, 1, 1, float("inf"), 0)
    assert m[2].tolist() == (0.0, 5, 1, 0, 1, -4.0, 0)
    assert m[3].tobytes() == a[3].tobytes()
    assert ru.merge(b, a).tobytes() == m.tobytes()
    assert ru.merge(a, ru.empty(4)).tobytes() == a.tobytes()


def test_command_line_writer(tmp_path):
    t, keys = _canned()
    scans = ["scan=10", "scan=11", "scan=12"]
    rows = [batch_cli.site_table_fields(r, scans) for r in ru.table(t, keys)]
    assert rows[0] == ["ASPTK", "2", "S", "0.98", "scan=11", "3", "2", "2", "19.5"]
    assert rows[1] == ["ASPTK", "4", "T", "0.5", "scan=10", "3", "0", "1", "inf"]
    assert rows[2] == ["MSTK", "3", "T", "0.02", "scan=12", "1", "0", "0", ""]
    path = str(tmp_path / "site_table.tsv")
    batch_cli.write_site_table_tsv(rows, path)
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == list(batch_cli.SITE_TABLE_COLUMNS) and len(lines) == 4
    assert lines[1].split("\t") == rows[0]
    from pyascore_amd.__main__ import parse_args
    args = parse_args(["--site_table", "x.tsv", "--site_table_threshold", "0.9", "a", "b", "c"])
    assert args.site_table == "x.tsv" and args.site_table_threshold == 0.9
    assert parse_args(["a", "b", "c"]).site_table is None and parse_args(["a", "b", "c"]).site_table_threshold == 0.75


def test_wrapper_checks_the_request():
    from pyascore_amd.ascore import _rollup_request
    r = _rollup_request(dict(slot=[0, 1, -1], n_slots=2), 2)
    assert r["slot"].dtype == np.int32 and r["threshold"] == 0.75 and r["psm_id"] is None and r["n_slots"] == 2
    for bad in (dict(slot=[0]), dict(n_slots=1), dict(slot=[0.5], n_slots=1), dict(slot=[0], n_slots=-1), dict(slot=[0], n_slots=1, k=2),
                dict(slot=[0], n_slots=1, psm_id=[1, 2, 3]), dict(slot=[1 << 40], n_slots=1), dict(slot=[[0]], n_slots=1)):
        with pytest.raises(ValueError):
            _rollup_request(bad, 2)


def test_new_symbols_are_declared_in_the_header():
    import test_c_abi
    names = test_c_abi.declared_symbols()
    for n in ("pya_plan_rollup", "pya_rollup_clear", "pya_set_rollup", "pya_last_batch_rollup", "pya_debug_last_rollup_launch"):
        assert n in names and n in _lib.SYMBOLS, n
    assert sorted(_lib.SYMBOLS) == names
