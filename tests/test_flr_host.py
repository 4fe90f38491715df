"""The host side of the site FLR stage, without a GPU: pyascore_amd.rollup.flr against the yardstick (tests/flr_ref.py), the
helpers around it, the --site_table writer with and without --site_table_flr, and the record as header, ctypes and numpy see it."""
import os
import re

import numpy as np
import pytest

import flr_ref
import flr_tables
from conftest import ROOT
from pyascore_amd import _lib, batch_cli, rollup as ru

T = _lib.PYA_FLR_TILE


@pytest.mark.parametrize("n", flr_tables.SIZES)
def test_host_form_equals_the_yardstick(n):
    kinds = flr_tables.KINDS if n <= 2 * T + 1 else ("same", "eight", "byte6", "special")
    for kind in kinds:
        table, cls, flag = flr_tables.make(n, kind)
        want = flr_ref.flr(table, cls, flag)
        rec, order, n_ranked = ru.flr(table, cls, reported_only=flag)
        assert n_ranked == want[2], (n, kind)
        assert rec.dtype == ru.FLR_DTYPE and rec.tobytes() == want[0].tobytes(), (n, kind)
        assert order.dtype == np.uint32 and order.tobytes() == want[1].tobytes(), (n, kind)


def test_host_form_refuses_what_the_library_refuses():
    table, _, _ = flr_tables.make(10, "eight")
    with pytest.raises(ValueError, match="class byte 3 of slot 4"):
        ru.flr(table, np.array([0, 1, 2, 0, 3, 0, 0, 0, 0, 0], np.uint8))
    with pytest.raises(ValueError):
        ru.flr(table, np.zeros(9, np.uint8))
    unranked = table.copy()
    unranked["n_psm"] = 0
    rec, order, n_ranked = ru.flr(unranked)
    assert n_ranked == 0 and rec.tobytes() == bytes(320) and order.tolist() == list(range(10))


def _three():
    t = ru.empty(4)
    t["best_prob"] = [0.5, 0.0, 1.0, 0.75]
    t["best_psm"] = [1, ru.NO_PSM, 0, 2]
    t["n_psm"] = [2, 0, 1, 1]
    t["n_confident"] = [0, 0, 1, 1]
    t["n_in_best"] = [1, 0, 1, 0]
    t["best_ascore"] = [12.5, 0.0, np.inf, 0.0]
    keys = [("PEPSIDEK", 4), ("PEPSIDEK", 3), ("ASTK", 2), ("ASTK", 1)]
    return t, keys


def test_decoy_classes():
    _, keys = _three()
    assert ru.decoy_classes(keys, decoys="A").tolist() == [0, 0, 0, 1]
    assert ru.decoy_classes(keys, decoys="SP").tolist() == [1, 1, 1, 0]
    assert ru.decoy_classes(keys, "SPSA", decoys="A").tolist() == [0, 0, 0, 1]
    assert ru.decoy_classes([("P1", 3), ("P2", 1), ("P3", 1)], {"P1": "GGAG", "P2": "AK"}, decoys="A").tolist() == [1, 1, 0]
    assert ru.decoy_classes([(b"ASTK", 1), ("ASTK", 9)]).tolist() == [1, 0]
    with pytest.raises(ValueError):
        ru.decoy_classes(keys, "SP")


def test_cut_and_the_rows():
    t, keys = _three()
    cls = ru.decoy_classes(keys, decoys="A")
    res = ru.flr(t, cls)
    rec, order, n_ranked = res
    assert n_ranked == 3 and order.tolist() == [2, 3, 0, 1]
    assert rec["flr"][[2, 3, 0]].tolist() == [0.0, 0.125, 0.25] and rec["decoy_q"][[2, 3, 0]].tolist() == [0.0, 0.5, 0.5]
    assert ru.cut(*res, flr=0.01).tolist() == [2] and ru.cut(*res, flr=0.125).tolist() == [2, 3]
    assert ru.cut(*res, flr=1.0).tolist() == [2, 3, 0] and ru.cut(*ru.flr(t[:0])).size == 0
    tied, _, _ = flr_tables.make(500, "eight")
    r, o, m = ru.flr(tied)
    for level in (0.0, 0.01, 0.1, 0.3):                       # a tie group is taken or left as a whole
        took = ru.cut(r, o, m, flr=level)
        assert set(tied["best_prob"][took]).isdisjoint(tied["best_prob"][o[took.size:m]])
        assert (r["flr"][took] <= level).all() and (r["flr"][o[took.size:m]] > level).all()
    plain = ru.table(t, keys)
    assert [row["key"] for row in plain] == [keys[0], keys[2], keys[3]] and all("rank" not in row for row in plain)
    rows = ru.table(t, keys, flr=res)
    assert [row["key"] for row in rows] == [keys[2], keys[3], keys[0]]
    assert [(row["rank"], row["flr"], row["decoy_q"]) for row in rows] == [(1, 0.0, 0.0), (2, 0.125, 0.5), (3, 0.25, 0.5)]
    for row in rows:                                          # the other fields are the plain rows'
        assert {k: v for k, v in row.items() if k not in ("rank", "flr", "decoy_q")} == [p for p in plain if p["key"] == row["key"]][0]
    cls[0] = 2
    rows = ru.table(t, keys, flr=ru.flr(t, cls))
    assert [row["key"] for row in rows] == [keys[2], keys[3], keys[0]] and rows[2]["rank"] is None and rows[2]["flr"] is None
    with pytest.raises(ValueError):
        ru.table(t, keys, flr=ru.flr(t[:3]))


OLD_FILE = ("Peptide\tPosition\tResidue\tBestProb\tBestScan\tPSMs\tConfident\tInBest\tBestAscore\n"
            "PEPSIDEK\t4\tS\t0.5\tscan=11\t2\t0\t1\t12.5\n"
            "ASTK\t2\tS\t1.0\tscan=10\t1\t1\t1\tinf\n"
            "ASTK\t1\tA\t0.75\tscan=12\t1\t1\t0\t\n")


def test_site_table_file_with_and_without_the_flag(tmp_path):
    t, keys = _three()
    scans = ["scan=10", "scan=11", "scan=12"]
    path = str(tmp_path / "sites.tsv")
    batch_cli.write_site_table_tsv([batch_cli.site_table_fields(row, scans) for row in ru.table(t, keys)], path)
    assert open(path).read() == OLD_FILE                      # without the flag: the bytes of the file as it was
    batch_cli.write_site_table_tsv([], path)
    assert open(path).read() == OLD_FILE.split("\n")[0] + "\n"
    flr = ru.flr(t, ru.decoy_classes(keys, decoys="A"))
    batch_cli.write_site_table_tsv([batch_cli.site_table_fields(row, scans) for row in ru.table(t, keys, flr=flr)], path, flr=True)
    old = [line.split("\t") for line in OLD_FILE.rstrip("\n").split("\n")]
    new = [line.split("\t") for line in open(path).read().rstrip("\n").split("\n")]
    assert new[0] == old[0] + ["Rank", "FLR", "DecoyQ"] == list(batch_cli.SITE_TABLE_COLUMNS + batch_cli.SITE_TABLE_FLR_COLUMNS)
    assert new[1:] == [old[2] + ["1", "0.0", "0.0"], old[3] + ["2", "0.125", "0.5"], old[1] + ["3", "0.25", "0.5"]]
    left_out = ru.flr(t, np.array([2, 0, 0, 0], np.uint8))
    rows = [batch_cli.site_table_fields(row, scans) for row in ru.table(t, keys, flr=left_out)]
    assert rows[2] == old[1] + ["", "", ""]
    batch_cli.write_site_table_tsv([], path, flr=True)
    assert open(path).read().rstrip("\n").split("\t") == new[0]


def test_command_line_options_exist():
    text = open(os.path.join(ROOT, "pyascore_amd", "__main__.py")).read()
    assert '"--site_table_flr"' in text and '"--site_table_decoys"' in text


def _header():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_ctypes_and_numpy_agree_on_the_record():
    text, code = _header()
    body = re.search(r"typedef struct pya_site_flr \{(.*?)\} pya_site_flr;", code, flags=re.S).group(1)
    fields = re.findall(r"(uint32_t|uint64_t|double)\s+(\w+);", body)
    size = {"uint32_t": 4, "uint64_t": 8, "double": 8}
    kind = {"uint32_t": "<u4", "uint64_t": "<u8", "double": "<f8"}
    at, offsets = 0, {}
    for ctype, name in fields:
        at = (at + size[ctype] - 1) // size[ctype] * size[ctype]             # natural alignment
        offsets[name] = at
        at += size[ctype]
    assert at == 32 and [n for _, n in fields] == ["rank", "n_decoy", "err_sum", "flr", "decoy_q"]
    dt = np.dtype(_lib.FLR_DTYPE)
    assert dt.itemsize == 32 == ru.FLR_DTYPE.itemsize and dt == flr_ref.DTYPE
    assert [(n, dt.fields[n][1], dt.fields[n][0].str) for n in dt.names] == [(n, offsets[n], kind[c]) for c, n in fields]
    import ctypes as C
    assert C.sizeof(_lib.SiteFlr) == 32
    assert [(n, getattr(_lib.SiteFlr, n).offset) for n, _ in _lib.SiteFlr._fields_] == [(n, offsets[n]) for _, n in fields]
    defines = dict(re.findall(r"#define (PYA_FLR_\w+) (\d+)u", code))
    assert {k: int(v) for k, v in defines.items()} == {"PYA_FLR_TARGET": _lib.PYA_FLR_TARGET, "PYA_FLR_DECOY": _lib.PYA_FLR_DECOY,
                                                        "PYA_FLR_LEFT_OUT": _lib.PYA_FLR_LEFT_OUT,
                                                        "PYA_FLR_REPORTED_ONLY": _lib.PYA_FLR_REPORTED_ONLY, "PYA_FLR_TILE": _lib.PYA_FLR_TILE}
    for name in ("pya_flr_workspace_bytes", "pya_rollup_flr", "pya_rollup_flr_host"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, code)
    assert len(_lib.SYMBOLS["pya_rollup_flr"][1]) == 11 and len(_lib.SYMBOLS["pya_rollup_flr_host"][1]) == 8
    assert "MULTISET" in text and "non-decreasing" in text                   # the two statements the record's comment owes


def test_workspace_size_without_a_device():
    from pyascore_amd import build
    build.build()
    lib = _lib.load()
    assert lib.pya_flr_workspace_bytes(0) == 0
    for n in (1, T, T + 1, 300 * T, 10 ** 7):
        b = lib.pya_flr_workspace_bytes(n)
        assert 24 * n <= b <= 32 * n + 16384, (n, b)
    assert lib.pya_flr_workspace_bytes(10 ** 7) < 26 * 10 ** 7
    # the caller lends the workspace, so its size is public: the values of the library before the sort and the scans moved
    # into csrc/tile_sort.hip.h (one, two and three scan levels under the histogram)
    want = {1: 2560, T: 26112, T + 1: 28416, 256 * T + 1: 6567680, 10 ** 7: 250432256}
    assert {n: lib.pya_flr_workspace_bytes(n) for n in want} == want
