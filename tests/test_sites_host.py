"""The public surface of the site tables without a GPU: header, bindings, record layout, the pure-Python helpers of
pyascore_amd.sites, the command line's --sites option."""
import ctypes
import os
import re

import numpy as np
import pytest

from pyascore_amd import batch_cli, sites as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSETS = dict(with_sig=0, without_sig=8, with_score=16, without_score=20, pos=24, kind=26, flags=27, reserved=28)


def test_header_declares_the_site_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert re.search(r"#define\s+PYA_FLAG_SITES\s+64u", text)
    assert re.search(r"int\s+pya_plan_site_offsets\s*\(\s*const\s+pya_plan\s*\*", text)
    assert re.search(r"int\s+pya_plan_sites\s*\(\s*pya_plan\s*\*", text)
    assert re.search(r"int\s+pya_last_batch_sites\s*\(\s*pya_handle\s*\*", text)
    assert re.search(r"int\s+pya_set_site_sig_cap\s*\(\s*pya_handle\s*\*", text)
    for name in ("PYA_SITE_NONE 0", "PYA_SITE_SCORED 1", "PYA_SITE_OVER 2", "PYA_SITE_IN_BEST 1", "PYA_SITE_WITH_TIED 2",
                 "PYA_SITE_WITHOUT_TIED 4", "PYA_SITE_NO_WITHOUT 8"):
        assert re.search(r"#define\s+" + name.replace(" ", r"\s+"), text), name
    assert "typedef struct pya_site" in text
    host = open(os.path.join(ROOT, "pyascore_amd", "csrc", "host_internal.h")).read()
    assert re.search(r"static_assert\(sizeof\(pya_site\) == 32", host)            # the C side of the layout below
    for field, off in OFFSETS.items():
        if field != "with_sig":
            assert "offsetof(pya_site, %s) == %d" % (field, off) in host, field
    assert os.path.exists(os.path.join(ROOT, "pyascore_amd", "csrc", "sites.hip"))


def test_bindings_and_record_layout():
    from pyascore_amd import _lib, ascore, build, device
    lib = _lib.load()
    assert _lib.PYA_FLAG_SITES == 64
    assert (_lib.PYA_SITE_NONE, _lib.PYA_SITE_SCORED, _lib.PYA_SITE_OVER) == (0, 1, 2)
    for name in ("pya_plan_site_offsets", "pya_plan_sites", "pya_last_batch_sites", "pya_set_site_sig_cap", "pya_get_site_sig_cap"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(_lib.Site) == 32
    dt = np.dtype(_lib.SITE_DTYPE)
    assert dt.itemsize == 32 and ascore.SITE_DTYPE == dt and device.SITE_DTYPE == dt and st.SITE_DTYPE == dt
    for field, off in OFFSETS.items():
        assert getattr(_lib.Site, field).offset == off and dt.fields[field][1] == off, field
    raw = np.zeros((3, 32), np.uint8)
    raw[1, 26] = 2
    raw[1, 24] = 9
    got = device.site_records(raw)
    assert got["kind"].tolist() == [0, 2, 0] and got["pos"].tolist() == [0, 9, 0]
    with pytest.raises(ValueError):
        device.site_records(np.zeros((3, 16), np.uint8))
    # the kernel's source is part of what pya_version() digests
    assert any(os.path.basename(p) == "sites.hip" for p in build.source_files())
    assert build.tree_digest().encode() in lib.pya_version()


def _records():
    """two PSMs: 0b110 wins a k = 2 PSM of three sites with 0b011 four points behind; a k = 1 PSM of two sites"""
    rec = np.zeros(5, st.SITE_DTYPE)
    rec["kind"] = st.SCORED
    rec["pos"] = [2, 3, 7, 1, 4]
    rec["with_sig"] = [0b011, 0b110, 0b110, 1, 2]
    rec["without_sig"] = [0b110, 0b101, 0b011, 2, 1]
    rec["with_score"] = [20.0, 24.0, 24.0, 3.5, 11.0]
    rec["without_score"] = [24.0, 9.0, 20.0, 11.0, 3.5]
    rec["flags"] = [0, st.IN_BEST, st.IN_BEST, 0, st.IN_BEST]
    return rec, np.array([0, 3, 5], np.int64), np.array([0b110, 2], np.uint64)


def test_deltas_and_runner_up():
    rec, off, best = _records()
    d = st.deltas(rec)
    assert d.dtype == np.float32 and d.tolist() == [-4.0, 15.0, 4.0, -7.5, 7.5]
    ru = st.runner_up(rec, off, best)
    assert ru["sig"].tolist() == [0b011, 1] and ru["score"].tolist() == [20.0, 3.5] and ru["delta"].tolist() == [4.0, 7.5]
    assert ru["found"].all() and ru["sig"].dtype == np.uint64
    # no pair: not scored, over the cap, nothing on one side
    rec2 = rec.copy()
    rec2["kind"][:3] = st.OVER
    rec2["flags"][4] |= st.NO_WITHOUT
    rec2["without_score"][4] = -1
    d2 = st.deltas(rec2)
    assert np.isnan(d2[:3]).all() and np.isnan(d2[4]) and d2[3] == -7.5
    ru2 = st.runner_up(rec2, off, best)
    assert not ru2["found"].any() and not ru2["sig"].any() and (ru2["score"] == -1).all() and np.isnan(ru2["delta"]).all()
    empty = st.runner_up(np.zeros(0, st.SITE_DTYPE), np.array([0, 0], np.int64), np.array([0], np.uint64))
    assert not empty["found"][0]


def test_table_rows_and_cli_fields():
    rec, off, _ = _records()
    rows = st.table(rec, off, ["ASTGGGYK", b"SAATK"])
    assert [r["psm"] for r in rows] == [0, 0, 0, 1, 1] and [r["residue"] for r in rows] == ["S", "T", "Y", "S", "T"]
    assert rows[1]["in_best"] and not rows[0]["in_best"] and rows[2]["delta"] == 4.0 and rows[0]["kind"] == "scored"
    f = batch_cli.site_fields(rec[1], "ASTGGGYK", "AST[80]GGGY[80]K", "AS[80]TGGGY[80]K")
    assert f == ["ASTGGGYK", "3", "T", "1", "24.0", "9.0", "15.0", "AST[80]GGGY[80]K", "AS[80]TGGGY[80]K"]
    over = rec[0].copy()
    over["kind"] = st.OVER
    assert batch_cli.site_fields(over, "ASTGGGYK", "x", "y") == ["ASTGGGYK", "2", "S", "0", "", "", "", "", ""]
    assert len(batch_cli.SITE_COLUMNS) == 1 + len(f)
    assert batch_cli.SITE_COLUMNS == ("Scan", "Peptide", "Position", "Residue", "InBest", "WithScore", "WithoutScore", "Delta",
                                      "BestWith", "BestWithout")


def test_default_tsv_is_unchanged_and_the_option_parses(tmp_path):
    rows = [[100, "AS[80]TK", 41.5, "17.3", "3"], [101, "", float("nan"), "", ""]]
    plain, wide, table = tmp_path / "a.tsv", tmp_path / "b.tsv", tmp_path / "c.tsv"
    batch_cli.write_tsv(rows, str(plain))
    assert plain.read_text() == "Scan\tLocalizedSequence\tPepScore\tAscores\tAltSites\n100\tAS[80]TK\t41.5\t17.3\t3\n101\t\tnan\t\t\n"
    batch_cli.write_tsv([rows[0] + ["AST[80]K", "12.25"], rows[1] + ["", ""]], str(wide), sites=True)
    lines = wide.read_text().split("\n")
    assert lines[0].split("\t") == list(batch_cli.COLUMNS + batch_cli.RUNNER_UP_COLUMNS)
    assert batch_cli.RUNNER_UP_COLUMNS == ("RunnerUpSequence", "DeltaPepScore")
    assert lines[1].split("\t")[5:] == ["AST[80]K", "12.25"] and lines[2].split("\t")[5:] == ["", ""]
    batch_cli.write_sites_tsv([[100, "ASTK", "2", "S", "1", "41.5", "12.25", "29.25", "AS[80]TK", "AST[80]K"]], str(table))
    assert table.read_text().split("\n")[0].split("\t") == list(batch_cli.SITE_COLUMNS)
    assert table.read_text().split("\n")[1].split("\t")[0] == "100"
    from pyascore_amd.__main__ import build_parser
    args = build_parser().parse_args(["a", "b", "c"])
    assert args.sites == "" and build_parser().parse_args(["--sites", "s.tsv", "a", "b", "c"]).sites == "s.tsv"
