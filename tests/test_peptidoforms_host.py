"""The host side of the peptidoform stage: the record layout, the group builder, the report rows, the TSV writer, the CLI
options and the argument checks of score_batch(peptidoforms=...) that need no device.  No GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest

from pyascore_amd import __main__ as cli, _lib, batch_cli, rollup as ru
from pyascore_amd.ascore import PEPTIDOFORM_DTYPE, PyAscore, _peptidoform_request


def test_layout_is_48_bytes():
    assert PEPTIDOFORM_DTYPE.itemsize == 48 == C.sizeof(_lib.Peptidoform) == ru.PEPTIDOFORM_DTYPE.itemsize
    want = dict(sig_bits=0, group=8, n_psm=12, n_confident=16, best_psm=20, best_min_prob=24, best_z=32, best_min_ascore=40, n_isomers=44)
    for name, off in want.items():
        assert PEPTIDOFORM_DTYPE.fields[name][1] == off == getattr(_lib.Peptidoform, name).offset, name
    assert _lib.PYA_FLAG_PEPTIDOFORMS == 1024 and _lib.PYA_PFORM_TILE == 1024


def test_peptide_groups_number_by_first_appearance():
    group, n, keys = ru.peptide_groups(["PEPS", b"ASTK", "PEPS", "XYZ", b"ASTK"])
    assert group.dtype == np.int32 and group.tolist() == [0, 1, 0, 2, 1] and n == 3 and keys == ["PEPS", "ASTK", "XYZ"]
    assert ru.peptide_groups([])[1] == 0


def _list():
    r = np.zeros(3, PEPTIDOFORM_DTYPE)
    r["group"], r["sig_bits"] = [0, 0, 1], [0b01, 0b10, 0b101]
    r["n_psm"], r["n_confident"], r["best_psm"] = [2, 1, 3], [1, 0, 3], [1, 0, 2]
    r["best_min_prob"], r["best_z"], r["best_min_ascore"], r["n_isomers"] = [0.9, 0.5, 1.0], [1.25, 2.0, 1.0], [12.5, -1.0, np.inf], [2, 2, 1]
    return r


def test_table_rows_and_tsv(tmp_path):
    keys = ["ASPTK", "SGSYS"]
    rows = ru.peptidoform_table(_list(), keys, residues="STY")
    assert [r["sites"] for r in rows] == [[2], [4], [1, 4]] and [r["peptide"] for r in rows] == ["ASPTK", "ASPTK", "SGSYS"]
    assert rows[0]["best_posterior"] == 0.8 and rows[1]["n_isomers"] == 2 and rows[2]["best_min_ascore"] == np.inf
    assert [r["sites"] for r in ru.peptidoform_table(_list(), keys)] == [[0], [1], [0, 2]]
    with pytest.raises(ValueError):
        ru.peptidoform_table(_list(), keys[:1])
    with pytest.raises(ValueError):
        ru.peptidoform_table(_list(), ["AK", "SGSYS"], residues="STY")
    scans = ["s10", "s11", "s12"]
    fields = [batch_cli.peptidoform_table_fields(r, scans) for r in rows]
    assert fields[0] == ["ASPTK", "2", "2", "1", "s11", "0.9", "0.8", "12.5", "2"]
    assert fields[2] == ["SGSYS", "1;4", "3", "3", "s12", "1.0", "1.0", "inf", "1"]
    path = tmp_path / "forms.tsv"
    batch_cli.write_peptidoform_table_tsv(fields, str(path))
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == list(batch_cli.PEPTIDOFORM_TABLE_COLUMNS) and len(lines) == 4 and lines[3].split("\t") == fields[2]


def test_cli_options():
    a = cli.parse_args(["spec", "ident", "out"])
    assert a.peptidoform_table is None and a.peptidoform_threshold == 0.75
    a = cli.parse_args(["--peptidoform_table", "f.tsv", "--peptidoform_threshold", "0.9", "spec", "ident", "out"])
    assert a.peptidoform_table == "f.tsv" and a.peptidoform_threshold == 0.9 and a.site_table is None
    sig = inspect.signature(batch_cli.localize).parameters
    assert sig["peptidoform_table"].default is None and sig["peptidoform_threshold"].default == 0.75
    assert inspect.signature(PyAscore.score_batch).parameters["peptidoforms"].default is None


def test_request_checks():
    ok = _peptidoform_request(dict(group=[1, 0, -1]), 3)
    assert ok["group"].dtype == np.int32 and ok["threshold"] == 0.75 and ok["psm_id"] is None
    assert _peptidoform_request(dict(group=np.arange(2), psm_id=[5, 6], threshold=0.5), 2)["psm_id"].dtype == np.uint32
    empty = _peptidoform_request(dict(group=[]), 0)     # an empty list has no dtype to check
    assert empty["group"].dtype == np.int32 and empty["group"].size == 0
    for bad in (dict(), dict(group=[0, 1]), dict(group=[0.5, 1, 2]), dict(group=[0, 1, 2], slot=1), dict(group=[0, 1, 1 << 31]),
                dict(group=[0, 1, 2], psm_id=[1, 2]), [0, 1, 2]):
        with pytest.raises(ValueError):
            _peptidoform_request(bad, 3)


def test_workspace_size_without_a_device():
    """The caller lends the workspace, so its size is public: the values of the library before the sort and the scans moved
    into csrc/tile_sort.hip.h (one, two and three scan levels under the histogram, one and two under the tile totals)."""
    from pyascore_amd import build
    build.build()
    lib = _lib.load()
    T = _lib.PYA_PFORM_TILE
    want = {0: 0, 1: 2560, T: 136704, T + 1: 139008, 256 * T + 1: 34881280, 10 ** 7: 1330510848}
    assert {n: lib.pya_peptidoform_workspace_bytes(n) for n in want} == want
