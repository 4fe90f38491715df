"""``--channel_spill`` / ``--channel_normalize`` of the command line and ``batch_cli.localize(channels=...)``: what is parsed, what
the request carries, and what is refused before anything is read or scored.  No GPU."""
import numpy as np
import pytest

from pyascore_amd import batch_cli, rollup as ru
from pyascore_amd.__main__ import channels_request, parse_args

FILES = ["spec.mzML", "ident.pepXML", "out.tsv"]
SITE = ["--site_table", "s.tsv", "--marker_mz", "126.5,127.5,128.5", "--site_quant", "q.tsv"]
PFORM = ["--marker_mz", "126.5,127.5,128.5", "--peptidoform_quant", "p.tsv"]


def _sheet(tmp_path, text, name="lot.tsv"):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def test_options_are_parsed(tmp_path):
    assert channels_request(parse_args(FILES)) is None and channels_request(parse_args(SITE + FILES)) is None
    assert channels_request(parse_args(SITE + ["--channel_normalize"] + FILES)) == dict(normalize=True)
    sheet = _sheet(tmp_path, "from\tto\tfraction\n# the lot of the day\n0\t1\t0.05\n\n1\t0\t0.02\n1\t2\t0.04\n2\t-1\t0.03\n")
    want = ru.channel_matrix(ru.channel_spill(3, [(0, 1, 0.05), (1, 0, 0.02), (1, 2, 0.04), (2, -1, 0.03)]))
    for quant in (SITE, PFORM, SITE + PFORM[2:]):
        req = channels_request(parse_args(quant + ["--channel_spill", sheet] + FILES))
        assert sorted(req) == ["matrix", "normalize"] and req["normalize"] is False
        assert req["matrix"].tobytes() == want.tobytes() and req["matrix"].shape == (3, 3)
        req = channels_request(parse_args(quant + ["--channel_spill", sheet, "--channel_normalize"] + FILES))
        assert req["normalize"] is True and req["matrix"].tobytes() == want.tobytes()
    assert ru.read_channel_spill(_sheet(tmp_path, "0\t1\t0.05\n", "plain.tsv"), 2).tolist() == [[0.95, 0.0], [0.05, 1.0]]


def test_refused_without_a_quant_table(tmp_path):
    sheet = _sheet(tmp_path, "0\t1\t0.05\n")
    for bad in (["--channel_normalize"], ["--channel_spill", sheet], ["--channel_normalize", "--marker_mz", "126.5,127.5", "--markers", "m.tsv"],
                ["--channel_spill", sheet, "--site_table", "s.tsv", "--marker_mz", "126.5,127.5"]):
        with pytest.raises(ValueError, match="--site_quant"):
            parse_args(bad + FILES)


def test_refused_on_a_malformed_spill_file(tmp_path):
    for n, text in enumerate(("0\t1\n", "0\t1\t0.05\textra\n", "0\t1\tmuch\n", "0 1 0.05\n", "0\t3\t0.05\n", "3\t0\t0.05\n", "0\t0\t0.05\n",
                              "0\t1\t-0.05\n", "0\t1\tnan\n", "0\t1\t0.05\n0\t1\t0.05\n", "0\t1\t0.7\n0\t2\t0.3\n", "0\t1\t0.05\nfrom\tto\tfraction\n",
                              "0.5\t1\t0.05\n", "0\t1\t0.5\n1\t0\t0.5\n")):
        with pytest.raises(ValueError, match="--channel_spill"):
            parse_args(SITE + ["--channel_spill", _sheet(tmp_path, text, "bad%d.tsv" % n)] + FILES)
    with pytest.raises(ValueError, match="--channel_spill"):
        parse_args(SITE + ["--channel_spill", str(tmp_path / "none.tsv")] + FILES)


def test_localize_checks_the_request_before_anything_is_read():
    quant = dict(site_quant=dict(threshold=0.5), site_quant_rows=[], site_table=[], markers=dict(mz=(1.0, 2.0)), marker_rows=[])
    for bad in (dict(channels=dict(normalize=True)),                                                 # no table to correct for
                dict(quant, channels=dict()), dict(quant, channels=dict(normalize=False)), dict(quant, channels=3),
                dict(quant, channels=dict(normalize=True, select=[1])), dict(quant, channels=dict(matrix=np.eye(3))),
                dict(quant, channels=dict(matrix=np.eye(2), window=1)), dict(quant, channels=dict(normalize="yes"))):
        with pytest.raises(ValueError):
            batch_cli.localize(None, [], {}, "STY", 79.966331, **bad)
    with pytest.raises(TypeError):                                                                  # (a good request reaches the scorer check)
        batch_cli.localize(None, [], {}, "STY", 79.966331, **dict(quant, channels=dict(matrix=np.eye(2), normalize=True)))
