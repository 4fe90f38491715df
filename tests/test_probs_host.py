"""The public surface of the site probabilities without a GPU: header, bindings, record layout, argument errors of the C
ABI, the pure-Python helpers of pyascore_amd.probs, the command line's --probs columns."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pyascore_amd import batch_cli, probs as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_probability_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert re.search(r"#define\s+PYA_FLAG_PROBS\s+128u", text)
    flags = {name: int(v) for name, v in re.findall(r"#define\s+(PYA_FLAG_\w+)\s+(\d+)u", text)}
    assert len(set(flags.values())) == len(flags) and all(v & (v - 1) == 0 for v in flags.values())   # one bit each, all distinct
    assert re.search(r"int\s+pya_plan_probs\s*\(\s*pya_plan\s*\*", text)
    assert re.search(r"int\s+pya_last_batch_probs\s*\(\s*pya_handle\s*\*", text)
    assert "typedef struct pya_site_prob" in text and "typedef struct pya_psm_prob" in text
    assert "0.33219280948873623" in text and "MaxQuant" in text and "not part of the Ascore publication" in text.replace("NOT", "not")
    host = open(os.path.join(ROOT, "pyascore_amd", "csrc", "host_internal.h")).read()
    assert "sizeof(pya_site_prob) == 16" in host and "sizeof(pya_psm_prob) == 16" in host
    assert "offsetof(pya_psm_prob, n_summed) == 8" in host and "offsetof(pya_psm_prob, kind) == 12" in host
    debug = open(os.path.join(ROOT, "include", "pyascore_debug.h")).read()
    assert "PYA_NO_PROB_CNT" in debug
    for name in ("probs.hip", "probs_cnt.hip.h"):
        assert os.path.exists(os.path.join(ROOT, "pyascore_amd", "csrc", name))
    # no new variable is read from the environment for the switch
    assert "getenv" not in open(os.path.join(ROOT, "pyascore_amd", "csrc", "probs.hip")).read()


def test_bindings_and_record_layout():
    from pyascore_amd import _lib, ascore, build, device
    lib = _lib.load()
    assert _lib.PYA_FLAG_PROBS == 128
    others = [_lib.PYA_FLAG_KEEP, _lib.PYA_FLAG_TIMING, _lib.PYA_FLAG_SKIP_INVALID, _lib.PYA_FLAG_EVIDENCE, _lib.PYA_FLAG_IONS,
              _lib.PYA_FLAG_NAMED, _lib.PYA_FLAG_SITES]
    assert all(_lib.PYA_FLAG_PROBS & f == 0 for f in others)
    for name in ("pya_plan_probs", "pya_last_batch_probs"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert C.sizeof(_lib.SiteProb) == 16 and C.sizeof(_lib.PsmProb) == 16
    sd, pd = np.dtype(_lib.SITE_PROB_DTYPE), np.dtype(_lib.PSM_PROB_DTYPE)
    assert sd.itemsize == 16 and pd.itemsize == 16 and ascore.SITE_PROB_DTYPE == sd and ascore.PSM_PROB_DTYPE == pd
    assert pb.SITE_PROB_DTYPE == sd and pb.PSM_PROB_DTYPE == pd and device.PSM_PROB_DTYPE == pd
    assert (_lib.SiteProb.with_prob.offset, _lib.SiteProb.without_prob.offset) == (0, 8) == (sd.fields["with_prob"][1], sd.fields["without_prob"][1])
    for field, off in dict(z=0, n_summed=8, kind=12, pad=13).items():
        assert getattr(_lib.PsmProb, field).offset == off and pd.fields[field][1] == off, field
    raw = np.zeros((2, 16), np.uint8)
    raw[1, 12] = 2
    raw[1, 8] = 7
    got = device.psm_prob_records(raw)
    assert got["kind"].tolist() == [0, 2] and got["n_summed"].tolist() == [0, 7]
    with pytest.raises(ValueError):
        device.psm_prob_records(np.zeros((2, 32), np.uint8))
    names = [os.path.basename(p) for p in build.source_files()]
    assert "probs.hip" in names and "probs_cnt.hip.h" in names                # part of what pya_version() digests
    assert build.tree_digest().encode() in lib.pya_version()


def test_argument_errors():
    """what the entry points refuse before anything touches a device"""
    from pyascore_amd import _lib
    lib = _lib.load()
    off = np.zeros(4, np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.pya_last_batch_probs(None, vp(off), None, None, 0) == _lib.PYA_ERR_ARG
    assert lib.pya_plan_probs(None, None, None, 0, None, None) == _lib.PYA_ERR_ARG


def test_count_node_tables_take_the_bytes_of_score_cnt():
    """the LDS condition of the stage: its count-node tables need what score_cnt.hip needs for the same caps, byte for byte
    (the launch adds the slice's 64 (w, bits) pairs: 1024 bytes)"""
    from pyascore_amd import _lib
    lib = _lib.load()

    class Caps(C.Structure):
        _fields_ = [(n, C.c_uint32) for n in ("cap", "pos_cap", "kc", "k_cap", "n_cap")]

    lib.pya_probs_cnt_bytes.restype = C.c_size_t
    lib.pya_probs_cnt_bytes.argtypes = [C.POINTER(Caps)]
    lib.pya_score_cnt_lds_bytes.restype = C.c_size_t
    lib.pya_score_cnt_lds_bytes.argtypes = [C.c_uint32] * 5
    lib.pya_probs_lds_bytes.restype = C.c_size_t
    lib.pya_probs_lds_bytes.argtypes = [C.c_uint32, C.POINTER(Caps), C.c_uint32]
    seen = 0
    for cap in (0, 32, 320, 1024, 8192):
        for pos_cap in (1, 7, 19, 39, 63):
            for k_cap in (0, 1, 4, 7, 8, 15, 30):
                kc = 8
                while kc < k_cap + 1:
                    kc <<= 1
                for n_cap in (0, 1, 6, 15, 32):
                    caps = Caps(cap, pos_cap, kc, k_cap, n_cap)
                    want = lib.pya_score_cnt_lds_bytes(cap, pos_cap, kc, k_cap, n_cap)
                    assert lib.pya_probs_cnt_bytes(C.byref(caps)) == want, (cap, pos_cap, kc, k_cap, n_cap)
                    # the tables alone (front ends = 1): that, rounded up to 16, plus the 64 pairs
                    assert lib.pya_probs_lds_bytes(64, C.byref(caps), 1) == ((want + 15) & ~15) + 1024
                    seen += 1
    assert seen == 5 * 5 * 7 * 5


def _records():
    """a k = 1 PSM of two sites, 10 : 1; a PSM over the cap; a PSM that was not scored (no records)"""
    sites = np.zeros(4, pb.SITE_PROB_DTYPE)
    sites["with_prob"] = [1 / 1.1, 0.1 / 1.1, -1, -1]
    sites["without_prob"] = [0.1 / 1.1, 1 / 1.1, -1, -1]
    psms = np.zeros(3, pb.PSM_PROB_DTYPE)
    psms["z"], psms["n_summed"], psms["kind"] = [1.1, 0, 0], [2, 0, 0], [pb.SCORED, pb.OVER, pb.NONE]
    return sites, psms, np.array([0, 2, 4, 4], np.int64)


def test_helpers():
    sites, psms, off = _records()
    best = pb.best_prob(psms)
    assert best[0] == 1 / 1.1 and np.isnan(best[1]) and np.isnan(best[2])
    assert pb.positions_of("ASPTK", "STY") == [2, 4] and pb.positions_of(b"PEPK", "STY") == []
    rows = pb.table(sites, psms, off, ["ASPTK", b"KSAYK", "AAK"], residues="STY")
    assert [(r["psm"], r["position"], r["residue"]) for r in rows] == [(0, 2, "S"), (0, 4, "T"), (1, 2, "S"), (1, 4, "Y")]
    assert rows[0]["probability"] == 1 / 1.1 and rows[1]["probability"] == 0.1 / 1.1 and rows[2]["probability"] is None
    assert pb.table(sites, psms, off, ["ASPTK", "KSAYK", "AAK"], positions=[2, 4, 2, 4]) == rows
    with pytest.raises(ValueError):
        pb.table(sites, psms, off, ["ASPTK", "KSAYK", "AAK"])
    with pytest.raises(ValueError):
        pb.table(sites, psms, off, ["AAPTK", "KSAYK", "AAK"], residues="STY")  # one candidate residue, two records
    assert pb.annotate("ASPTK", [2, 4], [0.98, 0.02]) == "AS(0.98)PT(0.02)K"
    assert pb.annotate(b"ASPTK", [2], [1.0], digits=3) == "AS(1.000)PTK"


def test_command_line_columns(tmp_path):
    sites, psms, off = _records()
    assert batch_cli.PROB_COLUMNS == ("SiteProbs", "BestProb")
    got = batch_cli.prob_fields(sites[0:2], psms[0], "ASPTK", "STY")
    assert got == ["AS(0.91)PT(0.09)K", repr(1 / 1.1)]
    assert batch_cli.prob_fields(sites[2:4], psms[1], "KSAYK", "STY") == ["", ""]
    assert batch_cli.prob_fields(sites[4:4], psms[2], "AAK", "STY") == ["", ""]
    assert batch_cli.prob_fields(sites[0:2], psms[0], "ASPTK", "nSTY")[0] == "AS(0.91)PT(0.09)K"
    rows = [[7, "AS[80]PTK", 31.5, "12.0", "4"] + got]
    path = str(tmp_path / "out.tsv")
    batch_cli.write_tsv(rows, path, probs=True)
    head, line = open(path).read().splitlines()
    assert head.split("\t")[-2:] == ["SiteProbs", "BestProb"] and line.split("\t")[-2:] == got
    from pyascore_amd.__main__ import build_parser
    assert build_parser().parse_args(["--probs", "a", "b", "c"]).probs is True
