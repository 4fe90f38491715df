"""The public surface of the ranked localisations without a GPU: header, bindings, record layout, argument errors of the C
ABI and of the Python fronts, the pure-Python helpers of pyascore_amd.ranked, the command line's --ranked table."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pyascore_amd import batch_cli, ranked as rk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_ranked_interface():
    text = open(os.path.join(ROOT, "include", "pyascore_hip.h")).read()
    assert re.search(r"#define\s+PYA_FLAG_RANKED\s+256u", text)
    flags = {name: int(v) for name, v in re.findall(r"#define\s+(PYA_FLAG_\w+)\s+(\d+)u", text)}
    assert len(set(flags.values())) == len(flags) and all(v & (v - 1) == 0 for v in flags.values())   # one bit each, all distinct
    for name, value in dict(PYA_MAX_RANKED=64, PYA_RANK_NONE=0, PYA_RANK_SCORED=1, PYA_RANK_OVER=2, PYA_RANK_TIED_PREV=1,
                            PYA_RANK_IN_BEST_TIE=2).items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    assert re.search(r"int\s+pya_plan_ranked\s*\(\s*pya_plan\s*\*[^;]*uint32_t\s+top_k\s*,\s*uint32_t\s+sig_cap", text)
    assert re.search(r"int\s+pya_last_batch_ranked\s*\(\s*pya_handle\s*\*", text)
    assert re.search(r"int\s+pya_set_ranked_k\s*\(", text) and re.search(r"uint32_t\s+pya_get_ranked_k\s*\(", text)
    assert "typedef struct pya_ranked" in text and "prefix" in text and "ascending sig_bits" in text
    host = open(os.path.join(ROOT, "pyascore_amd", "csrc", "host_internal.h")).read()
    assert "sizeof(pya_ranked) == 16" in host and "offsetof(pya_ranked, rank) == 12" in host and "offsetof(pya_ranked, flags) == 15" in host
    debug = open(os.path.join(ROOT, "include", "pyascore_debug.h")).read()
    assert "pya_debug_last_ranked_launch" in debug
    csrc = os.path.join(ROOT, "pyascore_amd", "csrc")
    for name in ("ranked.hip", "slice_score.hip.h"):
        assert os.path.exists(os.path.join(csrc, name))
    # one copy of the general front end's count loop, in the header both stages include
    assert "pb_gen_score(" in open(os.path.join(csrc, "slice_score.hip.h")).read()
    for name in ("ranked.hip", "probs.hip"):
        body = open(os.path.join(csrc, name)).read()
        assert '#include "slice_score.hip.h"' in body and "DEV float pb_gen_score" not in body and "getenv" not in body
    # the flag keeps a small plan off the one-launch kernel, and pya_score_one refuses it
    assert re.search(r"PYA_FLAG_PROBS \| PYA_FLAG_RANKED\)\) \|\| p->n_psm >", open(os.path.join(csrc, "host_run.cpp")).read())
    assert "pya_score_one does not take PYA_FLAG_RANKED" in open(os.path.join(csrc, "host_one.cpp")).read()


def test_bindings_and_record_layout():
    from pyascore_amd import _lib, ascore, build, device
    lib = _lib.load()
    assert _lib.PYA_FLAG_RANKED == 256 and _lib.PYA_MAX_RANKED == 64
    others = [_lib.PYA_FLAG_KEEP, _lib.PYA_FLAG_TIMING, _lib.PYA_FLAG_SKIP_INVALID, _lib.PYA_FLAG_EVIDENCE, _lib.PYA_FLAG_IONS,
              _lib.PYA_FLAG_NAMED, _lib.PYA_FLAG_SITES, _lib.PYA_FLAG_PROBS]
    assert all(_lib.PYA_FLAG_RANKED & f == 0 for f in others)
    for name in ("pya_plan_ranked", "pya_last_batch_ranked", "pya_set_ranked_k", "pya_get_ranked_k", "pya_debug_last_ranked_launch"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert C.sizeof(_lib.Ranked) == 16
    rd = np.dtype(_lib.RANKED_DTYPE)
    assert rd.itemsize == 16 and ascore.RANKED_DTYPE == rd and rk.RANKED_DTYPE == rd and device.RANKED_DTYPE == rd
    for field, off in dict(sig_bits=0, pep_score=8, rank=12, kind=14, flags=15).items():
        assert getattr(_lib.Ranked, field).offset == off and rd.fields[field][1] == off, field
    assert (rk.NONE, rk.SCORED, rk.OVER, rk.TIED_PREV, rk.IN_BEST_TIE, rk.MAX_RANKED) == (0, 1, 2, 1, 2, 64)
    raw = np.zeros((2, 3, 16), np.uint8)
    raw[1, 2, 14], raw[1, 2, 12], raw[1, 2, 0] = 1, 2, 9
    got = device.ranked_records(raw)
    assert got.shape == (2, 3) and got["kind"][1].tolist() == [0, 0, 1] and got["rank"][1, 2] == 2 and got["sig_bits"][1, 2] == 9
    with pytest.raises(ValueError):
        device.ranked_records(np.zeros((2, 32), np.uint8))
    names = [os.path.basename(p) for p in build.source_files()]
    assert "ranked.hip" in names and "slice_score.hip.h" in names             # part of what pya_version() digests
    assert build.tree_digest().encode() in lib.pya_version()


def test_argument_errors():
    """what the entry points refuse before anything touches a device"""
    from pyascore_amd import _lib, ascore, device
    lib = _lib.load()
    out = np.zeros((2, 5), rk.RANKED_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.pya_last_batch_ranked(None, vp(out), 2, 5) == _lib.PYA_ERR_ARG
    assert lib.pya_plan_ranked(None, None, None, 5, 0, None) == _lib.PYA_ERR_ARG
    for k in (0, 5, 65):
        assert lib.pya_set_ranked_k(None, k) == _lib.PYA_ERR_ARG
    assert lib.pya_get_ranked_k(None) == 0
    sw, lds = (C.c_uint32 * 2)(), (C.c_uint64 * 2)()
    assert lib.pya_debug_last_ranked_launch(None, sw, lds) == _lib.PYA_ERR_ARG
    # the Python fronts share one check
    assert ascore.check_ranked_k is rk.check_k and device.check_ranked_k is rk.check_k
    assert rk.check_k(1) == 1 and rk.check_k(64) == 64 and rk.check_k(np.int64(5)) == 5 and rk.check_k(5.0) == 5
    for bad in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError):
            rk.check_k(bad)
    import inspect
    assert "ranked=None" in str(inspect.signature(ascore.PyAscore.score_batch))
    assert "top_k=5" in str(inspect.signature(ascore.PyAscore.ranked)) and "top_k=5, sig_cap=0, out=None" in str(inspect.signature(device.DevicePlan.ranked))
    # the handle's setter refuses 0 and 65 where there is a device to make a handle on
    try:
        scorer = ascore.PyAscore(100.0, 10, "STY", 79.966331, 0.05, "by")
    except Exception:
        return
    assert lib.pya_get_ranked_k(scorer._h) == 5
    assert lib.pya_set_ranked_k(scorer._h, 0) == _lib.PYA_ERR_ARG and lib.pya_set_ranked_k(scorer._h, 65) == _lib.PYA_ERR_ARG
    assert lib.pya_set_ranked_k(scorer._h, 64) == 0 and lib.pya_get_ranked_k(scorer._h) == 64


def _rows():
    """K = 4: a PSM whose winner ties its runner-up, with a third row 2.5 behind; a PSM over the cap; one not scored; one with
    a single site assignment"""
    rows = np.zeros((4, 4), rk.RANKED_DTYPE)
    rows[0, :3] = [(2, 30.0, 0, rk.SCORED, rk.IN_BEST_TIE), (1, 30.0, 1, rk.SCORED, rk.TIED_PREV | rk.IN_BEST_TIE), (4, 27.5, 2, rk.SCORED, 0)]
    rows[1, 0] = (5, 41.0, 0, rk.OVER, 0)
    rows[3, 0] = (0, 12.5, 0, rk.SCORED, rk.IN_BEST_TIE)
    return rows


def test_helpers():
    rows = _rows()
    assert rk.lengths(rows).tolist() == [3, 1, 0, 1] and rk.lengths(rows).dtype == np.int64
    assert rk.best_tie_size(rows).tolist() == [2, 0, 0, 1]
    assert rk.within(rows, 0).tolist() == [[True, True, False, False], [False] * 4, [False] * 4, [True, False, False, False]]
    assert rk.within(rows, 2.5)[0].tolist() == [True, True, True, False] and rk.within(rows, 2.4)[0].tolist() == [True, True, False, False]
    assert rk.lengths(rows[0]).tolist() == [3] and rk.within(rows[0], 3).shape == (1, 4)          # one PSM's rows
    with pytest.raises(ValueError):
        rk.lengths(np.zeros((2, 2, 2), rk.RANKED_DTYPE))


def test_command_line_table(tmp_path):
    rows = _rows()
    assert batch_cli.RANKED_COLUMNS == ("Scan", "Hit", "Rank", "LocalizedSequence", "PepScore", "DeltaToBest", "Tied")
    assert batch_cli.ranked_fields(rows[0, 0], rows[0, 0], "AS[80]PTK") == ["1", "AS[80]PTK", "30.0", "0.0", "0"]
    assert batch_cli.ranked_fields(rows[0, 1], rows[0, 0], "ASPT[80]K") == ["2", "ASPT[80]K", "30.0", "0.0", "1"]
    assert batch_cli.ranked_fields(rows[0, 2], rows[0, 0], "ASPTK[80]") == ["3", "ASPTK[80]", "27.5", "2.5", "0"]
    table = [[7, 1] + batch_cli.ranked_fields(rows[0, r], rows[0, 0], s) for r, s in enumerate(("AS[80]PTK", "ASPT[80]K", "ASPTK[80]"))]
    path = str(tmp_path / "ranked.tsv")
    batch_cli.write_ranked_tsv(table, path)
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == list(batch_cli.RANKED_COLUMNS) and len(lines) == 4
    assert lines[2].split("\t") == ["7", "1", "2", "ASPT[80]K", "30.0", "0.0", "1"]
    from pyascore_amd.__main__ import build_parser
    args = build_parser().parse_args(["--ranked", "r.tsv", "a", "b", "c"])
    assert args.ranked == "r.tsv" and args.ranked_depth == 5
    args = build_parser().parse_args(["--ranked", "r.tsv", "--ranked_depth", "16", "a", "b", "c"])
    assert args.ranked_depth == 16 and build_parser().parse_args(["a", "b", "c"]).ranked is None
    # the main table's writer is what it was: no column of this stage
    batch_cli.write_tsv([[7, "AS[80]PTK", 31.5, "12.0", "4"]], path)
    assert open(path).read().splitlines()[0].split("\t") == list(batch_cli.COLUMNS)
