"""The C ABI of the precursor-XIC stage, no device: the new symbols resolve in the built library, the records have the sizes and
offsets the header gives them (asked of the C compiler), and the ctypes structures and numpy dtypes say the same."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("pya_xic_survey_check", "pya_xic_spectra", "pya_xic_spectra_host", "pya_xic_values")
PARAM_FIELDS = ("tol", "tol_ppm", "step", "rise", "isotopes", "max_gap")
RECORD_FIELDS = ("area", "apex_intensity", "seed_intensity", "sum_intensity", "apex_scan", "left_scan", "right_scan", "start_scan", "n_points",
                 "n_present", "iso_hit", "flags")
MACROS = ("PYA_XIC_MAX_SCANS", "PYA_XIC_MAX_ISOTOPES", "PYA_XIC_MAX_GAP", "PYA_XIC_ACTIVE", "PYA_XIC_SEEN", "PYA_XIC_SEED_PRESENT",
          "PYA_XIC_LEFT_VALLEY", "PYA_XIC_RIGHT_VALLEY", "PYA_XIC_UNSORTED", "PYA_XIC_LEFT_OPEN", "PYA_XIC_RIGHT_OPEN", "PYA_XIC_AREA",
          "PYA_XIC_APEX", "PYA_XIC_SEED", "PYA_XIC_SUM")


@pytest.fixture(scope="module")
def lib():
    from pyascore_amd import build
    build.build()                      # hipcc cross-compiles gfx950 without a GPU
    from pyascore_amd import _lib
    return _lib.load()


def test_the_new_symbols_resolve(lib):
    from pyascore_amd import _lib
    for name in SYMBOLS:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert getattr(lib, name).restype is C.c_int


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """what the C compiler makes of the header: {"sizeof pya_xic": 64, "pya_xic.flags": 60, "PYA_XIC_SEEN": 2, ...}"""
    d = tmp_path_factory.mktemp("xic_abi")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pyascore_hip.h"', 'int main(void) {',
             '    printf("sizeof pya_xic %zu\\n", sizeof(pya_xic));', '    printf("sizeof pya_xic_params %zu\\n", sizeof(pya_xic_params));']
    lines += ['    printf("pya_xic_params.%s %%zu\\n", offsetof(pya_xic_params, %s));' % (f, f) for f in PARAM_FIELDS]
    lines += ['    printf("pya_xic.%s %%zu\\n", offsetof(pya_xic, %s));' % (f, f) for f in RECORD_FIELDS]
    lines += ['    printf("%s %%ld\\n", (long)%s);' % (m, m) for m in MACROS]
    lines += ['    return 0;', '}']
    src, exe = d / "layout.c", d / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True)
    return {line.rsplit(" ", 1)[0]: int(line.rsplit(" ", 1)[1]) for line in out.splitlines()}


def test_the_records_have_the_sizes_of_the_header(layout):
    assert layout["sizeof pya_xic"] == 64
    assert layout["sizeof pya_xic_params"] == 40


def test_ctypes_and_dtypes_match_the_header(layout):
    from pyascore_amd import _lib, rollup as ru
    assert C.sizeof(_lib.Xic) == 64 and C.sizeof(_lib.XicParams) == 40 and ru.XIC_DTYPE.itemsize == 64
    assert [f[0] for f in _lib.XicParams._fields_] == list(PARAM_FIELDS)
    assert [f[0] for f in _lib.Xic._fields_] == list(RECORD_FIELDS) and ru.XIC_DTYPE.names == RECORD_FIELDS
    for f in PARAM_FIELDS:
        assert getattr(_lib.XicParams, f).offset == layout["pya_xic_params." + f], f
    for f in RECORD_FIELDS:
        assert getattr(_lib.Xic, f).offset == layout["pya_xic." + f] == ru.XIC_DTYPE.fields[f][1], f
        assert ru.XIC_DTYPE.fields[f][0] == (np.dtype("<f8") if f in ru.XIC_COLUMNS else np.dtype("<u4")), f
    for m in MACROS:
        assert getattr(_lib, m) == layout[m], m
    assert ru.XIC_COLUMNS == RECORD_FIELDS[:4] and [layout["PYA_XIC_" + n] for n in ("AREA", "APEX", "SEED", "SUM")] == [0, 1, 2, 3]
