"""What the four spectrum transforms (deisotope, decharge, strip, centroid) refuse in the part they share, word for word: the
NumPy forms of pyascore_amd.rollup on the CPU, the device and host forms of the C ABI on the GPU (calls that are refused before
anything is launched), and the empty inputs of the ``*_spectra`` methods.  The texts are the ones the four stages had when each
carried a copy of this part; they are written out here so that a change to the shared code that moves one of them fails."""
import ctypes as C

import numpy as np
import pytest

from pyascore_amd import _lib, rollup as ru

STAGES = ("deisotope", "decharge", "strip", "centroid")
RULES = {"deisotope": ru.deisotope_params(), "decharge": ru.decharge_params(), "strip": ru.strip_params(0.01),
         "centroid": ru.centroid_params(0.05)}
C_PARAMS = {"deisotope": ru.deisotope_c_params, "decharge": ru.decharge_c_params, "strip": ru.strip_c_params,
            "centroid": ru.centroid_c_params}


# ---- the NumPy forms: two spectra of three peaks ----

MZ = np.array([100.0, 200.0, 300.0, 150.0, 250.0, 350.0])
IT = np.array([5.0, 9.0, 2.0, 7.0, 1.0, 3.0])
OFF = np.array([0, 3, 6], np.int64)

BAD_NUMPY = {
    "mz of two dimensions": (dict(mz=MZ.reshape(2, 3)), "%s: mz is a one-dimensional float64 or float32 array"),
    "int32 intensity": (dict(intensity=IT.astype(np.int32)), "%s: intensity is a one-dimensional float64 or float32 array"),
    "descending peak_off": (dict(peak_off=np.array([0, 4, 3], np.int64)), "%s: peak_off has n_spectra + 1 offsets that do not descend"),
    "negative peak_off[0]": (dict(peak_off=np.array([-1, 3, 6], np.int64)), "%s: peak_off has n_spectra + 1 offsets that do not descend"),
    "peak_off past the end": (dict(peak_off=np.array([0, 3, 7], np.int64)), "%s: peak_off runs past the end of the spectrum arrays"),
}


def _numpy_form(stage, mz, intensity, peak_off):
    if stage == "strip":
        return ru.strip(mz, intensity, peak_off, np.full(2, 400.0), np.full(2, 2, np.int32), RULES[stage])
    return getattr(ru, stage)(mz, intensity, peak_off, RULES[stage])


@pytest.mark.parametrize("stage", STAGES)
def test_the_numpy_forms_take_the_good_input(stage):
    assert _numpy_form(stage, MZ, IT, OFF)[2].dtype == np.int64


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("what", sorted(BAD_NUMPY))
def test_numpy_form_refusals(stage, what):
    change, text = BAD_NUMPY[what]
    with pytest.raises(ValueError) as e:
        _numpy_form(stage, **dict(dict(mz=MZ, intensity=IT, peak_off=OFF), **change))
    assert str(e.value) == text % stage


# ---- the C ABI: six spectra of at most eight peaks; every call is refused before anything is launched ----

LENGTHS = (3, 0, 8, 1, 5, 2)
N_SPEC, N_PEAKS = len(LENGTHS), sum(LENGTHS)
_state = {}


def _gpu():
    if "gpu" not in _state:
        from oracle import harness
        from pyascore_amd import PyAscore, synth
        _state["gpu"] = harness.make_scorer(PyAscore, synth.describe("cfg2", 1, seed=1)["settings"])
    return _state["gpu"]


def _arrays(mz_t=np.float64, it_t=np.float64):
    """the arguments of a good call as host arrays: the spectra, what the stages take beside them, everything they write"""
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    mz = np.concatenate([100.0 + 50.0 * np.arange(n) for n in LENGTHS]).astype(mz_t)
    return dict(mz=mz, it=np.ones(N_PEAKS, it_t), off=off, o_mz=np.zeros(N_PEAKS, mz_t), o_it=np.zeros(N_PEAKS, it_t),
                new_off=np.zeros(N_SPEC + 1, np.int64), over=np.zeros(2, np.uint32), pm=np.full(N_SPEC, 400.0),
                pz=np.full(N_SPEC, 2, np.int32), select=np.ones(N_SPEC, np.uint8), charge=np.zeros(N_PEAKS, np.uint8),
                report=np.zeros(N_SPEC * 2, np.uint64), work=np.zeros(1 << 12, np.int64))


def _call(stage, host, a, **change):
    """pya_<stage>_spectra(_host) on the pointers of ``a`` (``ptr`` of every array; ``change`` replaces some): (rc, message)"""
    gpu = _gpu()
    p = dict({k: v["ptr"] for k, v in a.items()}, n=N_SPEC, work_bytes=8 * (1 << 12))
    p.update(change)
    t_in = _lib.TypedSpectra(p["mz"], p["it"], _lib.spectrum_type(a["mz"]["dtype"]), _lib.spectrum_type(a["it"]["dtype"]))
    t_out = _lib.TypedSpectra(p["o_mz"], p["o_it"], t_in.mz_type, t_in.intensity_type)
    p.update(t_in=None if p["mz"] is None else C.byref(t_in), t_out=C.byref(t_out), params=C.byref(C_PARAMS[stage](RULES[stage])), stream=None)
    side_in = {"strip": ["pm", "pz"], "centroid": ["select"]}.get(stage, [])
    side_out = {"decharge": ["charge"], "strip": ["report"]}.get(stage, [])
    names = ["t_in", "off", "n"] + side_in + ["params"] + ([] if host else ["stream", "work", "work_bytes"])
    names += ["t_out", "new_off"] + side_out + ["over"]
    fn = getattr(gpu._lib, "pya_%s_spectra%s" % (stage, "_host" if host else ""))
    rc = fn(gpu._h, *[p[k] for k in names])
    return rc, gpu._lib.pya_last_error(gpu._h).decode()


def _on_device(arrays):
    import torch
    dev = torch.device("cuda", _gpu().device)
    out = {}
    for k, v in arrays.items():
        t = torch.from_numpy(v).to(dev)
        out[k] = dict(ptr=t.data_ptr(), dtype=v.dtype, keep=t)
    return out


def _on_host(arrays):
    return {k: dict(ptr=v.ctypes.data, dtype=v.dtype, keep=v) for k, v in arrays.items()}


def _need(stage):
    return int(getattr(_gpu()._lib, "pya_%s_workspace_bytes" % stage)(N_SPEC, 0))


# what is wrong -> (the arrays' dtypes, the changed arguments, the format of the message: function, sizer, bytes given, bytes needed)
BAD_DEVICE = {
    "NULL in": ((np.float64, np.float64), lambda a, need: dict(mz=None), "NULL pointer passed to {fn}"),
    "an out array is an in array": ((np.float64, np.float64), lambda a, need: dict(o_mz=a["mz"]["ptr"]),
                                    "{fn}: an out array is an in array (the filter does not work in place)"),
    "f32 m/z beside f64 intensity": ((np.float32, np.float64), lambda a, need: {},
                                     "{fn}: float32 m/z beside float64 intensities is not supported"),
    "2^32 - 1 spectra": ((np.float64, np.float64), lambda a, need: dict(n=0xFFFFFFFF), "{fn}: 4294967295 spectra are more than 2^32 - 2"),
    "NULL workspace": ((np.float64, np.float64), lambda a, need: dict(work=None), "{fn}: the workspace is NULL or not 8-byte aligned"),
    "misaligned workspace": ((np.float64, np.float64), lambda a, need: dict(work=a["work"]["ptr"] + 4),
                             "{fn}: the workspace is NULL or not 8-byte aligned"),
    "workspace 8 bytes too small": ((np.float64, np.float64), lambda a, need: dict(work_bytes=need - 8),
                                    "{fn}: a workspace of {given} bytes is smaller than {sizer} ({need} for no peaks)"),
}
BAD_HOST = {
    "descending peak_off": (lambda off: off[[0, 1, 2, 4, 3, 5, 6]], "{fn}: peak_off descends at spectrum 3"),
    "negative peak_off[0]": (lambda off: np.concatenate([[-1], off[1:]]), "{fn}: peak_off[0] is negative"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("what", sorted(BAD_DEVICE))
def test_device_form_refusals(what):
    types, change, text = BAD_DEVICE[what]
    said = set()
    for stage in STAGES:
        a = _on_device(_arrays(*types))
        need = _need(stage)
        names = dict(fn="pya_%s_spectra" % stage, sizer="pya_%s_workspace_bytes" % stage, given=need - 8, need=need)
        rc, message = _call(stage, False, a, **change(a, need))
        assert rc == _lib.PYA_ERR_ARG, (stage, rc, message)
        assert message == text.format(**names), stage
        for k in ("fn", "sizer", "given", "need"):
            if "{%s}" % k in text:
                message = message.replace(str(names[k]), "{%s}" % k, 1)
        said.add(message)
    assert said == {text}


@pytest.mark.gpu
@pytest.mark.parametrize("what", sorted(BAD_HOST))
def test_host_form_refusals(what):
    change, text = BAD_HOST[what]
    said = set()
    for stage in STAGES:
        arrays = _arrays()
        arrays["off"] = np.ascontiguousarray(change(arrays["off"]), np.int64)
        fn = "pya_%s_spectra_host" % stage
        rc, message = _call(stage, True, _on_host(arrays))
        assert rc == _lib.PYA_ERR_ARG, (stage, rc, message)
        assert message == text.format(fn=fn), stage
        assert not arrays["new_off"].any() and not arrays["o_mz"].any()
        said.add(message.replace(fn, "{fn}"))
    assert said == {text}


@pytest.mark.gpu
def test_the_forms_take_the_good_input():
    """the arguments the refusals above start from are themselves accepted, by both forms of every stage"""
    import torch
    for stage in STAGES:
        arrays = _arrays()
        rc, message = _call(stage, True, _on_host(arrays))
        assert rc == 0, (stage, message)
        assert arrays["new_off"][-1] <= N_PEAKS
        a = _on_device(_arrays())
        rc, message = _call(stage, False, a)                 # (on the default stream)
        assert rc == 0, (stage, message)
        torch.cuda.synchronize()
        assert a["new_off"]["keep"].cpu().numpy().tobytes() == arrays["new_off"].tobytes(), stage


# ---- the methods of the scorer: the checks in front of the library and the inputs without a peak ----

def _method(stage, mz, intensity, peak_off):
    n = len(peak_off) - 1
    side = (np.full(n, 400.0), np.full(n, 2, np.int32)) if stage == "strip" else ()
    return getattr(_gpu(), stage + "_spectra")(mz, intensity, peak_off, *side, RULES[stage])


@pytest.mark.gpu
@pytest.mark.parametrize("stage", STAGES)
def test_method_refusals(stage):
    for change, text in ((dict(mz=MZ.reshape(2, 3)), "%s_spectra: mz, intensity and peak_off are one-dimensional, peak_off has n_spectra + 1 entries"),
                         (dict(peak_off=[0, 4, 3]), "%s_spectra: peak_off must not be negative or descend"),
                         (dict(peak_off=[-1, 3, 6]), "%s_spectra: peak_off must not be negative or descend"),
                         (dict(peak_off=[0, 3, 7]), "peak_off runs past the end of the spectrum arrays")):
        with pytest.raises(ValueError) as e:
            _method(stage, **dict(dict(mz=MZ, intensity=IT, peak_off=OFF), **change))
        assert str(e.value) == (text % stage if "%s" in text else text)


@pytest.mark.gpu
@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("n_spec", [0, 3])
def test_methods_without_a_peak(stage, n_spec):
    """no spectra, and three spectra without a peak between peaks that belong to nobody: arrays of no element of the inputs'
    dtypes, n_spec + 1 zero offsets, no charge, a report that still counts the windows, nothing out of order"""
    got = _method(stage, MZ.astype(np.float32), IT.astype(np.float32), np.full(n_spec + 1, 2, np.int64))
    assert len(got) == (5 if stage in ("decharge", "strip") else 4)
    assert [a.dtype for a in got[:3]] == [np.float32, np.float32, np.int64]
    assert got[0].shape == (0,) and got[1].shape == (0,) and got[2].tolist() == [0] * (n_spec + 1)
    assert got[-1] == (0, None)
    if stage == "decharge":
        assert got[3].dtype == np.uint8 and got[3].shape == (0,)
    if stage == "strip":
        assert got[3].dtype == ru.STRIP_REPORT_DTYPE and got[3].shape == (n_spec,)
        assert got[3]["n_windows"].tolist() == [1] * n_spec and not got[3]["n_removed"].any() and not got[3]["hit"].any()
