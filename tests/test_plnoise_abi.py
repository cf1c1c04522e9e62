"""dfmi_plnoise's and dfmi_synth_asd_coloured's argument checks without a GPU: every argument
error is reported on the host before any device work; more than 64 sections is
DFMI_ERR_UNSUPPORTED; the table layouts mirror the header."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NODEV, ERR_UNSUPPORTED = -1, -3, -4


def _plnoise(nsec=3, sections=True, scale=1.0, sigma=1.0, seeds=True, nser=2, n_warm=8, n=4, out=True):
    from deepfmkit_amd import _lib
    lib = _lib.load()
    sec = np.tile([1.0, -0.5, 0.5], (max(nsec, 1), 1)) if sections is True else sections
    s = np.arange(max(nser, 1), dtype=np.uint32)
    o = np.zeros((max(nser, 1), min(max(n, 1), 64)))  # never written: these calls fail on the host
    return lib.dfmi_plnoise(_lib.ptr(sec) if sections is not False else None, nsec, scale, sigma,
                            _lib.ptr(s) if seeds else None, nser, n_warm, n, _lib.ptr(o) if out else None,
                            _lib.DFMI_MEM_HOST, None)


def _coloured(nsec=3, sections=True, trials=True, n_samp=8, gain=1.0, sigma=1.0, out=True, n_warm=16):
    from deepfmkit_amd import _lib, physics as P
    lib = _lib.load()
    tab = np.zeros(2, dtype=P.SYNTH_TRIAL_DTYPE)
    col = np.zeros(2, dtype=P.SYNTH_COLOUR_DTYPE)
    col["g_freq"], col["sigma"] = gain, sigma
    sec = np.tile([1.0, -0.5, 0.5], (max(nsec, 1), 1))
    o = np.zeros((2, max(n_samp, 1)))
    return lib.dfmi_synth_asd_coloured(tab.ctypes.data if trials else None, col.ctypes.data,
                                       sec.ctypes.data if sections else None, nsec, 1.0, n_warm, 2, n_samp, 200000.0,
                                       o.ctypes.data if out else None, _lib.DFMI_MEM_HOST, None)


def test_symbols_are_declared_and_bound():
    from deepfmkit_amd import _lib
    with open(os.path.join(ROOT, "include", "dfmi.h")) as f:
        hdr = f.read()
    for name in ("dfmi_plnoise_design", "dfmi_plnoise", "dfmi_synth_asd_coloured"):
        assert name in _lib.SYMBOLS and f" {name}(" in hdr
        getattr(_lib.load(), name)


def test_plnoise_argument_errors_before_any_device_work():
    from deepfmkit_amd import _lib
    assert _plnoise(nsec=65) == ERR_UNSUPPORTED
    assert b"64" in _lib.load().dfmi_last_error()
    assert _plnoise(nsec=1000) == ERR_UNSUPPORTED
    assert _plnoise(nsec=0) == ERR_ARG
    assert _plnoise(nsec=-1) == ERR_ARG
    assert _plnoise(sections=False) == ERR_ARG
    assert _plnoise(n=0) == ERR_ARG
    assert _plnoise(n_warm=-1) == ERR_ARG
    assert _plnoise(n_warm=2 ** 62, n=2 ** 62) == ERR_ARG
    assert _plnoise(nser=-1) == ERR_ARG
    assert _plnoise(seeds=False) == ERR_ARG
    assert _plnoise(out=False) == ERR_ARG
    assert _plnoise(sigma=float("nan")) == ERR_ARG
    assert _plnoise(scale=float("inf")) == ERR_ARG
    assert _plnoise(sections=np.array([[1.0, float("nan"), 0.5]]), nsec=1) == ERR_ARG


def test_coloured_argument_errors_before_any_device_work():
    assert _coloured(nsec=65) == ERR_UNSUPPORTED
    assert _coloured(nsec=0) == ERR_ARG
    assert _coloured(sections=False) == ERR_ARG
    assert _coloured(trials=False) == ERR_ARG
    assert _coloured(out=False) == ERR_ARG
    assert _coloured(n_samp=1) == ERR_ARG
    assert _coloured(n_warm=-2) == ERR_ARG
    assert _coloured(sigma=float("nan")) == ERR_ARG
    assert _coloured(gain=float("inf")) == ERR_ARG


def test_valid_arguments_without_a_gpu_fail_loudly():
    """No CPU fallback: with valid arguments and no device the calls answer DFMI_ERR_NODEV."""
    import torch
    if not torch.cuda.is_available():
        assert _plnoise() == ERR_NODEV
        assert _plnoise(nsec=64) == ERR_NODEV
        assert _coloured() == ERR_NODEV
        assert _coloured(gain=0.0) == ERR_NODEV  # the white-only path: dfmi_synth_asd's answer


def test_design_entry_codes():
    from deepfmkit_amd import _lib
    lib = _lib.load()
    sec, scale = np.zeros((64, 3)), np.zeros(1)
    assert lib.dfmi_plnoise_design(200000.0, 4000, 2.0, sec.ctypes.data, 64, scale.ctypes.data) == 15
    assert scale[0] == 100000.0 ** -1.0
    assert lib.dfmi_plnoise_design(200000.0, 4000, 2.0, None, 0, None) == 15
    assert lib.dfmi_plnoise_design(200000.0, 4000, 2.0, sec.ctypes.data, 14, None) == ERR_ARG
    assert lib.dfmi_plnoise_design(200000.0, 4000, 2.0, sec.ctypes.data, -1, None) == ERR_ARG
    assert lib.dfmi_plnoise_design(200000.0, 3, 2.0, None, 0, None) == ERR_ARG
    assert lib.dfmi_plnoise_design(200000.0, 4000, 0.0, None, 0, None) == ERR_ARG
    assert lib.dfmi_plnoise_design(200000.0, 4000, 2.0001, None, 0, None) == ERR_ARG
    # more than 64 sections needs a record beyond any the project can hold
    assert lib.dfmi_plnoise_design(200000.0, 2 ** 62, 2.0, None, 0, None) == ERR_UNSUPPORTED
