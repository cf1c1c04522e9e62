"""dfmi_lpsd_plan / dfmi_lpsd are declared, bound and exported; dfmi_lpsd reports every argument
error before any device work, and valid arguments without a GPU are DFMI_ERR_NODEV (no CPU
fallback); the Python layer refuses unsupported settings on the host. CPU only."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call(nser=1, stride=None, N=500, fs=50.0, J=None, order=0, psll=200.0, x=True, Lbad=None, Kbad=None, bbad=None,
          outs=(1, 1), plan=True):
    from deepfmkit_amd import _lib
    from deepfmkit_amd import lpsd as M
    lib = _lib.load()
    p = M.plan(500, 50.0, Jdes=100)
    b, L, K = p.b.copy(), p.L.copy(), p.K.copy()
    if Lbad is not None:
        L[3] = Lbad
    if Kbad is not None:
        K[3] = Kbad
    if bbad is not None:
        b[3] = bbad
    J = b.size if J is None else J
    xs = np.zeros((max(nser, 1), 500))
    Sxx, enbw = np.zeros((max(nser, 1), b.size)), np.zeros(b.size)
    return lib.dfmi_lpsd(_lib.ptr(xs) if x else None, nser, 500 if stride is None else stride, N, fs,
                         _lib.ptr(b) if plan else None, _lib.ptr(L), _lib.ptr(K), J, order, psll,
                         _lib.ptr(Sxx) if outs[0] else None, _lib.ptr(enbw) if outs[1] else None,
                         _lib.DFMI_MEM_HOST, None)


def test_symbols_are_declared_bound_and_exported():
    from deepfmkit_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "dfmi.h")) as f:
        hdr = f.read()
    for s in ("dfmi_lpsd_plan", "dfmi_lpsd"):
        assert s in _lib.SYMBOLS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), s)
    assert "int64_t dfmi_lpsd_plan(" in hdr and "int dfmi_lpsd(" in hdr
    i64, dbl, P, i32 = ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.c_int32
    assert lib.dfmi_lpsd_plan.argtypes == [i64, dbl, dbl, dbl, i64, i64, i64, P, P, P, P, P, i64]
    assert lib.dfmi_lpsd_plan.restype is i64
    assert lib.dfmi_lpsd.argtypes == [P, i64, i64, i64, dbl, P, P, P, i64, i32, dbl, P, P, i32, P]
    assert lib.dfmi_lpsd.restype is ctypes.c_int


def test_argument_errors_before_any_device_work():
    from deepfmkit_amd import _lib
    assert _call(nser=0) == -1
    assert _call(nser=70000) == -1
    assert _call(nser=2, stride=499) == -1
    assert _call(N=0) == -1
    assert _call(J=0) == -1
    assert _call(fs=0.0) == -1
    assert _call(fs=float("nan")) == -1
    assert _call(order=1) == -1
    assert _call(order=-2) == -1
    assert _call(x=False) == -1
    assert _call(plan=False) == -1
    assert _call(outs=(0, 1)) == -1
    assert _call(outs=(1, 0)) == -1
    assert _call(psll=0.0) == -1      # alpha(0) < 0
    assert _call(psll=2000.0) == -1   # pi alpha beyond the I0 series' table
    assert _call(Lbad=0) == -1
    assert _call(Lbad=501) == -1      # a segment longer than the series would read past its end
    assert _call(N=400) == -1         # the same through N
    assert _call(Kbad=0) == -1
    assert _call(bbad=float("nan")) == -1
    assert b"plan entry" in _lib.load().dfmi_last_error()


def test_valid_arguments_without_a_gpu_fail_loudly():
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _call() == -3  # DFMI_ERR_NODEV
    assert _call(nser=3, order=-1) == -3
    from deepfmkit_amd import lpsd as M
    from deepfmkit_amd._lib import DFMIError
    with pytest.raises(DFMIError):
        M.lpsd(np.zeros(500), 50.0)


def test_python_layer_refuses_unsupported_settings_on_the_host():
    from deepfmkit_amd import lpsd as M
    x = np.zeros(500)
    with pytest.raises(ValueError, match="Kaiser"):
        M.lpsd(x, 50.0, win=np.hanning)
    with pytest.raises(ValueError, match="Kaiser"):
        M.lpsd(x, 50.0, win="hann")
    with pytest.raises(ValueError, match="order"):
        M.lpsd(x, 50.0, order=1)
    with pytest.raises(ValueError, match="olap"):
        M.lpsd(x, 50.0, olap="auto")
    with pytest.raises(ValueError, match="psll"):
        M.lpsd(x, 50.0, psll=0)
    with pytest.raises(ValueError):
        M.lpsd(np.zeros(7), 50.0)
    with pytest.raises(ValueError):
        M.lpsd(np.zeros((2, 3, 500)), 50.0)


def test_fit_object_has_the_reference_lpsd_attributes_as_class_defaults():
    import deepfmkit_amd as dfm
    o = dfm.DeepFitObject()
    assert (o.f, o.Sxx, o.olap, o.bmin, o.Lmin, o.Jdes, o.Kdes, o.order, o.psll) == \
        (None, None, "default", 1, 0, 500, 100, 0, 200)
    assert o.win is np.kaiser
    assert not {"f", "Sxx", "olap", "bmin", "Lmin", "Jdes", "Kdes", "order", "win", "psll"} & set(vars(o))
    assert callable(o.calc_lpsd) and callable(dfm.DeepFitFramework().calc_lpsd)
