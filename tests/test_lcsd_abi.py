"""dfmi_lcsd is declared, bound and exported; it reports every argument error before any device
work, and valid arguments without a GPU are DFMI_ERR_NODEV (no CPU fallback); the Python layer
refuses unsupported settings and mismatched inputs on the host. CPU only."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, NODEV = -1, -3


def _call(npair=1, xs=500, ys=500, N=500, fs=50.0, J=None, order=0, psll=200.0, x=True, y=True, Lbad=None, Kbad=None,
          bbad=None, outs=(1, 1, 1, 1, 1, 1), plan=(1, 1, 1)):
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
    rows = max(min(npair, 4), 1)
    xa, ya = np.zeros((rows, 500)), np.zeros((rows, 500))
    o = [np.zeros((rows, b.size)) for _ in range(5)] + [np.zeros(b.size)]
    return lib.dfmi_lcsd(_lib.ptr(xa) if x else None, xs, _lib.ptr(ya) if y else None, ys, npair, N, fs,
                         *(_lib.ptr(a) if on else None for a, on in zip((b, L, K), plan)), J, order, psll,
                         *(_lib.ptr(a) if on else None for a, on in zip(o, outs)), _lib.DFMI_MEM_HOST, None)


def test_symbol_is_declared_bound_and_exported():
    from deepfmkit_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "dfmi.h")) as f:
        hdr = f.read()
    assert "dfmi_lcsd" in _lib.SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dfmi_lcsd")
    assert "int dfmi_lcsd(const double* x, int64_t x_stride, const double* y, int64_t y_stride, int64_t npair" in hdr
    i64, dbl, P, i32 = ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.c_int32
    assert lib.dfmi_lcsd.argtypes == [P, i64, P, i64, i64, i64, dbl, P, P, P, i64, i32, dbl, P, P, P, P, P, P, i32, P]
    assert lib.dfmi_lcsd.restype is ctypes.c_int


def test_argument_errors_before_any_device_work():
    from deepfmkit_amd import _lib
    err = _lib.load().dfmi_last_error
    assert _call(x=False) == ARG and b"null" in err()
    assert _call(y=False) == ARG
    for k in range(3):
        assert _call(plan=tuple(int(i != k) for i in range(3))) == ARG
    assert _call(outs=(0, 0, 0, 0, 0, 1)) == ARG and b"at least one" in err()
    assert _call(npair=2, xs=499) == ARG and b"x_stride" in err()
    assert _call(npair=2, xs=1) == ARG
    assert _call(npair=2, ys=499) == ARG and b"y_stride" in err()
    assert _call(npair=2, ys=0) == ARG and b"y_stride" in err()
    assert _call(npair=2, xs=0, ys=0) == ARG
    assert _call(npair=0) == ARG and b"npair" in err()
    assert _call(npair=65536) == ARG
    assert _call(N=0) == ARG
    assert _call(N=2 ** 31) == ARG
    assert _call(J=0) == ARG
    assert _call(fs=0.0) == ARG and b"fs" in err()
    assert _call(fs=float("nan")) == ARG
    assert _call(fs=float("inf")) == ARG
    assert _call(order=1) == ARG and b"order" in err()
    assert _call(order=-2) == ARG
    assert _call(psll=0.0) == ARG and b"psll" in err()
    assert _call(psll=2000.0) == ARG
    assert _call(Lbad=0) == ARG and b"plan entry" in err()
    assert _call(Lbad=501) == ARG
    assert _call(N=400) == ARG
    assert _call(Kbad=0) == ARG
    assert _call(bbad=float("nan")) == ARG
    assert _call(bbad=-1.0) == ARG and b"plan entry" in err()


def test_valid_arguments_reach_the_device_check():
    """Without a GPU every valid geometry is DFMI_ERR_NODEV: the argument checks let it through
    and there is no CPU fallback. (With one, tests/test_gpu_lcsd.py runs them.)"""
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _call() == NODEV
    assert _call(npair=3, xs=0, order=-1) == NODEV            # one x for every y
    assert _call(npair=3, xs=513, ys=500) == NODEV
    assert _call(npair=1, xs=0, ys=0) == NODEV                 # strides are not read for one pair
    for k in range(6):                                         # any one output may be NULL
        assert _call(outs=tuple(int(i != k) for i in range(6))) == NODEV
    assert _call(outs=(0, 0, 0, 0, 1, 0)) == NODEV
    from deepfmkit_amd import lpsd as M
    from deepfmkit_amd._lib import DFMIError
    with pytest.raises(DFMIError):
        M.lcsd(np.zeros(500), np.zeros(500), 50.0)


def test_python_layer_refuses_bad_input_on_the_host():
    from deepfmkit_amd import lpsd as M
    x = np.zeros(500)
    for kw, match in ((dict(win=np.hanning), "Kaiser"), (dict(win="hann"), "Kaiser"), (dict(order=1), "order"),
                      (dict(olap="auto"), "olap"), (dict(psll=0), "psll")):
        with pytest.raises(ValueError, match=match):
            M.lcsd(x, x, 50.0, **kw)
    with pytest.raises(ValueError, match="length"):
        M.lcsd(x, np.zeros(499), 50.0)
    with pytest.raises(ValueError, match="shapes"):
        M.lcsd(np.zeros((2, 500)), np.zeros((3, 500)), 50.0)
    with pytest.raises(ValueError, match="shapes"):
        M.lcsd(np.zeros((2, 500)), x, 50.0)
    with pytest.raises(ValueError):
        M.lcsd(x, np.zeros((2, 3, 500)), 50.0)
    with pytest.raises(ValueError):
        M.lcsd(np.zeros(7), np.zeros(7), 50.0)
    assert M.LCSDResult._fields == ("f", "Sxx", "Syy", "Sxy", "coh", "H", "resid", "enbw", "L", "K", "b")


def test_facade_has_calc_lcsd_and_an_unknown_label_warns(caplog):
    import deepfmkit_amd as dfm
    dff = dfm.DeepFitFramework()
    assert callable(dff.calc_lcsd)
    with caplog.at_level("WARNING"):
        assert dff.calc_lcsd("nope", "neither") is None
        assert dff.calc_lcsd("nope", ["a", "b"]) is None
    assert "Specified label is invalid!" in caplog.text
