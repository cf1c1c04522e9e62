"""dfmi_unwrap's declaration and argument checks, without a GPU: every argument error is reported
before any device work, valid arguments without a GPU are DFMI_ERR_NODEV (no CPU fallback)."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call(nser=2, stride=8, N=8, period=2 * np.pi, status=True, sstride=8, fill=0, outs=(1, 1), ystride=8, cstride=8,
          inplace=False):
    from deepfmkit_amd import _lib
    lib = _lib.load()
    x, y = np.zeros(16), np.zeros(16)
    st, c = np.zeros(16, dtype=np.int32), np.zeros(16, dtype=np.int64)
    rc = lib.dfmi_unwrap(_lib.ptr(x), nser, stride, N, period, _lib.ptr(st) if status else None, sstride, 1, fill,
                         _lib.ptr(x if inplace else y) if outs[0] else None, ystride, _lib.ptr(c) if outs[1] else None,
                         cstride, _lib.DFMI_MEM_HOST, None)
    return rc, lib.dfmi_last_error().decode()


def test_symbol_is_declared_listed_and_exported():
    from deepfmkit_amd import _lib
    with open(os.path.join(ROOT, "include", "dfmi.h")) as f:
        assert "int dfmi_unwrap(const double* x, int64_t nser, int64_t ser_stride, int64_t N, double period," in f.read()
    assert "dfmi_unwrap" in _lib.SYMBOLS and hasattr(_lib.load(), "dfmi_unwrap")


@pytest.mark.parametrize("bad", [dict(period=0.0), dict(period=-1.0), dict(period=np.inf), dict(period=np.nan),
                                 dict(nser=-1), dict(N=-1), dict(N=2 ** 31), dict(stride=7), dict(sstride=7),
                                 dict(ystride=7), dict(cstride=7), dict(fill=-1), dict(fill=2), dict(outs=(0, 0)),
                                 dict(inplace=True)], ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_argument_errors_before_any_device_work(bad):
    rc, msg = _call(**bad)
    assert rc == -1 and msg


def test_valid_arguments_without_a_gpu_fail_loudly():
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _call()[0] == -3  # DFMI_ERR_NODEV
    assert _call(nser=1, stride=0, sstride=0, ystride=0, cstride=0)[0] == -3  # one series: the strides do not count
    assert _call(status=False, sstride=0, outs=(0, 1), ystride=0)[0] == -3  # strides of absent arrays do not count
    assert _call(nser=0)[0] == -3 and _call(N=0)[0] == -3
