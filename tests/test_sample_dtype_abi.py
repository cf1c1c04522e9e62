"""The typed sample entry points (dfmi_demod_typed, dfmi_demod_rows_typed,
dfmi_nls_record_typed) at the ABI level: declared, bound, exported, and their argument
checks, which run on the host before any device work (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPED = ("dfmi_demod_typed", "dfmi_demod_rows_typed", "dfmi_nls_record_typed")
W0 = 2 * np.pi * 1000.0 / 200000.0


def test_typed_symbols_declared_listed_and_exported():
    from deepfmkit_amd import _lib
    with open(os.path.join(ROOT, "include", "dfmi.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(dfmi_[a-z_]+)\s*\(", src))
    _lib.load()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for s in TYPED:
        assert s in declared, s
        assert s in _lib.SYMBOLS, s
        assert hasattr(so, s), s
    assert re.search(r"#define\s+DFMI_F64\s+0\b", src) and re.search(r"#define\s+DFMI_F32\s+1\b", src)
    assert (_lib.DFMI_F64, _lib.DFMI_F32) == (0, 1)


def _calls(lib, _lib, x, xtype):
    """The three typed calls on one host record of 2 buffers x 4000 samples -> return codes."""
    H = _lib.DFMI_MEM_HOST
    qi, dc = np.zeros((20, 2)), np.zeros(2)
    rows = np.zeros((2, lib.dfmi_qi_row_stride(10)))
    g = np.array([1.6, 6.0, 0.0, 0.0])
    out, ok = np.zeros((6, 2)), np.zeros(2, dtype=np.int32)
    return (lib.dfmi_demod_typed(_lib.ptr(x), xtype, 2, 4000, 4000, 10, W0, 0, _lib.ptr(qi), _lib.ptr(dc), H, None),
            lib.dfmi_demod_rows_typed(_lib.ptr(x), xtype, 2, 4000, 4000, 10, W0, 0, _lib.ptr(rows), H, None),
            lib.dfmi_nls_record_typed(_lib.ptr(x), xtype, 1, 8000, 2, 4000, 10, W0, 0, _lib.ptr(g), 1, 1, None,
                                      _lib.ptr(out), _lib.ptr(ok), H, None))


def _untyped(lib, _lib, x):
    H = _lib.DFMI_MEM_HOST
    qi, dc = np.zeros((20, 2)), np.zeros(2)
    rows = np.zeros((2, lib.dfmi_qi_row_stride(10)))
    g = np.array([1.6, 6.0, 0.0, 0.0])
    out, ok = np.zeros((6, 2)), np.zeros(2, dtype=np.int32)
    return (lib.dfmi_demod(_lib.ptr(x), 2, 4000, 4000, 10, W0, 0, _lib.ptr(qi), _lib.ptr(dc), H, None),
            lib.dfmi_demod_rows(_lib.ptr(x), 2, 4000, 4000, 10, W0, 0, _lib.ptr(rows), H, None),
            lib.dfmi_nls_record(_lib.ptr(x), 1, 8000, 2, 4000, 10, W0, 0, _lib.ptr(g), 1, 1, None, _lib.ptr(out),
                                _lib.ptr(ok), H, None))


def _record():
    t = np.arange(8000) / 200000.0
    return 1.0 + np.cos(0.3 + 6.0 * np.cos(2 * np.pi * 1000.0 * t + 0.1))


def test_unknown_sample_type_is_an_argument_error():
    """xtype is checked with the other arguments, before the device is looked for: -1
    (DFMI_ERR_ARG) with or without a GPU, and the message names the sample type."""
    from deepfmkit_amd import _lib
    lib = _lib.load()
    x = _record().astype(np.float32)
    for bad in (7, -1, 2):
        assert _calls(lib, _lib, x, bad) == (-1, -1, -1), bad
        assert b"sample type" in lib.dfmi_last_error()


def test_other_argument_checks_hold_for_typed_calls():
    from deepfmkit_amd import _lib
    lib = _lib.load()
    x = _record().astype(np.float32)
    H = _lib.DFMI_MEM_HOST
    qi, dc = np.zeros((20, 2)), np.zeros(2)
    # seg_stride < R, and a null sample pointer
    assert lib.dfmi_demod_typed(_lib.ptr(x), _lib.DFMI_F32, 2, 100, 4000, 10, W0, 0, _lib.ptr(qi), _lib.ptr(dc), H,
                                None) == -1
    assert lib.dfmi_demod_typed(None, _lib.DFMI_F32, 2, 4000, 4000, 10, W0, 0, _lib.ptr(qi), _lib.ptr(dc), H,
                                None) == -1


def test_valid_float32_call_returns_what_the_untyped_call_returns():
    """Valid arguments: the float32 and the float64 typed calls end like the untyped call on
    the widened record, DFMI_ERR_NODEV (-3) on a machine without a GPU (no host fallback)."""
    from deepfmkit_amd import _lib
    lib = _lib.load()
    x64 = _record().astype(np.float32).astype(np.float64)
    want = _untyped(lib, _lib, x64)
    assert _calls(lib, _lib, x64.astype(np.float32), _lib.DFMI_F32) == want
    assert _calls(lib, _lib, x64, _lib.DFMI_F64) == want
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        assert want == (-3, -3, -3)
    else:
        assert want == (0, 0, 0)


def test_python_layer_keeps_float32_host_records_narrow():
    """fitters._host_samples: float32 stays float32 (no host widening), everything else
    becomes float64 as before."""
    from deepfmkit_amd.fitters import _host_samples
    a32 = np.arange(6, dtype=np.float32)
    assert _host_samples(a32) is a32
    for other in (np.arange(6, dtype=np.float64), np.arange(6, dtype=np.int32), np.arange(6, dtype=np.float16),
                  [1.0, 2.0]):
        assert _host_samples(other).dtype == np.float64


def test_read_raw_dtype_needs_a_device(tmp_path):
    from deepfmkit_amd import textio
    p = str(tmp_path / "raw.txt")
    textio.write_raw(p, [np.arange(8.0)], t0=0, f_samp=200000.0, f_mod=1000.0)
    with pytest.raises(ValueError):
        textio.read_raw(p, dtype="float32")
    with pytest.raises(ValueError):
        textio.read_raw(p, device="cuda:0", dtype="int32")
