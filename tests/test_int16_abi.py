"""int16 sample records (DFMI_I16) at the ABI level: the typed entry points accept the type,
their argument checks hold for it, and the Python layer keeps an int16 record int16. All of
this runs on the host before any device work (no GPU needed)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W0 = 2 * np.pi * 1000.0 / 200000.0


def _record16():
    """One record of 2 buffers x 4000 samples as 12-bit-scale counts."""
    t = np.arange(8000) / 200000.0
    x = 1.0 + np.cos(0.3 + 6.0 * np.cos(2 * np.pi * 1000.0 * t + 0.1))
    return np.clip(np.rint(4096.0 * x), -32768, 32767).astype(np.int16)


def _outputs(lib):
    return dict(qi=np.zeros((20, 2)), dc=np.zeros(2), rows=np.zeros((2, lib.dfmi_qi_row_stride(10))),
                g=np.array([1.6 * 4096, 6.0, 0.0, 0.0]), out=np.zeros((6, 2)), ok=np.zeros(2, dtype=np.int32))


def _typed(lib, _lib, x, xtype):
    o, H, p = _outputs(lib), _lib.DFMI_MEM_HOST, _lib.ptr
    return (lib.dfmi_demod_typed(p(x), xtype, 2, 4000, 4000, 10, W0, 0, p(o["qi"]), p(o["dc"]), H, None),
            lib.dfmi_demod_rows_typed(p(x), xtype, 2, 4000, 4000, 10, W0, 0, p(o["rows"]), H, None),
            lib.dfmi_nls_record_typed(p(x), xtype, 1, 8000, 2, 4000, 10, W0, 0, p(o["g"]), 1, 1, None, p(o["out"]),
                                      p(o["ok"]), H, None))


def _untyped(lib, _lib, x):
    o, H, p = _outputs(lib), _lib.DFMI_MEM_HOST, _lib.ptr
    return (lib.dfmi_demod(p(x), 2, 4000, 4000, 10, W0, 0, p(o["qi"]), p(o["dc"]), H, None),
            lib.dfmi_demod_rows(p(x), 2, 4000, 4000, 10, W0, 0, p(o["rows"]), H, None),
            lib.dfmi_nls_record(p(x), 1, 8000, 2, 4000, 10, W0, 0, p(o["g"]), 1, 1, None, p(o["out"]), p(o["ok"]), H,
                                None))


def test_i16_is_declared_as_3():
    from deepfmkit_amd import _lib
    with open(os.path.join(ROOT, "include", "dfmi.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"#define\s+DFMI_I16\s+3\b", src)
    assert _lib.DFMI_I16 == 3


def test_valid_int16_call_returns_what_the_untyped_call_returns():
    """Valid arguments: each of the three typed calls on an int16 record ends like the untyped
    call on the widened record: DFMI_ERR_NODEV (-3) on a machine without a GPU, 0 with one
    (an unknown sample type would be -1)."""
    from deepfmkit_amd import _lib
    lib = _lib.load()
    x16 = _record16()
    want = _untyped(lib, _lib, x16.astype(np.float64))
    assert _typed(lib, _lib, x16, _lib.DFMI_I16) == want
    torch = pytest.importorskip("torch")
    assert want == ((0, 0, 0) if torch.cuda.is_available() else (-3, -3, -3))


def test_argument_checks_hold_for_int16():
    from deepfmkit_amd import _lib
    lib = _lib.load()
    x, o, H, p, I16 = _record16(), _outputs(lib), _lib.DFMI_MEM_HOST, _lib.ptr, _lib.DFMI_I16
    # seg_stride < R, R = 0, ndata = 0, and null sample / output pointers
    assert lib.dfmi_demod_typed(p(x), I16, 2, 100, 4000, 10, W0, 0, p(o["qi"]), p(o["dc"]), H, None) == -1
    assert lib.dfmi_demod_typed(p(x), I16, 2, 4000, 0, 10, W0, 0, p(o["qi"]), p(o["dc"]), H, None) == -1
    assert lib.dfmi_demod_typed(None, I16, 2, 4000, 4000, 10, W0, 0, p(o["qi"]), p(o["dc"]), H, None) == -1
    assert lib.dfmi_demod_typed(p(x), I16, 2, 4000, 4000, 10, W0, 0, None, p(o["dc"]), H, None) == -1
    assert lib.dfmi_demod_rows_typed(p(x), I16, 2, 100, 4000, 10, W0, 0, p(o["rows"]), H, None) == -1
    assert lib.dfmi_demod_rows_typed(p(x), I16, 2, 4000, 4000, 0, W0, 0, p(o["rows"]), H, None) == -1
    assert lib.dfmi_demod_rows_typed(None, I16, 2, 4000, 4000, 10, W0, 0, p(o["rows"]), H, None) == -1
    args = (p(o["g"]), 1, 1, None, p(o["out"]), p(o["ok"]), H, None)
    assert lib.dfmi_nls_record_typed(p(x), I16, 2, 4000, 2, 4000, 10, W0, 0, *args) == -1  # rec_stride < nbuf R
    assert b"rec_stride" in lib.dfmi_last_error()
    assert lib.dfmi_nls_record_typed(None, I16, 1, 8000, 2, 4000, 10, W0, 0, *args) == -1
    assert b"null" in lib.dfmi_last_error()
    assert lib.dfmi_nls_record_typed(p(x), I16, 1, 8000, 2, 4000, 10, W0, 0, None, 1, 1, None, p(o["out"]),
                                     p(o["ok"]), H, None) == -1


def test_python_layer_keeps_int16_host_records_narrow():
    from deepfmkit_amd.fitters import _host_samples
    a16 = np.arange(6, dtype=np.int16)
    assert _host_samples(a16) is a16
    for other in (np.arange(6, dtype=np.uint16), np.arange(6, dtype=np.int8), np.arange(6, dtype=np.int64)):
        assert _host_samples(other).dtype == np.float64


def test_read_raw_int16_needs_a_device(tmp_path):
    from deepfmkit_amd import textio
    p = str(tmp_path / "raw.txt")
    textio.write_raw(p, [np.arange(8.0)], t0=0, f_samp=200000.0, f_mod=1000.0)
    with pytest.raises(ValueError, match="device"):
        textio.read_raw(p, dtype="int16")
