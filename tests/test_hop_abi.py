"""Overlapped segments at the ABI level: dfmi_demod_hop / dfmi_nls_record_hop exist with the declared
argument types, and their argument checks answer before any device work. No GPU needed."""
import ctypes

import numpy as np
import pytest

W0 = 2 * np.pi * 1000.0 / 200000.0


def test_symbols_and_argtypes():
    from deepfmkit_amd import _lib
    lib = _lib.load()
    P, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert {"dfmi_demod_hop", "dfmi_nls_record_hop"} <= set(_lib.SYMBOLS)
    assert lib.dfmi_demod_hop.argtypes == [P, i32, i64, i64, i64, i32, i32, i32, dbl, i32, P, P, i32, P]
    assert lib.dfmi_nls_record_hop.argtypes == [P, i32, i64, i64, i64, i32, i32, i32, dbl, i32, P, i32, i64,
                                                ctypes.POINTER(_lib.LMConfig), P, P, i32, P]


@pytest.mark.parametrize("xtype,nrec,stride,hop,msg", [
    (3, 1, 0, 0, b"hop"), (3, 1, 0, -200, b"hop"), (3, 1, 0, 402, b"hop"), (3, 2, 799, 200, b"rec_stride"),
    (2, 1, 0, 200, b"sample type"), (7, 1, 0, 200, b"sample type")])
def test_argument_errors(xtype, nrec, stride, hop, msg):
    """nseg = 3 windows of R = 400 at hop 200 need 800 samples a record."""
    from deepfmkit_amd import _lib
    lib, p, n = _lib.load(), _lib.ptr, 3 * max(nrec, 1)
    x, qi, dc, out = np.zeros((2, 800), dtype=np.int16), np.zeros((20, n)), np.zeros(n), np.zeros((6, n))
    ok, g = np.zeros(n, dtype=np.int32), np.tile([1.6 * 4096, 6.0, 0.0, 0.0], (2, 1))
    for rc in (lib.dfmi_demod_hop(p(x), xtype, nrec, stride, 3, 400, hop, 10, W0, 0, p(qi), p(dc), 0, None),
               lib.dfmi_nls_record_hop(p(x), xtype, nrec, stride, 3, 400, hop, 10, W0, 0, p(g), 1, 1, None, p(out), p(ok),
                                       0, None)):
        assert rc == -1
        assert msg in lib.dfmi_last_error()


def test_nls_records_refuses_a_bad_hop():
    from deepfmkit_amd.fitters import nls_records
    x = np.zeros((1, 800), dtype=np.int16)
    with pytest.raises(ValueError, match="hop"):
        nls_records(x, 200000.0, 1000.0, 400, None, hop=401)
    with pytest.raises(ValueError, match="shorter"):
        nls_records(x, 200000.0, 1000.0, 400, 4, hop=200)
