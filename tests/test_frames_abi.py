"""Frame-interleaved records at the ABI level: dfmi_demod_frames / dfmi_nls_record_frames exist
with the declared argument types, their argument checks answer before any device work, and
nls_frames refuses input that is not a (samples, channels) block. No GPU needed."""
import ctypes

import numpy as np
import pytest

W0 = 2 * np.pi * 1000.0 / 200000.0


def _call(lib, _lib, x, xtype, nch, fs, nbuf=2, R=400):
    """Both entry points on host frames x -> their two return codes."""
    nseg = max(nch, 1) * nbuf
    qi, dc, out = np.zeros((20, nseg)), np.zeros(nseg), np.zeros((6, nseg))
    ok, g, p, H = np.zeros(nseg, dtype=np.int32), np.tile([1.6 * 4096, 6.0, 0.0, 0.0], (max(nch, 1), 1)), _lib.ptr, 0
    return (lib.dfmi_demod_frames(p(x), xtype, nch, fs, nbuf, R, 10, W0, 0, p(qi), p(dc), H, None),
            lib.dfmi_nls_record_frames(p(x), xtype, nch, fs, nbuf, R, 10, W0, 0, p(g), 1, 1, None, p(out), p(ok), H,
                                       None))


def test_symbols_and_argtypes():
    from deepfmkit_amd import _lib
    lib = _lib.load()
    P, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert {"dfmi_demod_frames", "dfmi_nls_record_frames"} <= set(_lib.SYMBOLS)
    assert lib.dfmi_demod_frames.argtypes == [P, i32, i32, i64, i64, i32, i32, dbl, i32, P, P, i32, P]
    assert lib.dfmi_nls_record_frames.argtypes == [P, i32, i32, i64, i64, i32, i32, dbl, i32, P, i32, i64,
                                                   ctypes.POINTER(_lib.LMConfig), P, P, i32, P]


@pytest.mark.parametrize("xtype,nch,fs,msg", [(3, 0, 2, b"nch"), (3, -1, 2, b"nch"), (3, 2, 1, b"frame_stride"),
                                              (2, 2, 2, b"sample type"), (7, 2, 2, b"sample type")])
def test_argument_errors(xtype, nch, fs, msg):
    from deepfmkit_amd import _lib
    lib = _lib.load()
    x = np.zeros((800, 2), dtype=np.int16)
    for rc in _call(lib, _lib, x, xtype, nch, fs):
        assert rc == -1
    assert msg in lib.dfmi_last_error()


def test_nls_frames_refuses_what_is_not_a_frames_block():
    torch = pytest.importorskip("torch")
    from deepfmkit_amd.fitters import nls_frames
    with pytest.raises(ValueError, match="2-D"):
        nls_frames(np.zeros(800, dtype=np.int16), 200000.0, 1000.0, 400, 2)
    with pytest.raises(ValueError, match="stride"):
        nls_frames(torch.zeros((2, 800), dtype=torch.int16).T, 200000.0, 1000.0, 400, 2)
    with pytest.raises(ValueError, match="fewer"):
        nls_frames(np.zeros((700, 2), dtype=np.int16), 200000.0, 1000.0, 400, 2)
