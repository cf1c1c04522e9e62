"""Windowed demodulation at the ABI level: dfmi_demod_window / dfmi_nls_record_window exist, their
argument checks answer before any device work, valid arguments without a GPU are DFMI_ERR_NODEV
(no CPU fallback), and the window= keyword's refusals. No GPU needed."""
import numpy as np
import pytest

W0 = 2 * np.pi * 1000.0 / 200000.0
HANN = (0.5, -0.5)


def _calls(xtype=0, wcoef=HANN, nw=None, stride=400, hop=400, nrec=1, rec_stride=0):
    """(demodulation rc, record rc) for 3 segments of R = 400 (float64 zeros)."""
    from deepfmkit_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    w = None if wcoef is None else np.array(wcoef, dtype=np.float64)
    nw = (0 if w is None else w.size) if nw is None else nw
    n = 3 * nrec
    x, qi, dc, out = np.zeros(2 * 1200), np.zeros((20, n)), np.zeros(n), np.zeros((6, n))
    ok, g = np.zeros(n, dtype=np.int32), np.tile([1.6, 6.0, 0.0, 0.0], (nrec, 1))
    return (lib.dfmi_demod_window(p(x), xtype, 3, stride, 400, 10, W0, 0, p(w), nw, p(qi), p(dc), 0, None),
            lib.dfmi_nls_record_window(p(x), xtype, nrec, rec_stride, 3, 400, hop, 10, W0, 0, p(w), nw, p(g), 1, 2, None,
                                       p(out), p(ok), 0, None))


def test_symbols_exported():
    from deepfmkit_amd import _lib
    lib = _lib.load()
    for name in ("dfmi_demod_window", "dfmi_nls_record_window"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)


@pytest.mark.parametrize("kw,msg", [
    (dict(nw=0), b"nwcoef"), (dict(nw=5, wcoef=(1, 0, 0, 0, 0)), b"nwcoef"), (dict(wcoef=None, nw=2), b"null wcoef"),
    (dict(wcoef=(0.0, -0.5)), b"wcoef[0]"), (dict(wcoef=(0.5, np.nan)), b"non-finite"),
    (dict(wcoef=(np.inf, 0.5)), b"non-finite"), (dict(xtype=2), b"sample type"), (dict(xtype=7), b"sample type"),
    (dict(stride=0, hop=0), b""), (dict(stride=-400, hop=401), b""), (dict(wcoef=(1.0,), stride=0, hop=0), b"")])
def test_argument_errors(kw, msg):
    from deepfmkit_amd import _lib
    for rc in _calls(**kw):
        assert rc == -1
        assert msg in _lib.load().dfmi_last_error()


def test_valid_arguments_without_a_gpu_fail_loudly():
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for kw in ({}, dict(wcoef=(1.0,)), dict(stride=200, hop=200), dict(stride=403, nrec=2, rec_stride=1200, xtype=1)):
        assert _calls(**kw) == (-3, -3)  # DFMI_ERR_NODEV


@pytest.mark.parametrize("call,match", [
    (lambda d, f, n: f.nls_records(np.ones((1, 800)), 2e5, 1e3, 400, 2, window="hann", residuals=True), "residuals=True"),
    (lambda d, f, n: f.nls_records(np.ones((1, 800)), 2e5, 1e3, 400, 2, window="hann", errors=True), "errors=True"),
    (lambda d, f, n: d.fit("r", n=1, window="hann", devices=[0]), "devices="),
    (lambda d, f, n: d.fit_many(["r"], n=1, window="hann"), "fit_many"),
    (lambda d, f, n: f.nls_frames(np.ones((800, 2)), 2e5, 1e3, 200, 4, window="hann"), "nls_frames"),
    (lambda d, f, n: d.fit("r", method="ekf", n=1, window="hann"), "'nls' only"),
    (lambda d, f, n: f.nls_records(np.ones((1, 800)), 2e5, 1e3, 400, 2, window="kaiser"), "unknown window"),
    (lambda d, f, n: d.fit("r", n=1, window="kaiser"), "unknown window"),
    (lambda d, f, n: f.nls_records(np.ones((1, 800)), 2e5, 1e3, 400, 2, window=[1, 0, 0, 0, 0]), "1 to 4"),
    (lambda d, f, n: n.demodulate(np.ones((2, 400)), 10, W0, window=[]), "1 to 4")])
def test_window_keyword_refusals(call, match):
    import deepfmkit_amd as dfm
    from deepfmkit_amd import fit as nfit, fitters
    dff = dfm.DeepFitFramework()
    raw = dfm.DeepRawObject(np.ones(800))
    raw.label, raw.f_samp, raw.f_mod, raw.t0 = "r", 200000.0, 1000.0, 0.0
    dff.raws["r"] = raw
    with pytest.raises(ValueError, match=match):
        call(dff, fitters, nfit)
    assert not dff.fits and not dff.fits_df
