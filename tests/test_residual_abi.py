"""dfmi_residual's argument checks and the residuals= keyword's refusals, without a GPU: every
argument error is reported before any device work, valid arguments without a GPU are
DFMI_ERR_NODEV (no CPU fallback)."""
import numpy as np
import pytest


def _call(xtype=0, nseg=3, seg_stride=200, R=200, ld=None, dc=True, outs=(1, 1, 1, 1), resid_stride=None):
    from deepfmkit_amd import _lib
    lib = _lib.load()
    x = np.zeros(4 * 200)
    p = np.ones((5, max(nseg, 1) if ld is None else max(ld, 1)))
    bufs = [np.zeros(4), np.zeros(4), np.zeros(4, dtype=np.int32), np.zeros((4, 256))]
    rss, peak, ipeak, resid = [_lib.ptr(b) if on else None for b, on in zip(bufs, outs)]
    return lib.dfmi_residual(_lib.ptr(x), xtype, nseg, seg_stride, R, 2 * np.pi / 200, 0, _lib.ptr(p),
                             nseg if ld is None else ld, _lib.ptr(p[4]) if dc else None, rss, peak, ipeak, resid,
                             256 if resid_stride is None else resid_stride, _lib.DFMI_MEM_HOST, None)


@pytest.mark.parametrize("bad", [dict(xtype=2), dict(R=0), dict(seg_stride=0), dict(ld=2), dict(resid_stride=199),
                                 dict(dc=False), dict(outs=(0, 0, 0, 0))])
def test_argument_errors_before_any_device_work(bad):
    from deepfmkit_amd import _lib
    assert "dfmi_residual" in _lib.SYMBOLS and hasattr(_lib.load(), "dfmi_residual")
    assert _call(**bad) == -1


def test_valid_arguments_without_a_gpu_fail_loudly():
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _call() == -3  # DFMI_ERR_NODEV
    assert _call(outs=(0, 0, 1, 0), seg_stride=50, xtype=3) == -3
    assert _call(outs=(1, 1, 1, 0), resid_stride=0) == -3  # resid_stride counts only with resid


def test_residuals_keyword_refusals():
    import deepfmkit_amd as dfm
    from deepfmkit_amd import fitters
    dff = dfm.DeepFitFramework()
    raw = dfm.DeepRawObject(np.ones(800))
    raw.label, raw.f_samp, raw.f_mod, raw.t0 = "r", 200000.0, 1000.0, 0.0
    dff.raws["r"] = raw
    with pytest.raises(ValueError, match="'nls' only"):
        dff.fit("r", method="ekf", n=1, residuals=True)
    with pytest.raises(ValueError, match="residuals=True"):
        dff.fit_many(["r"], n=1, residuals=True)
    with pytest.raises(ValueError, match="residuals=True"):
        dff.fit("r", n=1, residuals=True, devices=[0])
    with pytest.raises(ValueError, match="residuals=True"):
        fitters.nls_frames(np.ones((800, 2)), 200000.0, 1000.0, 200, 4, residuals=True)
    assert not dff.fits and not dff.fits_df
