"""deepfmkit_amd.lpsd.lcsd and DeepFitFramework.calc_lcsd on the GPU: numpy arrays and CUDA
tensors give the same bits (non-contiguous tensors included), a 1-D x is shared by the rows of a
2-D y, mismatched inputs raise ValueError; after fit_many of short snr-mode records calc_lcsd
equals lcsd of the fitted phi arrays, singly and for a list of labels, mismatched lengths
raise, and an unknown label logs calc_lpsd's warning and returns None."""
import logging
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lcsd_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import deepfmkit_amd as dfm  # noqa: E402
from deepfmkit_amd.lpsd import LCSDResult, lcsd  # noqa: E402

SPECTRA = ("Sxx", "Syy", "Sxy", "coh", "H", "resid", "enbw")


def same(a, b):
    """Every field of two results bit for bit (tensors are read back)."""
    for n in LCSDResult._fields:
        u, v = (t.cpu().numpy() if torch.is_tensor(t) else t for t in (getattr(a, n), getattr(b, n)))
        if u.shape != v.shape or u.dtype != v.dtype or not np.array_equal(u, v, equal_nan=True):
            return False
    return True


def _stack(shape):
    X, Y = zip(*(C.pair(shape, m) for m in C.MEANS))
    return np.stack(X), np.stack(Y)


@pytest.mark.parametrize("shape", ["s1", "s3"])
def test_numpy_and_tensors_give_the_same_bits(shape):
    kw = C.settings(shape)
    X, Y = _stack(shape)
    host = lcsd(X, Y, C.FS, **kw)
    assert host.Sxy.dtype == np.complex128 and host.H.dtype == np.complex128 and host.Sxy.shape == (3, host.f.size)
    dX, dY = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    dev = lcsd(dX, dY, C.FS, **kw)
    for n in SPECTRA:
        assert getattr(dev, n).is_cuda
    assert dev.Sxy.dtype == torch.complex128 and dev.H.dtype == torch.complex128
    assert same(dev, host)
    # one pair: (J,) results, the batch's row
    one = lcsd(dX[1], dY[1], C.FS, **kw)
    one_host = lcsd(X[1], Y[1], C.FS, **kw)
    assert one.Sxy.shape == (host.f.size,) and same(one, one_host)
    assert np.array_equal(one_host.Sxy, host.Sxy[1]) and np.array_equal(one_host.coh, host.coh[1])
    # rows of a wider buffer (row stride > N) are read in place; a transposed buffer is copied first
    wide = torch.full((3, X.shape[1] + 37), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, :X.shape[1]] = dY
    assert same(lcsd(dX, wide[:, :X.shape[1]], C.FS, **kw), host)
    transposed = dX.t().contiguous().t()
    every_other = torch.from_numpy(np.repeat(Y, 2, axis=1)).cuda()[:, ::2]
    assert transposed.stride(1) == 3 and every_other.stride(1) == 2
    assert same(lcsd(transposed, every_other, C.FS, **kw), host)


def test_one_x_against_many_y():
    kw = C.settings("s1")
    X, Y = _stack("s1")
    shared = lcsd(X[0], Y, C.FS, **kw)
    assert shared.Sxx.shape == shared.Sxy.shape == (3, shared.f.size)
    for i in range(3):
        one = lcsd(X[0], Y[i], C.FS, **kw)
        for n in SPECTRA[:-1]:
            assert np.array_equal(getattr(shared, n)[i], getattr(one, n))
    dev = lcsd(torch.from_numpy(X[0]).cuda(), torch.from_numpy(Y).cuda(), C.FS, **kw)
    assert same(dev, shared)
    assert lcsd(X[0], Y[:1], C.FS, **kw).Sxy.shape == (1, shared.f.size)


def test_value_errors():
    x, y = C.pair("s1", 0.0)
    dx, dy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    with pytest.raises(ValueError, match="both"):
        lcsd(dx, y, C.FS)
    with pytest.raises(ValueError, match="both"):
        lcsd(x, dy, C.FS)
    with pytest.raises(ValueError, match="length"):
        lcsd(dx, dy[:-1], C.FS)
    with pytest.raises(ValueError, match="float64"):
        lcsd(dx.float(), dy.float(), C.FS)
    with pytest.raises(ValueError, match="float64"):
        lcsd(dx, dy.float(), C.FS)
    with pytest.raises(ValueError, match="shapes"):
        lcsd(torch.stack([dx, dx]), dy, C.FS)
    with pytest.raises(ValueError, match="Kaiser"):
        lcsd(dx, dy, C.FS, win=np.hanning)
    with pytest.raises(ValueError, match="order"):
        lcsd(dx, dy, C.FS, order=1)
    with pytest.raises(ValueError, match="psll"):
        lcsd(dx, dy, C.FS, psll=0)


@pytest.fixture(scope="module")
def fitted():
    """Three 300-buffer records (m = 6, 40 dB, 200 kS/s, n = 20: 50 fits per second) and a shorter
    fourth, fitted by fit_many (labels '<label>_nls')."""
    dff = dfm.DeepFitFramework()
    for label, seconds, trial in (("a", 6.0, 0), ("b", 6.0, 1), ("c", 6.0, 2), ("short", 4.0, 3)):
        laser, ifo = dfm.LaserConfig(), dfm.InterferometerConfig()
        dfm.set_laser_df_for_effect(laser, ifo, 6.0)
        dff.load_sim(dfm.DFMIObject(label, laser, ifo, f_samp=200000.0))
        dff.simulate(label, n_seconds=seconds, mode="snr", snr_db=40.0, trial_num=trial)
    dff.fit_many(["a", "b", "c"], n=20)
    dff.fit_many(["short"], n=20)
    return dff


def test_calc_lcsd_is_lcsd_of_the_fitted_series(fitted):
    fa, fb, fc = (fitted.fits[f"{l}_nls"] for l in "abc")
    assert fa.phi.size == 300 and fa.fs == 50.0
    before = {k: dict(vars(v)) for k, v in fitted.fits.items()}
    r = fitted.calc_lcsd("a_nls", "b_nls")
    assert isinstance(r, LCSDResult) and same(r, lcsd(fa.phi, fb.phi, fa.fs))
    assert np.isfinite(r.coh).all() and r.Sxy.shape == (r.f.size,)
    assert same(fitted.calc_lcsd("a_nls", "b_nls", which="m"), lcsd(fa.m, fb.m, fa.fs))
    # the list form: one x against several fits, a dict by label
    d = fitted.calc_lcsd("a_nls", ["b_nls", "c_nls"])
    assert list(d) == ["b_nls", "c_nls"]
    assert same(d["b_nls"], r) and same(d["c_nls"], lcsd(fa.phi, fc.phi, fa.fs))
    # the fit objects' LPSD settings are used, and must agree
    fa.Jdes = fb.Jdes = 100
    try:
        assert same(fitted.calc_lcsd("a_nls", "b_nls"), lcsd(fa.phi, fb.phi, fa.fs, Jdes=100))
        with pytest.raises(ValueError, match="settings"):
            fitted.calc_lcsd("a_nls", ["b_nls", "c_nls"])
    finally:
        del fa.Jdes, fb.Jdes
    # nothing is stored on the fits
    for k, v in fitted.fits.items():
        assert set(vars(v)) == set(before[k])


def test_calc_lcsd_mismatched_lengths_raise_and_unknown_labels_warn(fitted, caplog):
    with pytest.raises(ValueError, match="length"):
        fitted.calc_lcsd("a_nls", "short_nls")
    with pytest.raises(ValueError, match="length"):
        fitted.calc_lcsd("a_nls", ["b_nls", "short_nls"])
    with caplog.at_level(logging.WARNING):
        assert fitted.calc_lcsd("a_nls", "nope") is None
    assert "Specified label is invalid!" in caplog.text
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        assert fitted.calc_lcsd("nope", ["a_nls"]) is None
        assert fitted.calc_lcsd("a_nls", ["b_nls", "nope"]) is None
    assert caplog.text.count("Specified label is invalid!") == 2
