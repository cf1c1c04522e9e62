"""calc_lpsd through the drop-in facade on the GPU: after a fit of a 500-buffer snr-mode record,
DeepFitFramework.calc_lpsd / DeepFitObject.calc_lpsd set f and Sxx to what
deepfmkit_amd.lpsd.lpsd gives for the fitted series, bit for bit, alone or batched with other
fits; an unknown label logs the reference's warning and changes nothing; an unsupported
window raises ValueError."""
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import deepfmkit_amd as dfm  # noqa: E402
from deepfmkit_amd.lpsd import lpsd  # noqa: E402


@pytest.fixture(scope="module")
def fitted():
    """Two 500-buffer records (m = 6, 40 dB, 200 kS/s, n = 20: 50 fits per second) and a
    shorter third, fitted once."""
    dff = dfm.DeepFitFramework()
    for label, seconds, trial in (("a", 10.0, 0), ("b", 10.0, 1), ("short", 4.0, 2)):
        laser, ifo = dfm.LaserConfig(), dfm.InterferometerConfig()
        dfm.set_laser_df_for_effect(laser, ifo, 6.0)
        dff.load_sim(dfm.DFMIObject(label, laser, ifo, f_samp=200000.0))
        dff.simulate(label, n_seconds=seconds, mode="snr", snr_db=40.0, trial_num=trial)
        dff.fit(label, n=20, fit_label=label)
    return dff


def test_calc_lpsd_sets_f_and_sxx_bit_for_bit(fitted):
    dff = fitted
    fit = dff.fits["a"]
    assert fit.phi.size == 500 and fit.fs == 50.0
    dff.calc_lpsd()
    for label in ("a", "b", "short"):  # a and b share one call, short has its own plan
        fo = dff.fits[label]
        r = lpsd(fo.phi, fo.fs)
        assert isinstance(fo.f, np.ndarray) and isinstance(fo.Sxx, np.ndarray)
        assert np.array_equal(fo.f, r.f) and np.array_equal(fo.Sxx, r.Sxx)
        assert np.isfinite(fo.Sxx).all() and (fo.Sxx > 0).all()
    assert dff.fits["short"].f.size != fit.f.size
    # the object's own method, and a parameter other than phi
    sxx_phi = fit.Sxx.copy()
    fit.calc_lpsd(which="m")
    assert np.array_equal(fit.Sxx, lpsd(fit.m, fit.fs).Sxx) and not np.array_equal(fit.Sxx, sxx_phi)
    dff.calc_lpsd(labels=["a"], which="m")
    assert np.array_equal(fit.Sxx, lpsd(fit.m, fit.fs).Sxx)
    fit.calc_lpsd()
    assert np.array_equal(fit.Sxx, sxx_phi)


def test_settings_of_the_fit_object_are_used(fitted):
    fit = fitted.fits["b"]
    fit.Jdes, fit.order = 100, -1
    try:
        fitted.calc_lpsd(labels=["a", "b"])
        r = lpsd(fit.phi, fit.fs, Jdes=100, order=-1)
        assert np.array_equal(fit.f, r.f) and np.array_equal(fit.Sxx, r.Sxx)
        assert fitted.fits["a"].f.size != fit.f.size
    finally:
        del fit.Jdes, fit.order


def test_unknown_label_logs_the_warning_and_changes_nothing(fitted, caplog):
    fitted.calc_lpsd(labels=["a"])
    before = {k: (v.f.copy(), v.Sxx.copy()) for k, v in fitted.fits.items() if v.f is not None}
    with caplog.at_level(logging.WARNING):
        fitted.calc_lpsd(labels=["nope"])
    assert "Specified label is invalid!" in caplog.text
    assert set(fitted.fits) == {"a", "b", "short"}
    for k, (f, s) in before.items():
        assert np.array_equal(fitted.fits[k].f, f) and np.array_equal(fitted.fits[k].Sxx, s)


def test_unsupported_window_raises(fitted):
    fit = fitted.fits["a"]
    fit.win = np.hanning
    try:
        with pytest.raises(ValueError, match="Kaiser"):
            fit.calc_lpsd()
        with pytest.raises(ValueError, match="Kaiser"):
            fitted.calc_lpsd(labels=["a"])
    finally:
        del fit.win
