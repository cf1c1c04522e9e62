"""DeepFitFramework.fit(errors=True) / fit_many(errors=True) on the GPU: the per-buffer standard
errors of the NLS fit (dfmi_fisher behind dfmi_nls_record, fitters.nls_records).

Records use R = 200 (n = 1 cycle at f_samp 200 kHz, f_mod 1 kHz), the 40 dB record of
tests/helpers/fisher_cases.py. Invariants, over nbuf 1, 2, 65, 130 x ndata 3, 10, 13, 17, 30,
62 x float64 / float32 x host / device input x parallel=False / True / n_cores=3 /
devices=[0], fit_many over 3 channels, one noise-only buffer (nbuf >= 65):
  (a) the seven base columns and tau are bit for bit those of the same call without errors;
  (b) the four error columns equal, bit for bit, a stand-alone dfmi_fisher on the returned
      parameters and ssq;
  (c) they meet the sigma gate against the numpy reference at the returned parameters
      (parity then does not depend on which path the LM took);
  (d) column order, dtypes, the DeepFitObject attributes and tau_err.
Statistical: on 2,000 buffers, sqrt(mean(err^2)) / std(fitted, ddof=1) within 1 +- 0.079 for
amp, m, phi, psi (five standard errors of an empirical standard deviation), every fitok 0.
Measured on the MI355X: worst sigma ratio 0.0012; statistical ratios amp 1.0064,
m 0.9921, phi 1.0021, psi 0.9983."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import fisher_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import deepfmkit_amd as dfm  # noqa: E402
from deepfmkit_amd import helpers  # noqa: E402

R = 200
BASE = ["amp", "m", "phi", "psi", "dc", "ssq", "fitok"]
ERR = ["amp_err", "m_err", "phi_err", "psi_err"]
MODES = (dict(parallel=False), dict(parallel=True), dict(parallel=True, n_cores=3), dict(devices=[0]))


def record(nbuf, shift=0):
    """nbuf buffers of the 40 dB record starting at buffer `shift`; buffer 7 is noise only
    (no signal, the same noise level) when there are at least 65."""
    y = np.array(C.stat_record()[shift * R:(shift + nbuf) * R])
    if nbuf >= 65:
        y[7 * R:8 * R] = 1.0 + np.random.RandomState(5).normal(0.0, np.sqrt(0.5e-4), R)
    return y


def framework(ys, dtype, device, with_sim=True):
    dff = dfm.DeepFitFramework()
    laser, ifo = dfm.LaserConfig(), dfm.InterferometerConfig()
    dfm.set_laser_df_for_effect(laser, ifo, 6.0)
    for k, y in enumerate(ys):
        raw = dfm.DeepRawObject()
        x = np.ascontiguousarray(y, dtype=dtype)
        raw.data = torch.from_numpy(x).cuda() if device else x
        raw.label, raw.f_samp, raw.f_mod, raw.t0 = f"c{k}", 200000.0, 1000.0, 0.0
        raw.sim = dfm.DFMIObject(f"c{k}", laser, ifo, f_samp=200000.0) if with_sim else None
        dff.raws[raw.label] = raw
    return dff, 2 * np.pi * laser.df


def check_pair(df0, fit0, df1, fit1, ndata, tau_div, worst):
    # (d) layout
    assert list(df0.columns) == BASE + ["tau"]
    assert list(df1.columns) == BASE + ERR + ["tau", "tau_err"]
    assert all(df1[k].dtype == np.float64 for k in ERR + ["tau", "tau_err"]) and df1["fitok"].dtype == np.int64
    assert not any(hasattr(fit0, k) for k in ERR + ["tau_err"])
    # (a) the base columns and tau
    for k in BASE + ["tau"]:
        assert np.array_equal(df0[k].to_numpy(), df1[k].to_numpy(), equal_nan=True), k
    for k in ("amp", "m", "phi", "psi", "dc", "ssq", "tau"):
        assert np.array_equal(getattr(fit0, k), getattr(fit1, k), equal_nan=True), k
    for k in ERR + ["tau_err"]:
        assert np.array_equal(getattr(fit1, k), df1[k].to_numpy(), equal_nan=True), k
    err = np.array([df1[k].to_numpy() for k in ERR])
    te = err[1] / tau_div if tau_div is not None else np.zeros(err.shape[1])
    assert np.array_equal(df1["tau_err"].to_numpy(), te)
    # (b) a stand-alone dfmi_fisher on what was returned
    p = np.array([df1[k].to_numpy() for k in ("amp", "m", "phi", "psi")])
    alone = helpers.fisher(p, ndata, var=df1["ssq"].to_numpy(), var_mul=1.0 / (2 * ndata - 4))
    assert np.array_equal(alone["sigma"], err, equal_nan=True)
    # (c) the numpy reference at the returned parameters
    assert (alone["ok"] == 1).all() and np.isfinite(err).all()
    A, X, cond = C.reference(p, ndata)
    worst[0] = max(worst[0], C.ratio_sigma(err, X, cond, df1["ssq"].to_numpy() / (2 * ndata - 4)))


@pytest.mark.parametrize("ndata", [3, 10, 13, 17, 30, 62])
def test_invariants(ndata):
    worst = [0.0]
    for nbuf, (dtype, device), mode in itertools.product((1, 2, 65, 130), itertools.product(
            (np.float64, np.float32), (False, True)), MODES):
        dff, tau_div = framework([record(nbuf)], dtype, device)
        fit0 = dff.fit("c0", n=1, ndata=ndata, fit_label="plain", **mode)
        fit1 = dff.fit("c0", n=1, ndata=ndata, fit_label="err", errors=True, **mode)
        assert fit1.nbuf == nbuf and dff.fits_df["err"].shape == (nbuf, 13)
        check_pair(dff.fits_df["plain"], fit0, dff.fits_df["err"], fit1, ndata, tau_div, worst)
    print(f"fit(errors=True) ndata {ndata}: worst sigma ratio {worst[0]:.3g}")
    assert worst[0] <= 1.0


@pytest.mark.parametrize("device", [False, True])
def test_fit_many_three_channels_and_no_simulation(device):
    worst = [0.0]
    ys = [record(65, shift) for shift in (0, 100, 300)]
    for ndata, dtype in ((10, np.float64), (17, np.float32)):
        dff, tau_div = framework(ys, dtype, device)
        labels = ["c0", "c1", "c2"]
        plain = dff.fit_many(labels, n=1, ndata=ndata)
        frames0 = {l: dff.fits_df[f"{l}_nls"] for l in labels}
        witherr = dff.fit_many(labels, n=1, ndata=ndata, errors=True)
        for l in labels:
            check_pair(frames0[l], plain[l], dff.fits_df[f"{l}_nls"], witherr[l], ndata, tau_div, worst)
            # one channel of the batch equals the single-channel call
            one = dff.fit(l, n=1, ndata=ndata, errors=True, fit_label="one")
            assert all(np.array_equal(getattr(one, k), getattr(witherr[l], k)) for k in ERR + ["tau_err"])
    dff, _ = framework(ys[:1], np.float64, device, with_sim=False)
    f0 = dff.fit("c0", n=1, fit_label="plain")
    f1 = dff.fit("c0", n=1, fit_label="err", errors=True)
    check_pair(dff.fits_df["plain"], f0, dff.fits_df["err"], f1, 10, None, worst)
    assert (f1.tau_err == 0).all() and (f1.tau == 0).all()
    assert worst[0] <= 1.0


def test_nls_records_returns_the_errors_on_the_input_side():
    from deepfmkit_amd import fitters
    y = record(65)
    cols, ok, sig = fitters.nls_records(y.reshape(1, -1), 200000.0, 1000.0, R, 65, errors=True)
    assert isinstance(sig, np.ndarray) and sig.shape == (4, 65)
    side = torch.cuda.Stream()
    x = torch.from_numpy(y).cuda().view(1, -1)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # stream-ordered behind the record call, on the caller's stream
        dcols, dok, dsig = fitters.nls_records(x, 200000.0, 1000.0, R, 65, errors=True)
    side.synchronize()
    assert dsig.is_cuda and np.array_equal(dsig.cpu().numpy(), sig) and np.array_equal(dcols.cpu().numpy(), cols)
    assert len(fitters.nls_records(x, 200000.0, 1000.0, R, 65)) == 2


def test_errors_match_the_scatter_of_the_fitted_values():
    S = C.STAT
    dff, _ = framework([C.stat_record()], np.float64, False)
    fit = dff.fit("c0", n=S["n"], ndata=S["ndata"], errors=True)
    df = dff.fits_df["c0_nls"]
    assert fit.nbuf == S["nbuf"] and (df["fitok"].to_numpy() == 0).all()
    r = C.stat_ratios([fit.amp, fit.m, fit.phi, fit.psi], [fit.amp_err, fit.m_err, fit.phi_err, fit.psi_err])
    print("gpu ratios sqrt(mean err^2)/std(fitted): amp %.4f m %.4f phi %.4f psi %.4f" % tuple(r))
    assert (np.abs(r - 1.0) <= C.STAT_BAND).all(), r
