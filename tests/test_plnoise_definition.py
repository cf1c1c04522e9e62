"""Properties of the coloured-noise definition on the CPU: the
Welch spectrum of generated series against the analytic response, the band in which
PSD f^alpha stays flat, and the known answer of frequency noise through the oracle fit."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
sys.path.insert(0, os.path.dirname(HERE))
import plnoise_cases as C  # noqa: E402
import plnoise_ref as R  # noqa: E402


@pytest.mark.parametrize("alpha,seed", [(2.0, 2), (1.0, 6), (2.0, 10)])
def test_welch_spectrum(alpha, seed):
    """nperseg = 2^11 over N = 2^15 at 200 kHz, bins 16 ... fs/8 (240 bins): the median of
    measured over analytic PSD within 0.9-1.1, the fitted slope within 0.1 of -alpha."""
    from scipy.signal import welch
    from deepfmkit_amd import physics as P
    fs, n = 200000.0, 2 ** 15
    x = P.alpha_noise(fs, n, alpha, [seed])[0]
    f, pxx = welch(x, fs=fs, nperseg=2 ** 11)
    sel = slice(16, 2 ** 11 // 8)
    assert sel.stop - sel.start == 240 and abs(f[sel.stop] - fs / 8) < 1e-6
    sec, scale = P.alpha_noise_design(fs, n, alpha)
    ratio = np.median(pxx[sel] / R.response2(sec, scale, fs, f[sel]))
    slope = np.polyfit(np.log10(f[sel]), np.log10(pxx[sel]), 1)[0]
    print(f"alpha {alpha} seed {seed}: median ratio {ratio:.4f} slope {slope:.3f}")
    assert 0.9 <= ratio <= 1.1
    assert abs(slope + alpha) <= 0.1


@pytest.mark.parametrize("alpha,lo", [(2.0, 0.941), (1.0, 0.971)])
def test_analytic_response_band(alpha, lo):
    """|H(f)|^2 f^alpha of the designed cascade stays in [lo, 1] for 4 f_min <= f <= fs/8
    (lo = 0.941 at alpha 2, 0.971 at alpha 1, the definition's own figures), at every
    record length the project uses."""
    from deepfmkit_amd import physics as P
    fs = 200000.0
    for n in (4000, 200000, 2 ** 20):
        sec, scale = P.alpha_noise_design(fs, n, alpha)
        f = np.geomspace(4 * fs / n, fs / 8, 4000)
        flat = R.response2(sec, scale, fs, f) * f ** alpha
        print(f"alpha {alpha} n {n}: PSD f^alpha in [{flat.min():.4f}, {flat.max():.4f}]")
        assert lo - 5e-4 <= flat.min() and flat.max() <= 1.0 + 5e-4


def test_known_answer_through_oracle_fit():
    """Default configuration, m = 6, f_n = 1e6 and no other noise, trial 0, 1 s fitted by the
    oracle with n = 20: the fitted phase follows the buffer means of the frequency noise.
    Residual std <= 1e-2 x excursion std (3.9e-3 rad), every fitok 0."""
    from oracle import nls_oracle as O
    from deepfmkit_amd import physics as P
    cfg = C.quickstart_config()
    x = np.asarray(P.SignalGenerator().generate(cfg, 1.0, mode="asd", trial_num=0)["main"].samples())
    fit = O.fit_record_sequential(x, cfg.f_samp, cfg.laser.f_mod, 20)
    noise = P.asd_noise_arrays(cfg, x.size, 0)["laser_frequency"]
    resid, exc = C.known_answer(fit[:, 2], cfg, noise, 4000)
    print(f"known answer: residual std {resid:.3e} rad, excursion std {exc:.3e} rad, ratio {resid / exc:.2e}")
    assert np.all(fit[:, 6] == 0)
    assert exc > 1e-3
    assert resid <= 1e-2 * exc
