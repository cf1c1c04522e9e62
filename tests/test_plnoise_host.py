"""The coloured-noise generator on the CPU, through the test-only host
build tests/hostcheck_plnoise: the design against the numpy restatement, the cascade bit for
bit against scipy.signal.lfilter, whole coloured asd-mode trials bit for bit against
SignalGenerator.generate, and white-only configurations unchanged."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import plnoise_cases as C  # noqa: E402
import plnoise_ref as R  # noqa: E402

HC = os.path.join(os.path.dirname(__file__), "hostcheck_plnoise", "libhostcheck_plnoise.so")
P_, I64, DBL = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double


@pytest.fixture(scope="module")
def hc():
    assert os.path.exists(HC), "tests/hostcheck_plnoise not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(HC)
    lib.hc_plnoise_design.argtypes = [DBL, I64, DBL, P_, ctypes.c_int, P_]
    lib.hc_plnoise_design.restype = ctypes.c_int
    lib.hc_plnoise.argtypes = [P_, ctypes.c_int, DBL, DBL, ctypes.c_uint32, I64, I64, P_]
    lib.hc_plnoise.restype = None
    lib.hc_sizeof_synth_colour.restype = I64
    lib.hc_synth_trial_coloured.argtypes = [P_, P_, P_, ctypes.c_int, DBL, I64, I64, DBL, P_]
    lib.hc_synth_trial_coloured.restype = None
    return lib


def _ulps(a, b):
    return np.max(np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b))))


def _hc_design(hc, fs, n, alpha):
    sec, scale = np.zeros((64, 3)), np.zeros(1)
    nsec = hc.hc_plnoise_design(fs, n, alpha, sec.ctypes.data, 64, scale.ctypes.data)
    return nsec, sec, scale[0]


@pytest.mark.parametrize("fs", [50.0, 30000.0, 200000.0])
@pytest.mark.parametrize("alpha", [0.5, 1.0, 2.0])
def test_design_matches_restatement(hc, fs, alpha):
    from deepfmkit_amd import physics as P
    for n in (4, 5, 64, 200, 4000, 4096, 200000, 2 ** 20, 10 ** 7):
        want, wscale = R.design(fs, n, alpha)
        nsec, sec, scale = _hc_design(hc, fs, n, alpha)
        assert nsec == len(want) <= 64
        assert _ulps(sec[:nsec], want) <= 4 and _ulps(np.array([scale]), np.array([wscale])) <= 4
        # the library's entry (what Python and the device use) is the same table
        lsec, lscale = P.alpha_noise_design(fs, n, alpha)
        assert lsec.shape == (nsec, 3)
        assert _ulps(lsec, want) <= 4 and _ulps(np.array([lscale]), np.array([wscale])) <= 4
    assert len(R.design(200000.0, 4000, 2.0)[0]) == 15 and len(R.design(200000.0, 200000, 2.0)[0]) == 23
    assert len(R.design(200000.0, 2 ** 20, 2.0)[0]) == 26


def test_design_rejections(hc):
    from deepfmkit_amd import physics as P
    for fs, n, alpha in ((200000.0, 3, 2.0), (200000.0, 0, 2.0), (200000.0, 4000, 0.0), (200000.0, 4000, -1.0),
                         (200000.0, 4000, 2.5), (0.0, 4000, 2.0), (float("nan"), 4000, 2.0)):
        assert _hc_design(hc, fs, n, alpha)[0] < 0
        with pytest.raises(ValueError):
            P.alpha_noise_design(fs, n, alpha)
    assert hc.hc_plnoise_design(200000.0, 4000, 2.0, None, 0, None) == 15  # count only
    assert hc.hc_plnoise_design(200000.0, 4000, 2.0, np.zeros(42).ctypes.data, 14, None) < 0  # no room


@pytest.mark.parametrize("nsec", [1, 2, 13, 63, 64])
def test_cascade_equals_lfilter(hc, nsec):
    """pl_series (the recurrence the kernel's lanes run) against scipy.signal.lfilter on the
    same table and the same RandomState draws, bit for bit, incl. fewer samples than sections."""
    from scipy.signal import lfilter
    sec, scale = R.table(nsec)
    sigma = np.sqrt(200000.0 / 2.0)
    for n in (1, 3, 64, 65, 313, 1000):
        for n_warm in (0, 2 * n):
            seed = 7 + nsec + n
            x = np.random.RandomState(seed).normal(scale=sigma, size=n_warm + n)
            for a0, a1, b1 in sec:
                x = lfilter([a0, a1], [1.0, -b1], x)
            want = scale * x[n_warm:]
            got = np.zeros(n)
            hc.hc_plnoise(sec.ctypes.data, nsec, scale, sigma, seed, n_warm, n, got.ctypes.data)
            np.testing.assert_array_equal(got, want)


def test_scalar_restatement_equals_lfilter():
    """The helper's own scalar loop (the GPU gate's float64 restatement) is lfilter's arithmetic."""
    from scipy.signal import lfilter
    sec, _ = R.table(13)
    x = np.random.RandomState(3).normal(size=3072)
    y = x
    for a0, a1, b1 in sec:
        y = lfilter([a0, a1], [1.0, -b1], y)
    np.testing.assert_array_equal(R.cascade(sec, x), y)


def _twin(hc, cfg, tn, n, dynamic):
    from deepfmkit_amd import physics as P
    rec = P.synth_trial_table([cfg], [tn], dynamic)
    col = P.synth_colour_table([cfg], [tn])
    sec, scale = P.alpha_noise_design(cfg.f_samp, n, 2.0)
    out = np.zeros(n)
    hc.hc_synth_trial_coloured(rec.ctypes.data, col.ctypes.data, sec.ctypes.data, len(sec), scale, 2 * n, n,
                               cfg.f_samp, out.ctypes.data)
    return out


@pytest.mark.parametrize("case", C.COLOUR_CASES)
def test_coloured_trials_bit_exact(hc, case):
    """synth.h + plnoise.h built for the host against the numpy generator (asd_noise_arrays'
    lfilter cascade + exact_model_signal): main and witness channels bit for bit."""
    from deepfmkit_amd import physics as P
    assert hc.hc_sizeof_synth_colour() == P.SYNTH_COLOUR_DTYPE.itemsize
    cfg, wit = C.configs(*case)
    assert P.device_synth_supported(cfg) and P.device_synth_supported(wit)
    for tn, ns in ((0, 0.02), (3, 0.02)) + (((1, 0.005),) if case == C.COLOUR_CASES[3] else ()):
        chans = P.SignalGenerator().generate(cfg, ns, mode="asd", trial_num=tn, witness_config=wit)
        for c, key, dyn in ((cfg, "main", True), (wit, "witness", False)):
            x = np.asarray(chans[key].samples())
            np.testing.assert_array_equal(_twin(hc, c, tn, x.size, dyn), x)


def test_noise_arrays_match_restatement():
    """asd_noise_arrays against the helper's scalar-loop restatement: the reference's order,
    one shared basis, seeds 1 + 4 t and 2 + 4 t; absent sources stay the scalar 0.0."""
    from deepfmkit_amd import physics as P
    cfg, _ = C.configs(1e6, 1e-12, 1e-4, 2e3)
    got = P.asd_noise_arrays(cfg, 600, trial_num=2)
    want = R.noise_arrays(cfg.f_samp, 600, 2, 1e6, 1e-4, 2e3, 1e-12)
    for k in ("laser_frequency", "amplitude", "df", "armlength"):
        np.testing.assert_array_equal(got[k], want[k])
    sec, scale = R.design(cfg.f_samp, 600, 2.0)
    np.testing.assert_array_equal(P.alpha_noise(cfg.f_samp, 600, 2.0, [10, 11])[1],
                                  R.series(sec, scale, np.sqrt(cfg.f_samp / 2.0), 11, 1200, 600))
    only = P.asd_noise_arrays(C.configs(0.0, 1e-12, 0.0, 0.0)[0], 600, trial_num=2)
    assert only["laser_frequency"] == 0.0 and np.isscalar(only["laser_frequency"]) and only["amplitude"] == 0.0


def test_white_only_unchanged(hc):
    """White-only configurations: today's arrays exactly (the white stream is untouched by the
    coloured one), and the coloured twin with a zero colour row is synth_trial's bits."""
    from deepfmkit_amd import physics as P
    cfg, _ = C.configs(0.0, 0.0, 1e-4, 2e3)
    nz = P.asd_noise_arrays(cfg, 4000, trial_num=3)
    rng = np.random.RandomState(13)
    assert nz["laser_frequency"] == 0.0 and nz["armlength"] == 0.0
    np.testing.assert_array_equal(nz["amplitude"], rng.normal(scale=1e-4 * np.sqrt(cfg.f_samp / 2.0), size=4000))
    np.testing.assert_array_equal(nz["df"], rng.normal(scale=2e3 * np.sqrt(cfg.f_samp / 2.0), size=4000))
    x = np.asarray(P.SignalGenerator().generate(cfg, 0.02, mode="asd", trial_num=3)["main"].samples())
    np.testing.assert_array_equal(_twin(hc, cfg, 3, x.size, True), x)
    # the white draws of a coloured configuration are the white-only configuration's
    both = P.asd_noise_arrays(C.configs(1e6, 1e-12, 1e-4, 2e3)[0], 4000, trial_num=3)
    np.testing.assert_array_equal(both["amplitude"], nz["amplitude"])
    np.testing.assert_array_equal(both["df"], nz["df"])
