"""dfmi_fisher's argument checks and the host-side helpers, without a GPU: every argument
error is reported before any device work, valid arguments without a GPU are DFMI_ERR_NODEV
(no CPU fallback); helpers.snr_to_asd / calculate_jacobian against the fixture (the same numpy
arithmetic: 1e-15 relative); errors=True refuses ndata < 3 and any method but 'nls' before the
engine is touched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import fisher_cases as C  # noqa: E402


def _call(n=3, ld=None, ndata=10, params=True, var=None, outs=(1, 1, 1, 1)):
    from deepfmkit_amd import _lib
    lib = _lib.load()
    ld = max(n, 0) if ld is None else ld
    p = np.ones((4, max(ld, 1)))
    p[1] = 6.0
    bufs = [np.zeros((10, max(n, 1))), np.zeros((10, max(n, 1))), np.zeros((4, max(n, 1))),
            np.zeros(max(n, 1), dtype=np.int32)]
    return lib.dfmi_fisher(_lib.ptr(p) if params else None, n, ld, ndata, _lib.ptr(var), 1.0,
                           *[_lib.ptr(b) if on else None for b, on in zip(bufs, outs)], _lib.DFMI_MEM_HOST, None)


def test_symbol_is_declared_and_bound():
    from deepfmkit_amd import _lib
    assert "dfmi_fisher" in _lib.SYMBOLS
    with open(os.path.join(C.ROOT, "include", "dfmi.h")) as f:
        assert "int dfmi_fisher(" in f.read()


def test_argument_errors_before_any_device_work():
    assert _call(n=-1, ld=0) == -1
    assert _call(n=3, ld=2) == -1
    assert _call(ndata=0) == -1
    assert _call(ndata=-4) == -1
    assert _call(params=False) == -1
    assert _call(outs=(0, 0, 0, 1)) == -1  # jtj, cov and sigma all NULL
    assert _call(outs=(0, 0, 0, 0)) == -1
    from deepfmkit_amd import _lib
    assert b"jtj" in _lib.load().dfmi_last_error()


def test_valid_arguments_without_a_gpu_fail_loudly():
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _call() == -3  # DFMI_ERR_NODEV
    assert _call(outs=(0, 0, 1, 0)) == -3
    assert _call(n=0, params=False) == -3  # n == 0 is valid; the device guard still answers
    from deepfmkit_amd import helpers
    from deepfmkit_amd._lib import DFMIError
    with pytest.raises(DFMIError):
        helpers.calculate_m_precision(np.linspace(1, 30, 5), 10, 80.0)
    with pytest.raises(DFMIError):
        helpers.calculate_crlb_for_m(6.0, 10, 40.0, 200)


def test_host_helpers_match_the_reference_fixture():
    import deepfmkit_amd as dfm
    from deepfmkit_amd import helpers
    g = C.golden()
    assert dfm.calculate_jacobian is helpers.calculate_jacobian and dfm.snr_to_asd is helpers.snr_to_asd
    assert helpers.set_laser_df_for_effect is dfm.set_laser_df_for_effect
    asd = np.array([helpers.snr_to_asd(s, f) for s, f in g["asd_args"]])
    assert (np.abs(asd - g["asd"]) <= 1e-15 * g["asd"]).all()
    for p, nd, J in zip(g["jac_p"], g["jac_nd"], g["jac"]):
        ours = helpers.calculate_jacobian(int(nd), p)
        assert ours.shape == (2 * nd, 4)
        ref = J[:2 * nd]
        assert (np.abs(ours - ref) <= 1e-15 * np.abs(ref)).all()
        if p[0] == 0.0:
            assert (ours == 0).all()


def test_fisher_binding_rejects_bad_requests_on_the_host():
    from deepfmkit_amd import helpers
    with pytest.raises(ValueError):
        helpers.fisher(np.ones((4, 3)), 10, want=())
    with pytest.raises(ValueError):
        helpers.fisher(np.ones((4, 3)), 10, want=("sigma", "chi"))
    with pytest.raises(ValueError):
        helpers.fisher(np.ones((5, 3)), 10)
    with pytest.raises(ValueError):
        helpers.fisher(np.ones((4, 3)), 10, var=np.ones(2))


def _framework(nbuf=4):
    import deepfmkit_amd as dfm
    dff = dfm.DeepFitFramework()
    raw = dfm.DeepRawObject(np.ones(200 * nbuf))
    raw.label, raw.f_samp, raw.f_mod, raw.t0 = "r", 200000.0, 1000.0, 0.0
    dff.raws["r"] = raw
    return dff


def test_errors_needs_degrees_of_freedom_and_the_nls_method():
    from deepfmkit_amd import fitters
    dff = _framework()
    with pytest.raises(ValueError, match="ndata >= 3"):
        dff.fit("r", n=1, ndata=2, errors=True)
    with pytest.raises(ValueError, match="ndata >= 3"):
        dff.fit_many(["r"], n=1, ndata=2, errors=True)
    with pytest.raises(ValueError, match="ndata >= 3"):
        fitters.nls_records(np.ones((1, 800)), 200000.0, 1000.0, 200, 4, ndata=1, errors=True)
    with pytest.raises(ValueError, match="ndata >= 3"):
        fitters.nls_record_devices(np.ones(800), 200000.0, 1000.0, 200, 4, [0], ndata=2, errors=True)
    with pytest.raises(ValueError, match="'nls' only"):
        dff.fit("r", method="ekf", n=1, errors=True)
    with pytest.raises(ValueError, match="'nls' only"):
        dff.fit_many(["r"], method="ekf", n=1, errors=True)
    assert not dff.fits and not dff.fits_df
