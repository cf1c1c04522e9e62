"""Demodulation under a cosine-sum window (dfmi_demod_window, dfmi_nls_record_window, window=).

Reference: the definition in np.longdouble (`reference` below): w[t] = sum_m a_m cos(2 pi m t / R),
Q_h = sum w x cos(w_h t) / sum w with w_h = longdouble(float64(h w0)), I_h with sin, dc = sum w x / sum w.
Gates (tests/test_gpu_demod_blocks.py): max |dQI| <= 1e-12 max|x|, dc relative <= 1e-13.
Signal: 1.6 (1 + cos(phi + 6 cos(w0 t + psi))) + 1 % noise, dc of order 1; int16 scaled to +-20000 counts."""
import numpy as np
import pytest

from conftest import compare_fit, wrapped

pytestmark = pytest.mark.gpu
PI = 4 * np.arctan(np.longdouble(1))
A, B, C, D, E, F = (200e3, 1e3), (128e3, 1e3), (256e3, 1e3), (200e3, 500.0), (512e3, 1e3), (30e3, 400.0)  # L 200 .. 75
CASES = [  # (f_samp, f_mod), R in half periods, window, ndata, dtype
    (A, 4, "hann", 10, "float64"), (A, 5, "blackmanharris", 10, "float64"), (A, 10, "blackmanharris", 20, "float64"),
    (A, 10, "hann", 10, "float32"), (A, 5, "blackmanharris", 10, "int16"), (A, 10, "hann", 20, "int16"),
    (A, 4, "blackmanharris", 10, "float64"), (B, 4, "hann", 10, "float64"), (B, 5, "blackmanharris", 20, "float32"),
    (B, 10, "blackmanharris", 10, "int16"), (B, 10, "hann", 20, "float64"), (C, 4, "blackmanharris", 10, "float64"),
    (C, 5, "hann", 20, "float64"), (C, 10, "blackmanharris", 10, "float32"), (C, 10, "hann", 10, "int16"),
    (D, 4, "hann", 10, "float64"), (D, 5, "blackmanharris", 10, "float64"), (D, 10, "blackmanharris", 20, "float64"),
    (D, 10, "blackmanharris", 10, "float32"), (D, 5, "hann", 10, "int16"), (E, 4, "hann", 10, "float64"),
    (E, 5, "blackmanharris", 10, "float64"), (E, 10, "blackmanharris", 10, "float32"), (E, 10, "hann", 10, "int16"),
    (F, 4, "hann", 10, "float64"), (F, 5, "blackmanharris", 20, "float64"), (F, 10, "blackmanharris", 10, "float32"),
    (F, 10, "hann", 10, "int16")]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not pytest.importorskip("torch").cuda.is_available():
        pytest.skip("no GPU")


def coefs(window):
    from deepfmkit_amd import _lib
    return _lib.window_coefficients(window)


def signal(n, w0, dtype="float64", seed=1, noise=0.01, phi=0.4, drift=3e-5, psi=0.3):
    t = np.arange(n)
    x = 1.6 * (1 + np.cos(phi + drift * t + 6 * np.cos(w0 * t + psi))) + noise * np.random.RandomState(seed).randn(n)
    return np.round(x * 6000).astype(np.int16) if dtype == "int16" else x.astype(dtype)


def reference(segs, window, nd, w0):
    """(n, R) segments -> QI (2 nd, n), dc (n,) of the definition, in long double."""
    x = np.asarray(segs).astype(np.longdouble)
    t = np.arange(x.shape[1], dtype=np.longdouble)
    w = sum(np.longdouble(a) * np.cos(2 * PI * m * t / x.shape[1]) for m, a in enumerate(coefs(window)))
    wh = [np.longdouble(np.float64((h + 1) * w0)) for h in range(nd)]
    qi = np.array([(x * w * f(v * t)).sum(axis=1) / w.sum() for f in (np.cos, np.sin) for v in wh])
    return qi, (x * w).sum(axis=1) / w.sum()


def demod(x, nseg, stride, R, nd, w0, window, period=0, check=True):
    """dfmi_demod_window on a numpy array (host memory) or a CUDA tensor -> (qi, dc, kernel) or the error code."""
    import torch
    from deepfmkit_amd import _lib
    from deepfmkit_amd.fitters import _xtype
    lib, a, dev = _lib.load(), coefs(window), hasattr(x, "data_ptr")
    qi, dc = np.full((2 * nd, nseg), np.nan), np.full(nseg, np.nan)
    if dev:
        qi, dc = torch.from_numpy(qi).cuda(), torch.from_numpy(dc).cuda()
    rc = lib.dfmi_demod_window(_lib.ptr(x), _xtype(x.dtype), nseg, stride, R, nd, w0, period, _lib.ptr(a), a.size,
                               _lib.ptr(qi), _lib.ptr(dc), 1 if dev else 0,
                               torch.cuda.current_stream().cuda_stream if dev else None)
    if not check:
        return rc
    assert rc == 0, lib.dfmi_last_error()
    if dev:
        qi, dc = qi.cpu().numpy(), dc.cpu().numpy()
    return qi, dc, lib.dfmi_last_demod_kernel().decode()


def gate(qi, dc, segs, window, nd, w0, what):
    rq, rd = reference(segs, window, nd, w0)
    eq = float(np.abs(qi - rq).max() / np.abs(segs).max())
    ed = float(np.abs((dc - rd) / rd).max())
    print(f"{what}: QI err {eq:.2e} of max|x|, dc err {ed:.2e} relative")
    assert eq <= 1e-12 and ed <= 1e-13


@pytest.mark.parametrize("fs_fm,halves,window,nd,dtype", CASES)
def test_against_long_double(fs_fm, halves, window, nd, dtype):
    fs, fm = fs_fm
    L, w0 = int(round(fs / fm)), 2 * np.pi * fm / fs
    R = halves * (L // 2) + (L % 2) * (halves // 2)  # 2 L, 2 L + L // 2, 5 L
    x = signal(5 * R, w0, dtype).reshape(5, R)
    qi, dc, kern = demod(x, 5, R, R, nd, w0, window)
    assert kern.startswith("demod_window_kernel<") and f"K={len(coefs(window)) - 1}]" in kern, kern
    gate(qi, dc, x, window, nd, w0, f"L={L} R={R} {window} ndata={nd} {dtype} ({kern})")
    if dtype != "float64":
        q64, d64, _ = demod(x.astype(np.float64), 5, R, R, nd, w0, window)
        np.testing.assert_array_equal(qi, q64)
        np.testing.assert_array_equal(dc, d64)


def test_odd_alignment_view():
    """A device view starting one sample in loads sample by sample (VEC 1, four slots at L = 256)."""
    import torch
    L, R, w0 = 256, 640, 2 * np.pi / 256
    x = torch.from_numpy(signal(5 * R + 1, w0)).cuda()
    odd, even = x[1:], x[1:].clone()
    qo, do, ko = demod(odd, 5, R, R, 10, w0, "blackman")
    qe, de, ke = demod(even, 5, R, R, 10, w0, "blackman")
    assert ko.startswith("demod_window_kernel<1,4>") and ke.startswith("demod_window_kernel<2,2>"), (ko, ke)
    gate(qo, do, odd.cpu().numpy().reshape(5, R), "blackman", 10, w0, "odd view")
    assert np.abs(qo - qe).max() <= 1e-12 * float(x.max()) and np.abs(do / de - 1).max() <= 1e-13


@pytest.mark.parametrize("stride", [200, 403], ids=["overlap", "gaps"])
def test_segment_stride(stride):
    R, w0 = 400, 2 * np.pi / 200
    x = signal(6 * stride + R, w0)
    segs = np.stack([x[s * stride:s * stride + R] for s in range(7)])
    qi, dc, _ = demod(x, 7, stride, R, 10, w0, "hann")
    gate(qi, dc, segs, "hann", 10, w0, f"seg_stride {stride}")


def test_many_segments_per_wave():
    """20,000 segments: every wave of the persistent grid takes several, reusing its per-bin factors."""
    nseg, R, w0 = 20000, 400, 2 * np.pi / 200
    x = signal(nseg * R, w0).reshape(nseg, R)
    qi, dc, _ = demod(x, nseg, R, R, 10, w0, "blackmanharris")
    pick = np.unique(np.r_[0, nseg - 1, np.linspace(1, nseg - 2, 14).astype(int)])
    gate(qi[:, pick], dc[pick], x[pick], "blackmanharris", 10, w0, "20000 segments")
    assert not np.isnan(qi).any() and not np.isnan(dc).any()


def test_one_coefficient_is_the_rectangular_call():
    from deepfmkit_amd import _lib
    R, w0 = 500, 2 * np.pi / 200
    x = signal(5 * R, w0, "float32").reshape(5, R)
    qi, dc, _ = demod(x, 5, R, R, 10, w0, [1.0])
    q0, d0 = np.empty_like(qi), np.empty_like(dc)
    _lib.check(_lib.load().dfmi_demod_typed(_lib.ptr(x), _lib.DFMI_F32, 5, R, R, 10, w0, 0, _lib.ptr(q0), _lib.ptr(d0),
                                            0, None), "dfmi_demod_typed")
    np.testing.assert_array_equal(qi, q0)
    np.testing.assert_array_equal(dc, d0)


@pytest.mark.parametrize("f_mod", [997.0, 100.0], ids=["no-period", "L2000"])
def test_unsupported_geometry(f_mod):
    from deepfmkit_amd import _lib
    assert demod(np.ones((2, 4000)), 2, 4000, 4000, 10, 2 * np.pi * f_mod / 200e3, "hann", check=False) == -4
    assert b"period" in _lib.load().dfmi_last_error()


@pytest.mark.parametrize("parallel,hop", [(True, None), (False, None), (True, 400)])
def test_record_against_the_oracle(parallel, hop):
    """12 buffers of R = 800 at 40 dB: nls_records(window='hann') against oracle.nls_oracle.fit_segment driven
    over the reference's windowed QI with the same seeding and chaining, at compare_fit's defaults."""
    from oracle import nls_oracle as O
    from deepfmkit_amd.fitters import nls_records
    R, nbuf, nd, w0, step = 800, 12, 10, 2 * np.pi / 200, hop or 800
    x = signal((nbuf - 1) * step + R, w0, noise=0.016, drift=5e-6)
    segs = np.stack([x[s * step:s * step + R] for s in range(nbuf)])
    qi, dc = reference(segs, "hann", nd, w0)
    qi, rows, g = qi.astype(np.float64).T, [], np.array([1.6, 6.0, 0.0, 0.0])
    for b in range(nbuf):
        st, p, ssq = O.fit_segment(nd, qi[b], g)
        g = p if not parallel or b == 0 else g
        rows.append((*p, float(dc[b]), ssq, st))
    cols, ok = nls_records(x.reshape(1, -1), 200e3, 1e3, R, nbuf, nd, parallel=parallel, hop=hop, window="hann")
    ours = dict(zip(O.COLUMNS, list(cols) + [ok]))
    compare_fit(ours, dict(zip(O.COLUMNS, np.array(rows).T)))


def test_facade_returns_the_record_call():
    import deepfmkit_amd as dfm
    from deepfmkit_amd.fitters import nls_records
    dff, laser, ifo = dfm.DeepFitFramework(), dfm.LaserConfig(), dfm.InterferometerConfig()
    dfm.set_laser_df_for_effect(laser, ifo, 6.0)
    dff.load_sim(dfm.DFMIObject("ch", laser, ifo, f_samp=200e3))
    dff.simulate("ch", n_seconds=0.048, mode="snr", snr_db=40.0, trial_num=0)
    fit = dff.fit("ch", n=4, window="hann")
    cols, ok = nls_records(dff.raws["ch"].samples().reshape(1, -1), 200e3, 1e3, fit.R, fit.nbuf, window="hann")
    cols = cols.cpu().numpy() if hasattr(cols, "cpu") else cols
    for i, k in enumerate(("amp", "m", "phi", "psi", "dc", "ssq")):
        np.testing.assert_array_equal(getattr(fit, k), cols[i])


def test_known_answer_blackmanharris():
    """Noiseless, R = 5 L (n = 5 > K = 3 whole periods): the windowed QI are the Bessel model's."""
    from deepfmkit_amd.fitters import nls_records
    x = signal(3 * 1000, 2 * np.pi / 200, noise=0.0, drift=0.0)
    cols, ok = nls_records(x.reshape(1, -1), 200e3, 1e3, 1000, 3, window="blackmanharris")
    err = [np.abs(cols[0] - 1.6).max(), np.abs(cols[1] - 6.0).max(), wrapped(cols[2] - 0.4).max(), np.abs(cols[3] - 0.3).max()]
    print("known answer |d amp, m, phi, psi|:", [f"{e:.2e}" for e in err])
    assert (ok == 0).all() and max(err) <= 1e-9
