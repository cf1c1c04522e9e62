"""int16 sample records (ADC counts) through the typed entry points (DFMI_I16, include/dfmi.h).

The contract: an int16 record gives, BIT FOR BIT, what the float64 path gives on the same
counts (`x16.double()`) in the same layout — QI, dc, the six result columns and fitok; there is
no tolerance. int16 -> double is exact and the kernels keep every phase bin's ascending-time
order, so anything else is a load-path bug (sign extension, the half of the 4-byte pair load).
Records come from the package's snr-mode generator (f_samp 200 kHz, m = 6, 40 dB), quantised
once per module as a 12-bit-scale ADC would: x16 = clamp(round(4096 x), -32768, 32767). The
fits start from an amplitude of 1.6 * 4096 counts. Shapes follow tests/test_gpu_sample_dtype.py
(the same kernels' edges).

The bin kernels have two int16 folds behind the tuning key demod_i16_int: 1 (default) the
integer-accumulating fold (" [i16 int]" in dfmi_last_demod_kernel), 0 the float kernels' LDS-bin
fold on widened-in-register samples (" [i16]"). Every test that reaches a bin kernel runs at both
settings (the `i16_int` fixture) against the same float64 result, so the two are equal too."""
import numpy as np
import pytest

from conftest import compare_fit, record_tol

pytestmark = pytest.mark.gpu

F_SAMP = 200000.0
NMAX = 4097 * 4000  # the largest shape's samples (8193 x 2000, 12289 x 1000 and 12289 x 200 fit inside)
SCALE = 4096.0
GUESS = (1.6 * SCALE, 6.0, 0.0, 0.0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deepfmkit_amd import _lib
    assert _lib.load().dfmi_device_count() >= 1


@pytest.fixture(params=[1, 0], ids=["int-fold", "lds-bins"])
def i16_int(request):
    """Both settings of the tuning key demod_i16_int, restored to the default afterwards."""
    from deepfmkit_amd import _lib
    lib = _lib.load()
    _lib.check(lib.dfmi_set_tuning(b"demod_i16_int", request.param), "tune")
    yield request.param
    _lib.check(lib.dfmi_set_tuning(b"demod_i16_int", 1), "tune")


def native_tag(k64, int_fold=1):
    """The tag of a native int16 read: the integer fold where the float64 call ran a bin kernel
    (and the key is on and ceil(R / L) <= 65535, which holds for every shape but the guard test's)."""
    bins = k64.startswith("demod_bins_kernel") or k64.startswith("demod_seed_bins_kernel")
    return " [i16 int]" if bins and int_fold else " [i16]"


_CACHE = {}


def quantise(x):
    import torch
    return torch.clamp(torch.round(SCALE * x), -32768, 32767).to(torch.int16)


def record(f_mod=1000.0, n=NMAX, snr_db=40.0):
    """(x16, x64 = x16.double()) of the quantised snr-mode record at f_mod, on the GPU, made once."""
    import torch
    from deepfmkit_amd.physics import SnrSpec, synth_snr
    key = (f_mod, n, snr_db)
    if key not in _CACHE:
        x = torch.empty(n, dtype=torch.float64, device="cuda")
        synth_snr(SnrSpec(seed=77, f_samp=F_SAMP, f_mod=f_mod, m=6.0, snr_db=snr_db), 0, n, out=x)
        x16 = quantise(x)
        _CACHE[key] = (x16, x16.double())
    return _CACHE[key]


def w0_of(f_mod):
    from deepfmkit_amd.fitters import w0_of as w
    return w(f_mod, F_SAMP)


def demod(x, nseg, R, nd, f_mod, rows=False):
    """dfmi_demod(_typed) / dfmi_demod_rows(_typed) on nseg contiguous segments of the device
    tensor x (int16 through the typed call, float64 through the untyped one) ->
    (return code, outputs as numpy, kernel string)."""
    import torch
    from deepfmkit_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    i16 = x.dtype == torch.int16
    D = _lib.DFMI_MEM_DEVICE
    if rows:
        out = [torch.zeros((nseg, lib.dfmi_qi_row_stride(nd)), dtype=torch.float64, device="cuda")]
        args = (nseg, R, R, nd, w0_of(f_mod), 0, out[0].data_ptr(), D, st)
        rc = (lib.dfmi_demod_rows_typed(x.data_ptr(), _lib.DFMI_I16, *args) if i16
              else lib.dfmi_demod_rows(x.data_ptr(), *args))
    else:
        out = [torch.zeros((2 * nd, nseg), dtype=torch.float64, device="cuda"),
               torch.zeros(nseg, dtype=torch.float64, device="cuda")]
        args = (nseg, R, R, nd, w0_of(f_mod), 0, out[0].data_ptr(), out[1].data_ptr(), D, st)
        rc = lib.dfmi_demod_typed(x.data_ptr(), _lib.DFMI_I16, *args) if i16 else lib.dfmi_demod(x.data_ptr(), *args)
    kern = lib.dfmi_last_demod_kernel().decode() if rc == 0 else ""
    torch.cuda.synchronize()
    return rc, [o.cpu().numpy() for o in out], kern


def fit(x, R, nbuf, nd, f_mod=1000.0, **kw):
    """nls_records on a (nrec, >= nbuf R) tensor / array -> (cols, fitok, kernel string)."""
    from deepfmkit_amd import _lib
    from deepfmkit_amd.fitters import nls_records
    cols, ok = nls_records(x, F_SAMP, f_mod, R, nbuf, nd, init_guess=GUESS, **kw)
    kern = _lib.load().dfmi_last_demod_kernel().decode()
    if hasattr(cols, "cpu"):
        cols, ok = cols.cpu().numpy(), ok.cpu().numpy()
    return cols, ok, kern


def check_tags(k16, k64, native=None, int_fold=1):
    """The float64 string carries no tag; the int16 one is the same string + its tag."""
    assert "[" not in k64, k64
    if native is None:
        assert k16 in (k64 + native_tag(k64, int_fold), k64 + " [i16 widened]"), (k16, k64)
    else:
        assert k16 == k64 + (native_tag(k64, int_fold) if native else " [i16 widened]"), (k16, k64)


def check_all(f_mod, R, nbuf, nd, native=None, rows_native=True, snr_db=40.0, n=NMAX, demod_wide=1, int_fold=1):
    """QI + dc (component-major), the row layout and the whole record fit of the first nbuf
    buffers: int16 against float64 on the same counts, bit for bit. native: whether the
    component-major / record-fit kernels must report a native int16 read (None: either).
    demod_wide = 0: the many-harmonic kernel does not go ahead of the bin kernels."""
    from deepfmkit_amd import _lib
    lib = _lib.load()
    _lib.check(lib.dfmi_set_tuning(b"demod_wide", demod_wide), "tune")
    try:
        return _check_all(f_mod, R, nbuf, nd, native, rows_native, snr_db, n, int_fold)
    finally:
        _lib.check(lib.dfmi_set_tuning(b"demod_wide", 1), "tune")


def _check_all(f_mod, R, nbuf, nd, native, rows_native, snr_db, n, int_fold):
    x16, x64 = record(f_mod, n, snr_db)
    a16, a64 = x16[: nbuf * R], x64[: nbuf * R]
    rc16, o16, k16 = demod(a16, nbuf, R, nd, f_mod)
    rc64, o64, k64 = demod(a64, nbuf, R, nd, f_mod)
    assert rc16 == rc64 == 0
    np.testing.assert_array_equal(o16[0], o64[0])
    np.testing.assert_array_equal(o16[1], o64[1])
    check_tags(k16, k64, native, int_fold)
    rr16, r16, kr16 = demod(a16, nbuf, R, nd, f_mod, rows=True)
    rr64, r64, kr64 = demod(a64, nbuf, R, nd, f_mod, rows=True)
    assert rr16 == rr64 and rr64 in (0, -4)  # the row layout exists for the bin kernel's geometry only
    if rr64 == 0:
        np.testing.assert_array_equal(r16[0], r64[0])
        check_tags(kr16, kr64, rows_native, int_fold)
    c16, ok16, kf16 = fit(a16.view(1, -1), R, nbuf, nd, f_mod)
    c64, ok64, kf64 = fit(a64.view(1, -1), R, nbuf, nd, f_mod)
    np.testing.assert_array_equal(c16, c64)
    np.testing.assert_array_equal(ok16, ok64)
    check_tags(kf16, kf64, native, int_fold)
    return dict(demod=(k16, k64), rows=(kr16, kr64), fit=(kf16, kf64), cols=c16, ok=ok16)


def test_the_fits_converge_in_count_units():
    """The comparisons below are between fits that found the signal: amplitude ~ 4096 counts and
    m ~ 6 in every buffer. fitok compares ssq (here in counts^2) with the reference's absolute
    FITOK_THRESHOLD: 2 at the default 1e-3, 0 once the caller states the threshold in counts^2
    too — either way the float64 fit of the same counts says the same."""
    from deepfmkit_amd import fit as F
    x16, x64 = record()
    a16, a64 = x16[: 64 * 2000].view(1, -1), x64[: 64 * 2000].view(1, -1)
    cols, ok, _ = fit(a16, 2000, 64, 10)
    assert np.all(np.abs(cols[0] / SCALE - 1.0) < 0.05) and np.all(np.abs(cols[1] - 6.0) < 0.05)
    assert np.all(np.abs(cols[4] / SCALE - 1.0) < 0.3)  # dc in counts: 1 + J0(6) cos(phi), |J0(6)| = 0.15
    assert (ok == 2).all()
    old = F.FITOK_THRESHOLD
    F.FITOK_THRESHOLD = old * SCALE ** 2
    try:
        c16, ok16, _ = fit(a16, 2000, 64, 10)
        c64, ok64, _ = fit(a64, 2000, 64, 10)
    finally:
        F.FITOK_THRESHOLD = old
    assert (ok16 == 0).all()
    np.testing.assert_array_equal(c16, c64)
    np.testing.assert_array_equal(ok16, ok64)


# (1) bin / fused kernel: f_mod 1 kHz (L = 200). R = 200: fewer chunks than the prefetch depth
# and a 72-sample tail; R = 2000: prefetch, one full load group, a remainder group and an
# 80-sample tail; more segments than resident waves (grid-stride loop + next-segment prefetch).
@pytest.mark.parametrize("R,nbuf,nd", [(200, 12289, 10), (1000, 12289, 10), (2000, 8193, 10), (4000, 4097, 10),
                                       (2000, 8193, 16)])
def test_bins_and_fused_kernels(R, nbuf, nd, i16_int):
    # from 13 harmonics the many-harmonic kernel goes first by default (test_many_harmonic_kernel):
    # off here, so that ndata 16 reaches the <.., 16> bin instantiations
    k = check_all(1000.0, R, nbuf, nd, native=True, demod_wide=0 if nd == 16 else 1, int_fold=i16_int)
    tag = "[i16 int]" if i16_int else "[i16]"
    for pair in k["demod"], k["rows"], k["fit"]:
        assert "widened" not in pair[0], pair
    assert k["rows"][0].startswith("demod_bins_kernel<2,") and k["rows"][0].endswith(tag), k["rows"]
    if R == 4000:
        assert k["fit"][0].startswith("demod_seed_bins_kernel<2,12,4,10>") and k["fit"][0].endswith(tag), k["fit"]
        assert k["fit"][1] == "demod_seed_bins_kernel<2,12,4,10> (prefetch 4)", k["fit"]
    if nd == 16:
        assert k["fit"][0].startswith("demod_seed_bins_kernel<2,16,0,8>"), k["fit"]


# (2) many-harmonic kernel; 4,097 segments: the last wave's segment group is partial
@pytest.mark.parametrize("nd", [30, 62])
@pytest.mark.parametrize("R", [2000, 4000])
def test_many_harmonic_kernel(nd, R):
    k = check_all(1000.0, R, 4097, nd, native=True, rows_native=None)
    want = "demod_wide_kernel<1,8,10,4,0>" if nd == 30 else "demod_wide_kernel<2,8,10,4,0>"
    for pair in k["demod"], k["fit"]:
        assert pair[0] == want + " [i16]" and pair[1] == want, pair


# (3) other periods, 2,049 buffers: L = 256 (the two-slot boundary); L = 400 at ndata 3 and
# L = 1000 at ndata 2 (the 4- and 8-slot bin instantiations); L = 400 / 1000 at ndata 10 (their
# LDS basis exceeds the bin kernels' 64 KB) and L = 100 (below the bin geometry): the fold
# kernel, i.e. the widening fallback.
@pytest.mark.parametrize("f_mod,L,R,nd", [(781.25, 256, 2560, 10), (500.0, 400, 4000, 3), (200.0, 1000, 5000, 2)])
def test_other_periods_native(f_mod, L, R, nd, i16_int):
    from deepfmkit_amd import _lib
    assert _lib.load().dfmi_detect_period(w0_of(f_mod), R, nd) == L
    k = check_all(f_mod, R, 2049, nd, native=True, n=2049 * R, int_fold=i16_int)
    slots = 2 if L <= 256 else 4 if L <= 512 else 8
    assert k["fit"][0].startswith(f"demod_seed_bins_kernel<{slots},12,"), k["fit"]


@pytest.mark.parametrize("f_mod,L,R,nd", [(500.0, 400, 4000, 10), (200.0, 1000, 5000, 10), (2000.0, 100, 1000, 10)])
def test_other_periods_widened(f_mod, L, R, nd):
    from deepfmkit_amd import _lib
    assert _lib.load().dfmi_detect_period(w0_of(f_mod), R, nd) == L
    k = check_all(f_mod, R, 2049, nd, native=False, n=2049 * R)
    assert k["demod"][0].startswith("demod_fold_kernel") and k["demod"][0].endswith("[i16 widened]"), k["demod"]


# (4) two records: contiguous (the fused launch), rec_stride = nbuf R + 2 (unfused: seed kernel
# beside the bulk demodulation), rec_stride = nbuf R + 1 (record 1's rows lose their pair
# alignment: fold kernel on the widened rows, as the float64 record of that layout)
@pytest.mark.parametrize("pad", [0, 2, 1])
def test_two_records(pad, i16_int):
    import torch
    R, nbuf, nd = 2000, 2049, 10
    x16, x64 = record()
    res = {}
    for x in (x16, x64):
        stride = nbuf * R + pad
        buf = torch.zeros(2 * stride, dtype=x.dtype, device="cuda")
        recs = buf.as_strided((2, nbuf * R), (stride, 1))
        recs.copy_(x[: 2 * nbuf * R].view(2, nbuf * R))
        res[x.dtype] = fit(recs, R, nbuf, nd)
    (c16, ok16, k16), (c64, ok64, k64) = res[torch.int16], res[torch.float64]
    np.testing.assert_array_equal(c16, c64)
    np.testing.assert_array_equal(ok16, ok64)
    check_tags(k16, k64, native=pad != 1, int_fold=i16_int)
    assert k64.startswith("demod_seed_bins_kernel") == (pad == 0), k64
    if pad == 1:
        assert k16.startswith("demod_fold_kernel<1,"), k16


# (5) alignment: the view x16[1:] is 2-byte aligned only (no 4-byte pair load: the fallback);
# x16[2:] is 4-byte but not 8-byte aligned and stays native
@pytest.mark.parametrize("off,native", [(1, False), (2, True)])
def test_base_alignment(off, native, i16_int):
    R, nbuf, nd = 2000, 513, 10
    x16, x64 = record()
    assert x16[off:].data_ptr() % 8 == 2 * off
    c16, ok16, k16 = fit(x16[off: off + nbuf * R].view(1, -1), R, nbuf, nd)
    c64, ok64, k64 = fit(x64[off: off + nbuf * R].view(1, -1), R, nbuf, nd)
    np.testing.assert_array_equal(c16, c64)
    np.testing.assert_array_equal(ok16, ok64)
    check_tags(k16, k64, native=native, int_fold=i16_int)
    r16, o16, kd16 = demod(x16[off: off + nbuf * R], nbuf, R, nd, 1000.0)
    r64, o64, kd64 = demod(x64[off: off + nbuf * R], nbuf, R, nd, 1000.0)
    assert r16 == r64 == 0
    np.testing.assert_array_equal(o16[0], o64[0])
    np.testing.assert_array_equal(o16[1], o64[1])
    check_tags(kd16, kd64, native=native, int_fold=i16_int)


# (6) full scale: the record holds -32768 and 32767, its buffers 0 and 1 are constant -32768 and
# constant 32767 (sign extension of both halves of the pair load, the largest bin magnitudes)
def test_full_scale(i16_int):
    R, nbuf, nd = 2000, 513, 10
    x16, _ = record()
    a16 = x16[: nbuf * R].clone()
    a16[:R] = -32768
    a16[R: 2 * R] = 32767
    a16[2 * R] = -32768  # and both extremes beside ordinary samples, in either half of a pair
    a16[2 * R + 1] = 32767
    a16[3 * R] = 32767
    a16[3 * R + 1] = -32768
    a64 = a16.double()
    assert int(a16.min()) == -32768 and int(a16.max()) == 32767
    for rows in (False, True):
        r16, o16, k16 = demod(a16, nbuf, R, nd, 1000.0, rows=rows)
        r64, o64, k64 = demod(a64, nbuf, R, nd, 1000.0, rows=rows)
        assert r16 == r64 == 0
        for u, v in zip(o16, o64):
            np.testing.assert_array_equal(u, v)
        check_tags(k16, k64, native=True, int_fold=i16_int)
    dc = demod(a16, nbuf, R, nd, 1000.0)[1][1]
    assert dc[0] == -32768.0 and dc[1] == 32767.0
    c16, ok16, kf16 = fit(a16.view(1, -1), R, nbuf, nd)
    c64, ok64, kf64 = fit(a64.view(1, -1), R, nbuf, nd)
    np.testing.assert_array_equal(c16, c64)
    np.testing.assert_array_equal(ok16, ok64)
    check_tags(kf16, kf64, native=True, int_fold=i16_int)


# (7) warm-start chains (component-major QI): one chain, and np.array_split into 3
def _warm_start(nd, kw, int_fold=1):
    R, nbuf = 2000, 257
    x16, x64 = record()
    c16, ok16, k16 = fit(x16[: nbuf * R].view(1, -1), R, nbuf, nd, **kw)
    c64, ok64, k64 = fit(x64[: nbuf * R].view(1, -1), R, nbuf, nd, **kw)
    np.testing.assert_array_equal(c16, c64)
    np.testing.assert_array_equal(ok16, ok64)
    check_tags(k16, k64, native=True, int_fold=int_fold)
    return k64


@pytest.mark.parametrize("kw", [dict(parallel=False), dict(n_cores=3)], ids=["sequential", "n_cores3"])
def test_warm_start_chains_bin_kernel(kw, i16_int):
    assert _warm_start(10, kw, i16_int).startswith("demod_bins_kernel")


@pytest.mark.parametrize("kw", [dict(parallel=False), dict(n_cores=3)], ids=["sequential", "n_cores3"])
def test_warm_start_chains_many_harmonics(kw):
    assert _warm_start(30, kw).startswith("demod_wide_kernel")


# (8) host input: int16 numpy arrays (staged and copied as int16) == the device-resident fit
def _host_input(R, nbuf, nd, tag):
    x16, _ = record()
    a = x16[: nbuf * R]
    cd, okd, kd = fit(a.view(1, -1), R, nbuf, nd)
    h = a.cpu().numpy()
    assert h.dtype == np.int16
    ch, okh, kh = fit(h.reshape(1, -1), R, nbuf, nd)  # a 2-D array
    assert isinstance(ch, np.ndarray)
    np.testing.assert_array_equal(ch, cd)
    np.testing.assert_array_equal(okh, okd)
    assert kh == kd and kh.endswith(tag), (kh, kd)
    half = (nbuf // 2) * R
    two = fit([h[:half], h[half: 2 * half]], R, nbuf // 2, nd)  # a list of 1-D records
    assert two[2].endswith(tag), two[2]
    one = fit(a[: 2 * half].view(2, half), R, nbuf // 2, nd)
    np.testing.assert_array_equal(two[0], one[0])
    np.testing.assert_array_equal(two[1], one[1])
    mixed = fit([h[:half], h[half: 2 * half].astype(np.float64)], R, nbuf // 2, nd)  # not all int16: float64
    assert "[" not in mixed[2]
    np.testing.assert_array_equal(mixed[0], one[0])


def test_host_int16_input(i16_int):
    _host_input(2000, 8193, 10, "[i16 int]" if i16_int else "[i16]")


def test_host_int16_input_many_harmonics():
    _host_input(2000, 4097, 30, "[i16]")


# (9) noise-dominated record (-10 dB, clamped by the quantiser): status 1 / 2 and the m-grid retry
def test_noise_dominated_record(i16_int):
    k = check_all(1000.0, 2000, 513, 10, native=True, snr_db=-10.0, n=513 * 2000, int_fold=i16_int)
    assert (k["ok"] != 0).any()
    x16, _ = record(1000.0, 513 * 2000, -10.0)
    assert int(x16.min()) == -32768 and int(x16.max()) == 32767  # the quantiser clamped


def _raw(data, label="ch"):
    from deepfmkit_amd.data import DeepRawObject
    raw = DeepRawObject(data=data)
    raw.label, raw.f_samp, raw.f_mod, raw.t0 = label, F_SAMP, 1000, 0
    return raw


# (10) the facade
def test_facade_fit_on_int16_device_tensor(i16_int):
    import pandas as pd
    import deepfmkit_amd as dfm
    x16, x64 = record()
    dff = dfm.DeepFitFramework()
    dff.raws["a"] = _raw(x16[: 40 * 4000], "a")
    dff.raws["b"] = _raw(x64[: 40 * 4000], "b")
    fa = dff.fit("a", n=20, fit_label="fa", init_a=GUESS[0])
    fb = dff.fit("b", n=20, fit_label="fb", init_a=GUESS[0])
    pd.testing.assert_frame_equal(dff.fits_df["fa"], dff.fits_df["fb"], check_exact=True)
    for k in ("amp", "m", "phi", "psi", "dc", "ssq", "tau"):
        np.testing.assert_array_equal(np.asarray(getattr(fa, k)), np.asarray(getattr(fb, k)))
    assert len(dff.fits_df["fa"]) == 40


def test_facade_other_methods_treat_int16_as_float32_device_tensors():
    """Only method 'nls' reads a narrow device tensor; every other method does with an int16
    one what it does with a float32 one (the EKF's host path cannot take a device tensor)."""
    import deepfmkit_amd as dfm
    x16, _ = record()
    dff = dfm.DeepFitFramework()
    dff.raws["i"] = _raw(x16[: 4 * 4000], "i")
    dff.raws["f"] = _raw(x16[: 4 * 4000].float(), "f")
    ends = {}
    for label in ("f", "i"):
        try:
            ends[label] = ("returned", type(dff.fit(label, method="ekf", n=20)))
        except Exception as e:  # noqa: BLE001 - whatever float32 raises is the expectation
            ends[label] = ("raised", type(e))
    assert ends["i"] == ends["f"], ends


def test_facade_load_raw_int16(tmp_path):
    import pandas as pd
    import torch
    import deepfmkit_amd as dfm
    from deepfmkit_amd import textio
    x16, _ = record()
    path = str(tmp_path / "raw_data.txt")
    src = x16[: 5 * 4000].cpu().numpy()
    src[:2] = (-32768, 32767)
    textio.write_raw(path, [src.astype(np.float64)], t0=20250101, f_samp=F_SAMP, f_mod=1000.0)
    dff = dfm.DeepFitFramework()
    dff.load_raw(path, labels=["i16"], device="cuda:0", dtype="int16")
    x = dff.raws["i16"].samples()
    assert x.dtype == torch.int16 and x.is_cuda
    assert torch.equal(x.cpu(), torch.from_numpy(src))
    dff.raws["wide"] = _raw(x.double(), "wide")
    dff.fit("i16", n=20, fit_label="i", init_a=GUESS[0])
    dff.fit("wide", n=20, fit_label="w", init_a=GUESS[0])
    pd.testing.assert_frame_equal(dff.fits_df["i"], dff.fits_df["w"], check_exact=True)
    for k, bad in enumerate((0.5, 32768.0, -32769.0)):
        p2 = str(tmp_path / f"raw_bad{k}.txt")
        vals = src.astype(np.float64)
        vals[7] = bad
        textio.write_raw(p2, [vals], t0=20250101, f_samp=F_SAMP, f_mod=1000.0)
        with pytest.raises(ValueError, match="sample 7"):
            dfm.DeepFitFramework().load_raw(p2, device="cuda:0", dtype="int16")


def test_record_devices_shards_keep_int16():
    """nls_record_devices allocates its per-device shards in the record's dtype: an int16
    record (device tensor or numpy array), split over two shards of one GPU, gives the single
    call's result and reads int16 natively in every shard."""
    from deepfmkit_amd import _lib
    from deepfmkit_amd.fitters import nls_record_devices
    R, nbuf, nd = 2000, 257, 10
    x16, x64 = record()
    want, ok_want, _ = fit(x64[: nbuf * R].view(1, -1), R, nbuf, nd)
    for x in (x16[: nbuf * R], x16[: nbuf * R].cpu().numpy()):
        cols, ok = nls_record_devices(x, F_SAMP, 1000.0, R, nbuf, [0, 0], nd, init_guess=GUESS)
        assert _lib.load().dfmi_last_demod_kernel().decode().endswith("[i16 int]")
        np.testing.assert_array_equal(cols, want)
        np.testing.assert_array_equal(ok, ok_want)


# (11) one tie to the reference
def test_int16_fit_matches_numpy_oracle():
    """Shape (1) at R = 2000, 64 buffers; the int16 fit against the numpy oracle (_fit_parallel,
    every buffer its own chunk seeded by buffer 0) run on x16.astype(float64) from the same seed
    amplitude, under the parity bounds of tests/test_gpu_parity.py."""
    from oracle import nls_oracle as O
    R, nbuf, nd = 2000, 64, 10
    x16, _ = record()
    a = x16[: nbuf * R]
    cols, ok, kern = fit(a.view(1, -1), R, nbuf, nd)
    assert kern.endswith("[i16 int]")
    bufs = a.cpu().numpy().astype(np.float64).reshape(nbuf, R)
    first = O.fit_chunk((bufs[:1], list(GUESS), nd, 1000.0, F_SAMP, dict(O.C0)))
    rest = [O.fit_chunk((bufs[b:b + 1], first[0, :4], nd, 1000.0, F_SAMP, dict(O.C0)))[0] for b in range(1, nbuf)]
    ref = np.concatenate([first, np.array(rest)])
    names = ("amp", "m", "phi", "psi", "dc", "ssq", "fitok")
    refd = {k: ref[:, i] for i, k in enumerate(names)}
    ours = {k: cols[i] for i, k in enumerate(names[:6])}
    ours["fitok"] = ok
    qi = np.array([O.demod_buffer(bufs[b], nd, w0_of(1000.0)) for b in range(nbuf)])
    compare_fit(ours, refd, tol=record_tol(nd, qi, refd))


# (12) the overflow guard of the integer fold: L = 128, constant -32768, one segment of
# 65535 cycles (the largest bin magnitude an int32 holds: 65535 * 32768 = 2^31 - 32768; integer
# fold) and one of 65536 cycles (2^31: the LDS-bin fold, seen in the kernel string)
@pytest.mark.parametrize("ncyc,int_fold", [(65535, True), (65536, False)])
def test_integer_fold_overflow_guard(ncyc, int_fold):
    import torch
    L, nd, f_mod = 128, 10, F_SAMP / 128
    R = ncyc * L
    from deepfmkit_amd import _lib
    assert _lib.load().dfmi_detect_period(w0_of(f_mod), R, nd) == L
    a16 = torch.full((R,), -32768, dtype=torch.int16, device="cuda")
    a64 = a16.double()
    for rows in (False, True):
        r16, o16, k16 = demod(a16, 1, R, nd, f_mod, rows=rows)
        r64, o64, k64 = demod(a64, 1, R, nd, f_mod, rows=rows)
        assert r16 == r64 == 0
        for u, v in zip(o16, o64):
            np.testing.assert_array_equal(u, v)
        assert k64.startswith("demod_bins_kernel<2,"), k64
        assert k16 == k64 + (" [i16 int]" if int_fold else " [i16]"), (k16, k64)
    assert demod(a16, 1, R, nd, f_mod)[1][1][0] == -32768.0
