"""float32 sample records through the typed entry points (dfmi_*_typed, include/dfmi.h).

The contract: a float32 record gives, BIT FOR BIT, what the float64 path gives on the same
values (`x32.double()`, never the record before the cast) in the same layout — QI, dc, the
six result columns and fitok; there is no tolerance. float -> double is exact and the
kernels keep every phase bin's ascending-time order, so anything else is a load-path bug.
Records come from the package's snr-mode generator (f_samp 200 kHz, m = 6, 40 dB), cast to
float32 once per module."""
import numpy as np
import pytest

from conftest import compare_fit, record_tol

pytestmark = pytest.mark.gpu

F_SAMP = 200000.0
NMAX = 4097 * 4000  # the largest shape's samples (8193 x 2000, 12289 x 1000 and 12289 x 200 fit inside)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deepfmkit_amd import _lib
    assert _lib.load().dfmi_device_count() >= 1


_CACHE = {}


def record(f_mod=1000.0, n=NMAX, snr_db=40.0):
    """(x32, x64 = x32.double()) of the snr-mode record at f_mod, on the GPU, made once."""
    import torch
    from deepfmkit_amd.physics import SnrSpec, synth_snr
    key = (f_mod, n, snr_db)
    if key not in _CACHE:
        x = torch.empty(n, dtype=torch.float64, device="cuda")
        synth_snr(SnrSpec(seed=77, f_samp=F_SAMP, f_mod=f_mod, m=6.0, snr_db=snr_db), 0, n, out=x)
        x32 = x.float()
        assert not torch.equal(x32.double(), x)  # the cast rounds: the comparand is NOT the original
        _CACHE[key] = (x32, x32.double())
    return _CACHE[key]


def w0_of(f_mod):
    from deepfmkit_amd.fitters import w0_of as w
    return w(f_mod, F_SAMP)


def demod(x, nseg, R, nd, f_mod, rows=False):
    """dfmi_demod(_typed) / dfmi_demod_rows(_typed) on nseg contiguous segments of the device
    tensor x (float32 through the typed call, float64 through the untyped one) ->
    (return code, outputs as numpy, kernel string)."""
    import torch
    from deepfmkit_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    f32 = x.dtype == torch.float32
    D = _lib.DFMI_MEM_DEVICE
    if rows:
        out = [torch.zeros((nseg, lib.dfmi_qi_row_stride(nd)), dtype=torch.float64, device="cuda")]
        args = (nseg, R, R, nd, w0_of(f_mod), 0, out[0].data_ptr(), D, st)
        rc = (lib.dfmi_demod_rows_typed(x.data_ptr(), _lib.DFMI_F32, *args) if f32
              else lib.dfmi_demod_rows(x.data_ptr(), *args))
    else:
        out = [torch.zeros((2 * nd, nseg), dtype=torch.float64, device="cuda"),
               torch.zeros(nseg, dtype=torch.float64, device="cuda")]
        args = (nseg, R, R, nd, w0_of(f_mod), 0, out[0].data_ptr(), out[1].data_ptr(), D, st)
        rc = lib.dfmi_demod_typed(x.data_ptr(), _lib.DFMI_F32, *args) if f32 else lib.dfmi_demod(x.data_ptr(), *args)
    kern = lib.dfmi_last_demod_kernel().decode() if rc == 0 else ""
    torch.cuda.synchronize()
    return rc, [o.cpu().numpy() for o in out], kern


def fit(x, R, nbuf, nd, f_mod=1000.0, **kw):
    """nls_records on a (nrec, >= nbuf R) tensor / array -> (cols, fitok, kernel string)."""
    from deepfmkit_amd import _lib
    from deepfmkit_amd.fitters import nls_records
    cols, ok = nls_records(x, F_SAMP, f_mod, R, nbuf, nd, **kw)
    kern = _lib.load().dfmi_last_demod_kernel().decode()
    if hasattr(cols, "cpu"):
        cols, ok = cols.cpu().numpy(), ok.cpu().numpy()
    return cols, ok, kern


def check_tags(k32, k64, native=None):
    """The float64 string carries no tag; the float32 one is the same string + its tag."""
    assert "[" not in k64, k64
    if native is None:
        assert k32 in (k64 + " [f32]", k64 + " [f32 widened]"), (k32, k64)
    else:
        assert k32 == k64 + (" [f32]" if native else " [f32 widened]"), (k32, k64)


def check_all(f_mod, R, nbuf, nd, native=None, fit_native=None, rows_native=True, snr_db=40.0, n=NMAX,
              demod_wide=1):
    """QI + dc (component-major), the row layout and the whole record fit of the first nbuf
    buffers: float32 against float64 on the same values, bit for bit. native: whether the
    component-major / record-fit kernels must report a native float32 read (None: either).
    demod_wide = 0: the many-harmonic kernel does not go ahead of the bin kernels."""
    from deepfmkit_amd import _lib
    lib = _lib.load()
    _lib.check(lib.dfmi_set_tuning(b"demod_wide", demod_wide), "tune")
    try:
        return _check_all(f_mod, R, nbuf, nd, native, fit_native, rows_native, snr_db, n)
    finally:
        _lib.check(lib.dfmi_set_tuning(b"demod_wide", 1), "tune")


def _check_all(f_mod, R, nbuf, nd, native, fit_native, rows_native, snr_db, n):
    x32, x64 = record(f_mod, n, snr_db)
    a32, a64 = x32[: nbuf * R], x64[: nbuf * R]
    rc32, o32, k32 = demod(a32, nbuf, R, nd, f_mod)
    rc64, o64, k64 = demod(a64, nbuf, R, nd, f_mod)
    assert rc32 == rc64 == 0
    np.testing.assert_array_equal(o32[0], o64[0])
    np.testing.assert_array_equal(o32[1], o64[1])
    check_tags(k32, k64, native)
    rr32, r32, kr32 = demod(a32, nbuf, R, nd, f_mod, rows=True)
    rr64, r64, kr64 = demod(a64, nbuf, R, nd, f_mod, rows=True)
    assert rr32 == rr64 and rr64 in (0, -4)  # the row layout exists for the bin kernel's geometry only
    if rr64 == 0:
        np.testing.assert_array_equal(r32[0], r64[0])
        check_tags(kr32, kr64, rows_native)
    c32, ok32, kf32 = fit(a32.view(1, -1), R, nbuf, nd, f_mod)
    c64, ok64, kf64 = fit(a64.view(1, -1), R, nbuf, nd, f_mod)
    np.testing.assert_array_equal(c32, c64)
    np.testing.assert_array_equal(ok32, ok64)
    check_tags(kf32, kf64, native if fit_native is None else fit_native)
    return dict(demod=(k32, k64), rows=(kr32, kr64), fit=(kf32, kf64), cols=c32, ok=ok32)


# (1) bin / fused kernel: f_mod 1 kHz (L = 200). R = 200: fewer chunks than the prefetch depth
# and a 72-sample tail; R = 2000: prefetch, one full load group, a remainder group and an
# 80-sample tail; more segments than resident waves (grid-stride loop + next-segment prefetch).
@pytest.mark.parametrize("R,nbuf,nd", [(200, 12289, 10), (1000, 12289, 10), (2000, 8193, 10), (4000, 4097, 10),
                                       (2000, 8193, 16)])
def test_bins_and_fused_kernels(R, nbuf, nd):
    # from 13 harmonics the many-harmonic kernel goes first by default (test_many_harmonic_kernel):
    # off here, so that ndata 16 reaches the <.., 16> bin instantiations
    k = check_all(1000.0, R, nbuf, nd, native=True, demod_wide=0 if nd == 16 else 1)
    for pair in k["demod"], k["rows"], k["fit"]:
        assert "widened" not in pair[0], pair
    assert k["rows"][0].startswith("demod_bins_kernel<2,") and k["rows"][0].endswith("[f32]"), k["rows"]
    if R == 4000:
        assert k["fit"][0].startswith("demod_seed_bins_kernel<2,12,4,10>") and k["fit"][0].endswith("[f32]"), k["fit"]
        assert k["fit"][1] == "demod_seed_bins_kernel<2,12,4,10> (prefetch 4)", k["fit"]
    if nd == 16:
        assert k["fit"][0].startswith("demod_seed_bins_kernel<2,16,0,8>"), k["fit"]
        assert k["fit"][1] == "demod_seed_bins_kernel<2,16,0,8>", k["fit"]


# (2) many-harmonic kernel; 4,097 segments: the last wave's segment group is partial
@pytest.mark.parametrize("nd", [30, 62])
@pytest.mark.parametrize("R", [2000, 4000])
def test_many_harmonic_kernel(nd, R):
    k = check_all(1000.0, R, 4097, nd, native=True, rows_native=None)
    want = "demod_wide_kernel<1,8,10,4,0>" if nd == 30 else "demod_wide_kernel<2,8,10,4,0>"
    for pair in k["demod"], k["fit"]:
        assert pair[0].startswith("demod_wide_kernel") and pair[0].endswith("[f32]"), pair
        assert "widened" not in pair[0]
        assert pair[1] == want, pair


# (3) other periods, ndata 10, 2,049 buffers: L = 256 (the two-slot boundary), 400, 1000, and
# L = 100 (below the bin geometry: the fold kernel, i.e. the widening fallback). At ndata 10 the
# LDS basis of L = 400 / 1000 exceeds the bin kernels' 64 KB, so those run the fold kernel too;
# the 4- and 8-slot bin instantiations are reached at ndata 3 / 2 below.
@pytest.mark.parametrize("f_mod,L,R,nd,native", [(781.25, 256, 2560, 10, True), (500.0, 400, 4000, 10, False),
                                                 (200.0, 1000, 5000, 10, False), (2000.0, 100, 1000, 10, False),
                                                 (500.0, 400, 4000, 3, True), (200.0, 1000, 5000, 2, True)])
def test_other_periods(f_mod, L, R, nd, native):
    from deepfmkit_amd import _lib
    assert _lib.load().dfmi_detect_period(w0_of(f_mod), R, nd) == L
    k = check_all(f_mod, R, 2049, nd, native=native, n=2049 * R)
    if native:
        slots = 2 if L <= 256 else 4 if L <= 512 else 8
        assert k["fit"][0].startswith(f"demod_seed_bins_kernel<{slots},12,"), k["fit"]
    else:
        assert k["demod"][0].startswith("demod_fold_kernel") and k["demod"][0].endswith("[f32 widened]"), k["demod"]


# (4) several records: contiguous (the fused launch), rec_stride = nbuf R + 2 (unfused: seed
# kernel beside the bulk demodulation), rec_stride = nbuf R + 1 (record 1's rows lose their
# pair alignment: fold kernel on the widened rows, as the float64 record of that layout)
@pytest.mark.parametrize("pad", [0, 2, 1])
def test_several_records(pad):
    import torch
    R, nbuf, nd = 2000, 2049, 10
    x32, x64 = record()
    res = {}
    for x in (x32, x64):
        stride = nbuf * R + pad
        buf = torch.zeros(2 * stride, dtype=x.dtype, device="cuda")
        recs = buf.as_strided((2, nbuf * R), (stride, 1))
        recs.copy_(x[: 2 * nbuf * R].view(2, nbuf * R))
        res[x.dtype] = fit(recs, R, nbuf, nd)
    (c32, ok32, k32), (c64, ok64, k64) = res[torch.float32], res[torch.float64]
    np.testing.assert_array_equal(c32, c64)
    np.testing.assert_array_equal(ok32, ok64)
    check_tags(k32, k64, native=pad != 1)
    assert k64.startswith("demod_seed_bins_kernel") == (pad == 0), k64
    if pad == 1:
        assert k32.startswith("demod_fold_kernel<1,"), k32


# (5) a base that is 4-byte aligned only: the view x32[1:] against the same view of x32.double()
def test_misaligned_base():
    R, nbuf, nd = 2000, 513, 10
    x32, x64 = record()
    c32, ok32, k32 = fit(x32[1: 1 + nbuf * R].view(1, -1), R, nbuf, nd)
    c64, ok64, k64 = fit(x64[1: 1 + nbuf * R].view(1, -1), R, nbuf, nd)
    assert x32[1:].data_ptr() % 8 == 4
    np.testing.assert_array_equal(c32, c64)
    np.testing.assert_array_equal(ok32, ok64)
    check_tags(k32, k64, native=False)


# (6) warm-start chains (component-major QI): one chain, and np.array_split into 3
@pytest.mark.parametrize("nd", [10, 30])
@pytest.mark.parametrize("kw", [dict(parallel=False), dict(n_cores=3)], ids=["sequential", "n_cores3"])
def test_warm_start_chains(nd, kw):
    R, nbuf = 2000, 257
    x32, x64 = record()
    c32, ok32, k32 = fit(x32[: nbuf * R].view(1, -1), R, nbuf, nd, **kw)
    c64, ok64, k64 = fit(x64[: nbuf * R].view(1, -1), R, nbuf, nd, **kw)
    np.testing.assert_array_equal(c32, c64)
    np.testing.assert_array_equal(ok32, ok64)
    check_tags(k32, k64, native=True)


# (7) host input: float32 numpy arrays (staged and copied as float32) == the device-resident fit
@pytest.mark.parametrize("R,nbuf,nd", [(2000, 8193, 10), (4000, 4097, 10), (2000, 4097, 30)])
def test_host_float32_input(R, nbuf, nd):
    x32, _ = record()
    a = x32[: nbuf * R]
    cd, okd, kd = fit(a.view(1, -1), R, nbuf, nd)
    h = a.cpu().numpy()
    assert h.dtype == np.float32
    ch, okh, kh = fit(h.reshape(1, -1), R, nbuf, nd)
    assert isinstance(ch, np.ndarray)
    np.testing.assert_array_equal(ch, cd)
    np.testing.assert_array_equal(okh, okd)
    assert kh == kd and kh.endswith("[f32]")
    cl, okl, _ = fit([h], R, nbuf, nd)  # a list of 1-D records
    np.testing.assert_array_equal(cl, cd)
    np.testing.assert_array_equal(okl, okd)


def _raw(data, label="ch"):
    from deepfmkit_amd.data import DeepRawObject
    raw = DeepRawObject(data=data)
    raw.label, raw.f_samp, raw.f_mod, raw.t0 = label, F_SAMP, 1000, 0
    return raw


# (8) the facade
def test_facade_fit_on_float32_device_tensor():
    import pandas as pd
    import deepfmkit_amd as dfm
    x32, x64 = record()
    dff = dfm.DeepFitFramework()
    dff.raws["a"] = _raw(x32[: 40 * 4000], "a")
    dff.raws["b"] = _raw(x64[: 40 * 4000], "b")
    fa = dff.fit("a", n=20, fit_label="fa")
    fb = dff.fit("b", n=20, fit_label="fb")
    pd.testing.assert_frame_equal(dff.fits_df["fa"], dff.fits_df["fb"], check_exact=True)
    for k in ("amp", "m", "phi", "psi", "dc", "ssq", "tau"):
        np.testing.assert_array_equal(np.asarray(getattr(fa, k)), np.asarray(getattr(fb, k)))
    assert len(dff.fits_df["fa"]) == 40


def test_facade_load_raw_float32(tmp_path):
    import pandas as pd
    import torch
    import deepfmkit_amd as dfm
    from deepfmkit_amd import textio
    _, x64 = record()
    path = str(tmp_path / "raw_data.txt")
    src = (x64[: 5 * 4000] * 1.0000001).cpu().numpy()  # values that are not float32 numbers
    textio.write_raw(path, [src], t0=20250101, f_samp=F_SAMP, f_mod=1000.0)
    dff = dfm.DeepFitFramework()
    dff.load_raw(path, labels=["f32"], device="cuda:0", dtype="float32")
    x = dff.raws["f32"].samples()
    assert x.dtype == torch.float32 and x.is_cuda
    assert torch.equal(x.cpu(), torch.from_numpy(src.astype(np.float32)))  # parsed as float64, cast once
    dff.raws["wide"] = _raw(x.double(), "wide")
    dff.fit("f32", n=20, fit_label="f")
    dff.fit("wide", n=20, fit_label="w")
    pd.testing.assert_frame_equal(dff.fits_df["f"], dff.fits_df["w"], check_exact=True)
    with pytest.raises(ValueError):
        dfm.DeepFitFramework().load_raw(path, dtype="float32")  # only valid together with device
    host = dfm.DeepFitFramework()
    host.load_raw(path, labels=["h"])
    assert host.raws["h"].data["ch0"].dtype == np.float64  # the host frame stays float64


# (9) noise-dominated record: status 1 / 2 and the m-grid retry on float32-born QI
def test_noise_dominated_record():
    k = check_all(1000.0, 2000, 513, 10, native=True, snr_db=-10.0, n=513 * 2000)
    assert (k["ok"] != 0).any()


def test_other_dtypes_still_refused():
    import torch
    x32, _ = record()
    a = x32[: 8 * 4000]
    for bad in (a.half(), (a * 1000).to(torch.int32)):
        with pytest.raises(ValueError):
            fit(bad.view(1, -1), 4000, 8, 10)


def test_float32_fit_matches_numpy_oracle():
    """One tie to the reference: shape (1) at R = 2000, 64 buffers; the float32 fit against the
    numpy oracle (_fit_parallel, every buffer its own chunk seeded by buffer 0) run on
    x32.astype(float64), under the parity bounds of tests/test_gpu_parity.py."""
    from oracle import nls_oracle as O
    R, nbuf, nd = 2000, 64, 10
    x32, _ = record()
    a = x32[: nbuf * R]
    cols, ok, kern = fit(a.view(1, -1), R, nbuf, nd)
    assert kern.endswith("[f32]")
    bufs = a.cpu().numpy().astype(np.float64).reshape(nbuf, R)
    first = O.fit_chunk((bufs[:1], [1.6, 6.0, 0.0, 0.0], nd, 1000.0, F_SAMP, dict(O.C0)))
    rest = [O.fit_chunk((bufs[b:b + 1], first[0, :4], nd, 1000.0, F_SAMP, dict(O.C0)))[0] for b in range(1, nbuf)]
    ref = np.concatenate([first, np.array(rest)])
    names = ("amp", "m", "phi", "psi", "dc", "ssq", "fitok")
    refd = {k: ref[:, i] for i, k in enumerate(names)}
    ours = {k: cols[i] for i, k in enumerate(names[:6])}
    ours["fitok"] = ok
    qi = np.array([O.demod_buffer(bufs[b], nd, w0_of(1000.0)) for b in range(nbuf)])
    compare_fit(ours, refd, tol=record_tol(nd, qi, refd))


def test_record_devices_shards_keep_float32():
    """nls_record_devices allocates its per-device shards in the record's dtype: a float32
    record (device tensor or numpy array), split over two shards of one GPU, gives the single
    call's float32 result, i.e. the float64 one."""
    from deepfmkit_amd.fitters import nls_record_devices
    R, nbuf, nd = 2000, 257, 10
    x32, x64 = record()
    want, ok_want, _ = fit(x64[: nbuf * R].view(1, -1), R, nbuf, nd)
    for x in (x32[: nbuf * R], x32[: nbuf * R].cpu().numpy()):
        cols, ok = nls_record_devices(x, F_SAMP, 1000.0, R, nbuf, [0, 0], nd)
        np.testing.assert_array_equal(cols, want)
        np.testing.assert_array_equal(ok, ok_want)
