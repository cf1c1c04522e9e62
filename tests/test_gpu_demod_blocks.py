"""demod_blocks_kernel: demodulation of records whose modulation period is not a whole (or not a
short) sample count — the kernel demod_device selects when dfmi_detect_period finds no period.

Reference: numpy float64 as the reference forms it, mean(x cos(((h+1) w0) t)), mean(x sin(...)),
mean(x). Gates (test_gpu_parity.py's): |dQI| <= 1e-12 max|x|, dc relative <= 1e-13; the block algebra
stays within 1.9e-14 of the formula up to ndata 62, a mapping error shows at 1e-3 and above."""
import functools
import types

import numpy as np
import pytest

from conftest import compare_fit, record_tol

pytestmark = pytest.mark.gpu

# (f_samp, f_mod, n) -> R = int(f_samp / f_mod * n): shorter than a block; odd, 2 blocks + a tail;
# 4 and 5 row tiles; periodic with L = 2000 > 1024
SHAPES = [(200e3, 3500.7, 1, 57), (200e3, 1100.3, 1, 181), (200e3, 1234.5, 20, 3240), (200e3, 997.0, 20, 4012),
          (250e3, 1000.7, 20, 4996), (200e3, 100.0, 2, 4000)]
NSEG_MAX = 1027


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def w0_of(f_samp, f_mod):
    from deepfmkit_amd.fitters import w0_of as w
    return w(f_mod, f_samp)


@functools.lru_cache(maxsize=None)
def signal(f_samp, f_mod, R, nseg=NSEG_MAX, m=6.0, psi=0.3):
    """(nseg, R): 1.0 + 1.6 cos(phi_s + m cos(w0 t + psi)) + 0.016 Gaussian noise."""
    rng = np.random.default_rng(R)
    t = np.arange(nseg * R, dtype=np.float64).reshape(nseg, R)
    phi = 1.0 + 0.37 * np.arange(nseg)[:, None]
    x = 1.0 + 1.6 * np.cos(phi + m * np.cos(w0_of(f_samp, f_mod) * t + psi)) + 0.016 * rng.standard_normal((nseg, R))
    x.setflags(write=False)
    return x


def reference(x, nd, w0):
    t = np.arange(x.shape[1], dtype=np.float64)
    ang = ((np.arange(nd, dtype=np.float64) + 1.0) * w0)[:, None] * t[None, :]
    return x @ np.concatenate([np.cos(ang), np.sin(ang)]).T / x.shape[1], x.mean(axis=1)


def demod(xd, nseg, stride, R, nd, w0):
    """dfmi_demod / dfmi_demod_typed on a device tensor -> (QI (nseg, 2 nd), dc, kernel string)."""
    import torch
    from deepfmkit_amd import _lib
    from deepfmkit_amd.fitters import _xtype
    lib = _lib.load()
    qi = torch.full((2 * nd, nseg), float("nan"), dtype=torch.float64, device="cuda")
    dc = torch.full((nseg,), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.dfmi_demod_typed(xd.data_ptr(), _xtype(xd.dtype), nseg, stride, R, nd, w0, 0, qi.data_ptr(),
                                    dc.data_ptr(), _lib.DFMI_MEM_DEVICE, st), "dfmi_demod_typed")
    torch.cuda.synchronize()
    return qi.cpu().numpy().T, dc.cpu().numpy(), lib.dfmi_last_demod_kernel().decode()


def check(x, got, nd, w0):
    qi, dc, kern = got
    assert kern.startswith("demod_blocks_kernel"), kern
    rqi, rdc = reference(x, nd, w0)
    err, derr = np.abs(qi - rqi).max(), (np.abs(dc - rdc) / np.abs(rdc)).max()
    print(kern, x.shape, nd, "max|dQI| / max|x| = %.3g, dc rel = %.3g" % (err / np.abs(x).max(), derr))
    assert err <= 1e-12 * np.abs(x).max(), err
    assert derr <= 1e-13, derr


@pytest.mark.parametrize("nseg", [1, 5, NSEG_MAX])
@pytest.mark.parametrize("nd", [1, 7, 8, 10, 16, 30, 62])
@pytest.mark.parametrize("f_samp,f_mod,n,R", SHAPES)
def test_matches_reference_formula(f_samp, f_mod, n, R, nd, nseg):
    import torch
    from deepfmkit_amd import _lib
    w0 = w0_of(f_samp, f_mod)
    assert R == int(f_samp / f_mod * n) and _lib.load().dfmi_detect_period(w0, R, nd) == 0
    x = signal(f_samp, f_mod, R)[:nseg]
    check(x, demod(torch.from_numpy(x).cuda(), nseg, R, R, nd, w0), nd, w0)


@pytest.mark.parametrize("layout", ["stride", "offset"])
@pytest.mark.parametrize("dtype", ["float64", "float32", "int16"])
def test_unaligned_segments(layout, dtype):
    """seg_stride = R + 3; a base pointer one sample past an aligned one."""
    import torch
    f_samp, f_mod, _, R = SHAPES[3]
    nd, nseg, w0 = 10, 37, w0_of(f_samp, f_mod)
    x = signal(f_samp, f_mod, R)[:nseg]
    if dtype == "int16":
        x = np.round(2000.0 * x)
    x = x.astype(dtype).astype(np.float64)
    stride = R + 3 if layout == "stride" else R
    buf = torch.zeros(1 + nseg * stride, dtype=getattr(torch, dtype), device="cuda")
    view = buf[1:] if layout == "offset" else buf
    view[: nseg * stride].view(nseg, stride)[:, :R] = torch.from_numpy(x).cuda().to(buf.dtype)
    check(x, demod(view, nseg, stride, R, nd, w0), nd, w0)


@pytest.mark.parametrize("nd", [10, 30])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]])
def test_sample_types_bit_identical(shape, nd):
    """float32 and int16 records give the bits of the float64 record of the same values."""
    import torch
    f_samp, f_mod, _, R = shape
    nseg, w0 = 261, w0_of(f_samp, f_mod)
    x = signal(f_samp, f_mod, R)[:nseg]
    for dtype, tag, vals in (("float32", "[f32]", x.astype(np.float32)),
                             ("int16", "[i16]", np.round(3000.0 + 20000.0 * (x - 1.0) / 1.7).astype(np.int16))):
        q64, d64, k64 = demod(torch.from_numpy(vals.astype(np.float64)).cuda(), nseg, R, R, nd, w0)
        qt, dt, kt = demod(torch.from_numpy(vals).cuda(), nseg, R, R, nd, w0)
        assert k64.startswith("demod_blocks_kernel") and "[" not in k64, k64
        assert kt.startswith("demod_blocks_kernel") and kt.endswith(tag) and "widened" not in kt, kt
        np.testing.assert_array_equal(qt, q64)
        np.testing.assert_array_equal(dt, d64)


@pytest.mark.parametrize("shape,nd", [(SHAPES[1], 10), (SHAPES[3], 30)])
def test_agrees_with_direct_kernel(shape, nd):
    """Tuning key demod_blocks = 0 restores the per-sample-sincos route; both agree within the gate."""
    import torch
    from deepfmkit_amd import _lib
    lib = _lib.load()
    f_samp, f_mod, _, R = shape
    nseg, w0 = 261, w0_of(f_samp, f_mod)
    x = signal(f_samp, f_mod, R)[:nseg]
    xd = torch.from_numpy(x).cuda()
    _lib.check(lib.dfmi_set_tuning(b"demod_blocks", 0), "tune")
    try:
        q0, d0, k0 = demod(xd, nseg, R, R, nd, w0)
    finally:
        _lib.check(lib.dfmi_set_tuning(b"demod_blocks", 1), "tune")
    assert k0 == "demod_direct_kernel", k0
    q1, d1, k1 = demod(xd, nseg, R, R, nd, w0)
    assert k1.startswith("demod_blocks_kernel") and np.abs(q1 - q0).max() <= 1e-12 * np.abs(x).max()
    assert (np.abs(d1 - d0) / np.abs(d0)).max() <= 1e-13


@pytest.mark.parametrize("f_mod,n,R,parallel", [(997.0, 5, 1003, True), (1234.5, 3, 486, True), (997.0, 5, 1003, False)])
def test_record_fit_matches_oracle(f_mod, n, R, parallel):
    """nls_records on 24 buffers (m = 6, phi = 1, psi = 0) against the numpy oracle."""
    import torch
    from deepfmkit_amd import _lib
    from deepfmkit_amd.fitters import nls_records
    from oracle import nls_oracle as O
    f_samp, nd, nbuf = 200e3, 10, 24
    rng = np.random.default_rng(nbuf)
    t = np.arange(nbuf * R, dtype=np.float64)
    x = 1.0 + 1.6 * np.cos(1.0 + 6.0 * np.cos(w0_of(f_samp, f_mod) * t)) + 0.016 * rng.standard_normal(nbuf * R)
    assert O.buffer_params(x.size, f_samp, f_mod, n)[0] == R
    cols, ok = nls_records(torch.from_numpy(x).cuda().view(1, -1), f_samp, f_mod, R, nbuf, nd, parallel=parallel)
    assert _lib.load().dfmi_last_demod_kernel().decode().startswith("demod_blocks_kernel")
    if parallel:
        ref = O.fit_record_parallel(x, f_samp, f_mod, n, ndata=nd, n_cores=nbuf - 1, pool=types.SimpleNamespace(imap=map))
    else:
        ref = O.fit_record_sequential(x, f_samp, f_mod, n, ndata=nd)
    names = ("amp", "m", "phi", "psi", "dc", "ssq")
    ours = dict(zip(names, cols.cpu().numpy()), fitok=ok.cpu().numpy())
    refd = dict(zip(names + ("fitok",), ref.T))
    assert (refd["fitok"] == 0).all()
    qi = np.array([O.demod_buffer(b, nd, w0_of(f_samp, f_mod)) for b in x.reshape(nbuf, R)])
    compare_fit(ours, refd, tol=record_tol(nd, qi, refd), min_status_match=1.0)


def test_facade_fit_on_997_hz_record():
    import deepfmkit_amd as dfm
    from deepfmkit_amd import _lib
    from deepfmkit_amd.data import DeepRawObject
    laser, ifo = dfm.LaserConfig(), dfm.InterferometerConfig()
    laser.f_mod = 997.0
    dfm.set_laser_df_for_effect(laser, ifo, 6.0)
    dff = dfm.DeepFitFramework()
    dff.load_sim(dfm.DFMIObject("lab", laser, ifo, f_samp=200000.0))
    dff.simulate("lab", n_seconds=0.25, mode="snr", snr_db=40.0, trial_num=2)
    raw = DeepRawObject(data=np.asarray(dff.raws["lab"].samples())[: 12 * 4012])  # a whole number of buffers
    raw.label, raw.f_samp, raw.f_mod, raw.t0 = "cut", 200000.0, 997.0, 0
    dff.raws["cut"] = raw
    fit = dff.fit("cut", n=20)
    assert _lib.load().dfmi_last_demod_kernel().decode().startswith("demod_blocks_kernel")
    assert fit.R == 4012 and np.isfinite(np.asarray(fit.m)).all()
