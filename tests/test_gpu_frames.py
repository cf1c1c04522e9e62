"""Frame-interleaved records, x[t, c] (dfmi_demod_frames, dfmi_nls_record_frames, nls_frames).

The contract is bit identity: QI, dc, the six result columns and fitok equal, with no tolerance,
what the planar typed call gives on `frames.T.contiguous()`. Every case runs at the tuning key
demod_frames = 1 and 0 and checks through dfmi_last_demod_kernel() which path ran: the native
kernel (int16 frames of 2 / 4 / 8 channels, no padding, R even, base aligned to min(4 nch, 16)
bytes, and the planar call itself on the integer bin fold) or the copy (" [frames copied]").
test_default_tuning runs the routing users get; the short shapes, which that routing sends through
demod_wide_kernel (other last bits), take `bins` (demod_wide = 0): bin kernel and native kernel.
Frames: the package's snr generator, one spec per channel (m, phi, amplitude all differ, so a
channel mix-up cannot pass), quantised as clamp(round(4096 x)); `extremes` forces samples of
every channel to -32768 and 32767 in the first cycle, a middle one and the tail."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F_SAMP, SCALE = 200000.0, 4096.0
_CACHE = {}


def _tuned(key, value, default):
    from deepfmkit_amd import _lib
    _lib.check(_lib.load().dfmi_set_tuning(key, value), "tune")
    yield value
    _lib.check(_lib.load().dfmi_set_tuning(key, default), "tune")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not pytest.importorskip("torch").cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture
def bins():
    yield from _tuned(b"demod_wide", 0, 1)


@pytest.fixture(params=[1, 0], ids=["native", "copied"])
def path(request):
    yield from _tuned(b"demod_frames", request.param, 1)


def frames(nch, L, n, extremes=False):
    """(n, nch) int16 frames on the GPU, made once per shape."""
    import torch
    from deepfmkit_amd.physics import SnrSpec, synth_snr
    key = (nch, L, n, extremes)
    if key not in _CACHE:
        fr = torch.empty((n, nch), dtype=torch.int16, device="cuda")
        x = torch.empty(n, dtype=torch.float64, device="cuda")
        for c in range(nch):
            synth_snr(SnrSpec(seed=100 + c, f_samp=F_SAMP, f_mod=F_SAMP / L, amp=0.7 + 0.1 * c, m=5.0 + 0.3 * c,
                              phi=0.4 * c, snr_db=40.0), 0, n, out=x)
            fr[:, c] = torch.clamp(torch.round(SCALE * x), -32768, 32767).to(torch.int16)
            for t in (c, L + 2 * c + 1, n - 1 - c) if extremes else ():  # both parities
                fr[t, c], fr[(t + 64) % n, c] = -32768, 32767
        _CACHE[key] = fr
    return _CACHE[key]


def guess(nch):
    return np.array([[(0.7 + 0.1 * c) * SCALE, 6.0, 0.0, 0.0] for c in range(nch)])


def demod(x, nch, nbuf, R, nd, L, frames_call):
    """dfmi_demod_frames on (N, nch) frames / dfmi_demod_typed on (nch, N) records -> (qi, dc, kernel)."""
    import torch
    from deepfmkit_amd import _lib
    from deepfmkit_amd.fitters import _xtype, w0_of
    lib, dev, nseg = _lib.load(), hasattr(x, "is_cuda"), nch * nbuf
    qi, dc = np.zeros((2 * nd, nseg)), np.zeros(nseg)
    if dev:
        qi, dc = torch.from_numpy(qi).cuda(), torch.from_numpy(dc).cuda()
    tail = (R, nd, w0_of(F_SAMP / L, F_SAMP), 0, _lib.ptr(qi), _lib.ptr(dc), 1 if dev else 0,
            torch.cuda.current_stream().cuda_stream if dev else None)
    stride = x.stride(0) if dev else x.strides[0] // x.itemsize
    if frames_call:
        rc = lib.dfmi_demod_frames(_lib.ptr(x), _xtype(x.dtype), nch, stride, nbuf, *tail)
    else:
        assert stride == nbuf * R
        rc = lib.dfmi_demod_typed(_lib.ptr(x), _xtype(x.dtype), nseg, R, *tail)
    assert rc == 0, lib.dfmi_last_error()
    kern = lib.dfmi_last_demod_kernel().decode()
    return (qi.cpu().numpy(), dc.cpu().numpy(), kern) if dev else (qi, dc, kern)


def fit(x, nch, nbuf, R, nd, L, frames_call, **kw):
    from deepfmkit_amd import _lib
    from deepfmkit_amd.fitters import nls_frames, nls_records
    res = (nls_frames if frames_call else nls_records)(x, F_SAMP, F_SAMP / L, R, nbuf, nd, init_guess=guess(nch), **kw)
    return [r.cpu().numpy() if hasattr(r, "cpu") else r for r in res], _lib.load().dfmi_last_demod_kernel().decode()


def check(fr, nbuf, R, nd, L, native, record=True, behind="", **kw):
    """Frames call == planar call on fr.T.contiguous(), bit for bit, on the expected path (copied:
    the planar call's own string, which starts with `behind`, + " [frames copied]")."""
    nch = fr.shape[1]
    fr = fr[: nbuf * R]
    pl = fr.T.contiguous() if hasattr(fr, "is_cuda") else np.ascontiguousarray(fr.T)
    got, want = demod(fr, nch, nbuf, R, nd, L, True), demod(pl, nch, nbuf, R, nd, L, False)
    pairs = [(got[:2], want[:2], got[2], want[2])]
    if record:
        (gc, gk), (wc, wk) = fit(fr, nch, nbuf, R, nd, L, True, **kw), fit(pl, nch, nbuf, R, nd, L, False, **kw)
        pairs.append((gc, wc, gk, wk))
    for g, w, kern, planar in pairs:
        for a, b in zip(g, w):
            np.testing.assert_array_equal(a, b)
        if native:
            assert kern.startswith("demod_frames_kernel<") and kern.endswith(f"[i16 int, {nch} ch]"), kern
        else:
            assert kern == planar + " [frames copied]" and kern.startswith(behind), (kern, planar)
    return got


@pytest.mark.parametrize("R,nd,native,behind", [(400, 10, False, "demod_wide_kernel"), (2000, 10, True, ""),
                                                (2000, 16, False, "demod_wide_kernel")])
def test_default_tuning(R, nd, native, behind, path):
    """The routing a user gets: where the planar call runs demod_wide_kernel (R < 2000 or ndata >= 13)
    the frames are copied and take it too; otherwise the native kernel."""
    check(frames(4, 200, 9 * R), 9, R, nd, 200, native=bool(path) and native, behind=behind)


# L = 200: two slots, the second partly masked; L = 128: one full slot (with the extremes). R = 2L: fewer
# cycles than a load group after the prefetch; 5L: prefetch + groups; 3L + 37: odd, so the buffers lose
# the wide loads' alignment (and the planar call the bin kernels): copied; 3L + 38: the native ragged tail.
# per_cu 32: more buffers than wave slots (at most 32 a CU): the grid-stride loop and the prefetch hand-over.
@pytest.mark.parametrize("nch", [2, 4, 8, 3])
@pytest.mark.parametrize("L,k,extra,per_cu", [(L, k, e, 0) for L in (200, 128) for k, e in ((2, 0), (5, 0), (3, 37), (3, 38))]
                         + [(128, 2, 0, 32)])
def test_bits_of_the_planar_call(nch, L, k, extra, per_cu, path, bins):
    import torch
    R, nbuf = k * L + extra, 9 + per_cu * torch.cuda.get_device_properties(0).multi_processor_count
    check(frames(nch, L, nbuf * R, extremes=L == 128), nbuf, R, 10, L, native=bool(path) and nch != 3 and R % 2 == 0)


@pytest.mark.parametrize("nd,kw", [(16, {}), (10, dict(parallel=False)), (10, dict(n_cores=3))],
                         ids=["ndata16", "sequential", "chains"])
def test_other_block_size_and_lm_modes(nd, kw, path, bins):
    check(frames(4, 200, 9 * 1000), 9, 1000, nd, 200, native=bool(path), **kw)


@pytest.mark.parametrize("nch,start,pad,dtype,native", [
    (2, 1, 0, "int16", False), (2, 2, 0, "int16", True), (4, 1, 0, "int16", False), (8, 1, 0, "int16", True),
    (4, 0, 2, "int16", False), (2, 1, 1, "int16", False), (2, 0, 0, "float32", False), (2, 0, 0, "float64", False)])
def test_alignment_padding_and_type(nch, start, pad, dtype, native, path, bins):
    """Both sides of the alignment min(4 nch, 16) B (a view `start` frames in), padded and float frames."""
    import torch
    src = frames(nch, 200, 9 * 400 + 2)
    big = torch.zeros((src.shape[0], nch + pad), dtype=getattr(torch, dtype), device="cuda")
    big[:, :nch] = src
    check(big[start:, :nch], 9, 400, 10, 200, native=bool(path) and native)


@pytest.mark.parametrize("R,native", [(65535 * 128, True), (65535 * 128 + 2, False)])
def test_overflow_guard(R, native, path, bins):
    """65535 full-scale cycles per bin still fit int32, one more does not: the copy then takes the planar
    path's own guard (demodulation only: a seed wave alone on 8M samples would take seconds)."""
    import torch
    fr = torch.empty((R, 2), dtype=torch.int16, device="cuda")
    fr[:, 0], fr[:, 1] = -32768, 32767
    check(fr, 1, R, 10, 128, native=bool(path) and native, record=False)


def test_host_frames(path, bins):
    fr = frames(4, 200, 9 * 638)
    dev = check(fr, 9, 638, 10, 200, native=bool(path))
    host = check(fr.cpu().numpy(), 9, 638, 10, 200, native=bool(path))
    np.testing.assert_array_equal(host[0], dev[0])
    np.testing.assert_array_equal(host[1], dev[1])


@pytest.mark.parametrize("R", [637, 638])
def test_against_long_double(R, path, bins):
    """QI_h = mean(x cos / sin(h w0 t)), dc = mean(x) per channel in np.longdouble. Bounds: the parity suite's
    1e-12 on QI of a unit-scale record (test_gpu_parity.py; here QI / 4096), DESIGN.md §7's 1e-13 relative on dc."""
    from deepfmkit_amd.fitters import w0_of
    nch, nbuf, nd, L = 4, 3, 10, 200
    fr = frames(nch, L, 9 * 638)[: nbuf * R]
    qi, dc, _ = demod(fr, nch, nbuf, R, nd, L, True)
    x = fr.cpu().numpy().astype(np.longdouble).reshape(nbuf, R, nch)
    t, w0 = np.arange(R, dtype=np.longdouble), np.longdouble(w0_of(F_SAMP / L, F_SAMP))
    for c in range(nch):
        for b in range(nbuf):
            ref = [(x[b, :, c] * f((h + 1) * w0 * t)).mean() for f in (np.cos, np.sin) for h in range(nd)]
            err = np.abs(qi[:, c * nbuf + b] - np.array(ref, dtype=np.longdouble)).max() / SCALE
            assert err <= 1e-12, (c, b, float(err))
            assert abs(dc[c * nbuf + b] - x[b, :, c].mean()) <= 1e-13 * abs(x[b, :, c].mean())


def test_facade_and_errors():
    """At the default tuning: load_frames + fit_many fit the frames as they lie (the native
    kernel) and give the frames that contiguous int16 records of the same channels give; a single
    label is a one-column call; nls_frames(errors=True) equals nls_records(errors=True)."""
    import deepfmkit_amd as dfm
    from deepfmkit_amd import _lib
    from deepfmkit_amd.data import DeepRawObject
    from deepfmkit_amd.fitters import nls_frames, nls_records
    nch, R = 4, 2000
    fr = frames(nch, 200, 9 * R)
    a, b = dfm.DeepFitFramework(), dfm.DeepFitFramework()
    labels = a.load_frames(fr, F_SAMP, 1000.0, labels=[f"ch{c}" for c in range(nch)])
    assert all(a.raws[l].samples().data_ptr() == fr[:, c].data_ptr() for c, l in enumerate(labels))  # views, no copy
    for c, l in enumerate(labels):
        raw = DeepRawObject()
        raw.data, raw.label, raw.t0, raw.f_samp, raw.f_mod = fr[:, c].contiguous(), l, 0, F_SAMP, 1000.0
        b.raws[l] = raw
    a.fit_many(labels, n=10, init_a=SCALE)
    assert _lib.load().dfmi_last_demod_kernel().decode().startswith("demod_frames_kernel<4,")
    b.fit_many(labels, n=10, init_a=SCALE)
    for f in (a, b):
        f.fit(labels[1], n=10, init_a=SCALE, fit_label="single")  # a: a one-column frames call
    for l in [l + "_nls" for l in labels] + ["single"]:
        assert a.fits_df[l].equals(b.fits_df[l]), l
    got = nls_frames(fr, F_SAMP, 1000.0, R, 9, init_guess=guess(nch), errors=True)
    want = nls_records(fr.T.contiguous(), F_SAMP, 1000.0, R, 9, init_guess=guess(nch), errors=True)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w.cpu().numpy())
