"""The bin kernels' workgroup prologue (csrc/demod.h bins_kernel_body): a workgroup folds its
waves' first segments before the basis table is in LDS, and its one barrier stands before the
first contraction. Every wave of a workgroup must reach that barrier exactly once, whatever its
number of segments (none, one, several), and no bin may change the order of its samples.

Every case compares the bin kernel (the row layout of dfmi_demod_rows and the component-major
QI / dc of dfmi_demod) with the cycle-aligned fold kernel (demod_kernel = 0), whose code this
does not touch, bit for bit on the same input, checks through dfmi_last_demod_kernel() that
each side ran the kernel meant, and ties a handful of segments to the numpy oracle's
quadratures at the suite's QI bound (1e-12 for records of unit scale, tests/test_gpu_parity.py;
the quadratures are linear in the samples, so int16 counts carry their scale into the bound).
The record cases run the fused seed + bin kernel behind two seed workgroups against the
component-major path.

Shapes: G = 3 workgroups per CU is the bin kernel's resident grid at up to 12 harmonics, so
4 G + 1 and 8 G - 1 segments leave waves of one workgroup with different segment counts when
demod_spw = 0 pins the grid to the resident slots; demod_spw = 1 (the bin kernels' default) and
2 give the finer grids. nseg 1, 3, 4, 5: workgroups with waves that have no segment at all."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F_SAMP, F_MOD = 200000.0, 1000.0  # basis period L = 200
QI_BOUND = 1e-12
I16_SCALE = 20000.0
_X = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deepfmkit_amd import _lib
    assert _lib.load().dfmi_device_count() >= 1
    yield
    _X.clear()


def lib_():
    from deepfmkit_amd import _lib
    return _lib, _lib.load()


def w0():
    from deepfmkit_amd.fitters import w0_of
    return w0_of(F_MOD, F_SAMP)


def resident_grid():
    import torch
    return 3 * torch.cuda.get_device_properties(0).multi_processor_count


class tuning:
    """dfmi_set_tuning for the block, the former values put back afterwards."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        import ctypes
        _lib, lib = lib_()
        self.old = {}
        for k, v in self.kv.items():
            cur = ctypes.c_int64()
            _lib.check(lib.dfmi_get_tuning(k.encode(), ctypes.byref(cur)), "get_tuning")
            self.old[k] = cur.value
            _lib.check(lib.dfmi_set_tuning(k.encode(), v), "set_tuning")

    def __exit__(self, *exc):
        _lib, lib = lib_()
        for k, v in self.old.items():
            _lib.check(lib.dfmi_set_tuning(k.encode(), v), "set_tuning")


def samples(n, dtype, seed=1):
    """n samples on the GPU: unit-scale noise around 0.25 (float64 / float32) or int16 counts
    of it. One float64 draw per seed, made once at the largest size asked for so far."""
    import torch
    if seed not in _X or _X[seed].numel() < n:
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        _X[seed] = torch.randn(n, dtype=torch.float64, device="cuda", generator=g) + 0.25
    x = _X[seed][:n]
    if dtype == "f32":
        return x.float()
    if dtype == "i16":
        return torch.clamp(torch.round(I16_SCALE / 8 * x), -32768, 32767).to(torch.int16)
    return x


def xtype(x):
    import torch
    _lib, _ = lib_()
    return {torch.float64: _lib.DFMI_F64, torch.float32: _lib.DFMI_F32, torch.int16: _lib.DFMI_I16}[x.dtype]


def launch(x, nseg, stride, R, nd, rows):
    """One demodulation call on the current stream, not synchronised -> (outputs, kernel string)."""
    import torch
    _lib, lib = lib_()
    st = torch.cuda.current_stream().cuda_stream
    if rows:
        out = [torch.full((nseg, lib.dfmi_qi_row_stride(nd)), float("nan"), dtype=torch.float64, device="cuda")]
        rc = lib.dfmi_demod_rows_typed(x.data_ptr(), xtype(x), nseg, stride, R, nd, w0(), 0, out[0].data_ptr(),
                                       _lib.DFMI_MEM_DEVICE, st)
    else:
        out = [torch.full((2 * nd, nseg), float("nan"), dtype=torch.float64, device="cuda"),
               torch.full((nseg,), float("nan"), dtype=torch.float64, device="cuda")]
        rc = lib.dfmi_demod_typed(x.data_ptr(), xtype(x), nseg, stride, R, nd, w0(), 0, out[0].data_ptr(),
                                  out[1].data_ptr(), _lib.DFMI_MEM_DEVICE, st)
    _lib.check(rc, "demod")
    return out, lib.dfmi_last_demod_kernel().decode()


def check_rows(rows, qi, dc, nd):
    """The row layout carries exactly qi and dc (tests/test_gpu_parity.py, same pairing)."""
    _, lib = lib_()
    for h in range(nd):
        b, i = divmod(h, 8)
        np.testing.assert_array_equal(rows[:, 16 * b + i], qi[h])
        np.testing.assert_array_equal(rows[:, 16 * b + 8 + i], qi[nd + h])
    np.testing.assert_array_equal(rows[:, lib.dfmi_qi_row_dc(nd)], dc)


def check_oracle(x, nseg, stride, R, nd, qi, segs):
    from oracle import nls_oracle as O
    bound = QI_BOUND * max(1.0, float(x.abs().max()))
    for s in sorted({int(s) for s in segs if 0 <= s < nseg}):
        ref = O.demod_buffer(x[s * stride: s * stride + R].cpu().numpy().astype(np.float64), nd, w0())
        err = np.abs(qi[:, s] - ref).max()
        assert err <= bound, (s, err, bound)


def bins_against_fold(x, nseg, stride, R, nd, spw=None):
    """Rows, QI and dc of the bin kernel == the fold kernel's, and the oracle's quadratures."""
    import torch
    G = resident_grid()
    kv = {"demod_wide": 0}
    if spw is not None:
        kv["demod_spw"] = spw
    with tuning(demod_kernel=1, **kv):
        (rows,), krows = launch(x, nseg, stride, R, nd, True)
        (qi, dc), kqi = launch(x, nseg, stride, R, nd, False)
    with tuning(demod_kernel=0, **kv):
        (fqi, fdc), kfold = launch(x, nseg, stride, R, nd, False)
    torch.cuda.synchronize()
    assert krows.startswith("demod_bins_kernel<2,") and ",rows," in krows, krows
    assert kqi.startswith("demod_bins_kernel<2,") and ",rows," not in kqi, kqi
    assert kfold.startswith("demod_fold_kernel<"), kfold
    assert ("(prefetch" in krows) == (R // 128 >= 4), (krows, R)  # R = 400: the branch without prefetch
    if x.dtype == torch.int16:
        assert krows.endswith("[i16 int]"), krows
    rows, qi, dc, fqi, fdc = (a.cpu().numpy() for a in (rows, qi, dc, fqi, fdc))
    np.testing.assert_array_equal(qi, fqi)
    np.testing.assert_array_equal(dc, fdc)
    check_rows(rows, fqi, fdc, nd)
    check_oracle(x, nseg, stride, R, nd, fqi, [0, 1, 3, 4, 4 * G - 1, 4 * G, 4 * G + 3, 8 * G - 2, nseg - 1])


@pytest.mark.parametrize("dtype", ["f64", "f32", "i16"])
@pytest.mark.parametrize("nseg", [1, 3, 4, 5])
def test_workgroups_with_idle_waves(nseg, dtype):
    """Fewer segments than waves: the waves without one still stage their share of the basis and
    meet the others at the barrier."""
    R = 4000
    bins_against_fold(samples(nseg * R, dtype), nseg, R, R, 10)


@pytest.mark.parametrize("dtype", ["f64", "f32", "i16"])
@pytest.mark.parametrize("spw", [0, 1, 2])
@pytest.mark.parametrize("edge", ["4G+1", "8G-1"])
def test_mixed_segment_counts(edge, spw, dtype):
    """Waves of one workgroup with 1 and 2, or 2 and 1, segments on the resident grid
    (demod_spw 0), and the finer grids of demod_spw 1 and 2."""
    G = resident_grid()
    nseg = 4 * G + 1 if edge == "4G+1" else 8 * G - 1
    R = 4000
    bins_against_fold(samples(nseg * R, dtype), nseg, R, R, 10, spw)


@pytest.mark.parametrize("dtype", ["f64", "f32", "i16"])
@pytest.mark.parametrize("R,stride", [(4001, 4002), (400, 400)])
def test_tail_chunk_and_no_prefetch(R, stride, dtype):
    """R = 4001: a partial last chunk behind the last load group. R = 400: fewer chunks than the
    prefetch depth, the branch without prefetch (demod_wide = 0 keeps it on the bin kernel)."""
    nseg = 4 * resident_grid() + 1
    bins_against_fold(samples(nseg * stride, dtype), nseg, stride, R, 10, 0)


@pytest.mark.parametrize("dtype", ["f64", "f32", "i16"])
@pytest.mark.parametrize("nd", [12, 16])
def test_more_harmonics(nd, dtype):
    """A larger basis to stage (ndata 16: more than half of the first batch of table loads)."""
    nseg = 4 * resident_grid() + 1
    R = 4000
    bins_against_fold(samples(nseg * R, dtype), nseg, R, R, nd, 0)


def test_back_to_back_calls_on_one_stream():
    """Two calls in a row, other samples and another basis (ndata 10, then 12), no
    synchronisation between them: no stale table or bins from the call before."""
    import torch
    R, nseg = 4000, 4 * resident_grid() + 1
    x1, x2 = samples(nseg * R, "f64", seed=1), samples(nseg * R, "f64", seed=2)
    with tuning(demod_kernel=1, demod_wide=0):
        (r1,), k1 = launch(x1, nseg, R, R, 10, True)
        (r2,), k2 = launch(x2, nseg, R, R, 12, True)
        (r3,), k3 = launch(x2, nseg, R, R, 10, True)
    with tuning(demod_kernel=0, demod_wide=0):
        f1, kf = launch(x1, nseg, R, R, 10, False)
        f2, _ = launch(x2, nseg, R, R, 12, False)
        f3, _ = launch(x2, nseg, R, R, 10, False)
    torch.cuda.synchronize()
    assert all(k.startswith("demod_bins_kernel<2,") for k in (k1, k2, k3)), (k1, k2, k3)
    assert kf.startswith("demod_fold_kernel<"), kf
    for r, (fqi, fdc), nd in ((r1, f1, 10), (r2, f2, 12), (r3, f3, 10)):
        check_rows(r.cpu().numpy(), fqi.cpu().numpy(), fdc.cpu().numpy(), nd)
    check_oracle(x2, nseg, R, R, 10, f3[0].cpu().numpy(), [0, nseg - 1])


def two_records(nbuf, R, dtype):
    """Two snr-like records (m near 6, small noise) as a (2, nbuf R) tensor."""
    import torch
    t = torch.arange(nbuf * R, dtype=torch.float64, device="cuda") / F_SAMP
    w = 2 * np.pi * F_MOD
    x = torch.stack([1.0 + torch.cos(0.3 + 0.4 * k + (5.8 + 0.3 * k) * torch.cos(w * t + 0.1 * k)) for k in range(2)])
    x = x + 1e-3 * samples(2 * nbuf * R, "f64", seed=3).view(2, -1)
    if dtype == "f32":
        return x.float()
    if dtype == "i16":
        return torch.clamp(torch.round(I16_SCALE / 2 * x), -32768, 32767).to(torch.int16)
    return x


@pytest.mark.parametrize("nd,dtype", [(10, "f64"), (12, "f64"), (16, "f64"), (10, "f32"), (10, "i16")])
def test_two_records_behind_seed_workgroups(nd, dtype):
    """dfmi_nls_record on two records: two seed workgroups lead the grid of the fused kernel
    (block0 = 2) and the bulk workgroups follow with the late-staged basis. Outputs and status
    equal the component-major path's (demod_kernel = 0: fold kernel, seed and LM on their own),
    the pairing of test_record_rows_path_matches_component_path."""
    from deepfmkit_amd.fitters import nls_records
    _lib, lib = lib_()
    R, nbuf = 4000, 2 * resident_grid() + 1  # 4 G + 2 segments
    x = two_records(nbuf, R, dtype)
    guess = (1.6 * (I16_SCALE / 2 if dtype == "i16" else 1.0), 6.0, 0.0, 0.0)
    res = {}
    for kern in (1, 0):
        with tuning(demod_kernel=kern, demod_wide=0):  # from 13 harmonics demod_wide_kernel would run instead
            cols, ok = nls_records(x, F_SAMP, F_MOD, R, nbuf, nd, init_guess=guess)
            res[kern] = (cols.cpu().numpy(), ok.cpu().numpy(), lib.dfmi_last_demod_kernel().decode())
    assert res[1][2].startswith(f"demod_seed_bins_kernel<2,{12 if nd <= 12 else 16},"), res[1][2]
    assert not res[0][2].startswith("demod_seed_bins_kernel"), res[0][2]
    np.testing.assert_array_equal(res[1][1], res[0][1])
    np.testing.assert_array_equal(res[1][0], res[0][0])
    if dtype != "i16":  # in count units this record ends with status 2 on both paths alike
        assert (res[1][1] == 0).mean() >= 0.999
