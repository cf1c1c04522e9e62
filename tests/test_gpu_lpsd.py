"""dfmi_lpsd on the GPU (csrc/lpsd.hip) at the shapes and gates of tests/helpers/lpsd_cases.py
against the numpy restatement (tests/helpers/lpsd_ref.py): Sxx and ENBW for mean 0 / -1 / 100
at order 0 and -1; the sine known answer; bit-identity of a batch and its series alone, of
device and host memory, of two runs; strided device rows; NaN samples. The host-build twin is
tests/test_lpsd_host.py.

Worst observed ratio to the gate on the MI355X (profiles/lpsd/gate_ratios_gpu.txt):
0.153 (s1, mean -1, order 0), 0.142 (s2, mean -1, order 0), 0.104 (s3, mean -1, order 0); the known answer
-1.28e-12, -1.28e-12, -1.24e-12 at j = 25, 40, 50 against the bound 1e-9."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lpsd_cases as C  # noqa: E402
import lpsd_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from deepfmkit_amd import lpsd as M  # noqa: E402


@pytest.mark.parametrize("shape", list(C.SHAPES))
def test_sxx_against_the_restatement(shape):
    worst = 0.0
    for mean in C.MEANS:
        for order in C.ORDERS:
            x, _, enbw_ref, gate = C.reference(shape, mean, order)
            r = M.lpsd(x, C.FS, order=order, **C.settings(shape))
            f, _, b, L, K = R.plan(x.size, C.FS, **C.settings(shape))
            assert np.array_equal(r.L, L) and np.array_equal(r.K, K) and np.array_equal(r.f, f)
            ratio = C.ratio(r.Sxx, shape, mean, order)
            print(f"{shape} mean {mean:g} order {order}: gate {gate:.2e} ratio {ratio:.3g}")
            worst = max(worst, ratio)
            assert np.max(np.abs(r.enbw / enbw_ref - 1)) <= 1e-12
            assert np.array_equal(r.asd, np.sqrt(r.Sxx))
    print(f"{shape}: worst ratio to the gate {worst:.3g}")
    assert worst <= 1.0, worst


def test_sine_known_answer():
    """x = 2.5 + 0.01 sin(2 pi f_j t + 0.3) at plan frequencies with b >= 9: Sxx ENBW = A^2/2
    within 1e-9 relative (the restatement: 1.3e-12)."""
    x = np.stack([C.known_series(j) for j in C.KNOWN["js"]])
    r = M.lpsd(x, C.FS, Jdes=C.KNOWN["Jdes"])
    for i, j in enumerate(C.KNOWN["js"]):
        rel = r.Sxx[i, j] * r.enbw[j] / (C.KNOWN["amp"] ** 2 / 2) - 1
        print(f"j={j} b={r.b[j]:.3f}: Sxx ENBW / (A^2/2) - 1 = {rel:.2e}")
        assert abs(rel) <= C.KNOWN["tol"]


def test_batch_equals_each_series_alone_and_runs_repeat():
    kw = C.settings("s3")
    x = np.stack([C.series("s3", m, seed=5 + i) for i, m in enumerate(C.MEANS)])
    batch = M.lpsd(x, C.FS, **kw)
    assert batch.Sxx.shape == (3, batch.f.size)
    for i in range(3):
        alone = M.lpsd(x[i], C.FS, **kw)
        assert alone.Sxx.shape == (batch.f.size,)
        assert np.array_equal(alone.Sxx, batch.Sxx[i]) and np.array_equal(alone.enbw, batch.enbw)
    again = M.lpsd(x, C.FS, **kw)
    assert np.array_equal(again.Sxx, batch.Sxx) and np.array_equal(again.enbw, batch.enbw)


@pytest.mark.parametrize("shape", ["s1", "s3"])
def test_device_memory_equals_host_memory(shape):
    kw = C.settings(shape)
    x = np.stack([C.series(shape, m, seed=9 + i) for i, m in enumerate(C.MEANS)])
    host = M.lpsd(x, C.FS, **kw)
    dev = M.lpsd(torch.from_numpy(x).cuda(), C.FS, **kw)
    assert dev.Sxx.is_cuda and dev.enbw.is_cuda and dev.asd.is_cuda
    assert np.array_equal(dev.Sxx.cpu().numpy(), host.Sxx) and np.array_equal(dev.enbw.cpu().numpy(), host.enbw)
    one = M.lpsd(torch.from_numpy(x[1]).cuda(), C.FS, **kw)
    assert one.Sxx.shape == (host.f.size,) and np.array_equal(one.Sxx.cpu().numpy(), host.Sxx[1])
    # rows of a wider device buffer (ser_stride > N), on a side stream
    wide = torch.full((3, x.shape[1] + 37), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        strided = M.lpsd(wide[:, :x.shape[1]], C.FS, **kw)
    s.synchronize()
    assert np.array_equal(strided.Sxx.cpu().numpy(), host.Sxx)


def test_nan_sample_propagates_without_error():
    kw = C.settings("s1")
    x = C.series("s1", 0.0, seed=3).copy()
    clean = M.lpsd(x, C.FS, **kw)
    x[250] = np.nan
    r = M.lpsd(x, C.FS, **kw)
    assert (r.K == 1).any()
    assert np.isnan(r.Sxx[r.K == 1]).all()  # a single segment spans the whole series
    # a frequency is NaN exactly when one of its segments holds the sample
    for j in range(r.f.size):
        starts = [int(np.floor(k * (x.size - r.L[j]) / (r.K[j] - 1) + 0.5)) if r.K[j] > 1 else 0
                  for k in range(r.K[j])]
        hit = any(s <= 250 < s + r.L[j] for s in starts)
        assert np.isnan(r.Sxx[j]) == hit
        if not hit:
            assert r.Sxx[j] == clean.Sxx[j]
    assert np.array_equal(r.enbw, clean.enbw)


def test_frequency_batches_give_the_same_bits():
    """The workspace bound splits the frequencies of a call into batches (512 MiB by default,
    reached by one series of 5e6 samples). With the bound at 0 every frequency is its own batch."""
    from deepfmkit_amd import _lib
    lib = _lib.load()
    kw = C.settings("s3")
    x = np.stack([C.series("s3", m, seed=20 + i) for i, m in enumerate(C.MEANS)])
    whole = M.lpsd(x, C.FS, **kw)
    _lib.check(lib.dfmi_set_tuning(b"lpsd_batch_mb", 0), "dfmi_set_tuning")
    try:
        split = M.lpsd(x, C.FS, **kw)
        split_dev = M.lpsd(torch.from_numpy(x).cuda(), C.FS, **kw)
    finally:
        _lib.check(lib.dfmi_set_tuning(b"lpsd_batch_mb", 512), "dfmi_set_tuning")
    assert np.array_equal(split.Sxx, whole.Sxx) and np.array_equal(split.enbw, whole.enbw)
    assert np.array_equal(split_dev.Sxx.cpu().numpy(), whole.Sxx)


def test_workspaces_are_released_and_regrown():
    from deepfmkit_amd import _lib
    kw = C.settings("s1")
    x = C.series("s1", -1.0, seed=4)
    a = M.lpsd(x, C.FS, **kw)
    _lib.check(_lib.load().dfmi_release_workspaces(), "dfmi_release_workspaces")
    b = M.lpsd(x, C.FS, **kw)
    assert np.array_equal(a.Sxx, b.Sxx)
