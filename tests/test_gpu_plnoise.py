"""dfmi_plnoise on the GPU (csrc/plnoise.hip) against the numpy restatement
(tests/helpers/plnoise_ref.py) at the shapes of tests/test_plnoise_host.py: tables of
1, 2, 13, 63 and 64 sections, n in {1, 3, 64, 65, 313, 1000} with n_warm in {0, 2 n} (fewer
samples than sections included), 1, 3 and 130 series.

Gate (DESIGN.md section 13's rule): the largest deviation from the longdouble twin, relative to
the series' RMS, is at most 16 x the float64 restatement's own deviation from that twin, with a
floor of 1e-12: the device's log is within an ulp of libm's, so the gaussians differ in the last
place, and the filter is linear. The same bits come out run to run, alone or at any position of
a batch, in host or device memory, and sentinel guards around `out` stay untouched.

DFMI_GATE_DIR=<dir> writes the worst ratio per table to <dir>/gate_ratios_gpu.txt (the recorded
run: profiles/plnoise/gate_ratios_gpu.txt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import plnoise_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

FS = 200000.0
SIGMA = float(np.sqrt(FS / 2.0))
NSECS = (1, 2, 13, 63, 64)
SHAPES = [(n, w) for n in (1, 3, 64, 65, 313, 1000) for w in (0, 2 * n)]
SEEDS = (11 + 7 * np.arange(130)).astype(np.uint32)
TMAX = 3000


@pytest.fixture(scope="module")
def ratios():
    """Collects the worst ratio per case; written out after the module when DFMI_GATE_DIR is set."""
    seen = {}
    yield seen
    d = os.environ.get("DFMI_GATE_DIR")
    if d and seen:
        with open(os.path.join(d, "gate_ratios_gpu.txt"), "w") as f:
            f.write("# dfmi_plnoise: worst ratio to the gate per table and batch (<= 1 passes), MI355X\n")
            for (nsec, nser), r in sorted(seen.items()):
                f.write(f"nsec {nsec} nser {nser}: ratio {r:.3g}\n")
            f.write(f"worst: {max(seen.values()):.3g}\n")


@pytest.fixture(scope="module")
def refs():
    """Per table: the float64 and longdouble cascades of every seed's first TMAX gaussians.
    A shorter run is a prefix of it (RandomState(seed).normal(size=T) and the recurrence both
    run forward), so one pass serves every (n, n_warm). The float64 side is scipy.signal.lfilter,
    the restatement's scalar loop bit for bit (tests/test_plnoise_host.py pins that)."""
    from scipy.signal import lfilter
    out = {}
    X = np.stack([R.gaussians(int(s), SIGMA, TMAX) for s in SEEDS])
    for nsec in NSECS:
        sec, scale = R.table(nsec)
        y64 = X
        for a0, a1, b1 in sec:
            y64 = lfilter([a0, a1], [1.0, -b1], y64, axis=1)
        out[nsec] = (sec, scale, y64, R.cascade_many(sec, X, np.longdouble))
    return out


def _run(sec, scale, seeds, n_warm, n, mem="device", sigma=SIGMA):
    import torch
    from deepfmkit_amd import _lib
    lib = _lib.load()
    seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
    sec = np.ascontiguousarray(sec, dtype=np.float64)
    if mem == "host":
        out = np.zeros((seeds.size, n))
        _lib.check(lib.dfmi_plnoise(sec.ctypes.data, len(sec), scale, sigma, seeds.ctypes.data, seeds.size, n_warm, n,
                                    out.ctypes.data, _lib.DFMI_MEM_HOST, None), "dfmi_plnoise")
        return out
    out = torch.zeros((seeds.size, n), dtype=torch.float64, device="cuda")
    _lib.check(lib.dfmi_plnoise(sec.ctypes.data, len(sec), scale, sigma, seeds.ctypes.data, seeds.size, n_warm, n,
                                out.data_ptr(), _lib.DFMI_MEM_DEVICE, torch.cuda.current_stream().cuda_stream),
               "dfmi_plnoise")
    return out.cpu().numpy()


@pytest.mark.parametrize("nser", [1, 3, 130])
@pytest.mark.parametrize("nsec", NSECS)
def test_gate_against_longdouble_twin(refs, ratios, nsec, nser):
    sec, scale, y64, yld = refs[nsec]
    worst = 0.0
    for n, n_warm in SHAPES:
        got = _run(sec, scale, SEEDS[:nser], n_warm, n)
        twin = np.longdouble(scale) * yld[:nser, n_warm:n_warm + n]
        own = scale * y64[:nser, n_warm:n_warm + n]
        rms = np.sqrt(np.mean(twin ** 2, axis=1))
        assert np.all(rms > 0) and np.all(np.isfinite(got))
        dev = np.max(np.abs(got - twin), axis=1) / rms
        gate = np.maximum(16 * np.max(np.abs(own - twin), axis=1) / rms, np.longdouble(1e-12))
        ratio = float(np.max(dev / gate))
        worst = max(worst, ratio)
        ratios[(nsec, nser)] = worst
        print(f"nsec {nsec} nser {nser} n {n} n_warm {n_warm}: worst ratio to the gate {ratio:.3g}")
        assert ratio <= 1.0, (nsec, nser, n, n_warm, ratio)


@pytest.mark.parametrize("nsec,n,n_warm", [(13, 313, 626), (64, 65, 130), (63, 3, 0), (2, 1000, 2000)])
def test_same_bits_everywhere(nsec, n, n_warm):
    sec, scale = R.table(nsec)
    batch = _run(sec, scale, SEEDS, n_warm, n)
    np.testing.assert_array_equal(_run(sec, scale, SEEDS, n_warm, n), batch)  # run to run
    np.testing.assert_array_equal(_run(sec, scale, SEEDS, n_warm, n, mem="host"), batch)  # host memory
    for r in (0, 1, 63, 64, 129):  # alone
        np.testing.assert_array_equal(_run(sec, scale, SEEDS[r:r + 1], n_warm, n)[0], batch[r])
    perm = np.random.RandomState(5).permutation(SEEDS.size)  # any position of a batch
    np.testing.assert_array_equal(_run(sec, scale, SEEDS[perm], n_warm, n), batch[perm])
    np.testing.assert_array_equal(_run(sec, scale, SEEDS[:3], n_warm, n), batch[:3])


@pytest.mark.parametrize("nsec,n,n_warm,nser", [(13, 313, 626, 3), (64, 1, 0, 130), (1, 65, 130, 1)])
def test_guards_around_out_stay_untouched(nsec, n, n_warm, nser):
    import torch
    from deepfmkit_amd import _lib
    sec, scale = R.table(nsec)
    guard, sentinel = 512, -7.25
    buf = torch.full((2 * guard + nser * n,), sentinel, dtype=torch.float64, device="cuda")
    seeds = np.ascontiguousarray(SEEDS[:nser])
    _lib.check(_lib.load().dfmi_plnoise(sec.ctypes.data, nsec, scale, SIGMA, seeds.ctypes.data, nser, n_warm, n,
                                        buf.data_ptr() + 8 * guard, _lib.DFMI_MEM_DEVICE,
                                        torch.cuda.current_stream().cuda_stream), "dfmi_plnoise")
    h = buf.cpu().numpy()
    assert np.all(h[:guard] == sentinel) and np.all(h[guard + nser * n:] == sentinel)
    np.testing.assert_array_equal(h[guard:guard + nser * n].reshape(nser, n), _run(sec, scale, seeds, n_warm, n))


def test_alpha_noise_binding_matches_host_series():
    """physics.alpha_noise on the device against its host form (scipy.signal.lfilter over the
    same designed table) at the gate above: a record of 4000 samples, 8000 of warm-up."""
    from deepfmkit_amd import physics as P
    n = 4000
    host = P.alpha_noise(FS, n, 2.0, [2, 6, 10])
    dev = P.alpha_noise(FS, n, 2.0, [2, 6, 10], device="cuda").cpu().numpy()
    sec, scale = P.alpha_noise_design(FS, n, 2.0)
    X = np.stack([R.gaussians(s, SIGMA, 3 * n) for s in (2, 6, 10)])
    twin = np.longdouble(scale) * R.cascade_many(sec, X, np.longdouble)[:, 2 * n:]
    rms = np.sqrt(np.mean(twin ** 2, axis=1))
    gate = np.maximum(16 * np.max(np.abs(host - twin), axis=1) / rms, np.longdouble(1e-12))
    ratio = np.max(np.abs(dev - twin), axis=1) / rms / gate
    print(f"alpha_noise n {n}: ratio to the gate {float(ratio.max()):.3g}")
    assert np.all(ratio <= 1.0)
