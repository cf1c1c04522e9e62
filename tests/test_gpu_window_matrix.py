"""Every instance of demod_window_kernel and the call geometry of dfmi_demod_window against the
long-double definition (tests/helpers/window_ref.py, validated on the CPU by
tests/test_window_matrix_host.py).

Gates, the project's (tests/test_gpu_window.py): max |dQI| <= 1e-12 max|x|, dc
relative <= 1e-13. Every case prints its worst ratio to the gate; DFMI_GATE_DIR=<dir> writes them to
<dir>/gate_ratios.txt (the recorded run: profiles/window_matrix_gate.txt).

(a) all 36 instances, VEC 1 / 2 x MAXSLOT 2 / 4 x K 1 / 2 / 3 x float64 / float32 / int16, 5 segments
    of R = 5 L + 3 each, the kernel string asserted exactly (window_ref.INSTANCES says which shape
    reaches which); float32 / int16 also bit-equal to the widened float64 record at the same stride;
    and VEC 1 from a device view that starts one sample in.
(b) geometry edges: R < L, R = K + 1, R = K (refused), R = L, L = 2 / 3 / 4 / 8, an explicit period
    (L and 2 L), the harmonic-block boundaries of fold_finish (ndata 1 .. 30 at L = 128), the LDS
    refusal, nseg below one workgroup.
(c) a NaN and an Inf stay inside their own segments when a wave takes several; int16 at full scale.
(d) the table cache: two windows at one (R, L, K), and two R at one window, back to back.
(e) host memory gives the bits of device memory.  (f) fit.demodulate(window=) is the ABI call."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import window_ref as W  # noqa: E402

SEEN = set()  # the kernel strings of (a)
_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not pytest.importorskip("torch").cuda.is_available():
        pytest.skip("no GPU")
    yield
    d = os.environ.get("DFMI_GATE_DIR")
    if d and _RATIOS:
        with open(os.path.join(d, "gate_ratios.txt"), "w") as f:
            f.write("# dfmi_demod_window matrix: worst ratio to the gate per case (<= 1 passes), MI355X\n")
            f.writelines(f"{k}: QI {q:.3g} dc {c:.3g}\n" for k, (q, c) in sorted(_RATIOS.items()))
            f.write(f"worst: QI {max(q for q, _ in _RATIOS.values()):.3g} dc {max(c for _, c in _RATIOS.values()):.3g}\n")


def demod(x, nseg, stride, R, nd, w0, window, period=0, check=True):
    """dfmi_demod_window on a numpy array (host memory) or a CUDA tensor -> (qi, dc, kernel), or the
    error code when check is False. The outputs are NaN before the call."""
    import torch
    from deepfmkit_amd import _lib
    from deepfmkit_amd.fitters import _xtype
    lib, a, dev = _lib.load(), W.coefs(window), hasattr(x, "data_ptr")
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
        torch.cuda.synchronize()
        qi, dc = qi.cpu().numpy(), dc.cpu().numpy()
    return qi, dc, lib.dfmi_last_demod_kernel().decode()


def gate(qi, dc, segs, window, nd, w0, what):
    eq, ed = W.errors(qi, dc, segs, window, nd, w0)
    rq, rd = eq / W.QI_GATE, ed / W.DC_GATE
    old = _RATIOS.get(what, (0.0, 0.0))
    _RATIOS[what] = (max(old[0], rq), max(old[1], rd))
    print(f"{what}: QI err {eq:.2e} of max|x| (ratio {rq:.3g}), dc err {ed:.2e} relative (ratio {rd:.3g})")
    assert eq <= W.QI_GATE and ed <= W.DC_GATE, what


def same_bits(a, b, what):
    np.testing.assert_array_equal(a[0], b[0], err_msg=f"{what}: QI")
    np.testing.assert_array_equal(a[1], b[1], err_msg=f"{what}: dc")


# ---- (a) the 36 instances ----

def run_instance(row):
    x, w0 = W.instance_input(row)
    want = W.kernel_name(row["vec"], row["ms"], row["K"], row["dtype"])
    qi, dc, kern = demod(x, W.NSEG, row["stride"], row["R"], row["nd"], w0, row["window"])
    assert kern == want, (kern, want)
    SEEN.add(kern)
    gate(qi, dc, W.strided(x, W.NSEG, row["stride"], row["R"]), row["window"], row["nd"], w0, f"a {W.instance_id(row)}")
    if row["dtype"] != "float64":
        q64, d64, k64 = demod(x.astype(np.float64), W.NSEG, row["stride"], row["R"], row["nd"], w0, row["window"])
        assert k64 == W.kernel_name(row["vec"], row["ms"], row["K"], "float64"), k64
        same_bits((qi, dc), (q64, d64), f"{W.instance_id(row)} vs the widened record")


@pytest.mark.parametrize("row", W.INSTANCES, ids=W.instance_id)
def test_instance(row):
    run_instance(row)


def test_all_36_instances_ran():
    """The set of kernel strings the instance cases saw has 36 members (a case deselected from this run
    is run here first, so the count does not depend on the selection)."""
    for row in W.INSTANCES:
        if W.kernel_name(row["vec"], row["ms"], row["K"], row["dtype"]) not in SEEN:
            run_instance(row)
    print("\n".join(sorted(SEEN)))
    assert len(SEEN) == 36, sorted(SEEN)


@pytest.mark.parametrize("dtype", W.DTYPES)
def test_view_one_sample_in(dtype):
    """L = 200 at an even stride from a device view that starts one sample in: no sample pairs, so
    VEC 1 at four slots; the aligned copy of the same samples runs <2,2>."""
    import torch
    L, R, stride, nd = 200, 1003, 1004, 10
    w0 = 2 * np.pi / L
    x = torch.from_numpy(W.signal(4 * stride + R + 1, w0, dtype, seed=11)).cuda()
    odd, even = x[1:], x[1:].clone()
    qo, do, ko = demod(odd, 5, stride, R, nd, w0, "blackman")
    qe, de, ke = demod(even, 5, stride, R, nd, w0, "blackman")
    assert ko == W.kernel_name(1, 4, 2, dtype) and ke == W.kernel_name(2, 2, 2, dtype), (ko, ke)
    segs = W.strided(odd.cpu().numpy(), 5, stride, R)
    gate(qo, do, segs, "blackman", nd, w0, f"a view one sample in {dtype}")
    gate(qe, de, segs, "blackman", nd, w0, f"a view's aligned copy {dtype}")


# ---- (b) geometry edges ----

def run_case(what, L, R, window, nd, nseg=5, stride=None, dtype="float64", period=0, kernel=None, seed=2):
    stride = R if stride is None else stride
    w0 = 2 * np.pi / L
    x = W.signal((nseg - 1) * stride + R, w0, dtype, seed=seed)
    qi, dc, kern = demod(x, nseg, stride, R, nd, w0, window, period=period)
    if kernel is not None:
        assert kern == kernel, (kern, kernel)
    gate(qi, dc, W.strided(x, nseg, stride, R), window, nd, w0, f"b {what} ({kern})")
    return qi, dc, kern


def test_segment_shorter_than_the_period():
    """R = 130 < L = 200: no full cycle, the ragged cycle alone (rem = R)."""
    run_case("R=130 < L=200 hann", 200, 130, "hann", 10, kernel=W.kernel_name(2, 2, 1, "float64"))
    run_case("R=131 < L=200 blackman, odd stride", 200, 131, "blackman", 10, kernel=W.kernel_name(1, 4, 2, "float64"))


def test_fewest_samples():
    """R = K + 1 = 4 under Blackman-Harris runs; R = K = 3 is refused, naming R."""
    from deepfmkit_amd import _lib
    run_case("R=4 blackmanharris", 200, 4, "blackmanharris", 10)
    rc = demod(np.ones(15), 5, 3, 3, 10, 2 * np.pi / 200, "blackmanharris", check=False)
    err = _lib.load().dfmi_last_error()
    assert rc == -4 and b"R must exceed" in err, (rc, err)
    rc = demod(np.ones(5), 5, 1, 1, 10, 2 * np.pi / 200, "hann", check=False)
    assert rc == -4 and b"R must exceed" in _lib.load().dfmi_last_error()


def test_one_period():
    run_case("R=L=200 hann", 200, 200, "hann", 10, kernel=W.kernel_name(2, 2, 1, "float64"))
    run_case("R=L=75 blackmanharris", 75, 75, "blackmanharris", 10, kernel=W.kernel_name(1, 2, 3, "float64"))


@pytest.mark.parametrize("L", [2, 3, 4, 8])
@pytest.mark.parametrize("nd", [1, 3])
def test_smallest_periods(L, nd):
    """f_mod = f_samp / L, R = 7 L + 1; at the stride R (VEC 1 wherever R is odd) and at an even
    stride (VEC 2 for the even periods)."""
    from deepfmkit_amd import _lib
    R = 7 * L + 1
    assert _lib.load().dfmi_detect_period(2 * np.pi / L, R, nd) == L
    for K, window in W.WINDOW_OF_K.items():
        for stride in (R, R + 2 - (R & 1)):
            vec, ms = W.expected_instance(L, stride)
            run_case(f"L={L} ndata={nd} stride={stride} {window}", L, R, window, nd, stride=stride,
                     kernel=W.kernel_name(vec, ms, K, "float64"))


def test_explicit_period():
    """period = L gives the bits of the detected period; period = 2 L = 400 is a period of the basis
    too, runs the four-slot instance and meets the same gate."""
    L, R, stride = 200, 1003, 1004
    auto = run_case("period detected", L, R, "hann", 10, stride=stride, kernel=W.kernel_name(2, 2, 1, "float64"))
    given = run_case("period=L", L, R, "hann", 10, stride=stride, period=L, kernel=W.kernel_name(2, 2, 1, "float64"))
    same_bits(auto, given, "period = L against the detected period")
    for K, window in W.WINDOW_OF_K.items():
        run_case(f"period=2L {window}", L, R, window, 10, stride=stride, period=2 * L,
                 kernel=W.kernel_name(2, 4, K, "float64"))


@pytest.mark.parametrize("nd", [1, 7, 8, 9, 16, 30])
def test_harmonic_blocks(nd):
    """fold_finish contracts 8 harmonics per block: ndata below, at and past its boundaries, L = 128
    (61,440 B of basis at ndata 30). Hann keeps its factors in registers; the odd stride runs the
    four-slot instance, whose Blackman-Harris factors sit in LDS behind the basis."""
    run_case(f"ndata={nd} L=128 hann", 128, 643, "hann", nd, stride=644, kernel=W.kernel_name(2, 2, 1, "float64"))
    run_case(f"ndata={nd} L=129 blackmanharris", 129, 648, "blackmanharris", nd,
             kernel=W.kernel_name(1, 4, 3, "float64"))


def test_too_many_harmonics_for_lds():
    from deepfmkit_amd import _lib
    rc = demod(np.ones(2 * 2048), 2, 2048, 2048, 62, 2 * np.pi / 512, "hann", check=False)
    err = _lib.load().dfmi_last_error()
    assert rc == -4 and b"LDS" in err, (rc, err)


def test_period_beyond_the_single_sample_loads():
    """Documented refusal: L > 256 needs sample pairs; L = 400 at an odd stride has none."""
    from deepfmkit_amd import _lib
    rc = demod(np.ones(2 * 2003), 2, 2003, 2003, 10, 2 * np.pi / 400, "hann", check=False)
    err = _lib.load().dfmi_last_error()
    assert rc == -4 and b"period" in err, (rc, err)


@pytest.mark.parametrize("nseg", [1, 3, 4, 5])
def test_fewer_segments_than_a_workgroup(nseg):
    for dtype in W.DTYPES:
        run_case(f"nseg={nseg} {dtype}", 200, 1003, "blackman", 10, nseg=nseg, stride=1004, dtype=dtype,
                 kernel=W.kernel_name(2, 2, 2, dtype))


# ---- (c) isolation ----

def test_a_bad_sample_stays_in_its_segment():
    """3000 segments of R = 400 at ndata 30: 96,000 B of basis leave room for one workgroup per CU, so
    the persistent grid has fewer waves than segments and a wave takes several. A NaN in one segment
    and a +Inf in another: those two outputs are non-finite, every other segment keeps its bits."""
    nseg, R, nd, w0 = 3000, 400, 30, 2 * np.pi / 200
    x = W.signal(nseg * R, w0, seed=5).reshape(nseg, R)
    for window in ("hann", "blackmanharris"):
        clean = demod(x, nseg, R, R, nd, w0, window)
        pick = np.unique(np.r_[0, nseg - 1, np.linspace(1, nseg - 2, 10).astype(int)])
        gate(clean[0][:, pick], clean[1][pick], x[pick], window, nd, w0, f"c 3000 segments {window}")
        bad = x.copy()
        bad[7, 133], bad[1501, 399] = np.nan, np.inf
        qi, dc, _ = demod(bad, nseg, R, R, nd, w0, window)
        keep = np.ones(nseg, bool)
        keep[[7, 1501]] = False
        assert not np.isfinite(dc[[7, 1501]]).any() and not np.isfinite(qi[:, [7, 1501]]).any()
        same_bits((qi[:, keep], dc[keep]), (clean[0][:, keep], clean[1][keep]), f"{window}: the other segments")


def test_int16_full_scale():
    """Counts over the whole int16 range (both ends present) under Blackman-Harris."""
    R, w0 = 1003, 2 * np.pi / 200
    t = np.arange(4 * 1004 + R)
    x = np.clip(np.round(32767 * np.cos(0.4 + 6 * np.cos(w0 * t + 0.3)) + 40 * np.random.RandomState(8).randn(t.size)),
                -32767, 32767).astype(np.int16)
    x[5], x[6] = 32767, -32767
    segs = W.strided(x, 5, 1004, R)
    assert segs.max() == 32767 and segs.min() == -32767 and (segs.mean(axis=1) > 1000).all()
    qi, dc, kern = demod(x, 5, 1004, R, 10, w0, "blackmanharris")
    assert kern == W.kernel_name(2, 2, 3, "int16")
    gate(qi, dc, segs, "blackmanharris", 10, w0, "c int16 full scale")


# ---- (d) the table cache ----

def test_two_windows_at_one_geometry():
    """hann, hamming, hann at one (R, L, K = 1): the tables are cached per coefficient bits too."""
    x, w0 = W.signal(4 * 1004 + 1003, 2 * np.pi / 200, seed=9), 2 * np.pi / 200
    segs, got = W.strided(x, 5, 1004, 1003), []
    for i, window in enumerate(("hann", "hamming", "hann")):
        qi, dc, _ = demod(x, 5, 1004, 1003, 10, w0, window)
        gate(qi, dc, segs, window, 10, w0, f"d call {i + 1}: {window}")
        got.append((qi, dc))
    same_bits(got[0], got[2], "hann after hamming")
    assert np.abs(got[0][0] - got[1][0]).max() > 1e-6  # and the two windows do differ


def test_two_lengths_at_one_window():
    x, w0 = W.signal(4 * 1004 + 1003, 2 * np.pi / 200, seed=10), 2 * np.pi / 200
    got = []
    for i, R in enumerate((1000, 1003, 1000)):
        qi, dc, _ = demod(x, 5, 1004, R, 10, w0, "blackman")
        gate(qi, dc, W.strided(x, 5, 1004, R), "blackman", 10, w0, f"d call {i + 1}: R={R}")
        got.append((qi, dc))
    same_bits(got[0], got[2], "R = 1000 after R = 1003")


# ---- (e) memory, (f) Python ----

@pytest.mark.parametrize("dtype", W.DTYPES)
def test_host_memory_gives_the_device_bits(dtype):
    import torch
    row = next(r for r in W.INSTANCES if (r["vec"], r["ms"], r["K"], r["dtype"]) == (2, 4, 3, dtype))
    x, w0 = W.instance_input(row)
    host = demod(x, W.NSEG, row["stride"], row["R"], row["nd"], w0, row["window"])
    dev = demod(torch.from_numpy(x).cuda(), W.NSEG, row["stride"], row["R"], row["nd"], w0, row["window"])
    assert host[2] == dev[2] == W.kernel_name(2, 4, 3, dtype)
    same_bits(host, dev, f"{dtype}: host against device memory")


@pytest.mark.parametrize("dtype,window", [("float64", "hann"), ("float32", "blackman"), ("int16", "blackmanharris"),
                                          ("float64", [0.5, -0.3, 0.1])])
def test_fit_demodulate(dtype, window):
    from deepfmkit_amd import fit
    R, nd, w0 = 1000, 10, 2 * np.pi / 200
    x = W.signal(6 * R, w0, dtype, seed=12).reshape(6, R)
    qi, dc = fit.demodulate(x, nd, w0, window=window)
    assert qi.shape == (6, 2 * nd) and dc.shape == (6,)
    gate(qi.T, dc, x, window, nd, w0, f"f fit.demodulate {dtype} {window}")
    q, d, kern = demod(x, 6, R, R, nd, w0, window)
    assert kern == W.kernel_name(2, 2, len(W.coefs(window)) - 1, dtype)
    same_bits((qi.T, dc), (q, d), "fit.demodulate against dfmi_demod_window")
