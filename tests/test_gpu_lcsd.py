"""dfmi_lcsd on the GPU (csrc/lpsd.hip's pair kernels) at the shapes and gates of
tests/helpers/lcsd_cases.py against the numpy restatement (tests/helpers/lcsd_ref.py): Sxx, Syy,
Sxy and the coherence for mean 0 / -1 / 100 at order 0 and -1; Sxx, Syy and ENBW bit for bit
dfmi_lpsd's; the call geometry (pairs, strides, one x for every y, guarded outputs, every subset
of NULL outputs, a side stream, frequency batches, host and device memory); the swap of x and y;
the two-sine known answer; the white-noise statistics; NaN samples. The host-build twin is
tests/test_lcsd_host.py.

Worst observed ratio to the gate on the MI355X (profiles/lcsd/gate_ratios_gpu.txt):
Sxx 0.153 (s1), Syy 0.0624 (s3), Sxy 0.0737 (s2), coh 0.0662 (s2), each at mean -1, order 0; the
known answer 1.29e-12 (Sxy), 6.6e-14 (H), 2.3e-16 (coh) against the bound 1e-9; statistics: median
coh 0.0023 (independent), 0.486, |H| 0.986, resid 0.980 (x against x + n)."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lcsd_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from deepfmkit_amd import _lib  # noqa: E402
from deepfmkit_amd import lpsd as M  # noqa: E402

NAMES = ("Sxx", "Syy", "re", "im", "coh", "enbw")
SENT = -7.25e77  # sentinel (exactly representable, never a result)
GUARD = 13


def raw(X, Y, N, kw, order=0, outs=(1, 1, 1, 1, 1, 1), device=True, stream=None, shared_x=False, plan=None):
    """One dfmi_lcsd call on the rows of X and Y (row stride = their width, >= N; shared_x: X's
    one row for every row of Y; plan: (b, L, K) in place of the settings' own). The outputs live
    in ONE sentinel-filled block with 13-element guards before, between and after them. Returns
    (rc, {name: array}, nothing else was written)."""
    lib = _lib.load()
    X, Y = np.ascontiguousarray(np.atleast_2d(X)), np.ascontiguousarray(np.atleast_2d(Y))
    npair = Y.shape[0]
    p = M.plan(N, C.FS, **kw)
    b, L, K = (p.b, p.L, p.K) if plan is None else plan
    J = b.size
    sizes = [npair * J] * 5 + [J]
    offs, o = [], GUARD
    for s in sizes:
        offs.append(o)
        o += s + GUARD
    h = np.full(o, SENT)
    plan_args = (N, C.FS, _lib.ptr(b), _lib.ptr(L), _lib.ptr(K), J, order, 200.0)
    xs = 0 if shared_x else X.shape[1]
    if device:
        d, dX, dY = torch.from_numpy(h).cuda(), torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
        st = torch.cuda.current_stream()
        if stream is not None:
            stream.wait_stream(st)
            st = stream
        ptrs = [d.data_ptr() + 8 * off if on else None for off, on in zip(offs, outs)]
        rc = lib.dfmi_lcsd(dX.data_ptr(), xs, dY.data_ptr(), Y.shape[1], npair, *plan_args, *ptrs,
                           _lib.DFMI_MEM_DEVICE, st.cuda_stream)
        st.synchronize()
        h = d.cpu().numpy()
    else:
        ptrs = [h.ctypes.data + 8 * off if on else None for off, on in zip(offs, outs)]
        rc = lib.dfmi_lcsd(X.ctypes.data, xs, Y.ctypes.data, Y.shape[1], npair, *plan_args, *ptrs,
                           _lib.DFMI_MEM_HOST, None)
    clean = np.ones(h.size, dtype=bool)
    res = {}
    for name, off, s, on in zip(NAMES, offs, sizes, outs):
        if on:
            clean[off:off + s] = False
            res[name] = h[off:off + s].copy() if name == "enbw" else h[off:off + s].reshape(npair, J).copy()
    return rc, res, bool((h[clean] == SENT).all())


def same(a, b, names=NAMES):
    return all(np.array_equal(a[n], b[n], equal_nan=True) for n in names if n in a and n in b)


@pytest.mark.parametrize("shape", list(C.SHAPES))
def test_against_the_restatement_and_dfmi_lpsd_bits(shape):
    worst = dict.fromkeys(C.QUANTITIES, 0.0)
    for mean in C.MEANS:
        for order in C.ORDERS:
            x, y, ref, gates = C.reference(shape, mean, order)
            r = M.lcsd(x, y, C.FS, order=order, **C.settings(shape))
            assert np.array_equal(r.L, ref["L"]) and np.array_equal(r.K, ref["K"]) and np.array_equal(r.f, ref["f"])
            rat = C.ratios(r, shape, mean, order)
            print(f"{shape} mean {mean:g} order {order}: " +
                  ", ".join(f"{q} gate {gates[q]:.2e} ratio {rat[q]:.3g}" for q in C.QUANTITIES))
            worst = {q: max(worst[q], rat[q]) for q in C.QUANTITIES}
            assert np.max(np.abs(r.enbw / ref["enbw"].astype(np.float64) - 1)) <= 1e-12
            # the pair kernel's accumulation did not drift: dfmi_lpsd's bits on the same series and plan
            single = M.lpsd(np.stack([x, y]), C.FS, order=order, **C.settings(shape))
            assert np.array_equal(r.Sxx, single.Sxx[0]) and np.array_equal(r.Syy, single.Sxx[1])
            assert np.array_equal(r.enbw, single.enbw)
            assert np.array_equal(r.H.real, r.Sxy.real / r.Sxx) and np.array_equal(r.H.imag, r.Sxy.imag / r.Sxx)
            assert np.array_equal(r.resid, r.Syy * (1 - r.coh))
    print(f"{shape}: worst ratio to the gate " + ", ".join(f"{q} {worst[q]:.3g}" for q in C.QUANTITIES))
    assert max(worst.values()) <= 1.0, worst


def _rows(shape, pad):
    """Three pairs of a shape as rows of width N + pad (the padding holds NaN)."""
    N = C.SHAPES[shape]["N"]
    X, Y = np.full((3, N + pad), np.nan), np.full((3, N + pad), np.nan)
    for i, mean in enumerate(C.MEANS):
        X[i, :N], Y[i, :N] = C.pair(shape, mean)
    return N, X, Y


@pytest.mark.parametrize("shape", ["s1", "s3"])
def test_pairs_strides_and_guarded_outputs(shape):
    kw = C.settings(shape)
    N, X0, Y0 = _rows(shape, 0)
    alone = []
    for i in range(3):  # npair = 1
        rc, r, untouched = raw(X0[i], Y0[i], N, kw)
        assert rc == 0 and untouched
        alone.append(r)
        hi = M.lcsd(X0[i], Y0[i], C.FS, **kw)
        assert np.array_equal(r["Sxx"][0], hi.Sxx) and np.array_equal(r["Syy"][0], hi.Syy)
        assert np.array_equal(r["re"][0], hi.Sxy.real) and np.array_equal(r["im"][0], hi.Sxy.imag)
        assert np.array_equal(r["coh"][0], hi.coh) and np.array_equal(r["enbw"], hi.enbw)
    for pad in (0, 13):  # npair = 3 at strides N and N + 13
        _, X, Y = _rows(shape, pad)
        rc, r, untouched = raw(X, Y, N, kw)
        assert rc == 0 and untouched
        for i in range(3):
            assert all(np.array_equal(r[n][i], alone[i][n][0]) for n in NAMES[:5])
        assert np.array_equal(r["enbw"], alone[0]["enbw"])
        # x_stride = 0: row p is the single-pair call of (x, y_p)
        rc, sh, untouched = raw(X[1:2], Y, N, kw, shared_x=True)
        assert rc == 0 and untouched
        for i in range(3):
            rc, one, _ = raw(X0[1], Y0[i], N, kw)
            assert rc == 0 and all(np.array_equal(sh[n][i], one[n][0]) for n in NAMES[:5])


def test_every_subset_of_null_outputs():
    kw = C.settings("s1")
    N, X, Y = _rows("s1", 13)
    _, full, _ = raw(X, Y, N, kw)
    for outs in itertools.product((0, 1), repeat=6):
        rc, r, untouched = raw(X, Y, N, kw, outs=outs)
        assert untouched, outs
        if not any(outs[:5]):
            assert rc == -1
            continue
        assert rc == 0, outs
        assert set(r) == {n for n, on in zip(NAMES, outs) if on} and same(r, full), outs


def test_side_stream_batches_and_host_memory_give_the_same_bits():
    kw = C.settings("s3")
    N, X, Y = _rows("s3", 13)
    rc, dev, _ = raw(X, Y, N, kw)
    assert rc == 0
    rc, side, untouched = raw(X, Y, N, kw, stream=torch.cuda.Stream())
    assert rc == 0 and untouched and same(side, dev)
    rc, host, untouched = raw(X, Y, N, kw, device=False)
    assert rc == 0 and untouched and same(host, dev)
    rc, host_sh, untouched = raw(X[:1], Y, N, kw, device=False, shared_x=True)
    rc2, dev_sh, _ = raw(X[:1], Y, N, kw, shared_x=True)
    assert rc == 0 and rc2 == 0 and untouched and same(host_sh, dev_sh)
    # with the workspace bound at 0 every frequency is its own batch
    lib = _lib.load()
    _lib.check(lib.dfmi_set_tuning(b"lpsd_batch_mb", 0), "dfmi_set_tuning")
    try:
        rc, split, untouched = raw(X, Y, N, kw)
        rc2, split_host, _ = raw(X, Y, N, kw, device=False)
    finally:
        _lib.check(lib.dfmi_set_tuning(b"lpsd_batch_mb", 512), "dfmi_set_tuning")
    assert rc == 0 and rc2 == 0 and untouched and same(split, dev) and same(split_host, dev)
    # twice: the same bits
    rc, again, _ = raw(X, Y, N, kw)
    assert rc == 0 and same(again, dev)


@pytest.mark.parametrize("case", [("s1", -1.0, 0), ("s3", 100.0, -1)])
def test_swapping_x_and_y_conjugates_sxy(case):
    shape, mean, order = case
    x, y, ref, gates = C.reference(*case)
    a = M.lcsd(x, y, C.FS, order=order, **C.settings(shape))
    b = M.lcsd(y, x, C.FS, order=order, **C.settings(shape))
    assert np.array_equal(a.Sxx, b.Syy) and np.array_equal(a.Syy, b.Sxx)
    scale = np.sqrt(a.Sxx * a.Syy)
    # each is within its gate of the longdouble twin, so the two are within twice that of each other
    assert np.max(np.abs(np.conj(b.Sxy) - a.Sxy) / scale) <= 2 * gates["Sxy"]
    assert np.max(np.abs(b.coh - a.coh)) <= 2 * gates["coh"]
    swapped = dict(Sxx=b.Syy, Syy=b.Sxx, Sxy=np.conj(b.Sxy), coh=b.coh)
    assert max(C.ratios(swapped, *case).values()) <= 1.0


def test_two_sine_known_answer():
    """x = 2.5 + 0.01 sin(2 pi f_j t + 0.3), y = -1 + 0.004 sin(2 pi f_j t + 0.3 - 1.1):
    Sxy ENBW = 0.01 0.004 / 2 e^{-1.1i}, H = 0.4 e^{-1.1i}, coh = 1, each within 1e-9."""
    pairs = [C.known_pair(j) for j in C.KNOWN["js"]]
    r = M.lcsd(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), C.FS, Jdes=C.KNOWN["Jdes"])
    for i, j in enumerate(C.KNOWN["js"]):
        fig = C.check_known(r.Sxy[i], r.H[i], r.coh[i], r.enbw, j)
        print(f"j={j}: |Sxy ENBW / expected - 1| = {fig[0]:.2e}, |H - expected| = {fig[1]:.2e}, |coh - 1| = {fig[2]:.2e}")
        assert max(fig) <= C.KNOWN["tol"]


def test_white_noise_statistics():
    x, n = C.stat_series()
    r = M.lcsd(x, np.stack([n, x + n]), C.FS, Jdes=C.STAT["Jdes"])
    C.check_statistics((r.coh[0], r.H[0], r.resid[0]), (r.coh[1], r.H[1], r.resid[1]), r.K)


def test_nan_in_y_reaches_only_its_frequencies_and_not_sxx():
    kw = C.settings("s1")
    x, y = C.pair("s1", 0.0)
    clean = M.lcsd(x, y, C.FS, **kw)
    clean_y, y = y, y.copy()
    y[250] = np.nan
    r = M.lcsd(x, y, C.FS, **kw)
    assert np.array_equal(r.Sxx, clean.Sxx) and np.isfinite(r.Sxx).all() and np.array_equal(r.enbw, clean.enbw)
    hits = 0
    for j in range(r.f.size):
        starts = [int(np.floor(k * (x.size - r.L[j]) / (r.K[j] - 1) + 0.5)) if r.K[j] > 1 else 0
                  for k in range(r.K[j])]
        hit = any(s <= 250 < s + r.L[j] for s in starts)
        hits += hit
        for a, c in ((r.Syy, clean.Syy), (r.Sxy, clean.Sxy), (r.coh, clean.coh), (r.H, clean.H), (r.resid, clean.resid)):
            assert np.isnan(a[j]) == hit
            if not hit:
                assert a[j] == c[j]
    assert hits == r.f.size  # overlapped segments cover the whole series
    # a plan of the caller's own with two segments per frequency, the first and the last: the
    # short ones do not hold the sample
    p = M.plan(x.size, C.FS, **kw)
    K2 = np.minimum(p.K, 2)
    rc, c2, _ = raw(x, clean_y, x.size, kw, plan=(p.b, p.L, K2))
    rc2, r2, _ = raw(x, y, x.size, kw, plan=(p.b, p.L, K2))
    assert rc == 0 and rc2 == 0 and np.array_equal(r2["Sxx"], c2["Sxx"])
    hit = (K2 == 1) | (p.L > 250)  # segments [0, L) and [N - L, N) of N = 500
    assert 0 < hit.sum() < hit.size
    for n in ("Syy", "re", "im", "coh"):
        assert np.array_equal(np.isnan(r2[n][0]), hit) and np.array_equal(r2[n][0][~hit], c2[n][0][~hit])
