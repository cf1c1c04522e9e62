"""dfmi_unwrap on the GPU against a plain reference, on both geometries (tuning key "unwrap_path":
1 the series kernel, 2 the tiled path). T = 1,024 is the tile of both; the tiled path's carry
kernel scans 256 tiles per step, so N = 257 T + 1 takes two steps.

cycles must match exactly everywhere. Up to a few thousand points the reference is exact rational
arithmetic and y must match bit for bit; at N = 257 T + 1 it is numpy long double and y must be
within one np.spacing (the most a doubly rounded reference can differ from a single fma). Every
input keeps |frac(d / P) - 1/2| > 1e-9 (asserted by the reference), so one ulp in the device's
division cannot flip a count."""
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 1024
BIG = 257 * T + 1
SIZES = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, BIG]
GAPS = {"first": slice(0, 1), "last": slice(2 * T, 2 * T + 1), "boundary": slice(T - 2, T + 3),
        "tile": slice(T, 2 * T), "all": slice(0, 2 * T + 1)}


def series(kind, N):
    """(x, period): 'ramp' a wrapped ramp of 2.1 rad per point, up then down, plus noise (it wraps
    about every third point, in both directions); 'walk' an unwrapped random walk with steps of
    up to 3 periods at period 1."""
    rng = np.random.RandomState(1000 + N)
    if kind == "walk":
        return np.cumsum(rng.uniform(-3.0, 3.0, N)), 1.0
    i = np.arange(N)
    true = 2.1 * np.minimum(i, N - i) + 0.1 * rng.randn(N)
    return (true + np.pi) % (2 * np.pi) - np.pi, 2 * np.pi


def reference(x, P, valid, fill):
    """(y, cycles) of one series by the definition in include/dfmi.h."""
    n, v = x.size, np.flatnonzero(valid)
    if v.size == 0:
        return np.full(n, np.nan), np.zeros(n, dtype=np.int64)
    d = x[v][1:] - x[v][:-1]  # the double differences
    if n <= 2 * T + 1:
        q = [Fraction(float(a)) / Fraction(P) for a in d]
        off = [abs(a - (a.numerator // a.denominator) - Fraction(1, 2)) for a in q]
        cv = np.concatenate([[0], -np.cumsum([round(a) for a in q], dtype=np.int64)]).astype(np.int64)  # half to even
        yv = np.array([float(Fraction(float(a)) + int(c) * Fraction(P)) for a, c in zip(x[v], cv)])
    else:
        q = d.astype(np.longdouble) / np.longdouble(P)
        off = np.abs(q - np.floor(q) - 0.5)
        cv = np.concatenate([[0], -np.cumsum(np.rint(q).astype(np.int64))])
        yv = (x[v].astype(np.longdouble) + cv.astype(np.longdouble) * np.longdouble(P)).astype(np.float64)
    assert len(off) == 0 or min(off) > 1e-9, "an input sits on a rounding tie"
    held = np.maximum(np.searchsorted(v, np.arange(n), side="right") - 1, 0)
    y = yv[held]
    return (y if fill == "hold" else np.where(valid, y, np.nan)), cv[held]


@pytest.fixture(params=[1, 2], ids=["series", "tiled"])
def path(request):
    from deepfmkit_amd import _lib
    lib = _lib.load()
    _lib.check(lib.dfmi_set_tuning(b"unwrap_path", request.param), "dfmi_set_tuning")
    yield request.param
    lib.dfmi_set_tuning(b"unwrap_path", 0)


@pytest.mark.parametrize("kind", ["ramp", "walk"])
@pytest.mark.parametrize("N", SIZES, ids=lambda n: f"N={n}")
def test_sizes(path, N, kind):
    import torch
    from deepfmkit_amd import unwrap
    x, P = series(kind, N)
    y, c = unwrap(torch.from_numpy(x).cuda(), period=P, cycles=True)
    ry, rc = reference(x, P, np.ones(N, dtype=bool), "nan")
    assert np.array_equal(c.cpu().numpy(), rc)
    if N > 2 * T + 1:
        assert np.all(np.abs(y.cpu().numpy() - ry) <= np.spacing(np.abs(ry)))
    else:
        assert y.cpu().numpy().tobytes() == ry.tobytes()
    assert kind == "walk" or abs(rc).max() >= N // 8


@pytest.mark.parametrize("fill", ["nan", "hold"])
@pytest.mark.parametrize("how", ["status", "nan", "inf"])
@pytest.mark.parametrize("gap", list(GAPS))
def test_gaps(path, gap, how, fill):
    import torch
    from deepfmkit_amd import unwrap
    N = 2 * T + 1
    x, P = series("ramp", N)
    st = np.zeros(N, dtype=np.int32)
    st[5] = 1  # a retried fit is still valid at max_status = 1
    if how == "status":
        st[GAPS[gap]] = 2
    else:
        x[GAPS[gap]] = np.nan if how == "nan" else np.inf
    y, c = unwrap(torch.from_numpy(x).cuda(), period=P, status=torch.from_numpy(st).cuda(), fill=fill, cycles=True)
    ry, rc = reference(x, P, np.isfinite(x) & (st <= 1), fill)
    assert np.array_equal(c.cpu().numpy(), rc)
    assert np.array_equal(y.cpu().numpy(), ry, equal_nan=True)
    assert y.cpu().numpy()[np.isfinite(ry)].tobytes() == ry[np.isfinite(ry)].tobytes()


@pytest.mark.parametrize("nser", [1, 3])
def test_batches_rows_at_an_odd_stride_and_host_memory(path, nser):
    """Rows at ser_stride > N from an odd offset (the single-load path) give each series the bits
    it has alone on aligned rows, and a DFMI_MEM_HOST call gives the device call's bits."""
    import torch
    from deepfmkit_amd import unwrap
    N, stride = 2 * T + 1, 2 * T + 4
    rows = np.stack([series("ramp", N)[0], series("walk", N)[0], series("ramp", N)[0][::-1]])[:nser]
    st = np.zeros((nser, N), dtype=np.int32)
    st[:, T - 1:T + 1] = 2
    buf = torch.zeros(1 + nser * stride, dtype=torch.float64, device="cuda")
    xs = buf[1:].as_strided((nser, N), (stride, 1))
    xs.copy_(torch.from_numpy(rows))
    assert xs.data_ptr() % 16 == 8
    y, c = unwrap(xs, period=1.0, status=torch.from_numpy(st).cuda(), fill="hold", cycles=True)
    hy, hc = unwrap(rows, period=1.0, status=st, fill="hold", cycles=True)
    assert y.cpu().numpy().tobytes() == hy.tobytes() and np.array_equal(c.cpu().numpy(), hc)
    for r in range(nser):
        y1, c1 = unwrap(torch.from_numpy(rows[r]).cuda(), period=1.0, status=torch.from_numpy(st[r]).cuda(),
                        fill="hold", cycles=True)
        assert y1.cpu().numpy().tobytes() == hy[r].tobytes() and np.array_equal(c1.cpu().numpy(), hc[r])
    ry, rc = reference(rows[0], 1.0, st[0] <= 1, "hold")
    assert hy[0].tobytes() == ry.tobytes() and np.array_equal(hc[0], rc)


def test_facade_unwraps_a_fitted_ramp_across_a_failed_buffer():
    """64 buffers of R = 400 at L = 200 whose phase ramps 0.9 rad per buffer, one buffer replaced by
    noise (fitok 2). phi_unwrapped follows the ramp up to one multiple of 2 pi within twice the
    fit's own error (the same fit's phi against the wrapped truth; printed)."""
    import deepfmkit_amd as dfm
    from deepfmkit_amd import series as S
    nbuf, R, bad = 64, 400, 30
    rng = np.random.RandomState(7)
    t = np.arange(nbuf * R) / 200000.0
    truth = 0.9 * np.arange(nbuf)
    x = 1.6 * (1 + np.cos(np.repeat(truth, R) + 6.0 * np.cos(2 * np.pi * 1000.0 * t + 0.3))) + 1e-3 * rng.randn(nbuf * R)
    x[bad * R:(bad + 1) * R] = rng.randn(R)
    dff = dfm.DeepFitFramework()
    raw = dfm.DeepRawObject(x)
    raw.label, raw.f_samp, raw.f_mod, raw.t0 = "r", 200000.0, 1000.0, 0.0
    dff.raws["r"] = raw
    fit = dff.fit("r", n=2)
    fitok = dff.fits_df["r_nls"]["fitok"].to_numpy()
    good = fitok <= 1
    assert fitok[bad] == 2 and good[0] and not np.any(~good[1:] & ~good[:-1])  # single-buffer gaps: steps below pi
    err = np.abs((fit.phi - truth + np.pi) % (2 * np.pi) - np.pi)[good].max()
    print(f"fit error of phi against the wrapped truth: {err:.3e} rad over {good.sum()} of {nbuf} buffers")
    out = dff.unwrap()
    assert out["r_nls"] is fit.phi_unwrapped and np.isnan(fit.phi_unwrapped[bad])
    d = (fit.phi_unwrapped - truth)[good]
    assert np.abs(d - 2 * np.pi * np.rint(d[0] / (2 * np.pi))).max() <= 2 * err
    assert fit.phi_unwrapped.tobytes() == S.unwrap(np.asarray(fit.phi, dtype=np.float64), status=fitok).tobytes()
    dff.unwrap(fill="hold")
    dff.calc_lpsd(which="phi_unwrapped")
    assert np.all(np.isfinite(fit.Sxx)) and fit.Sxx.size > 0
