"""dfmi_residual on the GPU against its definition in numpy.longdouble, and fit(residuals=True).

Definition (include/dfmi.h): theta_t = w0 t + psi from the double w0 and exact t, ac(t) =
a cos(phi + m cos(theta_t)), k = dc - mean(ac), r(t) = x(t) - k - ac(t); rss = sum r^2,
peak = max |r|, ipeak its t.

Per-sample gate (derived, not measured):
    g = 1e-11 |a m| + 8 eps (|a m| (1 + theta_max) + |a| + max|x| + |dc|)
First term: the periodic route evaluates the model at t mod L, and dfmi_detect_period accepts an
L whose angle error accumulated over the segment is at most 1e-11; d ac / d theta is bounded by
|a m|. It is 0 on the non-periodic route. Second term, first-order rounding with a margin of 8:
the angle w0 t + psi is rounded at size theta_max (eps theta_max, times |a m|), the inner cosine
and its product with m at eps |m| (times |a|), the outer cosine and its product at eps |a|, k
and the two subtractions at eps (|dc| + |a| + max|x|). theta_max = w0 (L - 1) + |psi| on the
periodic route, w0 (R - 1) + |psi| otherwise. From it: |d r| <= g, |d rss| <= 2 g sqrt(R rss) +
R g^2, |d peak| <= g, |r_ref[ipeak]| >= peak_ref - 2 g.
DFMI_GATE_DIR=<dir> writes the worst ratio per case to <dir>/gate_ratios.txt (the recorded run:
profiles/residual/gate_ratios.txt)."""
import itertools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import deepfmkit_amd as dfm  # noqa: E402
from deepfmkit_amd import _lib, fitters  # noqa: E402

EPS, SENT, LD = np.finfo(float).eps, 7.25, np.longdouble


@pytest.fixture(scope="module")
def ratios():  # the worst ratio per case; written out after the module when DFMI_GATE_DIR is set
    seen = {}
    yield seen
    d = os.environ.get("DFMI_GATE_DIR")
    if d and seen:
        with open(os.path.join(d, "gate_ratios.txt"), "w") as f:
            f.write("# dfmi_residual: worst ratio to the gate per case (<= 1 passes), MI355X\n")
            f.writelines(f"{k}: ratio {r:.3g}\n" for k, r in sorted(seen.items()))
            f.write(f"worst: {max(seen.values()):.3g}\n")


def reference(x, w0, p, dc):
    """(r, rss, peak) of the segments x (nseg, R) in longdouble."""
    t = np.arange(x.shape[1], dtype=LD)[None, :]
    a, m, phi, psi = (p[i].astype(LD)[:, None] for i in range(4))
    ac = a * np.cos(phi + m * np.cos(LD(w0) * t + psi))
    r = x.astype(LD) - (dc.astype(LD)[:, None] - ac.mean(axis=1, keepdims=True)) - ac
    return r, (r * r).sum(axis=1), np.abs(r).max(axis=1)


def record(fs, fm, R, nseg, stride, dtype=np.float64, a=1.6, m=6.0, spike=None, seed=3):
    """x (flat, (nseg-1)*stride + R samples of dtype), the (4, nseg) parameters, dc and w0: one
    modulated record plus white noise of 1e-3 |a| (int16: |a| = 1000 counts), and per segment
    the parameters that describe it at the segment's local time."""
    rs = np.random.RandomState(seed)
    w0 = fitters.w0_of(fm, fs)
    a = a * (1000.0 if dtype == np.int16 else 1.0)
    n = (nseg - 1) * stride + R
    p = np.array([np.full(nseg, a), np.full(nseg, m), np.full(nseg, 0.7),
                  np.mod(0.1 + w0 * stride * np.arange(nseg), 2 * np.pi)])
    x = 1.1 * abs(a) + a * np.cos(0.7 + m * np.cos(w0 * np.arange(n) + 0.1))
    x += rs.normal(0.0, 1e-3 * abs(a), n)
    if spike is not None:
        x[spike] += abs(a)  # 1e3 times the noise
    x = np.round(x).astype(dtype) if dtype == np.int16 else x.astype(dtype)
    seg = np.lib.stride_tricks.sliding_window_view(x, R)[::stride][:nseg]
    return x, p, seg.astype(np.float64).mean(axis=1), w0


def call(x, xtype, nseg, stride, R, w0, period, p, dc, device=True, want=(1, 1, 1, 1), pad=0, xoff=0, roff=0):
    """One dfmi_residual call with x, params (ld = nseg + pad) and guarded outputs (resid_stride =
    R + 2 pad) in host or device memory; the outputs as numpy with their guards checked."""
    put = (lambda v: torch.from_numpy(v).cuda()) if device else (lambda v: v)
    ld, rstr = nseg + pad, R + 2 * pad
    xb = put(np.concatenate([np.zeros(8 + xoff, x.dtype), x]))
    blk = np.full((5, ld), np.nan)
    blk[:4, :nseg], blk[4, :nseg] = p, dc
    pb = put(blk)
    bufs = [put(np.full(nseg + 4, SENT)), put(np.full(nseg + 4, SENT)), put(np.full(nseg + 4, -77, dtype=np.int32)),
            put(np.full(nseg * rstr + 4 + roff, SENT))]
    lead = [2, 2, 2, 2 + roff]
    ptrs = [_lib.ptr(b) + k * (b.element_size() if device else b.itemsize) if w else None
            for b, k, w in zip(bufs, lead, want)]
    rc = _lib.load().dfmi_residual(_lib.ptr(xb) + (8 + xoff) * x.itemsize, xtype, nseg, stride, R, w0, period,
                                   _lib.ptr(pb), ld, _lib.ptr(pb) + 4 * ld * 8, *ptrs, rstr,
                                   _lib.DFMI_MEM_DEVICE if device else _lib.DFMI_MEM_HOST, None)
    _lib.check(rc, "dfmi_residual")
    torch.cuda.synchronize()
    out = []
    for i, (b, k, w, n) in enumerate(zip(bufs, lead, want, (nseg, nseg, nseg, nseg * rstr))):
        h = b.cpu().numpy() if device else b
        sent = -77 if h.dtype == np.int32 else SENT
        body = h[k:k + n]
        if i == 3:
            body = body.reshape(nseg, rstr)
            assert (body[:, R:] == sent).all()  # between the residual rows
            body = body[:, :R]
        assert (h[:k] == sent).all() and (h[k + n:] == sent).all()
        assert w or (body == sent).all()  # a NULL output is not written
        out.append(body if w else None)
    return out


def check(name, ratios, x, dtype, nseg, stride, R, w0, period, p, dc, **kw):
    xtype = {np.float64: _lib.DFMI_F64, np.float32: _lib.DFMI_F32, np.int16: _lib.DFMI_I16}[dtype]
    rss, peak, ipeak, resid = call(x, xtype, nseg, stride, R, w0, period, p, dc, **kw)
    seg = np.lib.stride_tricks.sliding_window_view(x, R)[::stride][:nseg]
    r, rss_ref, peak_ref = reference(seg, w0, p, dc)
    L = period if period > 0 else _lib.load().dfmi_detect_period(w0, R, 1) if period == 0 else 0  # <= 1024
    am = np.abs(p[0] * p[1])
    th = w0 * ((L if L else R) - 1) + np.abs(p[3])
    g = (1e-11 * am if L else 0.0) + 8 * EPS * (am * (1 + th) + np.abs(p[0]) + np.abs(seg).max(axis=1) + np.abs(dc))
    ratio = [np.abs(resid - r).max(axis=1) / g, np.abs(rss - rss_ref) / (2 * g * np.sqrt(R * rss_ref) + R * g * g),
             np.abs(peak - peak_ref) / g, (peak_ref - np.abs(r[np.arange(nseg), ipeak])) / (2 * g)]
    worst = float(np.max(ratio))
    ratios[name] = max(worst, ratios.get(name, 0.0))
    print(f"{name}: ratios to the gate (dr, drss, dpeak, ipeak)", [f"{v.max():.3g}" for v in ratio])
    assert worst <= 1.0, ratio
    return rss, peak, ipeak, resid, g


CASES = {  # fs, fm, R, nseg, stride (None: R), period, keywords of record() and call()
    "base": (200e3, 1e3, 4000, 5, None, 0, {}),
    "R4012": (200e3, 1e3, 4012, 5, None, 0, {}),
    "R130": (200e3, 1e3, 130, 5, None, 0, {}),
    "R50": (200e3, 1e3, 50, 5, None, 0, {}),
    "R1": (200e3, 1e3, 1, 5, None, 0, {}),
    "L75": (30e3, 400.0, 1500, 5, None, 0, {}),
    "L1024": (1024.0, 5.0, 2500, 5, None, 1024, {}),
    "xoff1": (200e3, 1e3, 4000, 5, None, 0, dict(xoff=1, roff=1)),
    "oddstride": (200e3, 1e3, 4000, 5, 4001, 0, {}),
    "overlap": (200e3, 1e3, 4000, 5, 1000, 0, {}),
    "np401": (200e3, 997.0, 401, 5, None, 0, {}),
    "np4012": (200e3, 997.0, 4012, 5, None, 0, {}),
    "np_forced": (200e3, 1e3, 4000, 5, None, -1, {}),
    "grid": (200e3, 1e3, 200, 5000, None, 0, {}),
    "m31": (200e3, 1e3, 4000, 5, None, 0, dict(m=31.4)),
    "aneg": (200e3, 1e3, 4000, 5, None, 0, dict(a=-1.6)),
    "mneg": (200e3, 1e3, 4000, 5, None, 0, dict(m=-6.0)),
    "layout": (200e3, 1e3, 1000, 5, None, 0, dict(pad=3)),
}


# every case in float64; float32 and int16 where the sample type changes the load path
TYPED = [(n, np.float64) for n in CASES] + [(n, d) for n in ("base", "R130", "xoff1", "np401", "overlap")
                                            for d in (np.float32, np.int16)]


@pytest.mark.parametrize("name,dtype", TYPED, ids=[f"{n}-{np.dtype(d).name}" for n, d in TYPED])
def test_against_the_definition(name, dtype, ratios):
    fs, fm, R, nseg, stride, period, kw = CASES[name]
    stride = R if stride is None else stride
    rkw, ckw = ({k: kw[k] for k in ks if k in kw} for ks in (("a", "m"), ("pad", "xoff", "roff")))
    spike = min(2 * stride + (3 * R) // 7, (nseg - 1) * stride + R - 1)  # inside segment 2 (and its neighbours' overlap)
    x, p, dc, w0 = record(fs, fm, R, nseg, stride, dtype, spike=spike if R > 1 else None, **rkw)
    rss, peak, ipeak, resid, g = check(f"{name}/{np.dtype(dtype).name}", ratios, x, dtype, nseg, stride, R, w0, period,
                                       p, dc, **ckw)
    if R > 1:
        assert ipeak[2] == spike - 2 * stride  # the planted outlier, exactly
    if name == "np_forced":  # the two evaluators on one record
        other = call(x, _lib.DFMI_F64, nseg, stride, R, w0, 0, p, dc)
        assert (np.abs(other[3] - resid).max(axis=1) <= 2 * g).all() and (np.abs(other[1] - peak) <= 2 * g).all()
    if dtype != np.float64:  # the widened record gives the same bits
        wide = call(x.astype(np.float64), _lib.DFMI_F64, nseg, stride, R, w0, period, p, dc, **ckw)
        for ours, theirs in zip((rss, peak, ipeak, resid), wide):
            assert np.array_equal(ours, theirs)
    host = call(x, {np.float64: 0, np.float32: 1, np.int16: 3}[dtype], nseg, stride, R, w0, period, p, dc, device=False,
                **ckw)
    for ours, theirs in zip((rss, peak, ipeak, resid), host):
        assert np.array_equal(ours, theirs)


def test_null_outputs_and_a_nan_parameter():
    x, p, dc, w0 = record(200e3, 1e3, 130, 3, 130)
    full = call(x, 0, 3, 130, 130, w0, 0, p, dc, pad=2)
    for want in itertools.product((0, 1), repeat=4):
        if any(want):
            got = call(x, 0, 3, 130, 130, w0, 0, p, dc, pad=2, want=want)
            assert all(g is None or np.array_equal(g, f) for g, f in zip(got, full))
    for row in range(5):  # amp, m, phi, psi, dc of segment 1
        q, d = p.copy(), dc.copy()
        (q[row] if row < 4 else d)[1] = np.nan if row % 2 else np.inf
        for period in (0, -1):
            rss, peak, ipeak, resid = call(x, 0, 3, 130, 130, w0, period, q, d)
            assert np.isnan(rss[1]) and np.isnan(peak[1]) and ipeak[1] == -1 and np.isnan(resid[1]).all()
            ref = call(x, 0, 3, 130, 130, w0, period, p, dc)
            for ours, theirs in zip((rss, peak, ipeak, resid), ref):
                assert np.array_equal(ours[[0, 2]], theirs[[0, 2]])


def test_facade_residual_columns():
    R, nbuf = 4000, 200
    dff = dfm.DeepFitFramework()
    t = np.arange(R * nbuf)
    sigma = 1.6 / np.sqrt(2.0) * 10 ** (-40.0 / 20.0)  # 40 dB below the carrier's rms
    y = 1.0 + 1.6 * np.cos(0.7 + 6.0 * np.cos(fitters.w0_of(1000.0, 200000.0) * t + 0.1))
    y += np.random.RandomState(11).normal(0.0, sigma, t.size)
    y[57 * R + 1234] += 50 * sigma
    raw = dfm.DeepRawObject()
    raw.data = torch.from_numpy(y).cuda()
    raw.label, raw.f_samp, raw.f_mod, raw.t0 = "c", 200000.0, 1000.0, 0.0
    dff.raws["c"] = raw
    dff.fit("c", n=20, ndata=10, fit_label="plain")
    fit = dff.fit("c", n=20, ndata=10, fit_label="res", residuals=True, errors=True)
    d0, d1 = dff.fits_df["plain"], dff.fits_df["res"]
    base = ["amp", "m", "phi", "psi", "dc", "ssq", "fitok"]
    assert list(d1.columns)[:14] == base + fitters.ERR_COLUMNS + fitters.RES_COLUMNS
    assert all(np.array_equal(d0[k].to_numpy(), d1[k].to_numpy()) for k in base)
    assert all(d1[k].dtype == np.float64 and np.array_equal(getattr(fit, k), d1[k].to_numpy()) for k in fitters.RES_COLUMNS)
    clean = np.arange(nbuf) != 57
    assert (np.abs(fit.res_rms[clean] / sigma - 1.0) <= 5 / np.sqrt(2 * R)).all()
    assert np.argmax(fit.res_peak) == 57 and fit.res_peak_t[57] == 1234.0
    r = dff.residual("res")
    alone = fitters.residual_record(raw.data, 200000.0, 1000.0, R, np.stack([fit.amp, fit.m, fit.phi, fit.psi]), fit.dc)
    assert r.is_cuda and r.shape == (nbuf, R) and torch.equal(r, alone)
