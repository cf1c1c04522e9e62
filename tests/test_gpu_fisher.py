"""dfmi_fisher on the GPU (csrc/fisher.hip) at the gates of tests/helpers/fisher_cases.py
against the numpy reference: point counts around the 64-lane block, parameter strides with
sentinel-guarded outputs, ndata on every Bessel / walk branch, negative and large |m|, the
points without an inverse, host and device memory (same bits), a side stream, every subset
of NULL outputs, per-point and shared variances; then helpers.py against the reference's
fixture. The host-build twin is tests/test_fisher_host.py.

Worst observed ratios to the gates on the MI355X: J^T J 0.737 (|m| = 150,
ndata 62; 0.08 below |m| = 64), sigma 0.0025, cov 0.0048."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import fisher_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from deepfmkit_amd import _lib, helpers  # noqa: E402

NMAX = 130
SENT = -7.25e77  # sentinel (exactly representable, never a result)


@functools.lru_cache(maxsize=None)
def points(ndata):
    """130 seeded points for `ndata` (m of both signs, |m| >= 64 at every 9th: the
    large-argument branch where 2 (ndata + 2) <= |m|), their per-point variances and the
    numpy reference, computed once."""
    rng = np.random.RandomState(1000 + ndata)
    p = np.array([rng.uniform(0.1, 3.0, NMAX), rng.uniform(-40.0, 40.0, NMAX), rng.uniform(-7.0, 7.0, NMAX),
                  rng.uniform(-3.2, 3.2, NMAX)])
    big = np.arange(0, NMAX, 9)
    p[1, big] = rng.uniform(64.0, 200.0, big.size) * np.where(big % 2, -1.0, 1.0)
    var = rng.uniform(1e-6, 1e-2, NMAX)
    p.setflags(write=False)
    var.setflags(write=False)
    return p, var, C.reference(p, ndata)


def call_host(p, n, ld, ndata, var, var_mul):
    lib = _lib.load()
    jtj, cov, sig = np.full((10, n), SENT), np.full((10, n), SENT), np.full((4, n), SENT)
    ok = np.full(n, -5, dtype=np.int32)
    pp = np.full((4, ld), np.nan)
    pp[:, :n] = p[:, :n]
    v = None if var is None else np.ascontiguousarray(var[:n])
    _lib.check(lib.dfmi_fisher(_lib.ptr(pp), n, ld, ndata, _lib.ptr(v), var_mul, _lib.ptr(jtj), _lib.ptr(cov),
                               _lib.ptr(sig), _lib.ptr(ok), _lib.DFMI_MEM_HOST, None), "dfmi_fisher")
    return jtj, cov, sig, ok


def call_device(p, n, ld, ndata, var, var_mul, outs=(1, 1, 1, 1), stream=None):
    """Device-memory call whose outputs live in ONE sentinel-filled block with 13-element guards
    between and after them; returns (rc, [jtj, cov, sig, ok as float block views], guards ok)."""
    lib = _lib.load()
    pp = np.full((4, ld), np.nan)
    pp[:, :n] = p[:, :n]
    dp = torch.from_numpy(pp).cuda()
    dv = None if var is None else torch.from_numpy(np.array(var[:n])).cuda()
    sizes = [10 * n, 10 * n, 4 * n, n]  # ok: n int32 in the first n/2 doubles of an n-double slot
    offs = np.cumsum([13] + [s + 13 for s in sizes])[:-1]
    block = torch.full((int(offs[-1] + sizes[-1] + 13),), SENT, dtype=torch.float64, device="cuda")
    ptrs = [block.data_ptr() + int(o) * 8 if on else None for o, on in zip(offs, outs)]
    st = stream if stream is not None else torch.cuda.current_stream()
    st.wait_stream(torch.cuda.current_stream())  # the block's fill and the uploads were enqueued there
    with torch.cuda.stream(st):
        rc = lib.dfmi_fisher(dp.data_ptr(), n, ld, ndata, None if dv is None else dv.data_ptr(), var_mul, *ptrs,
                             _lib.DFMI_MEM_DEVICE, st.cuda_stream)
    st.synchronize()
    h = block.cpu().numpy()
    if rc != 0:
        return rc, None, bool((h == SENT).all())
    res, clean = [], np.ones(h.size, bool)
    for k, (o, s, on) in enumerate(zip(offs, sizes, outs)):
        o = int(o)
        if not on:
            res.append(None)
            continue
        if k < 3:
            res.append(h[o:o + s].reshape(-1, n).copy())
            clean[o:o + s] = False
        else:
            res.append(h[o:o + s].view(np.int32)[:n].copy())
            clean[o:o + (n + 1) // 2] = False
            if n % 2:  # the upper half of the last touched double keeps the sentinel's bits
                assert h[o + n // 2:o + n // 2 + 1].view(np.int32)[1] == np.array([SENT]).view(np.int32)[1]
    untouched = bool((h[clean] == SENT).all())
    return rc, res, untouched


@pytest.mark.parametrize("ndata", [3, 8, 9, 10, 16, 17, 30, 62])
def test_counts_strides_and_memories(ndata):
    p, var, (A, X, cond) = points(ndata)
    worst = [0.0, 0.0, 0.0]
    full = call_host(p, NMAX, NMAX, ndata, var, 0.5)
    for n in (1, 63, 64, 65, 130):
        jtj, cov, sig, ok = call_host(p, n, n, ndata, var, 0.5)
        assert (ok == 1).all()
        v = var[:n] * 0.5
        for i, r in enumerate((C.ratio_jtj(jtj, A[:n]), C.ratio_sigma(sig, X[:n], cond[:n], v),
                               C.ratio_cov(cov, X[:n], cond[:n], v))):
            worst[i] = max(worst[i], r)
        # a lane's result does not depend on its neighbours, the stride or the memory kind
        for a, b in zip((jtj, cov, sig, ok), call_host(p, n, n + 13, ndata, var, 0.5)):
            assert np.array_equal(a, b)
        for ld in (n, n + 13):
            rc, res, untouched = call_device(p, n, ld, ndata, var, 0.5)
            assert rc == 0 and untouched
            for a, b in zip((jtj, cov, sig, ok), res):
                assert np.array_equal(a, b)
        assert all(np.array_equal(a, b[..., :n]) for a, b in zip((jtj, cov, sig, ok), full))
    print(f"gpu ndata {ndata}: jtj {worst[0]:.3g} sigma {worst[1]:.3g} cov {worst[2]:.3g}")
    assert max(worst) <= 1.0, worst
    # var == NULL: every point's factor is var_mul
    jtj, cov, sig, ok = call_host(p, NMAX, NMAX, ndata, None, 3e-5)
    assert np.array_equal(jtj, full[0])
    assert max(C.ratio_sigma(sig, X, cond, 3e-5), C.ratio_cov(cov, X, cond, 3e-5)) <= 1.0


def test_every_subset_of_null_outputs_on_a_side_stream():
    p, var, _ = points(10)
    n, ld = 65, 78
    side = torch.cuda.Stream()
    rc, full, untouched = call_device(p, n, ld, 10, var, 1.0, stream=side)
    assert rc == 0 and untouched
    for outs in itertools.product((0, 1), repeat=4):
        rc, res, untouched = call_device(p, n, ld, 10, var, 1.0, outs=outs, stream=side)
        assert untouched, outs  # nothing beyond n, nothing where an output is NULL
        if not any(outs[:3]):
            assert rc == -1  # DFMI_ERR_ARG, and (untouched) nothing was written
            continue
        assert rc == 0, outs
        for a, b, on in zip(full, res, outs):
            assert (b is None) == (not on)
            if on:
                assert np.array_equal(a, b), outs


def test_n_zero_launches_nothing():
    lib = _lib.load()
    out = np.full(4, SENT)
    assert lib.dfmi_fisher(None, 0, 0, 10, None, 1.0, None, None, _lib.ptr(out), None, _lib.DFMI_MEM_HOST, None) == 0
    assert (out == SENT).all()


@pytest.mark.parametrize("ndata", [3, 10, 17, 62])
def test_points_without_an_inverse(ndata):
    n = C.SINGULAR.shape[1]
    jtj, cov, sig, ok = call_host(C.SINGULAR, n, n, ndata, None, 1.0)
    C.check_singular(ok, sig, cov, jtj)
    rc, res, untouched = call_device(C.SINGULAR, n, n + 13, ndata, None, 1.0)
    assert rc == 0 and untouched
    C.check_singular(res[3], res[2], res[1], res[0])
    p = np.concatenate([C.REGULAR, C.REGULAR, C.REGULAR], axis=1)
    jtj, cov, sig, ok = call_host(p, 6, 6, ndata, np.array([1.0, np.inf, np.nan, 2.0, -1e-3, 0.0]), 1.0)
    assert list(ok) == [1, 0, 0, 1, 0, 1] and np.isnan(sig[:, [1, 2, 4]]).all() and np.isnan(cov[:, [1, 2, 4]]).all()
    assert np.isfinite(sig[:, [0, 3, 5]]).all() and (sig[:, 5] == 0).all() and (sig[:, [0, 3]] > 0).all()
    assert np.isfinite(jtj).all()


def test_fixture_random_points():
    wa = ws = wc = 0.0
    for nd, idx, p, (A, X, cond) in C.random_cases():
        r = helpers.fisher(p, nd, var_mul=2.5e-5, want=("jtj", "cov", "sigma"))
        assert (r["ok"] == 1).all(), nd
        wa = max(wa, C.ratio_jtj(r["jtj"], A))
        ws = max(ws, C.ratio_sigma(r["sigma"], X, cond, 2.5e-5))
        wc = max(wc, C.ratio_cov(r["cov"], X, cond, 2.5e-5))
    print(f"gpu fixture random points: jtj {wa:.3g} sigma {ws:.3g} cov {wc:.3g}")
    assert max(wa, ws, wc) <= 1.0, (wa, ws, wc)


def test_helpers_against_the_reference_fixture():
    g = C.golden()
    worst = 0.0
    for name, p, nd, var, expect, (A, X, cond) in C.grid_cases():
        snr = 80.0 if name.startswith("m80") else float(name.split("snr")[1])
        ours = helpers.calculate_m_precision(p[1], nd, snr)
        assert ours.shape == expect.shape
        worst = max(worst, float((np.abs(ours - expect) / expect / (C.GATE * (1 + cond))).max()))
        r = helpers.fisher(p, nd, var_mul=var, want=("jtj", "cov", "sigma"))
        assert (r["ok"] == 1).all()
        worst = max(worst, C.ratio_jtj(r["jtj"], A), C.ratio_sigma(r["sigma"], X, cond, var),
                    C.ratio_cov(r["cov"], X, cond, var))
    print(f"gpu grids (calculate_m_precision vs fixture, fisher vs numpy): worst ratio {worst:.3g}")
    assert worst <= 1.0
    wc = 0.0
    for (m, nd, snr, R), expect in zip(g["crlb_args"], g["crlb"]):
        ours = helpers.calculate_crlb_for_m(m, int(nd), snr, int(R))
        assert isinstance(ours, float)
        cond = C.reference(np.array([[1.0], [m], [0.0], [0.0]]), int(nd))[2][0]
        wc = max(wc, abs(ours - expect) / expect / (C.GATE * (1 + cond)))
    print(f"gpu calculate_crlb_for_m vs fixture: worst ratio {wc:.3g}")
    assert wc <= 1.0
    # no inverse: np.inf / np.nan, where the reference catches LinAlgError
    mp = helpers.calculate_m_precision(np.array([0.0, 6.0]), 10, 80.0)
    assert np.isinf(mp[0]) and np.isfinite(mp[1])
    cr = helpers.calculate_crlb_for_m(np.array([0.0, 6.0]), 10, 40.0, 200)
    assert np.isnan(cr[0]) and np.isfinite(cr[1]) and np.isnan(helpers.calculate_crlb_for_m(0.0, 10, 40.0, 200))


def test_binding_layouts_and_tensors():
    p, var, _ = points(10)
    a = helpers.fisher(p, 10, var=var, var_mul=0.5, want=("sigma", "cov"))
    b = helpers.fisher(np.ascontiguousarray(p.T), 10, var=var, var_mul=0.5, want=("cov", "sigma"))
    assert set(a) == {"sigma", "cov", "ok"} and all(np.array_equal(a[k], b[k]) for k in a)
    dp = torch.from_numpy(np.array(p)).cuda()
    for t in (dp, dp.t().contiguous(), torch.cat([dp, dp], dim=1)[:, :NMAX]):
        c = helpers.fisher(t, 10, var=torch.from_numpy(np.array(var)).cuda(), var_mul=0.5, want=("sigma", "cov"))
        assert all(c[k].is_cuda for k in c)
        assert all(np.array_equal(a[k], c[k].cpu().numpy()) for k in a)
    one_d = helpers.fisher(dp[:, 0], 10)  # a 1-D input of four values is one point, host or device
    assert one_d["sigma"].shape == (4, 1)
    assert np.array_equal(one_d["sigma"].cpu().numpy(), helpers.fisher(p[:, 0], 10)["sigma"])
    with pytest.raises(ValueError):
        helpers.fisher(dp[:3], 10)
    one = helpers.fisher(p[:, 0], 10)
    assert one["sigma"].shape == (4, 1) and one["sigma"][1, 0] == helpers.fisher(p[:, :1], 10)["sigma"][1, 0]
