"""Overlapped segments (dfmi_demod_hop, dfmi_nls_record_hop, nls_records(hop=), fit(hop=)): segment s of a
record is x[s*hop : s*hop + R]. The definition is the planar typed call on the gathered copy of the windows.
int16 records must give its bits (integer sums are exact in any order), on demod_hop_kernel ("demod_hop" = 1)
and on the planar kernels in place (0); float records are held to a long-double restatement of the reference.
Records: the package's snr generator, two records that differ, in a padded even rec_stride; int16 =
clamp(round(4096 x)), the L = 128 ones with -32768 / 32767 forced into the first, a middle and the last block.
Short segments would send the planar call through demod_wide_kernel (other last bits): `bins` pins the bin kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F_SAMP, SCALE, PAD = 200000.0, 4096.0, 6
GRID = [(L, k, V) for L in (128, 200, 256) for k in (1, 3) for V in (2, 4, 8)]  # nslot 1 / masked lanes / nslot 2
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


@pytest.fixture
def span3():
    yield from _tuned(b"demod_hop_span", 3, 0)


@pytest.fixture(params=[1, 0], ids=["native", "inplace"])
def path(request):
    yield from _tuned(b"demod_hop", request.param, 1)


def records(dtype, L, n, hop=0):
    """(2, n) records of `dtype` on the GPU, a view with row stride n + PAD; made once per shape."""
    import torch
    from deepfmkit_amd.physics import SnrSpec, synth_snr
    key = (dtype, L, n, hop)
    if key not in _CACHE:
        x = torch.empty((2, n + PAD), dtype=torch.float64, device="cuda")
        for r in range(2):
            synth_snr(SnrSpec(seed=50 + r, f_samp=F_SAMP, f_mod=F_SAMP / L, amp=0.7 + 0.2 * r, m=5.0 + r, phi=0.9 * r,
                              snr_db=40.0), 0, n, out=x[r, :n])
        if dtype == "int16":
            x = torch.clamp(torch.round(SCALE * x), -32768, 32767).to(torch.int16)
            for t in (0, (n // (2 * hop)) * hop + 3, n - 2) if hop else ():  # both parities
                x[:, t], x[:, t + 1] = -32768, 32767
        _CACHE[key] = x.to(getattr(torch, dtype))[:, :n]
    return _CACHE[key]


def gather(x, nseg, R, hop):
    return x.unfold(1, R, hop)[:, :nseg].reshape(x.shape[0], nseg * R).contiguous()


def demod(x, nseg, R, nd, L, hop=None):
    """dfmi_demod_hop on the records / dfmi_demod_typed on a gathered copy -> (qi, dc, kernel)."""
    import torch
    from deepfmkit_amd import _lib
    from deepfmkit_amd.fitters import _xtype, w0_of
    lib, ntot = _lib.load(), x.shape[0] * nseg
    qi, dc = torch.zeros((2 * nd, ntot), dtype=torch.float64, device="cuda"), torch.zeros(ntot, dtype=torch.float64, device="cuda")
    tail = (nd, w0_of(F_SAMP / L, F_SAMP), 0, qi.data_ptr(), dc.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
    if hop:
        rc = lib.dfmi_demod_hop(x.data_ptr(), _xtype(x.dtype), x.shape[0], x.stride(0), nseg, R, hop, *tail)
    else:
        rc = lib.dfmi_demod_typed(x.data_ptr(), _xtype(x.dtype), ntot, R, R, *tail)
    assert rc == 0, lib.dfmi_last_error()
    return qi.cpu().numpy(), dc.cpu().numpy(), lib.dfmi_last_demod_kernel().decode()


def fit(x, nseg, R, nd, L, hop=None, **kw):
    from deepfmkit_amd import _lib
    from deepfmkit_amd.fitters import nls_records
    g = np.array([[(0.7 + 0.2 * r) * (SCALE if "int16" in str(x.dtype) else 1.0), 6.0, 0.0, 0.0] for r in range(2)])
    res = nls_records(x, F_SAMP, F_SAMP / L, R, nseg, nd, init_guess=g, hop=hop, **kw)
    return [r.cpu().numpy() for r in res], _lib.load().dfmi_last_demod_kernel().decode()


def on_path(kern, planar, native, tag):
    if native:
        assert kern.startswith("demod_hop_kernel<") and tag in kern, kern
    else:  # the planar call's own kernel (the record call fuses the seed into its launch: another name)
        assert kern == planar + " [hop in place]" or (
            kern.endswith(" [hop in place]") and planar.startswith("demod_seed_bins_kernel")), (kern, planar)


def same_bits(x, nseg, R, nd, L, hop, native, tag, **kw):
    y = gather(x, nseg, R, hop)
    for got, want in ((demod(x, nseg, R, nd, L, hop), demod(y, nseg, R, nd, L)),
                      (fit(x, nseg, R, nd, L, hop, **kw), fit(y, nseg, R, nd, L, **kw))):
        for a, b in zip(got[0] if len(got) == 2 else got[:2], want[0] if len(want) == 2 else want[:2]):
            np.testing.assert_array_equal(a, b)
        on_path(got[-1], want[-1], native, tag)


@pytest.mark.parametrize("L,k,V", GRID)
def test_int16_bits_of_the_planar_call(L, k, V, path, bins, span3):
    """nseg 1, 2, V and 2 G + 1 at G = 3: one segment, fewer than a span, a short last span."""
    hop, R = k * L, V * k * L
    x = records("int16", L, 7 * hop + R, hop if L == 128 else 0)  # 8 windows
    for nseg, nd, kw in ((1, 10, {}), (2, 3, dict(parallel=False)), (V, 3, {}), (7, 10, {}), (7, 10, dict(parallel=False))):
        same_bits(x, nseg, R, nd, L, hop, bool(path), f"[i16 int, V={V}]", **kw)


@pytest.mark.parametrize("dtype,tag", [("float64", "f64"), ("float32", "f32"), ("int16", "i16 int")])
def test_span_independence(dtype, tag):
    """QI and dc do not depend on how the records were cut into spans (0: the host's choice; enough segments
    that it is not 1)."""
    from deepfmkit_amd import _lib
    L, nseg = 128, 40001
    x, res = records(dtype, L, (nseg + 1) * L), []
    for span in (1, 3, 0):
        _lib.check(_lib.load().dfmi_set_tuning(b"demod_hop_span", span), "tune")
        res.append(demod(x, nseg, 2 * L, 10, L, L))
        assert res[-1][2].startswith("demod_hop_kernel<") and f"[{tag}, V=2]" in res[-1][2]
    for q, d, _ in res[1:]:
        np.testing.assert_array_equal(q, res[0][0])
        np.testing.assert_array_equal(d, res[0][1])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("L,k,V", GRID)
def test_float_against_long_double(L, k, V, dtype, span3):
    """QI_h = mean(x cos / sin(h w0 t)), dc = mean(x) of every window in np.longdouble (calculate_quadratures
    restated). Bounds: tests/test_gpu_demod_wide.py's against its restatement, 1e-12 on QI and 1e-13 on dc
    of a unit-scale record."""
    from deepfmkit_amd.fitters import w0_of
    hop, R, nseg, nd = k * L, V * k * L, 7, 10
    x = records(dtype, L, 6 * hop + R)
    qi, dc, kern = demod(x, nseg, R, nd, L, hop)
    assert kern.startswith("demod_hop_kernel<"), kern
    w = gather(x, nseg, R, hop).cpu().numpy().astype(np.longdouble).reshape(2 * nseg, R)
    t, w0 = np.arange(R, dtype=np.longdouble), np.longdouble(w0_of(F_SAMP / L, F_SAMP))
    ref = np.array([(w * f((h + 1) * w0 * t)).mean(axis=1) for f in (np.cos, np.sin) for h in range(nd)])
    eq, ed = float(np.abs(qi - ref).max()), float(np.abs(dc - w.mean(axis=1)).max())
    print(f"L={L} hop={hop} V={V} {dtype}: QI err {eq:.2e}, dc err {ed:.2e}")
    assert eq <= 1e-12 and ed <= 1e-13


@pytest.mark.parametrize("V", [2, 4, 8])
def test_fit_level_float64(V):
    """R = 4000, L = 200, 300 segments at 40 dB: the six columns within DESIGN.md §7's flat 1e-9 of the planar
    call on the gathered copy, fitok equal. hop = 500 (V = 8) is no whole number of periods: in place, same bits."""
    R, L, nseg = 4000, 200, 300
    hop = R // V
    x = records("float64", L, (nseg - 1) * hop + R)
    (gc, gok), kern = fit(x, nseg, R, 10, L, hop)
    (wc, wok), planar = fit(gather(x, nseg, R, hop), nseg, R, 10, L)
    on_path(kern, planar, V != 8, f"[f64, V={V}]")
    err = float(np.abs(gc - wc).max())
    print(f"V={V}: max column difference {err:.2e}")
    assert err <= 1e-9
    np.testing.assert_array_equal(gok, wok)


@pytest.mark.parametrize("dtype", ["int16", "float64"])
@pytest.mark.parametrize("R,hop,nd", [(400, 202, 10), (600, 200, 10), (400, 200, 20)],
                         ids=["hop-not-periods", "V3", "ndata20"])
def test_fallback_in_place(R, hop, nd, dtype):
    """What demod_hop_kernel does not take runs the planar kernels in place: the definition's bits."""
    same_bits(records(dtype, 200, 6 * hop + R), 7, R, nd, 200, hop, False, "")


def test_facade():
    import deepfmkit_amd as dfm
    from deepfmkit_amd.fitters import nls_records
    dff, laser, ifo = dfm.DeepFitFramework(), dfm.LaserConfig(), dfm.InterferometerConfig()
    dfm.set_laser_df_for_effect(laser, ifo, 6.0)
    dff.load_sim(dfm.DFMIObject("ch", laser, ifo, f_samp=F_SAMP))
    dff.simulate("ch", n_seconds=0.2, mode="snr", snr_db=40.0, trial_num=0)
    plain = dff.fit("ch", n=20, fit_label="plain")
    R, hop = plain.R, plain.R // 4
    fit_ = dff.fit("ch", n=20, hop=hop, fit_label="slide")
    x = dff.raws["ch"].samples()
    nseg = (x.shape[0] - R) // hop + 1
    assert (fit_.nbuf, fit_.hop, fit_.R, fit_.fs) == (nseg, hop, R, F_SAMP / hop) and len(fit_.time) == nseg
    cols, ok = nls_records(x.reshape(1, -1), F_SAMP, 1000.0, R, None, hop=hop)
    cols = cols.cpu().numpy() if hasattr(cols, "cpu") else cols
    for i, k in enumerate(("amp", "m", "phi", "psi", "dc", "ssq")):
        np.testing.assert_array_equal(getattr(fit_, k), cols[i])
        assert np.abs(getattr(fit_, k)[::4] - getattr(plain, k)).max() <= 1e-9, k
    with pytest.raises(ValueError, match="nls"):
        dff.fit("ch", method="ekf", n=20, hop=hop)
