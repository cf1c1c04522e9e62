"""The windowed record call (dfmi_nls_record_window, fitters.nls_records(window=)) over every path of
nls_record_window_device, against the numpy oracle driven over the long-double windowed QI.

Records and reference: tests/helpers/window_ref.py (9 records of 7 buffers of R = 800, ndata 10,
40 dB, a guess of its own per record; tests/test_window_matrix_host.py shows on the CPU that every
oracle status is 0 and stays 0 under a 1e-15 change of the QI). The long-double windowed QI and dc of
every segment go through helpers.record_matrix.fits_from_qi (the oracle's chains in the call's mode)
and the result is compared with conftest.compare_fit at its defaults with record_tol: status equal on
every segment, status-0 parameters within max(1e-9, resolution), dc relative 1e-13, ssq relative 1e-6.
Outputs are filled with sentinels before every call and none may survive.

Matrix: windows hann / blackmanharris; modes parallel=False, n_cores = 3, default; layouts
    contig  the flat path (rec_stride == nbuf hop)
    pad2    records padded by 2 samples: the per-record loop, qi written at qi + r nbuf
    pad1    padded by 1: the loop with VEC 2 for the even records and VEC 1 (<1,4>) for the odd ones
    hop400  hop = 400 on the contiguous records: the loop with overlapped segments
    long400 hop = 400 on one record of 63 segments: the flat path with overlapped segments
(9 records: the device guess table of nrec > 8; padding samples are NaN). float64 everywhere; float32
and int16 for contig and pad1 at the default mode (int16 in counts, guess amplitude and status
threshold in counts too: window_ref.fitok_scale). Overlapping records (a strided view of one array with
rec_stride == nbuf hop < (nbuf - 1) hop + R) are refused with DFMI_ERR_ARG, as include/dfmi.h documents;
that refusal is asserted.

Same bits: record r of the 9-record call against the call on record r alone from the same address;
records 0-2 of 9 against the 3-record call (inline guesses); host memory against device memory;
fitters.nls_records against the ABI call."""
import os
import sys

import numpy as np
import pytest

from conftest import compare_fit, record_tol

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import window_ref as W  # noqa: E402

COLS = ("amp", "m", "phi", "psi", "dc", "ssq", "fitok")
LAYOUTS = {"contig": ("rec800", 0), "pad2": ("rec800", 2), "pad1": ("rec800", 1), "hop400": ("rec400", 0),
           "long400": ("long400", 0)}
_DEV = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not pytest.importorskip("torch").cuda.is_available():
        pytest.skip("no GPU")
    yield
    _DEV.clear()


def layout(name, dtype="float64", host=False):
    """(array kept alive, base address, record stride in samples, itemsize, mem)."""
    import torch
    from deepfmkit_amd import _lib
    key = (name, dtype, host)
    if key not in _DEV:
        dataset, pad = LAYOUTS[name]
        if dataset == "long400":
            flat, stride = np.array(W.long_record(dtype)), W.LONG_N
        else:
            x = W.records(dtype)
            stride = x.shape[1] + pad
            flat = np.full(W.NREC * stride, np.nan) if dtype != "int16" else np.full(W.NREC * stride, -32768)
            flat = flat.astype(dtype)
            for r in range(W.NREC):
                flat[r * stride:r * stride + x.shape[1]] = x[r]
        if host:
            _DEV[key] = (flat, flat.ctypes.data, stride, flat.itemsize, _lib.DFMI_MEM_HOST)
        else:
            t = torch.from_numpy(flat).cuda()
            assert t.data_ptr() % 16 == 0
            _DEV[key] = (t, t.data_ptr(), stride, flat.itemsize, _lib.DFMI_MEM_DEVICE)
    return _DEV[key]


def nchunk_of(mode, nbuf):
    # fitters.nls_records: n_cores None -> nbuf - 1, else min(n_cores, nbuf), at least 1
    return 1 if mode == "seq" else max(1, nbuf - 1 if mode is None else min(int(mode), nbuf))


def call(name, dtype, window, mode, rec0=0, nrec=None, host=False, stride=None, check=True):
    """One dfmi_nls_record_window call on records [rec0, rec0 + nrec) of a layout -> (result dict,
    last demodulation kernel)."""
    import torch
    from deepfmkit_amd import _lib
    from deepfmkit_amd import fit as F
    from deepfmkit_amd.fitters import _xtype
    lib = _lib.load()
    dataset = LAYOUTS[name][0]
    nrec_all, nbuf, hop = W.shape_of(dataset)
    nrec = nrec_all if nrec is None else nrec
    _, base, rec_stride, itemsize, mem = layout(name, dtype, host)
    rec_stride = rec_stride if stride is None else stride
    nseg = nrec * nbuf
    g = np.ascontiguousarray(W.mode_guesses(dataset, dtype)[rec0:rec0 + nrec])
    a = W.coefs(window)
    cfg = F.lm_config()
    cfg.fitok_threshold = cfg.fitok_threshold * W.fitok_scale(dtype)
    if host:
        out, ok, st = np.full((6, nseg), np.nan), np.full(nseg, -7, dtype=np.int32), None
    else:
        out = torch.full((6, nseg), float("nan"), dtype=torch.float64, device="cuda")
        ok = torch.full((nseg,), -7, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
    rc = lib.dfmi_nls_record_window(base + itemsize * rec0 * rec_stride, _xtype(np.dtype(dtype)), nrec, rec_stride, nbuf,
                                    W.R, hop, W.ND, W.W0, 0, _lib.ptr(a), a.size, _lib.ptr(g),
                                    0 if mode == "seq" else 1, nchunk_of(mode, nbuf), cfg, _lib.ptr(out), _lib.ptr(ok),
                                    mem, st)
    if not check:
        return rc
    assert rc == 0, lib.dfmi_last_error()
    if not host:
        torch.cuda.synchronize()
        out, ok = out.cpu().numpy(), ok.cpu().numpy()
    assert not np.isnan(out).any(), ("output never written", np.argwhere(np.isnan(out))[:8].tolist())
    assert not (ok == -7).any(), ("status never written", np.where(ok == -7)[0][:8].tolist())
    res = dict(amp=out[0], m=out[1], phi=out[2], psi=out[3], dc=out[4], ssq=out[5], fitok=ok)
    return res, lib.dfmi_last_demod_kernel().decode()


def check(ours, dataset, dtype, window, mode, what, rec0=0, nrec=None):
    ref = W.oracle(dataset, dtype, window, mode)
    nbuf = W.shape_of(dataset)[1]
    assert (ref["fitok"] == 0).all()
    tol = record_tol(W.ND, ref["qi"], ref)
    if nrec is not None:
        keep = np.arange(rec0 * nbuf, (rec0 + nrec) * nbuf)
        ref, tol = {k: np.asarray(v)[keep] for k, v in ref.items()}, tol[keep]
    try:
        rep = compare_fit(ours, ref, tol=tol, min_status_match=1.0)
    except AssertionError as exc:
        raise AssertionError(f"{what}: {exc}") from exc
    print(f"{what}: worst parameter / tolerance {max(rep[k + '_over_tol'] for k in COLS[:4]):.3g}, dc relative "
          f"{rep['dc_rel']:.2e}")


def same_bits(a, b, what):
    for k in COLS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def rows(res, r0, n, nbuf=W.NBUF):
    return {k: v[r0 * nbuf:(r0 + n) * nbuf] for k, v in res.items()}


def mode_id(mode):
    return "seq" if mode == "seq" else "default" if mode is None else f"cores{mode}"


@pytest.mark.parametrize("mode", W.MODES, ids=mode_id)
@pytest.mark.parametrize("window", W.WINDOWS)
def test_float64_layouts_vs_oracle(window, mode):
    K = len(W.coefs(window)) - 1
    for name, (dataset, _) in LAYOUTS.items():
        ours, kern = call(name, "float64", window, mode)
        # the last launch: the whole batch, or record 8 alone (an even offset in every layout)
        assert kern == W.kernel_name(2, 2, K, "float64"), (name, kern)
        check(ours, dataset, "float64", window, mode, f"{name} {window} {mode_id(mode)} ({kern})")
        if dataset == "long400":
            continue
        # inline guesses (nrec <= 8), and a record of the batch against the record alone
        few, _ = call(name, "float64", window, mode, 0, 3)
        same_bits(rows(ours, 0, 3), few, f"{name}: records 0-2 of 9 against the 3-record call")
        for r in (4, 5):
            alone, k1 = call(name, "float64", window, mode, r, 1)
            odd = name == "pad1" and r % 2 == 1  # record 5 of pad1 starts at an odd sample: no pairs
            assert k1 == (W.kernel_name(1, 4, K, "float64") if odd else W.kernel_name(2, 2, K, "float64")), (name, r, k1)
            check(alone, dataset, "float64", window, mode, f"{name} record {r} alone ({k1})", r, 1)
            same_bits(rows(ours, r, 1), alone, f"{name}: record {r} of 9 against the record alone")


@pytest.mark.parametrize("name", ["contig", "pad1"])
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("window", W.WINDOWS)
def test_typed_records_vs_oracle(window, dtype, name):
    K = len(W.coefs(window)) - 1
    ours, kern = call(name, dtype, window, None)
    assert kern == W.kernel_name(2, 2, K, dtype), kern
    check(ours, "rec800", dtype, window, None, f"{name} {dtype} {window} ({kern})")
    alone, k1 = call(name, dtype, window, None, 5, 1)
    assert k1 == W.kernel_name(*((1, 4) if name == "pad1" else (2, 2)), K, dtype), k1
    same_bits(rows(ours, 5, 1), alone, f"{name} {dtype}: record 5 of 9 against the record alone")
    if dtype == "int16":
        assert np.all(np.abs(ours["amp"] / W.I16_SCALE / (0.9 * np.repeat(1.0 + 0.05 * np.arange(W.NREC), W.NBUF)) - 1) < 0.05)


@pytest.mark.parametrize("name,dtype", [("contig", "float64"), ("pad1", "float64"), ("hop400", "float64"),
                                        ("pad1", "float32"), ("pad1", "int16")])
def test_host_memory_gives_the_device_bits(name, dtype):
    for mode in ("seq", None):
        dev, kd = call(name, dtype, "blackmanharris", mode)
        host, kh = call(name, dtype, "blackmanharris", mode, host=True)
        assert kd == kh
        same_bits(dev, host, f"{name} {dtype} {mode_id(mode)}: host against device memory")


def test_overlapping_records_are_refused():
    """nrec > 1 with rec_stride == nbuf hop = 2800 < (nbuf - 1) hop + R = 3200 (include/dfmi.h)."""
    from deepfmkit_amd import _lib
    rc = call("hop400", "float64", "hann", None, stride=W.NBUF * W.HOP, check=False)
    err = _lib.load().dfmi_last_error()
    assert rc == -1 and b"rec_stride" in err, (rc, err)


@pytest.mark.parametrize("hop", [None, W.HOP])
def test_nls_records_is_the_abi_call(hop):
    """fitters.nls_records(window=) with per-record guesses on a device tensor (contiguous, and a
    padded view: rec_stride from the tensor) and on a host array: the bits of the direct call."""
    import torch
    from deepfmkit_amd.fitters import nls_records
    g = W.guesses()
    for mode, kw in (("seq", dict(parallel=False)), (3, dict(n_cores=3)), (None, {})):
        for name in ("contig", "pad1") if hop is None else ("hop400",):
            want, _ = call(name, "float64", "blackmanharris", mode)
            t, _, stride, _, _ = layout(name)
            view = t.view(W.NREC, stride)[:, :W.NBUF * W.R]
            cols, ok = nls_records(view, W.F_SAMP, W.F_MOD, W.R, W.NBUF, W.ND, init_guess=g, hop=hop,
                                   window="blackmanharris", **kw)
            torch.cuda.synchronize()
            got = dict(zip(COLS, list(cols.cpu().numpy()) + [ok.cpu().numpy()]))
            same_bits(got, want, f"nls_records {name} {mode_id(mode)} (device)")
        cols, ok = nls_records(W.records(), W.F_SAMP, W.F_MOD, W.R, W.NBUF, W.ND, init_guess=g, hop=hop,
                               window="blackmanharris", **kw)
        want, _ = call("contig" if hop is None else "hop400", "float64", "blackmanharris", mode)
        same_bits(dict(zip(COLS, list(cols) + [ok])), want, f"nls_records {mode_id(mode)} (host)")
