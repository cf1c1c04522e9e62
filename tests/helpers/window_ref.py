"""The long-double definition of the windowed demodulation (dfmi_demod_window), the signals, the
instance table and the record set of the window matrix (tests/test_gpu_window_matrix.py and
tests/test_gpu_window_records.py on the GPU; tests/test_window_matrix_host.py validates this module
on the CPU). Plain numpy: no GPU, nothing forked.

Definition, for an (n, R) block of segments and coefficients a_0..a_K:
    w[t] = sum_m a_m cos(2 pi m t / R),   w_h = longdouble(float64(h w0)),
    Q_h = sum_t w x cos(w_h t) / sum_t w,   I_h with sin,   dc = sum_t w x / sum_t w,
all in np.longdouble. The window's angle is reduced exactly first (m t mod R is an integer), so
its error is one rounding of an angle below 2 pi; `brute` evaluates the same definition sample by
sample with no reduction, and the host test holds the two to 1e-16.

Gates (tests/test_gpu_window.py): max |dQI| <= 1e-12 max|x|, dc relative
<= 1e-13. Every signal here is positive with a mean of order 1 (1.6 (1 + 0.9 cos(..)) + 1 % noise,
minimum 0.16 less the noise), so the relative dc gate is well conditioned; int16 is that signal in
counts (x 6000: within +-20000).

Instances (INSTANCES): demod_window_kernel<VEC, MAXSLOT> [type, K] for VEC 1 / 2, MAXSLOT 2 / 4,
K 1 / 2 / 3 (hann, blackman, blackmanharris), float64 / float32 / int16: 36 rows, each with the
shape that reaches it under the rules of demod_window_device (expected_instance below):
    <2,2>: L = 200, stride R + 1 (even);   <2,4>: L = 400, same rule;
    <1,2>: L = 75 (odd period);            <1,4>: L = 200 at an odd segment stride;
R = 5 L + 3 everywhere: the unrolled loop (UNR = 4 at MAXSLOT 2, 2 at MAXSLOT 4), the single-cycle
tail and the ragged last cycle all run.

Records (section "record set"): 9 records of 7 buffers of R = 800 at 200 kHz / 1 kHz (4 periods a
buffer, more than K = 3), ndata 10, record r = A_r (1 + 0.9 cos(phi_r + m_r cos(w0 t + psi_r))) +
0.01 noise (40 dB) with tests/helpers/record_matrix.py's A_r, m_r, phi_r, psi_r and its guesses
(A_r, m_r +- 0.4 alternating, 0, 0); no m-grid record and no noise-only buffer, so every oracle
status is 0. Three segmentations: "rec800" (disjoint buffers), "rec400" (hop = 400 on the same
records) and "long400": ONE record of 63 segments at hop = 400 (one signal with a slow phase
drift, one guess). Records that overlap (nrec > 1 at rec_stride = nbuf hop < (nbuf - 1) hop + R)
are refused by the interface (DFMI_ERR_ARG, include/dfmi.h), so a single record is the only way
to the flat demodulation path with overlapped segments."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

LD = np.longdouble
PI = 4 * np.arctan(LD(1))
QI_GATE, DC_GATE = 1e-12, 1e-13
TAG = {"float64": "f64", "float32": "f32", "int16": "i16"}
DTYPES = ("float64", "float32", "int16")
WINDOW_OF_K = {1: "hann", 2: "blackman", 3: "blackmanharris"}
I16_SCALE = 6000.0


def coefs(window):
    """float64 coefficients of a window name or a coefficient sequence (the package's own table)."""
    from deepfmkit_amd import _lib
    return _lib.window_coefficients(window)


def weights(R, window):
    """w[t], t < R, in long double from exactly reduced angles."""
    t = np.arange(R, dtype=np.int64)
    w = np.zeros(R, dtype=LD)
    for m, a in enumerate(coefs(window)):
        w += LD(a) * np.cos(2 * PI * ((m * t) % R).astype(LD) / LD(R))
    return w


def reference(segs, window, nd, w0):
    """(n, R) segments -> QI (2 nd, n), dc (n,) of the definition, in long double."""
    x = np.asarray(segs).astype(LD)
    t = np.arange(x.shape[1], dtype=LD)
    w = weights(x.shape[1], window)
    sw = w.sum()
    wh = [LD(np.float64((h + 1) * w0)) for h in range(nd)]
    qi = np.array([(x * (w * f(v * t))).sum(axis=1) / sw for f in (np.cos, np.sin) for v in wh])
    return qi, (x * w).sum(axis=1) / sw


def brute(seg, window, nd, w0):
    """One segment, sample by sample, every angle formed as written (no reduction): QI (2 nd,), dc."""
    a = [LD(v) for v in coefs(window)]
    R = len(seg)
    wh = [LD(np.float64((h + 1) * w0)) for h in range(nd)]
    sw, sx, q, i = LD(0), LD(0), [LD(0)] * nd, [LD(0)] * nd
    for t in range(R):
        w = LD(0)
        for m, am in enumerate(a):
            w += am * np.cos(2 * PI * LD(m) * LD(t) / LD(R))
        wx = w * LD(seg[t])
        sw += w
        sx += wx
        for h in range(nd):
            q[h] += wx * np.cos(wh[h] * LD(t))
            i[h] += wx * np.sin(wh[h] * LD(t))
    return np.array(q + i) / sw, sx / sw


def errors(qi, dc, segs, window, nd, w0):
    """(QI error / max|x|, dc relative error) of a result (2 nd, n), (n,) against `reference`."""
    rq, rd = reference(segs, window, nd, w0)
    eq = float(np.abs(np.asarray(qi) - rq).max() / np.abs(np.asarray(segs).astype(LD)).max())
    ed = float(np.abs((np.asarray(dc) - rd) / rd).max())
    return eq, ed


def signal(n, w0, dtype="float64", seed=1, noise=0.01, phi=0.4, drift=3e-5, psi=0.3, m=6.0):
    t = np.arange(n)
    x = 1.6 * (1 + 0.9 * np.cos(phi + drift * t + m * np.cos(w0 * t + psi)))
    x = x + noise * np.random.RandomState(seed).randn(n)
    return np.round(x * I16_SCALE).astype(np.int16) if dtype == "int16" else x.astype(dtype)


def strided(x, nseg, stride, R):
    """The (nseg, R) segments of a 1-D array at `stride`."""
    return np.stack([x[s * stride:s * stride + R] for s in range(nseg)])


# ---- the instance table ----

def expected_instance(L, stride, base_aligned=True):
    """(VEC, MAXSLOT) of demod_window_device: vec2_ok = L even, stride even, base aligned to a
    sample pair; MAXSLOT 2 while ceil(L / (64 VEC)) <= 2, else 4."""
    vec = 2 if (L % 2 == 0 and stride % 2 == 0 and base_aligned) else 1
    return vec, (2 if -(-L // (64 * vec)) <= 2 else 4)


def kernel_name(vec, ms, K, dtype):
    return f"demod_window_kernel<{vec},{ms}> [{TAG[dtype]}, K={K}]"


def _even_up(n):
    return n + (n & 1)


# (VEC, MAXSLOT) -> (L, stride as a function of R)
SHAPES = {(2, 2): (200, lambda R: _even_up(R + 1)), (2, 4): (400, lambda R: _even_up(R + 1)),
          (1, 2): (75, lambda R: R), (1, 4): (200, lambda R: _even_up(R + 1) + 1)}
NSEG = 5


def _instances():
    rows = []
    for (vec, ms), (L, stride_of) in SHAPES.items():
        R = 5 * L + 3
        for K in (1, 2, 3):
            for dt in DTYPES:
                rows.append(dict(vec=vec, ms=ms, K=K, dtype=dt, L=L, R=R, stride=stride_of(R), window=WINDOW_OF_K[K],
                                 nd=10))
    return rows


INSTANCES = _instances()


def instance_id(row):
    return f"v{row['vec']}-ms{row['ms']}-K{row['K']}-{TAG[row['dtype']]}"


def instance_input(row):
    """The 1-D sample array of an instance row: NSEG segments of R at the row's stride (the gaps
    hold samples of the same signal), and w0 = 2 pi / L."""
    w0 = 2 * np.pi / row["L"]
    n = (NSEG - 1) * row["stride"] + row["R"]
    return signal(n, w0, row["dtype"], seed=row["L"] + row["K"]), w0


# ---- the record set ----

NREC, NBUF, R, ND, HOP = 9, 7, 800, 10, 400
F_SAMP, F_MOD = 200000.0, 1000.0
W0 = 2.0 * np.pi * F_MOD / F_SAMP
WINDOWS = ("hann", "blackmanharris")
MODES = ("seq", 3, None)  # parallel=False, n_cores=3, the default (record_matrix.chunks_of)
DATASETS = ("rec800", "rec400", "long400")
LONG_N = (NREC - 1) * NBUF * HOP + (NBUF - 1) * HOP + R
_RECORDS, _REFS = {}, {}


def guesses(dtype="float64"):
    """(NREC, 4): (A_r, m_r +- 0.4 alternating, 0, 0); the amplitude in counts for int16."""
    r = np.arange(NREC)
    g = np.zeros((NREC, 4))
    g[:, 0] = (1.0 + 0.05 * r) * (I16_SCALE if dtype == "int16" else 1.0)
    g[:, 1] = np.linspace(5.0, 7.0, NREC) + 0.4 * np.where(r % 2 == 0, 1.0, -1.0)
    return g


def _typed(x, dtype):
    return np.round(x * I16_SCALE).astype(np.int16) if dtype == "int16" else x.astype(dtype)


def records(dtype="float64"):
    """(NREC, NBUF R) contiguous records of `dtype` (read-only, built once)."""
    if "x" not in _RECORDS:
        rs = np.random.RandomState(5150)
        t = np.arange(NBUF * R)
        r = np.arange(NREC)
        amp, m, phi, psi = 1.0 + 0.05 * r, np.linspace(5.0, 7.0, NREC), 0.25 * r - 1.0, 0.02 * r
        x = np.stack([amp[k] * (1.0 + 0.9 * np.cos(phi[k] + m[k] * np.cos(W0 * t + psi[k]))) for k in range(NREC)])
        _RECORDS["x"] = x + 0.01 * rs.standard_normal(x.shape)
    return _cached(("x", dtype), lambda: _typed(_RECORDS["x"], dtype))


def long_record(dtype="float64"):
    """(LONG_N,) one array for the strided view: record r = samples [2800 r, 2800 r + 3200)."""
    if "y" not in _RECORDS:
        t = np.arange(LONG_N)
        y = 1.2 * (1.0 + 0.9 * np.cos(0.3 + 5e-6 * t + 6.0 * np.cos(W0 * t + 0.05)))
        _RECORDS["y"] = y + 0.01 * np.random.RandomState(5151).standard_normal(LONG_N)
    return _cached(("y", dtype), lambda: _typed(_RECORDS["y"], dtype))


def _cached(key, make):
    if key not in _RECORDS:
        v = make()
        v.setflags(write=False)
        _RECORDS[key] = v
    return _RECORDS[key]


def segments(dataset, dtype="float64"):
    """(NREC NBUF, R) segments of a dataset, record-major."""
    if dataset == "long400":
        y = long_record(dtype)
        return np.stack([y[(r * NBUF + s) * HOP:(r * NBUF + s) * HOP + R] for r in range(NREC) for s in range(NBUF)])
    hop = R if dataset == "rec800" else HOP
    x = records(dtype)
    return np.stack([x[r, s * hop:s * hop + R] for r in range(NREC) for s in range(NBUF)])


def window_qi(dataset, dtype, window):
    """The long-double windowed QI (n, 2 ND) and dc (n,) of a dataset, rounded once to float64."""
    key = ("qi", dataset, dtype, window)
    if key not in _REFS:
        qi, dc = reference(segments(dataset, dtype), window, ND, W0)
        qi, dc = np.ascontiguousarray(qi.T.astype(np.float64)), dc.astype(np.float64)
        qi.setflags(write=False)
        dc.setflags(write=False)
        _REFS[key] = (qi, dc)
    return _REFS[key]


def mode_guesses(dataset, dtype):
    if dataset == "long400":  # one record: amplitude 1.2, m = 6 guessed at 6.4
        return np.array([[1.2 * (I16_SCALE if dtype == "int16" else 1.0), 6.4, 0.0, 0.0]])
    return guesses(dtype)


def shape_of(dataset):
    """(nrec, nbuf, hop) of a dataset."""
    return {"rec800": (NREC, NBUF, R), "rec400": (NREC, NBUF, HOP), "long400": (1, NREC * NBUF, HOP)}[dataset]


def fitok_scale(dtype):
    """int16 records are fitted in counts and ssq comes back in counts^2, so the status threshold
    (absolute, 1e-3) is stated in counts^2 on both sides, as tests/test_gpu_int16_records.py does:
    left at 1e-3 every int16 fit has status 2 and compare_fit would compare no parameter."""
    return I16_SCALE ** 2 if dtype == "int16" else 1.0


def _fits(qi, dc, mode, g, dtype, nbuf):
    import record_matrix as M
    from oracle import nls_oracle as O
    old = O.C0["FITOK_THRESHOLD"]
    O.C0["FITOK_THRESHOLD"] = old * fitok_scale(dtype)
    try:
        return M.fits_from_qi(qi, dc, ND, mode, g, nbuf)
    finally:
        O.C0["FITOK_THRESHOLD"] = old


def oracle(dataset, dtype, window, mode, qi=None):
    """record_matrix.fits_from_qi over the long-double windowed QI (or over `qi`, uncached): the
    dict conftest.compare_fit takes, with "qi" for conftest.record_tol."""
    key = ("fit", dataset, dtype, window, mode)
    if qi is not None:
        return _fits(qi, window_qi(dataset, dtype, window)[1], mode, mode_guesses(dataset, dtype), dtype,
                     shape_of(dataset)[1])
    if key not in _REFS:
        q, dc = window_qi(dataset, dtype, window)
        fit = _fits(q, dc, mode, mode_guesses(dataset, dtype), dtype, shape_of(dataset)[1])
        for v in fit.values():
            v.setflags(write=False)
        _REFS[key] = fit
    return _REFS[key]
