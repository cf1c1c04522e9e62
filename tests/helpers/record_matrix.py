"""Inputs and numpy-oracle results of the multi-record / warm-start-chain parity matrix
(tests/test_gpu_record_matrix.py on the GPU, tests/test_record_matrix_host.py through the host
build of lm.h). Plain numpy: no GPU, no process pool (the oracle runs in the calling process from
O.demod_buffer and O.fit_segment, so nothing is forked after HIP is initialised).

Records (build_records): nrec = 9 records of nbuf = 23 buffers of R = 4000 samples at 200 kHz /
1 kHz (basis period L = 200), record r = A_r (1 + 0.9 cos(phi_r + m_r cos(2 pi f_mod t + psi_r)))
+ 0.01 noise with A_r = 1 + 0.05 r, m_r = linspace(5, 7, 9), phi_r = 0.25 r - 1, psi_r = 0.02 r,
and a per-record guess (A_r, m_r +- 0.4 alternating, 0, 0), so a guess read from another record
shows. Record 4 is m = 20 (phi 0.3, psi 0.05, amplitude 1.3) guessed at m = 6: its buffer 0 fails
from the guess and comes back from the m-grid seed with status 1. Buffer 7 of records 0, 3 and 8
is noise only at sigma = 3.0 (status != 0; in a chain the buffer after it starts from a bad
point). sigma = 3.0 and psi_r = 0.02 r keep the oracle's own statuses stable under a 1e-15
relative change of its QI (tests/test_record_matrix_host.py asserts it): at sigma = 0.8 some
noise-only buffers reach status 0 at ndata 7 / 10 on a fit decided by the last bits of ssq.

Call modes (MODES): "seq" is one warm-start chain per record (parallel=False); an integer is
n_cores of _fit_parallel (np.array_split chunks of buffers 1.., seeded by the record's buffer-0
fit, fitters.py:395-428); None is the default, every buffer its own chunk.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import nls_oracle as O  # noqa: E402

NREC, NBUF, R = 9, 23, 4000
F_SAMP, F_MOD = 200000.0, 1000.0
W0 = 2.0 * np.pi * F_MOD / F_SAMP
NDATAS = (7, 10, 12, 16, 20, 30, 62)
# 23 = 2 x 8 + 7 (the ladder's 8-segment staging tail); 22 = 8 + 7 + 7 = 5 + 5 + 4 + 4 + 4;
# 40 clamps to chunk size 1; None: the default (chunk size 1)
MODES = ("seq", 3, 5, 40, None)
NOISE_ONLY = {0: 7, 3: 7, 8: 7}  # record -> its noise-only buffer
NOISE_SIGMA = 3.0
GRID_RECORD = 4  # m = 20 guessed at 6: buffer 0 takes the m-grid seed
COLS = ("amp", "m", "phi", "psi", "dc", "ssq", "fitok")


def mode_id(mode):
    return "seq" if mode == "seq" else "default" if mode is None else f"cores{mode}"


def seed_of(nd):
    return 4100 + nd


def build_records(nd):
    """(x (NREC, NBUF * R) float64 contiguous, guesses (NREC, 4)) for harmonic count nd. The
    noise is np.random.RandomState(seed_of(nd)), whose stream numpy keeps frozen."""
    rs = np.random.RandomState(seed_of(nd))
    noise = rs.standard_normal((NREC, NBUF * R))
    t = np.arange(NBUF * R) / F_SAMP
    amp = 1.0 + 0.05 * np.arange(NREC)
    m = np.linspace(5.0, 7.0, NREC)
    phi = 0.25 * np.arange(NREC) - 1.0
    psi = 0.02 * np.arange(NREC)
    g = np.zeros((NREC, 4))
    g[:, 0] = amp
    g[:, 1] = m + 0.4 * np.where(np.arange(NREC) % 2 == 0, 1.0, -1.0)
    amp[GRID_RECORD], m[GRID_RECORD], phi[GRID_RECORD], psi[GRID_RECORD] = 1.3, 20.0, 0.3, 0.05
    g[GRID_RECORD] = (1.3, 6.0, 0.0, 0.0)
    x = np.empty((NREC, NBUF * R))
    for r in range(NREC):
        x[r] = amp[r] * (1.0 + 0.9 * np.cos(phi[r] + m[r] * np.cos(2.0 * np.pi * F_MOD * t + psi[r]))) + 0.01 * noise[r]
    for r, b in NOISE_ONLY.items():
        x[r, b * R:(b + 1) * R] = NOISE_SIGMA * noise[r, b * R:(b + 1) * R]
    return x, g


def alt_guesses(nd):
    """A second guess table for the sequential mode, where a guess read from another record
    changes a STATUS (the plain table's guesses all lead a clean record to its own minimum, so a
    swapped guess moves a fit by ~1e-12 only): the m = 20 record starts at m = 20.2 and reaches
    status 0 from its own guess, status 1 (m-grid retry) from any other record's; every other
    record reaches status 0 from its own guess and status 1 from the m = 20 record's."""
    g = np.array(records(nd)[1])
    g[GRID_RECORD] = (1.3, 20.2, 0.0, 0.0)
    return g


def chunks_of(mode, nbuf):
    """(first, chunks): the index arrays of one record's warm-start chains, in buffer order.
    first = True: buffer 0 is fitted from the record's guess and ITS result seeds every chain
    (fitters.py:403-421); False: the chains start from the record's guess itself."""
    if mode == "seq":
        return False, [np.arange(nbuf)]
    n_cores = min(nbuf - 1 if mode is None else int(mode), nbuf)
    if nbuf <= 1:
        return True, []
    return True, [c for c in np.array_split(np.arange(1, nbuf), n_cores) if c.size]


def demod_records(x, nd, nbuf):
    """The oracle's QI (nrec * nbuf, 2 nd) and dc (nrec * nbuf,) of the first nbuf buffers."""
    nrec = x.shape[0]
    qi = np.empty((nrec * nbuf, 2 * nd))
    dc = np.empty(nrec * nbuf)
    for r in range(nrec):
        for b in range(nbuf):
            buf = x[r, b * R:(b + 1) * R]
            qi[r * nbuf + b] = O.demod_buffer(buf, nd, W0)
            dc[r * nbuf + b] = np.mean(buf)
    return qi, dc


def oracle_chains(qi, nd, chunks, guess, out, base=0):
    """Warm-start chains (fitters.py:13-60) over rows base + chunk of qi, each from `guess`;
    fills out[base + i] = (amp, m, phi, psi, ssq, status)."""
    for ch in chunks:
        g = np.array(guess, dtype=np.float64)
        for i in ch:
            st, p, ssq = O.fit_segment(nd, qi[base + i], g)
            g = p
            out[base + i] = (p[0], p[1], p[2], p[3], ssq, st)


def fits_from_qi(qi, dc, nd, mode, guesses, nbuf):
    """The oracle's record fit from given QI: the dict conftest.compare_fit takes (flat arrays
    over nrec * nbuf, record-major) plus "qi" for conftest.record_tol."""
    nrec = qi.shape[0] // nbuf
    res = np.zeros((nrec * nbuf, 6))
    first, chunks = chunks_of(mode, nbuf)
    for r in range(nrec):
        base = r * nbuf
        if first:
            oracle_chains(qi, nd, [np.arange(1)], guesses[r], res, base)
            oracle_chains(qi, nd, chunks, res[base, :4].copy(), res, base)
        else:
            oracle_chains(qi, nd, chunks, guesses[r], res, base)
    return dict(amp=res[:, 0].copy(), m=res[:, 1].copy(), phi=res[:, 2].copy(), psi=res[:, 3].copy(), dc=dc.copy(),
                ssq=res[:, 4].copy(), fitok=res[:, 5].astype(np.int32), qi=qi)


def oracle_fit(x, nd, mode, guesses, nbuf=None):
    """The numpy oracle on records x (nrec, >= nbuf * R) in call mode `mode`."""
    nbuf = x.shape[1] // R if nbuf is None else nbuf
    qi, dc = demod_records(x, nd, nbuf)
    return fits_from_qi(qi, dc, nd, mode, guesses, nbuf)


_RECORDS, _QI, _FITS = {}, {}, {}


def records(nd):
    if nd not in _RECORDS:
        x, g = build_records(nd)
        x.setflags(write=False)
        g.setflags(write=False)
        _RECORDS[nd] = (x, g)
    return _RECORDS[nd]


def cached_qi(nd, nbuf=NBUF):
    """The oracle QI / dc of records(nd), shared by every mode (read-only)."""
    if nd not in _QI:
        qi, dc = demod_records(records(nd)[0], nd, NBUF)
        qi.setflags(write=False)
        dc.setflags(write=False)
        _QI[nd] = (qi, dc)
    qi, dc = _QI[nd]
    if nbuf == NBUF:
        return qi, dc
    keep = (np.arange(NREC)[:, None] * NBUF + np.arange(nbuf)[None, :]).ravel()
    return qi[keep], dc[keep]


def cached_oracle(nd, mode, nbuf=NBUF, alt=False):
    """oracle_fit(records(nd)) per (nd, chunking, nbuf, guess table), computed once per process
    and shared read-only. Modes that cut the same chunks (n_cores >= nbuf - 1 and the default)
    share one. alt: from alt_guesses(nd) instead of the records' own table."""
    first, chunks = chunks_of(mode, nbuf)
    key = (nd, nbuf, first, tuple(len(c) for c in chunks), bool(alt))
    if key not in _FITS:
        qi, dc = cached_qi(nd, nbuf)
        fit = fits_from_qi(qi, dc, nd, mode, alt_guesses(nd) if alt else records(nd)[1], nbuf)
        for v in fit.values():
            v.setflags(write=False)
        _FITS[key] = fit
    return _FITS[key]


def take_records(fit, recs, nbuf=NBUF):
    """The rows of records `recs` out of a record-major result dict."""
    keep = (np.asarray(recs)[:, None] * nbuf + np.arange(nbuf)[None, :]).ravel()
    return {k: np.asarray(v)[keep] for k, v in fit.items()}


def max_deltas(ours, ref):
    """max |d amp|, |d m|, wrapped |d phi|, |d psi| over the fits both sides call status 0."""
    ok = (np.asarray(ours["fitok"]) == 0) & (np.asarray(ref["fitok"]) == 0)
    if not ok.any():
        return [0.0] * 4
    d = []
    for k in ("amp", "m", "phi", "psi"):
        v = np.abs(np.asarray(ours[k]) - np.asarray(ref[k]))
        if k == "phi":
            v = np.abs((np.asarray(ours[k]) - np.asarray(ref[k]) + np.pi) % (2 * np.pi) - np.pi)
        d.append(float(v[ok].max()))
    return d
