"""CPU dry run of the multi-record / warm-start-chain parity matrix
(tests/test_gpu_record_matrix.py): the matrix's own inputs (tests/helpers/record_matrix.py)
through the host build of the product's LM (tests/hostcheck, hc_fit_segments) in a Python chain
loop that feeds every fit's result to the next guess, on the oracle's QI, held to the matrix's
gate (conftest.compare_fit at record_tol, status equal on every buffer). It shows without a GPU
that the chosen inputs do not sit on a rounding-decided stop for the product's arithmetic: a
GPU failure of the matrix is then an indexing / staging discrepancy, not the inputs.

And the condition the inputs were chosen for: the oracle re-run on its own QI perturbed by
1e-15 relative keeps every status and stays inside the same gate. If either test fails for a
seed, change record_matrix.seed_of or the noise-only placement, never the gate."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import compare_fit, record_tol

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import record_matrix as M  # noqa: E402

HC = os.path.join(os.path.dirname(__file__), "hostcheck", "libhostcheck.so")
CONSTS = np.array([100, 1e-9, 1e-9, 1e-3, 5.0, 30.0, 0.5, 0.05, 0.1, 1e-15])
LAMBDAS = np.array([0.0, 1e-7, 1e-5, 1e-3, 1e-1, 1.0, 10.0, 100.0])
# (mode, alt): the four distinct chunkings of the matrix (n_cores = 40 and the default cut the
# same chunks), and the sequential mode from the second guess table (record_matrix.alt_guesses)
HOST_CASES = (("seq", False), (3, False), (5, False), (None, False), ("seq", True))


def _case_id(case):
    return M.mode_id(case[0]) + ("-alt" if case[1] else "")


def _guesses(nd, alt):
    return M.alt_guesses(nd) if alt else M.records(nd)[1]


@pytest.fixture(scope="module")
def hc():
    if not os.path.exists(HC):
        pytest.skip("hostcheck not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(HC)
    P = ctypes.c_void_p
    lib.hc_fit_segments.argtypes = [P, ctypes.c_long, ctypes.c_int, P, P, P, ctypes.c_int, P, P, P, ctypes.c_int]
    return lib


def _host_chains(hc, qi, nd, chunks, guess, res, base, form):
    """record_matrix.oracle_chains with the product's fit: one hc_fit_segments call per segment
    (n = 1: its 2 nd QI values are the component-major layout), the result the next guess."""
    p, ssq, st = np.zeros(4), np.zeros(1), np.zeros(1, np.int32)
    for ch in chunks:
        g = np.array(guess, dtype=np.float64)
        for i in ch:
            q = np.ascontiguousarray(qi[base + i])
            hc.hc_fit_segments(q.ctypes.data, 1, nd, g.ctypes.data, CONSTS.ctypes.data, LAMBDAS.ctypes.data, 8,
                               p.ctypes.data, ssq.ctypes.data, st.ctypes.data, form)
            g = p.copy()
            res[base + i] = (p[0], p[1], p[2], p[3], ssq[0], st[0])


def _host_fit(hc, nd, mode, alt, form):
    qi, dc = M.cached_qi(nd)
    g = _guesses(nd, alt)
    res = np.zeros((M.NREC * M.NBUF, 6))
    first, chunks = M.chunks_of(mode, M.NBUF)
    for r in range(M.NREC):
        base = r * M.NBUF
        if first:
            _host_chains(hc, qi, nd, [np.arange(1)], g[r], res, base, form)
            _host_chains(hc, qi, nd, chunks, res[base, :4].copy(), res, base, form)
        else:
            _host_chains(hc, qi, nd, chunks, g[r], res, base, form)
    return dict(amp=res[:, 0], m=res[:, 1], phi=res[:, 2], psi=res[:, 3], dc=dc, ssq=res[:, 4],
                fitok=res[:, 5].astype(np.int32))


@pytest.mark.parametrize("case", HOST_CASES, ids=_case_id)
@pytest.mark.parametrize("nd", M.NDATAS)
def test_host_lm_chains_meet_the_matrix_gate(hc, nd, case):
    """force_general 0 (the register path up to 16 harmonics: exact-ndata at 10, masked 12 / 16)
    and 1 (the literal general path) for ndata <= 16; 1, 3 (many-harmonic, kWideNd) and 4 (one
    walk per trial, kWideNdF) beyond."""
    mode, alt = case
    ref = M.cached_oracle(nd, mode, alt=alt)
    tol = record_tol(nd, ref["qi"], ref)
    # the m = 20 record: through the m-grid seed from m = 6, straight from its own m = 20.2
    assert ref["fitok"][M.GRID_RECORD * M.NBUF] == (0 if alt else 1)
    assert abs(ref["m"][M.GRID_RECORD * M.NBUF] - 20.0) < 1e-2
    for r, b in M.NOISE_ONLY.items():
        assert ref["fitok"][r * M.NBUF + b] != 0
    for form in ((0, 1) if nd <= 16 else (1, 3, 4)):
        ours = _host_fit(hc, nd, mode, alt, form)
        compare_fit(ours, ref, tol=tol, min_status_match=1.0)
        print(f"host ndata={nd} {_case_id(case)} force_general={form}: max |d amp, m, phi, psi| =",
              [f"{v:.2e}" for v in M.max_deltas(ours, ref)])


@pytest.mark.parametrize("case", HOST_CASES, ids=_case_id)
@pytest.mark.parametrize("nd", M.NDATAS)
def test_oracle_is_stable_under_qi_rounding(nd, case):
    """The oracle against itself with every QI value moved by 1e-15 relative (+- at random, a
    few ulps: more than any summation order moves it): every status kept, status-0 fits inside
    the gate. Where this failed, a GPU comparison at 1e-9 would be decided by the oracle's last
    bits, not by the kernels."""
    mode, alt = case
    ref = M.cached_oracle(nd, mode, alt=alt)
    qi, dc = M.cached_qi(nd)
    sign = np.random.RandomState(77 + nd).choice([-1.0, 1.0], qi.shape)
    again = M.fits_from_qi(qi * (1.0 + 1e-15 * sign), dc, nd, mode, _guesses(nd, alt), M.NBUF)
    np.testing.assert_array_equal(again["fitok"], ref["fitok"])
    compare_fit(again, ref, tol=record_tol(nd, qi, ref), min_status_match=1.0)
    print(f"oracle ndata={nd} {_case_id(case)} under 1e-15 QI changes: max |d amp, m, phi, psi| =",
          [f"{v:.2e}" for v in M.max_deltas(again, ref)])
