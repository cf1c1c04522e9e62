"""Every call mode, record count, layout, harmonic class and LM launch form of the record
pipeline against the numpy oracle (oracle/nls_oracle.py), at the smallest shapes that reach
every branch of the index arithmetic in lm_chunks_kernel / lm_ladder_kernel (r = id / nchunk,
start = k qn + min(k, rm), s0 = r nbuf + first + start, the guess source, out_ld, the
first == 1 dc carry): a slip at a record boundary or at an uneven chunk boundary shifts a warm
start by one buffer and still produces plausible numbers, so only an independent reference
notices it.

Inputs and the oracle: tests/helpers/record_matrix.py (9 records of 23 buffers of R = 4000, a
distinct guess per record, an m = 20 record that takes the m-grid seed, noise-only buffers);
tests/test_record_matrix_host.py shows on the CPU that these inputs do not sit on a
rounding-decided stop.

The gate, everywhere: conftest.compare_fit(ours, oracle, tol=record_tol(nd, qi, oracle),
min_status_match=1.0): status equal on every buffer, status-0 fits within max(1e-9, resolution),
dc relative 1e-13, ssq relative 1e-6, with no exception rule (the _gn_step_check of
tests/test_gpu_full_scale.py is not used here: no fit needs it). Every output array is filled with a sentinel (NaN / -7) before each call and none may survive.

Axes. One test id = one (ndata, mode); inside it:
- records: all 9 (device guess table; 9 x nchunk items cross a wave boundary in every form), the
  first 3 (inline guesses), record 5 alone; for the odd stride also the first 4 (the last
  record's rows are then unaligned, so the call ends in the fold kernel);
- layout: contiguous; even padding (stride nbuf R + 6); odd padding (stride nbuf R + 7: the
  per-record demodulation, no rows, no wide kernel for the batch); a host array at the even
  stride (DFMI_MEM_HOST staging);
- LM form (dfmi_set_tuning): the default (the 8-lane ladder; beyond 16 harmonics the wave-split
  ladder, which is thereby held to the 1e-9 gate on noise-only and m-grid-retry buffers and in
  chains); lm_ladder = 0 (lm_chunks_kernel, CHAIN or not); beyond 16 harmonics lm_ladder_split = 0
  (the 8-lane ladder); lm_general = 1 at ndata 10 and 30.
The demodulation kernel family of every call is asserted from the rules of nls_record_device.

Bit-exact invariants (same bits): a record of a batch equals the same record fitted
alone (lm_ladder = 0 and the 8-lane ladder; contiguous and even layouts), contiguous equals
even-padded (every mode and form), the 8-lane ladder equals the one-lane kernel. The wave-split
form against the others and the odd stride against the others are held to the oracle gate only."""
import os
import sys

import numpy as np
import pytest

from conftest import compare_fit, record_tol

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import record_matrix as M  # noqa: E402

PAD = 6
LAYOUTS = ("contig", "even", "odd", "host")
_DEV = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture
def lib():
    from deepfmkit_amd import _lib
    lib = _lib.load()
    yield lib
    _lib.check(lib.dfmi_set_tuning(b"lm_ladder", 32), "dfmi_set_tuning")
    _lib.check(lib.dfmi_set_tuning(b"lm_ladder_split", 4), "dfmi_set_tuning")
    _lib.check(lib.dfmi_set_tuning(b"lm_general", 0), "dfmi_set_tuning")


def _forms(nd):
    """(name, lm_ladder, lm_ladder_split, lm_general)"""
    f = [("default", 32, 4, 0), ("one-lane", 0, 4, 0)]
    if nd > 16:
        f.append(("ladder8", 32, 0, 0))
    if nd in (10, 30):
        f.append(("general", 32, 4, 1))
    return f


def _set_form(lib, form):
    from deepfmkit_amd import _lib
    _, ladder, split, general = form
    _lib.check(lib.dfmi_set_tuning(b"lm_ladder", ladder), "dfmi_set_tuning")
    _lib.check(lib.dfmi_set_tuning(b"lm_ladder_split", split), "dfmi_set_tuning")
    _lib.check(lib.dfmi_set_tuning(b"lm_general", general), "dfmi_set_tuning")


def _stride(layout, nbuf=M.NBUF):
    return nbuf * M.R + {"contig": 0, "even": PAD, "host": PAD, "odd": PAD + 1}[layout]


def _layout(nd, layout):
    """The records of `nd` in `layout`: (array kept alive, base pointer, record stride in
    samples, DFMI_MEM_*). Padding samples are NaN: a kernel that read one would show it."""
    import torch
    from deepfmkit_amd import _lib
    key = (nd, layout)
    if key not in _DEV:
        for k in [k for k in _DEV if k[0] != nd]:  # one ndata's records at a time
            del _DEV[k]
        x = M.records(nd)[0]
        stride = _stride(layout)
        flat = np.full(M.NREC * stride, np.nan)
        for r in range(M.NREC):
            flat[r * stride:r * stride + M.NBUF * M.R] = x[r]
        if layout == "host":
            _DEV[key] = (flat, flat.ctypes.data, stride, _lib.DFMI_MEM_HOST)
        else:
            t = torch.from_numpy(flat).cuda()
            assert t.data_ptr() % 16 == 0
            _DEV[key] = (t, t.data_ptr(), stride, _lib.DFMI_MEM_DEVICE)
    return _DEV[key]


def _nchunk(mode, nbuf):
    # deepfmkit_amd.fitters.nls_records: n_cores None -> nbuf - 1, else min(n_cores, nbuf), >= 1
    return max(1, nbuf - 1 if mode is None else min(int(mode), nbuf)) if mode != "seq" else 1


def expected_kernel(nd, mode, nbuf, stride, rec0, nrec):
    """The demodulation family nls_record_device reports last for float64 records of R = 4000,
    L = 200 on a 16-B aligned base (dfmi_capi.hip): (prefix of dfmi_last_demod_kernel, whether
    the name says "rows")."""
    parallel = mode != "seq"
    chunk1 = parallel and (nbuf <= 1 or _nchunk(mode, nbuf) >= nbuf - 1)
    contiguous = nrec == 1 or stride == nbuf * M.R
    even_recs = nrec == 1 or stride % 2 == 0
    first_aligned = (rec0 * stride) % 2 == 0            # vec2_ok of the call's base pointer
    wide = even_recs and nd >= 13 and first_aligned     # demod_wide_from = 13, 128 <= L <= 256
    rows = chunk1 and even_recs and not wide and first_aligned
    if rows and contiguous and nbuf > 1:
        return "demod_seed_bins_kernel", False          # the fused seed + bulk launch
    # otherwise the last demod_device call: the whole batch, or record nrec - 1 on its own
    last_aligned = first_aligned if contiguous else ((rec0 + nrec - 1) * stride) % 2 == 0
    if not last_aligned:
        return "demod_fold_kernel<1,", False            # no sample pairs: the cycle-aligned fold
    if nd >= 13 and not rows:
        return "demod_wide_kernel", False
    return "demod_bins_kernel", rows


def _call(lib, base, mem, stride, rec0, nrec, nbuf, nd, mode, guesses):
    """One dfmi_nls_record call on records [rec0, rec0 + nrec) of a layout, outputs pre-filled
    with sentinels. Returns (result dict, demodulation kernel name)."""
    import torch
    from deepfmkit_amd import _lib
    from deepfmkit_amd import fit as F
    nseg = nrec * nbuf
    g = np.ascontiguousarray(guesses[rec0:rec0 + nrec], dtype=np.float64)
    if mem == _lib.DFMI_MEM_DEVICE:
        out = torch.full((6, nseg), float("nan"), dtype=torch.float64, device="cuda")
        ok = torch.full((nseg,), -7, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
    else:
        out = np.full((6, nseg), np.nan)
        ok = np.full(nseg, -7, dtype=np.int32)
        st = None
    _lib.check(lib.dfmi_nls_record(base + 8 * rec0 * stride, nrec, stride, nbuf, M.R, nd, M.W0, 0, _lib.ptr(g),
                                   0 if mode == "seq" else 1, _nchunk(mode, nbuf), F.lm_config(), _lib.ptr(out),
                                   _lib.ptr(ok), mem, st), "dfmi_nls_record")
    if mem == _lib.DFMI_MEM_DEVICE:
        torch.cuda.synchronize()
        out, ok = out.cpu().numpy(), ok.cpu().numpy()
    kern = lib.dfmi_last_demod_kernel().decode()
    assert not np.isnan(out).any(), ("output never written", np.argwhere(np.isnan(out))[:8].tolist())
    assert not (ok == -7).any(), ("status never written", np.where(ok == -7)[0][:8].tolist())
    res = dict(amp=out[0], m=out[1], phi=out[2], psi=out[3], dc=out[4], ssq=out[5], fitok=ok)
    return res, kern


def _same_bits(a, b, what):
    for k in M.COLS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _slice(res, r0, n, nbuf=M.NBUF):
    return {k: v[r0 * nbuf:(r0 + n) * nbuf] for k, v in res.items()}


def _subsets(layout):
    s = [(0, M.NREC), (0, 3), (5, 1)]
    if layout == "odd":
        s.append((0, 4))
    if layout == "host":
        s = [(0, M.NREC)]
    return s


@pytest.mark.parametrize("mode", M.MODES, ids=M.mode_id)
@pytest.mark.parametrize("nd", M.NDATAS)
def test_record_matrix_vs_oracle(lib, nd, mode):
    _, guesses = M.records(nd)
    ref = M.cached_oracle(nd, mode)
    tol = record_tol(nd, ref["qi"], ref)
    # the inputs do what they were built for (in the oracle; the gate carries it to the GPU)
    assert ref["fitok"][M.GRID_RECORD * M.NBUF] == 1 and abs(ref["m"][M.GRID_RECORD * M.NBUF] - 20.0) < 1e-2
    for r, b in M.NOISE_ONLY.items():
        assert ref["fitok"][r * M.NBUF + b] != 0
    worst, kernels, got = np.zeros(4), {}, {}
    for form in _forms(nd):
        _set_form(lib, form)
        for layout in LAYOUTS:
            if layout == "host" and form[0] != "default":
                continue
            _, base, stride, mem = _layout(nd, layout)
            for rec0, nrec in _subsets(layout):
                ours, kern = _call(lib, base, mem, stride, rec0, nrec, M.NBUF, nd, mode, guesses)
                want, want_rows = expected_kernel(nd, mode, M.NBUF, stride, rec0, nrec)
                assert kern.startswith(want) and ("rows" in kern) == want_rows, (layout, rec0, nrec, kern, want)
                kernels.setdefault((layout, nrec), kern)
                recs = np.arange(rec0, rec0 + nrec)
                sub = M.take_records(ref, recs)
                keep = (recs[:, None] * M.NBUF + np.arange(M.NBUF)[None, :]).ravel()
                try:
                    compare_fit(ours, sub, tol=tol[keep], min_status_match=1.0)
                except AssertionError as exc:
                    raise AssertionError(f"ndata {nd} {M.mode_id(mode)} form {form[0]} layout {layout} records "
                                         f"[{rec0}, {rec0 + nrec}) ({kern}): {exc}") from exc
                d = M.max_deltas(ours, sub)
                worst = np.maximum(worst, d)
                got[(form[0], layout, rec0, nrec)] = ours
    print(f"\nrecord matrix ndata={nd} mode={M.mode_id(mode)}: {len(got)} calls, max |d amp, m, phi, psi| vs the "
          f"oracle = {[f'{v:.2e}' for v in worst]}; demodulation kernels "
          f"(layout, nrec): { {f'{k[0]}/{k[1]}': v for k, v in kernels.items()} }")
    # same bits where DESIGN.md claims them
    names = [f[0] for f in _forms(nd)]
    lane8 = "ladder8" if nd > 16 else "default"  # the 8-lane ladder
    for form in names:
        for rec0, nrec in _subsets("contig"):  # contiguous == even-padded
            _same_bits(got[(form, "contig", rec0, nrec)], got[(form, "even", rec0, nrec)],
                       f"{form}: contiguous vs even-padded, records [{rec0}, {rec0 + nrec})")
    for layout in ("contig", "even", "odd"):  # the 8-lane ladder == the one-lane kernel (same QI)
        for rec0, nrec in _subsets(layout):
            _same_bits(got[(lane8, layout, rec0, nrec)], got[("one-lane", layout, rec0, nrec)],
                       f"8-lane ladder vs lm_chunks_kernel, {layout}, records [{rec0}, {rec0 + nrec})")
    for form in (lane8, "one-lane"):  # a record of the batch == the record alone / in a smaller batch
        for layout in ("contig", "even"):
            full = got[(form, layout, 0, M.NREC)]
            _same_bits(_slice(full, 5, 1), got[(form, layout, 5, 1)], f"{form} {layout}: record 5 in the batch vs alone")
            _same_bits(_slice(full, 0, 3), got[(form, layout, 0, 3)], f"{form} {layout}: records 0-2 of 9 vs of 3")


@pytest.mark.parametrize("nd", M.NDATAS)
def test_one_and_two_buffer_records_vs_oracle(lib, nd):
    """nbuf = 1 (no LM launch in the parallel mode: the seeds' dc through the nbuf <= 1 copy) and
    nbuf = 2 (one item per record), all 9 records, default and parallel=False, compact records
    and the same buffers at the full records' stride; lm_ladder default and 0."""
    import torch
    x, guesses = M.records(nd)
    _, base, stride, mem = _layout(nd, "contig")
    for nbuf in (1, 2):
        compact = torch.from_numpy(np.ascontiguousarray(x[:, :nbuf * M.R])).cuda()
        for mode in (None, "seq"):
            ref = M.cached_oracle(nd, mode, nbuf)
            tol = record_tol(nd, ref["qi"], ref)
            for form in _forms(nd)[:2]:
                _set_form(lib, form)
                res = []
                for b, s in ((compact.data_ptr(), nbuf * M.R), (base, stride)):
                    ours, kern = _call(lib, b, mem, s, 0, M.NREC, nbuf, nd, mode, guesses)
                    want, want_rows = expected_kernel(nd, mode, nbuf, s, 0, M.NREC)
                    assert kern.startswith(want) and ("rows" in kern) == want_rows, (nbuf, mode, kern, want)
                    compare_fit(ours, ref, tol=tol, min_status_match=1.0)
                    res.append(ours)
                    print(f"ndata={nd} nbuf={nbuf} mode={M.mode_id(mode)} form {form[0]} stride {s} ({kern}): "
                          f"max |d amp, m, phi, psi| = {[f'{v:.2e}' for v in M.max_deltas(ours, ref)]}")
                _same_bits(res[0], res[1], f"nbuf {nbuf} {M.mode_id(mode)} {form[0]}: compact vs strided")


@pytest.mark.parametrize("nd", [10, 30])
def test_dfmi_lm_shared_guess_chunks_vs_oracle(lib, nd):
    """dfmi_lm(guess_per_segment = 0): ONE 4-vector guess seeds nchunk np.array_split chunks of the
    nseg segments, warm start within a chunk (include/dfmi.h). Buffers 1..22 of record 0 (oracle
    QI, component-major, host pointers; its noise-only buffer is segment 6), nchunk 1 (one chain),
    3 (8 + 7 + 7), 5 (5 + 5 + 4 + 4 + 4), 22 and 29 (both chunk size 1; 29 > nseg clamps), in the
    default (ladder) and lm_ladder = 0 (lm_chunks_kernel) forms, against the oracle's chains."""
    from deepfmkit_amd import _lib
    from deepfmkit_amd import fit as F
    _, guesses = M.records(nd)
    qi_all, _ = M.cached_qi(nd)
    nseg = M.NBUF - 1
    qi = np.array(qi_all[1:M.NBUF])
    qcm = np.ascontiguousarray(qi.T)
    guess = np.array(guesses[0], dtype=np.float64)
    for nchunk in (1, 3, 5, 22, 29):
        res = np.zeros((nseg, 6))
        chunks = [c for c in np.array_split(np.arange(nseg), min(nchunk, nseg)) if c.size]
        M.oracle_chains(qi, nd, chunks, guess, res)
        ref = dict(amp=res[:, 0], m=res[:, 1], phi=res[:, 2], psi=res[:, 3], dc=np.zeros(nseg), ssq=res[:, 4],
                   fitok=res[:, 5].astype(np.int32), qi=qi)
        assert (ref["fitok"] != 0).any()
        tol = record_tol(nd, qi, ref)
        by_form = []
        for form in _forms(nd)[:2]:
            _set_form(lib, form)
            p = np.full((4, nseg), np.nan)
            ssq = np.full(nseg, np.nan)
            st = np.full(nseg, -7, dtype=np.int32)
            _lib.check(lib.dfmi_lm(_lib.ptr(qcm), nseg, nd, _lib.ptr(guess), 0, nchunk, F.lm_config(), _lib.ptr(p),
                                   _lib.ptr(ssq), _lib.ptr(st), _lib.DFMI_MEM_HOST, None), "dfmi_lm")
            assert not np.isnan(p).any() and not np.isnan(ssq).any() and not (st == -7).any(), (nchunk, form[0])
            ours = dict(amp=p[0], m=p[1], phi=p[2], psi=p[3], dc=np.zeros(nseg), ssq=ssq, fitok=st)
            try:
                compare_fit(ours, ref, tol=tol, min_status_match=1.0)
            except AssertionError as exc:
                raise AssertionError(f"dfmi_lm ndata {nd} nchunk {nchunk} form {form[0]}: {exc}") from exc
            print(f"dfmi_lm ndata={nd} nchunk={nchunk} form {form[0]}: max |d amp, m, phi, psi| vs the oracle = "
                  f"{[f'{v:.2e}' for v in M.max_deltas(ours, ref)]}")
            by_form.append(ours)
        if nd <= 16:  # the 8-lane ladder takes the one-lane kernel's points: same bits
            _same_bits(by_form[0], by_form[1], f"dfmi_lm nchunk {nchunk}: ladder vs lm_chunks_kernel")


@pytest.mark.parametrize("nd", M.NDATAS)
def test_sequential_guess_table_vs_oracle(lib, nd):
    """Which record's guess a warm-start chain starts from, shown by STATUS: from the matrix's own
    guess table every clean record reaches its own minimum from any record's guess (a swapped
    guess moves a fit by ~1e-12, inside the gate), so here the m = 20 record starts at m = 20.2
    (record_matrix.alt_guesses): status 0 from its own guess, status 1 from any other record's,
    and every other record status 1 from the m = 20 record's. parallel=False on all 9 records
    (the device guess table), records 0-4 and 4-8 (inline guesses; the m = 20 record last / first),
    every LM form, against the oracle's chains at the matrix's gate."""
    guesses = M.alt_guesses(nd)
    ref = M.cached_oracle(nd, "seq", alt=True)
    tol = record_tol(nd, ref["qi"], ref)
    assert (ref["fitok"].reshape(M.NREC, M.NBUF)[:, 0] == 0).all()
    _, base, stride, mem = _layout(nd, "contig")
    for form in _forms(nd):
        _set_form(lib, form)
        for rec0, nrec in ((0, M.NREC), (0, 5), (4, 5)):
            ours, kern = _call(lib, base, mem, stride, rec0, nrec, M.NBUF, nd, "seq", guesses)
            recs = np.arange(rec0, rec0 + nrec)
            keep = (recs[:, None] * M.NBUF + np.arange(M.NBUF)[None, :]).ravel()
            try:
                compare_fit(ours, M.take_records(ref, recs), tol=tol[keep], min_status_match=1.0)
            except AssertionError as exc:
                raise AssertionError(f"ndata {nd} form {form[0]} records [{rec0}, {rec0 + nrec}): {exc}") from exc
            print(f"ndata={nd} seq, second guess table, form {form[0]}, records [{rec0}, {rec0 + nrec}): max |d amp, m, "
                  f"phi, psi| = {[f'{v:.2e}' for v in M.max_deltas(ours, M.take_records(ref, recs))]}")
