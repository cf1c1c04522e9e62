"""Inputs, record layouts and runners of the EKF call matrix (tests/test_gpu_ekf_matrix.py,
tests/test_ekf_matrix_host.py): dfmi_ekf / dfmi_ekf_fit over every sequential kernel, the
parallel form and the hand-over, with rec_stride != n_samp, host and device memory, batches past
one wave and the loop tails, against the scalar C oracle (oracle/csrc/ekf_scalar.c through
ekf_stress.c_oracle; sensitivity and rel_err are ekf_stress's).

Channels: ekf_stress.batch_inputs' signal model, a (1 + C cos(phi + m cos(w_m t + psi))) + white
noise at 200 kHz / 1 kHz, drawn close enough to lock within a few hundred samples (m 3-9, SNR
30-50 dB, x0 within 10 % / 0.3 / 0.2 / 0.1 of the truth): the oracle's own sensitivity S stays
below 1e-12 on every channel, so the gate max(1e-12, 100 S) of tests/test_gpu_ekf_pit_stress.py is
the flat 1e-12 on nearly all of them (tests/test_ekf_matrix_host.py holds the inputs to that)."""
import ctypes
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ekf_stress as S  # noqa: E402

SEED = 4242
# (n_samp, channels, R); the case number is the index
SHAPES = [
    (1607, 130, 16),   # rot<16>, tail of 7; lane kernels 3 workgroups (last: 2 lanes), row kernels 33 waves (last: 2 rows)
    (2003, 65, 8),     # groups of 8, tail of 3; one lane past a full wave
    (1500, 64, 4),     # groups of 4, no tail; exactly one full wave
    (1501, 20, 500),   # groups of 4, tail of 1; 3 snapshots
    (4133, 5, 7),      # odd R: ekf_row_kernel / ekf_kernel with n % 8 = 5 and 590 snapshots; parallel by default
    (37, 5, 1),        # a snapshot after every sample
    (7, 5, 3),         # n < 8: only the tail loops run
    (4099, 5, 1024),   # parallel by default: block 16, 257 blocks, two scan levels (also blocks 16 and 49)
    (9000, 4, 3000),   # parallel, snapshots mid-block
    (6, 3, 8),         # nbuf = 0: the call succeeds and writes nothing
]
EXTRA = (0, 1, 13)     # rec_stride - n_samp
GUARD = 64             # doubles of guard on either side of a device block
SENTINEL = -7.25e77    # what the output guards (and the host output) hold before a call

# dfmi_set_tuning defaults, as tests/test_gpu_ekf_pit.py::_tune lists them
DEFAULTS = {"ekf_row": 1, "ekf_rot": 1, "ekf_pit": 1024, "ekf_pit_min": 4096, "ekf_pit_block": 0,
            "ekf_pit_passes": 0, "ekf_pit_head": 256, "ekf_pit_fused": 1, "ekf_pit_first": 5,
            "ekf_pit_every": 2, "ekf_pit_tol": 13, "ekf_pit_stall": 3, "ekf_pit_trace": 0, "ekf_pit_seq": 1}

# kernel families: the four sequential kernels and the parallel form (the defaults)
FAMILIES = {"row_rot": {"ekf_pit": 0, "ekf_row": 1, "ekf_rot": 1}, "row": {"ekf_pit": 0, "ekf_row": 1, "ekf_rot": 0},
            "lane_rot": {"ekf_pit": 0, "ekf_row": 0, "ekf_rot": 1}, "lane": {"ekf_pit": 0, "ekf_row": 0, "ekf_rot": 0},
            "pit": {}}
SEQUENTIAL = ("row_rot", "row", "lane_rot", "lane")


def families(case):
    """The families shape `case` can reach: the rotation kernels need R % 4 == 0 (without it
    ekf_rot = 1 picks the kernels of ekf_rot = 0), the parallel form ekf_pit_min samples."""
    n, _, R = SHAPES[case]
    fam = [f for f in SEQUENTIAL if R % 4 == 0 or not f.endswith("rot")]
    return fam + (["pit"] if n >= DEFAULTS["ekf_pit_min"] else [])


def tuning(family, **kw):
    t = dict(DEFAULTS)
    t.update(FAMILIES[family])
    t.update(kw)
    return t


def expected_kernel(nrec, n, R, t, n_cu):
    """The name dfmi_last_demod_kernel() reports for this call by the dispatch rule of ekf_impl /
    ekf_seq_launch / ekf_pit_run (without the hand-over suffix)."""
    if t["ekf_pit"] > 0 and nrec <= t["ekf_pit"] and n >= t["ekf_pit_min"] and n >= 2:
        B = t["ekf_pit_block"]
        if B <= 0:
            B = int(np.ceil(n * nrec ** (2.0 / 3.0) / 16384.0))
        B = max(B, 16)
        return f"ekf_pit (B={B}, nb={(n + B - 1) // B})"
    return seq_kernel(nrec, R, t, n_cu)


def seq_kernel(nrec, R, t, n_cu):
    row = t["ekf_row"] and nrec <= t["ekf_row"] * n_cu * 16
    rot = t["ekf_rot"] and R % 4 == 0
    return ("ekf_rot_kernel" if rot else "ekf_row_kernel") if row else ("ekf_lane_rot_kernel" if rot else "ekf_kernel")


class tune:
    """dfmi_set_tuning for the duration of a block, restoring DEFAULTS."""

    def __init__(self, lib, **kw):
        self.lib, self.kw = lib, kw

    def __enter__(self):
        from deepfmkit_amd import _lib
        for k, v in self.kw.items():
            _lib.check(self.lib.dfmi_set_tuning(k.encode(), v), "tune")
        return self

    def __exit__(self, *exc):
        from deepfmkit_amd import _lib
        for k in self.kw:
            _lib.check(self.lib.dfmi_set_tuning(k.encode(), DEFAULTS[k]), "tune")


@functools.lru_cache(maxsize=None)
def channels(case):
    """Records (nch, n), x0 (nch, 5), r_val (nch,) of shape `case` (read-only arrays)."""
    n, nch, _ = SHAPES[case]
    rng = np.random.default_rng([SEED, case])
    t = np.arange(n) / S.F_SAMP
    m = rng.uniform(3.0, 9.0, nch)
    phi = rng.uniform(-np.pi, np.pi, nch)
    psi = rng.uniform(-np.pi, np.pi, nch)
    amp = rng.uniform(0.5, 2.0, nch)
    vis = rng.uniform(0.5, 1.0, nch)
    snr_db = rng.uniform(30.0, 50.0, nch)
    x = np.empty((nch, n))
    for c in range(nch):
        clean = amp[c] * (1.0 + vis[c] * np.cos(phi[c] + m[c] * np.cos(S.W_M * t + psi[c])))
        noise_std = amp[c] * vis[c] / np.sqrt(2.0) / 10 ** (snr_db[c] / 20.0)
        x[c] = clean + rng.normal(0.0, noise_std, n)
    x0 = np.empty((nch, 5))
    x0[:, 0] = amp * vis * rng.uniform(0.9, 1.1, nch)
    x0[:, 1] = m + rng.uniform(-0.3, 0.3, nch)
    x0[:, 2] = phi + rng.uniform(-0.2, 0.2, nch)
    x0[:, 3] = psi + rng.uniform(-0.1, 0.1, nch)
    x0[:, 4] = x.mean(axis=1)
    r_val = x.var(axis=1) * 10 ** rng.uniform(-0.5, 0.5, nch)
    for a in (x, x0, r_val):
        a.setflags(write=False)
    return x, x0, r_val


def records_strided(x, stride):
    """The records in one flat array, `stride` doubles apart, NaN in the gaps (and after the
    last record): a read outside a record poisons that channel."""
    nch, n = x.shape
    flat = np.full(nch * stride, np.nan)
    flat.reshape(nch, stride)[:, :n] = x
    return flat


def records_back(flat, nch, n, stride):
    return flat.reshape(nch, stride)[:, :n]


def guarded(flat, fill=np.nan):
    """The block with GUARD doubles of `fill` before and after it (numpy): the whole array and
    the view of the block."""
    big = np.full(flat.size + 2 * GUARD, fill)
    big[GUARD:GUARD + flat.size] = flat
    return big, big[GUARD:GUARD + flat.size]


@functools.lru_cache(maxsize=None)
def _oracle_cached(case, nbuf):
    cl = S.c_oracle()
    x, x0, rv = channels(case)
    n, nch, R = SHAPES[case]
    if nbuf == 0:
        return np.zeros((nch, 0, 5)), np.zeros(nch)
    ref, sens = S.oracle_batch(cl, x, x0, rv, S.QD0, R, nbuf)
    ref.setflags(write=False)
    sens.setflags(write=False)
    return ref, sens


def oracle(case, nbuf=None):
    """C-oracle states (nch, nbuf, 5) and sensitivities (nch,) of shape `case`, computed once
    (nbuf defaults to n // R). None when oracle/libekf_scalar.so is missing."""
    if S.c_oracle() is None:
        return None
    n, _, R = SHAPES[case]
    return _oracle_cached(case, n // R if nbuf is None else nbuf)


def gate(sens):
    """Per-channel bound of tests/test_gpu_ekf_pit_stress.py: max(1e-12, 100 S), a flat 1e-12 on
    the well-conditioned channels (S <= 1e-14)."""
    return np.where(sens <= 1e-14, 1e-12, np.maximum(1e-12, 100.0 * sens))


def rel_err(got, ref):
    if got.shape[1] == 0:
        return np.zeros(got.shape[0])
    return S.rel_err(got, ref)


def misses(got, ref, sens):
    """Channels outside their gate, and every channel's error. A state that is not finite (a
    read outside the record takes in the NaN of a gap) is a miss."""
    err = rel_err(got, ref)
    return np.where(~(err <= gate(sens)))[0], err


def run(lib, x, R, nbuf, extra=0, device=False, x0=None, r_val=None, init4=None, qd=S.QD0):
    """One dfmi_ekf call (x0 (nch, 5) and r_val (nch,) given) or dfmi_ekf_fit call (init4 given;
    r_val None or a scalar) over the records x (nch, n) laid out rec_stride = n + extra apart
    with NaN gaps. Host memory: numpy arrays, the output prefilled with SENTINEL. Device memory:
    every pointer a device pointer, the records and the states each inside a larger tensor with
    GUARD doubles either side (NaN / SENTINEL), on a non-default torch stream that is
    synchronised before the states are read; the output guards must come back unchanged.
    Returns the states (nch, nbuf, 5), the reported kernel name and the pass counts."""
    from deepfmkit_amd import _lib
    nch, n = x.shape
    stride = n + extra
    flat = records_strided(x, stride)
    q = np.ascontiguousarray(qd, dtype=np.float64)
    fit = init4 is not None
    a0 = np.ascontiguousarray(init4 if fit else x0, dtype=np.float64)
    rv = None if r_val is None else np.array(np.atleast_1d(r_val), dtype=np.float64)
    assert a0.shape == ((4,) if fit else (nch, 5)) and (rv is None or rv.shape == ((1,) if fit else (nch,)))
    fn = lib.dfmi_ekf_fit if fit else lib.dfmi_ekf
    what = "dfmi_ekf_fit" if fit else "dfmi_ekf"
    if not device:
        st = np.full((nch, nbuf, 5), SENTINEL)
        _lib.check(fn(_lib.ptr(flat), nch, stride, n, _lib.ptr(a0), _lib.ptr(S.P0), _lib.ptr(q), _lib.ptr(rv), S.W_M,
                      S.F_SAMP, R, nbuf, _lib.ptr(st), _lib.DFMI_MEM_HOST, None), what)
    else:
        import torch
        dev = torch.device("cuda", 0)
        xbig = torch.from_numpy(guarded(flat)[0]).to(dev)
        sbig = torch.full((nch * nbuf * 5 + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=dev)
        d0, dp, dq = (torch.from_numpy(np.array(a)).to(dev) for a in (a0, S.P0, q))
        dr = None if rv is None else torch.from_numpy(rv).to(dev)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize(dev)  # the uploads above ran on the default stream
        _lib.check(fn(xbig.data_ptr() + GUARD * 8, nch, stride, n, d0.data_ptr(), dp.data_ptr(), dq.data_ptr(),
                      None if dr is None else dr.data_ptr(), S.W_M, S.F_SAMP, R, nbuf, sbig.data_ptr() + GUARD * 8,
                      _lib.DFMI_MEM_DEVICE, stream.cuda_stream), what)
        stream.synchronize()
        out = sbig.cpu().numpy()
        assert (out[:GUARD] == SENTINEL).all() and (out[out.size - GUARD:] == SENTINEL).all(), \
            "the call wrote outside its states block"
        st = out[GUARD:out.size - GUARD].reshape(nch, nbuf, 5).copy()
    kname = lib.dfmi_last_demod_kernel().decode()
    passes = (ctypes.c_int32 * nch)()
    _lib.check(lib.dfmi_ekf_pit_passes(ctypes.cast(passes, ctypes.c_void_p), nch), "passes")
    return st, kname, np.array(list(passes), dtype=np.int64)
