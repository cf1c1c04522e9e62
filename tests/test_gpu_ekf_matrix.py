"""The EKF entry points' call matrix: dfmi_ekf / dfmi_ekf_fit over every sequential kernel
(ekf_rot_kernel<16|8|4>, ekf_row_kernel, ekf_lane_rot_kernel<8|4>, ekf_kernel), the parallel form
(ekf_pit.h) and the hand-over through idx, with rec_stride != n_samp (NaN between the records),
host and device memory (device: every pointer on the device, a non-default stream, guarded
blocks), batches of 64 / 65 / 130 channels (a full wave, one lane past it, three lane workgroups
and 33 row waves with a part-filled last one), and the loop tails (n % 8, n % G, n < 8, R = 1,
odd R, nbuf below and above n / R) — tests/helpers/ekf_matrix.py has the shapes and what each is
for.

Reference: the scalar C oracle (oracle/csrc/ekf_scalar.c), under the per-channel gate of
tests/test_gpu_ekf_pit_stress.py, rel_err <= max(1e-12, 100 S) and a flat 1e-12 where the oracle's
own sensitivity S <= 1e-14 (tests/test_ekf_matrix_host.py holds the inputs to S <= 1e-12
everywhere and S <= 1e-14 on all but a few channels). Beside it the invariants that need no
tolerance: a channel's states are the same bits whatever the layout, the memory, the batch around
it, and (sequential kernels) the number of snapshots asked for.

Found by (a): at 4133 x 5, R = 7 the parallel form left the gate (a snapshot at sample 84 at
1.02e-12, S = 5.1e-15) — the scan's rounding while P collapses from P0; the snapshots inside the
head now come from the sequential kernel (dfmi_capi.hip ekf_pit_run, k_seq): worst 1.0e-13
there (DESIGN.md 7c has every figure).

Every run also asserts the kernel name dfmi_last_demod_kernel() reports against the dispatch
rule (ekf_matrix.expected_kernel)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ekf_matrix as M  # noqa: E402
import ekf_stress as S  # noqa: E402


def _configs():
    """(case, family, extra tuning): every family a shape reaches; the parallel form at its
    default block and at fixed ones (16 everywhere, 49 too at 4099 samples)."""
    out = []
    for case, (n, _, _) in enumerate(M.SHAPES):
        for fam in M.families(case):
            if fam != "pit":
                out.append((case, fam, ()))
                continue
            out.append((case, fam, ()))
            out.append((case, fam, (("ekf_pit_block", 16),)))
            if n == 4099:
                out.append((case, fam, (("ekf_pit_block", 49),)))
    return out


def _id(cfg):
    case, fam, kw = cfg
    n, nch, R = M.SHAPES[case]
    return f"{n}x{nch}-R{R}-{fam}" + "".join(f"-B{v}" for _, v in kw)


CONFIGS = _configs()
FIXED = [c for c in CONFIGS if (c[1] != "pit" or c[2]) and M.SHAPES[c[0]][0] // M.SHAPES[c[0]][2] > 0]


class _Runs:
    """The matrix's GPU runs, each made once and shared by the tests (read-only)."""

    def __init__(self, lib, n_cu):
        self.lib, self.n_cu, self.memo = lib, n_cu, {}

    def _call(self, x, x0, rv, R, nbuf, extra, device, t):
        nch, n = x.shape
        with M.tune(self.lib, **{k: v for k, v in t.items() if v != M.DEFAULTS[k]}):
            st, kname, passes = M.run(self.lib, x, R, nbuf, extra=extra, device=device, x0=x0, r_val=rv)
        exp = M.expected_kernel(nch, n, R, t, self.n_cu)
        if exp.startswith("ekf_pit"):
            nh = int((passes < 0).sum())  # handed over: re-run by the sequential kernel for that many channels
            exp += f" + {M.seq_kernel(nh, R, t, self.n_cu)} x{nh}" if nh else ""
        else:
            assert (passes == 0).all(), passes
        assert kname == exp, (kname, exp)
        st.setflags(write=False)
        return st, kname, passes

    def batch(self, cfg, extra=0, device=False, nbuf=None):
        case, fam, kw = cfg
        n, _, R = M.SHAPES[case]
        nbuf = n // R if nbuf is None else nbuf
        key = (cfg, extra, device, nbuf)
        if key not in self.memo:
            x, x0, rv = M.channels(case)
            self.memo[key] = self._call(x, x0, rv, R, nbuf, extra, device, M.tuning(fam, **dict(kw)))
        return self.memo[key]

    def one(self, cfg, c):
        """Channel c alone (nrec = 1, a contiguous copy, host memory)."""
        case, fam, kw = cfg
        n, _, R = M.SHAPES[case]
        key = (cfg, "one", c)
        if key not in self.memo:
            x, x0, rv = M.channels(case)
            self.memo[key] = self._call(x[c:c + 1].copy(), x0[c:c + 1].copy(), rv[c:c + 1].copy(), R, n // R, 0, False,
                                        M.tuning(fam, **dict(kw)))
        return self.memo[key]


@pytest.fixture(scope="module")
def lib():
    # torch first, as in the other GPU test files
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deepfmkit_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def runs(lib):
    import torch
    if S.c_oracle() is None:
        pytest.skip("oracle/libekf_scalar.so not built (make -C oracle)")
    return _Runs(lib, torch.cuda.get_device_properties(0).multi_processor_count)


def _check_gate(got, case, nbuf, what):
    ref, sens = M.oracle(case, nbuf)
    bad, err = M.misses(got, ref, sens)  # a NaN (a read outside the record) is a miss
    assert bad.size == 0, (what, [(int(c), float(err[c]), float(sens[c])) for c in bad[:10]])
    return float(err.max()), float(np.abs(got - ref).max()) if got.size else 0.0


@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_matrix_against_c_oracle(runs, cfg):
    """(a) every layout and both memories of one (shape, kernel family): every snapshot of every
    channel within the channel's gate of the C oracle."""
    case = cfg[0]
    n, nch, R = M.SHAPES[case]
    worst_rel = worst_abs = 0.0
    names, npass = set(), set()
    for extra in M.EXTRA:
        for device in (False, True):
            st, kname, passes = runs.batch(cfg, extra, device)
            assert st.shape == (nch, n // R, 5)
            rel, ab = _check_gate(st, case, n // R, (extra, device, kname))
            worst_rel, worst_abs = max(worst_rel, rel), max(worst_abs, ab)
            names.add(kname)
            npass.update(int(p) for p in passes)
    print(f"{_id(cfg)}: {sorted(names)} passes {sorted(npass)} worst |d| {worst_abs:.2e} rel {worst_rel:.2e}")


@pytest.mark.parametrize("cfg", FIXED, ids=_id)
def test_same_bits_across_layout_memory_and_batch(runs, cfg):
    """(b) a channel's states are bit-identical across the three layouts, across host and device
    memory, and between the batch and a one-channel call of that channel (channels 0, 63, 64
    and the last); the parallel form at a fixed ekf_pit_block."""
    case = cfg[0]
    nch = M.SHAPES[case][1]
    base, _, p0 = runs.batch(cfg, 0, False)
    assert np.isfinite(base).all()
    for extra in M.EXTRA:
        for device in (False, True):
            st, _, p = runs.batch(cfg, extra, device)
            np.testing.assert_array_equal(st, base, err_msg=f"extra {extra} device {device}")
            np.testing.assert_array_equal(p, p0)
    for c in sorted({0, 63, 64, nch - 1} & set(range(nch))):
        one, _, p = runs.one(cfg, c)
        np.testing.assert_array_equal(one[0], base[c], err_msg=f"channel {c} alone")
        assert p[0] == p0[c]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("cfg", [c for c in FIXED if M.SHAPES[c[0]][0] // M.SHAPES[c[0]][2] >= 2], ids=_id)
def test_fewer_snapshots_than_the_record_holds(runs, cfg, device):
    """nbuf < n / R (strided records): the sequential kernels give exactly the first nbuf
    snapshots of the full run; the parallel form, whose stop rule reads the output snapshots (so
    the pass count may differ), is held to the oracle gate."""
    case, fam, _ = cfg
    n, nch, R = M.SHAPES[case]
    nb = max(1, (n // R) // 2)
    st, _, _ = runs.batch(cfg, 13, device, nbuf=nb)
    assert st.shape == (nch, nb, 5)
    if fam == "pit":
        _check_gate(st, case, nb, "short nbuf")
    else:
        np.testing.assert_array_equal(st, runs.batch(cfg, 0, False)[0][:, :nb])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("cfg", [c for c in CONFIGS if c[1] != "pit" or c[2]], ids=_id)
def test_more_snapshots_than_the_record_holds(runs, cfg, device):
    """nbuf = n / R + 2 (the output prefilled with a sentinel): the two extra rows of every
    channel are exactly zero (the call's memset) and the others are the full run's (sequential
    kernels: the same bits; the parallel form: the oracle gate)."""
    case, fam, _ = cfg
    n, nch, R = M.SHAPES[case]
    nb = n // R
    st, _, _ = runs.batch(cfg, 1, device, nbuf=nb + 2)
    assert st.shape == (nch, nb + 2, 5)
    assert (st[:, nb:] == 0).all(), np.argwhere(st[:, nb:] != 0)[:5]
    if fam == "pit":
        _check_gate(st[:, :nb], case, nb, "long nbuf")
    else:
        np.testing.assert_array_equal(st[:, :nb], runs.batch(cfg, 0, False)[0])


INIT4 = (1.0, 6.0, 0.0, 0.0)


@pytest.mark.parametrize("r_given", [False, True], ids=["var", "r_val"])
@pytest.mark.parametrize("case,fam", [(0, "row_rot"), (0, "lane_rot"), (7, "pit")], ids=["1607x130-row", "1607x130-lane",
                                                                                       "4099x5-pit"])
def test_ekf_fit_device_path_equals_ekf_with_numpy_moments(lib, runs, case, fam, r_given):
    """(c) dfmi_ekf_fit on strided records with init4 / p0 / q (and r_val, when given: a scalar)
    on the device: bit-identical to dfmi_ekf given x0 = [init4, np.mean(record)] and r_val =
    np.var(record) (or the scalar repeated), and to the host-memory dfmi_ekf_fit call. Covers
    ekf_x0_kernel's device-pointer branch and the strided moments inside the EKF call."""
    n, nch, R = M.SHAPES[case]
    x = M.channels(case)[0]
    nbuf = n // R
    r_scalar = 0.0123 if r_given else None
    x0 = np.concatenate([np.tile(np.array(INIT4), (nch, 1)), x.mean(axis=1)[:, None]], axis=1)
    rv = np.full(nch, r_scalar) if r_given else x.var(axis=1)
    t = M.tuning(fam)
    with M.tune(lib, **M.FAMILIES[fam]):
        ref, kref, pref = M.run(lib, x, R, nbuf, x0=x0, r_val=rv)
        assert kref.startswith(M.expected_kernel(nch, n, R, t, runs.n_cu)), kref
        assert not np.array_equal(ref, runs.batch((case, fam, ()), 0, False)[0])  # another x0: other states
        for extra, device in ((1, True), (13, True), (13, False)):
            got, kname, passes = M.run(lib, x, R, nbuf, extra=extra, device=device, init4=INIT4, r_val=r_scalar)
            assert kname == kref, (kname, kref)
            np.testing.assert_array_equal(got, ref, err_msg=f"extra {extra} device {device}")
            np.testing.assert_array_equal(passes, pref)
    assert np.isfinite(ref).all()


HO = (7, "pit", (("ekf_pit_block", 16),))  # 4099 x 5, R = 1024


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_handover_all_channels_strided(lib, runs, device):
    """(d) one pass allowed: all five channels of the strided batch are handed over through idx
    and equal, bit for bit, five one-channel sequential runs on contiguous copies."""
    case, _, kw = HO
    n, nch, R = M.SHAPES[case]
    x, x0, rv = M.channels(case)
    with M.tune(lib, ekf_pit_passes=1, **dict(kw)):
        got, kname, passes = M.run(lib, x, R, n // R, extra=13, device=device, x0=x0, r_val=rv)
    assert kname == "ekf_pit (B=16, nb=257) + ekf_rot_kernel x5" and (passes == -1).all(), (kname, passes)
    for c in range(nch):
        one, k1, _ = runs.one((case, "row_rot", ()), c)
        assert k1 == "ekf_rot_kernel"
        np.testing.assert_array_equal(got[c], one[0], err_msg=f"channel {c}")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", [1, 0], ids=["row", "lane"])
def test_handover_middle_channels_strided(lib, runs, row, device):
    """(d) a NaN sample in channels 1 and 3 of the strided batch only (ordinary data to these
    kernels: the states after it are NaN): those two are handed over (negative pass counts,
    idx = [1, 3]) and equal their own sequential one-channel runs bit for bit, NaN where those
    have NaN; channels 0, 2 and 4 converge and stay within the oracle gate. ekf_row = 0: the
    re-run takes the lane kernel."""
    case, _, kw = HO
    n, nch, R = M.SHAPES[case]
    x, x0, rv = M.channels(case)
    xb = x.copy()
    xb[[1, 3], 3000] = np.nan  # after the second snapshot: two finite rows to compare
    seq = "ekf_rot_kernel" if row else "ekf_lane_rot_kernel"
    with M.tune(lib, ekf_row=row, **dict(kw)):
        got, kname, passes = M.run(lib, xb, R, n // R, extra=13, device=device, x0=x0, r_val=rv)
    assert kname == f"ekf_pit (B=16, nb=257) + {seq} x2", kname
    assert (passes[[1, 3]] < 0).all() and (passes[[0, 2, 4]] > 0).all(), passes
    with M.tune(lib, ekf_pit=0, ekf_row=row):
        for c in (1, 3):
            one, k1, _ = M.run(lib, xb[c:c + 1], R, n // R, x0=x0[c:c + 1], r_val=rv[c:c + 1])
            assert k1 == seq, k1
            assert np.isfinite(one[0, :2]).all() and np.isnan(one[0, 2:]).all()
            np.testing.assert_array_equal(got[c], one[0], err_msg=f"channel {c}")
    ref, sens = M.oracle(case)
    ok = [0, 2, 4]
    bad, err = M.misses(got[ok], ref[ok], sens[ok])
    assert bad.size == 0, (err, sens[ok])
