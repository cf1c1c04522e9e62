"""What the GPU gate of tests/test_gpu_ekf_matrix.py rests on, checked on the CPU with the C
oracle alone (oracle/csrc/ekf_scalar.c), so the gate cannot quietly widen: the matrix's channels
(tests/helpers/ekf_matrix.py) are well-conditioned — the oracle's own move under rounding-sized
perturbations (ekf_stress.sensitivity = S) is at most 1e-12 on every channel, and on all but a few
it is below 1e-14, where the gate is the flat 1e-12. A reseed changes ekf_matrix.SEED, never the
caps here. Also the layout builder: records recovered exactly from every stride, NaN gaps and
guards, and the oracle's snapshots for nbuf < n / R the prefix of the full run's.

Measured with this recipe (x86-64, glibc libm): worst S = 3.72e-13; 8 of the 303 channels with
snapshots above 1e-14: 3 of the 5 of (7, 5, 3), whose two snapshots come before the filter has
locked, 4 of the 130 of (1607, 130, 16) and 1 of the 64 of (1500, 64, 4)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ekf_matrix as M  # noqa: E402
import ekf_stress as S  # noqa: E402


@pytest.fixture(scope="module")
def cl():
    cl = S.c_oracle()
    if cl is None:
        pytest.skip("oracle/libekf_scalar.so not built (make -C oracle)")
    return cl


def test_shape_list_is_the_issue_s():
    """The shapes, strides and guard the matrix is specified with."""
    assert M.SHAPES == [(1607, 130, 16), (2003, 65, 8), (1500, 64, 4), (1501, 20, 500), (4133, 5, 7), (37, 5, 1),
                        (7, 5, 3), (4099, 5, 1024), (9000, 4, 3000), (6, 3, 8)]
    assert M.EXTRA == (0, 1, 13) and M.GUARD == 64
    assert [M.families(c) for c in range(len(M.SHAPES))] == [
        ["row_rot", "row", "lane_rot", "lane"], ["row_rot", "row", "lane_rot", "lane"],
        ["row_rot", "row", "lane_rot", "lane"], ["row_rot", "row", "lane_rot", "lane"], ["row", "lane", "pit"],
        ["row", "lane"], ["row", "lane"], ["row_rot", "row", "lane_rot", "lane", "pit"],
        ["row_rot", "row", "lane_rot", "lane", "pit"], ["row_rot", "row", "lane_rot", "lane"]]


def test_channels_are_well_conditioned(cl):
    """Every channel S <= 1e-12; at most 10 % of all channels, and at most 5 % of any shape but
    (7, 5, 3), above 1e-14."""
    tot = above = 0
    worst = 0.0
    for case, (n, nch, R) in enumerate(M.SHAPES):
        if n // R == 0:
            continue  # no snapshot: nothing to compare
        _, sens = M.oracle(case)
        k = int((sens > 1e-14).sum())
        print(f"shape {(n, nch, R)}: max S {sens.max():.2e}, {k} of {nch} above 1e-14")
        assert sens.max() <= 1e-12, (case, float(sens.max()), int(sens.argmax()))
        if (n, nch, R) != (7, 5, 3):
            assert k <= 0.05 * nch, (case, k, nch)
        tot += nch
        above += k
        worst = max(worst, float(sens.max()))
    print(f"worst S {worst:.2e}; {above} of {tot} channels above 1e-14")
    assert above <= 0.10 * tot, (above, tot)


def test_gate_is_the_stress_test_s():
    s = np.array([0.0, 1e-15, 1e-14, 1.0000001e-14, 5e-14, 3e-13])
    np.testing.assert_array_equal(M.gate(s), [1e-12, 1e-12, 1e-12, 100 * 1.0000001e-14, 100 * 5e-14, 100 * 3e-13])
    # the check itself: a state just outside the gate is a miss, and so is one that is not finite
    ref = np.ones((4, 2, 5))
    got = ref.copy()
    got[1, 0, 3] += 1.1e-12
    got[2, 1, 0] = np.nan
    got[3, 0, 0] += 9e-13
    bad, err = M.misses(got, ref, np.zeros(4))
    assert list(bad) == [1, 2] and err[0] == 0 and np.isnan(err[2])
    assert list(M.misses(got, ref, np.full(4, 2e-14))[0]) == [2]
    assert M.misses(np.zeros((3, 0, 5)), np.zeros((3, 0, 5)), np.zeros(3))[0].size == 0


def test_channels_follow_the_recipe():
    """Seeded by the case number, reproducible, and inside the drawn ranges: x0[4] the record's
    mean, r_val within 10^+-0.5 of its variance."""
    for case, (n, nch, R) in enumerate(M.SHAPES):
        x, x0, rv = M.channels(case)
        assert x.shape == (nch, n) and x0.shape == (nch, 5) and rv.shape == (nch,)
        np.testing.assert_array_equal(x0[:, 4], x.mean(axis=1))
        ratio = rv / x.var(axis=1)
        assert (ratio >= 10 ** -0.5 * (1 - 1e-12)).all() and (ratio <= 10 ** 0.5 * (1 + 1e-12)).all()
        assert (x0[:, 1] > 2.7).all() and (x0[:, 1] < 9.3).all() and (x0[:, 0] > 0.22).all() and (x0[:, 0] < 2.2).all()
        assert np.isfinite(x).all()
    a = M.channels(3)[0]
    M.channels.cache_clear()
    np.testing.assert_array_equal(a, M.channels(3)[0])
    assert not np.array_equal(M.channels(5)[0][:, :7], M.channels(6)[0])  # another case, other draws


@pytest.mark.parametrize("extra", M.EXTRA)
def test_layout_builder(extra):
    """Records recovered exactly from every stride; gaps and guards NaN (SENTINEL for an output
    block)."""
    for case in (3, 6, 9):
        n, nch, _ = M.SHAPES[case]
        x = M.channels(case)[0]
        flat = M.records_strided(x, n + extra)
        assert flat.size == nch * (n + extra)
        np.testing.assert_array_equal(M.records_back(flat, nch, n, n + extra), x)
        assert np.isnan(flat.reshape(nch, n + extra)[:, n:]).all() and np.isnan(flat).sum() == nch * extra
        big, view = M.guarded(flat)
        assert big.size == flat.size + 2 * M.GUARD and np.shares_memory(big, view)
        assert np.isnan(big[:M.GUARD]).all() and np.isnan(big[-M.GUARD:]).all()
        np.testing.assert_array_equal(view, flat)
        out, _ = M.guarded(np.zeros(10), fill=M.SENTINEL)
        assert (out[:M.GUARD] == M.SENTINEL).all() and (out[-M.GUARD:] == M.SENTINEL).all()


def test_oracle_short_nbuf_is_the_prefix(cl):
    """nbuf < n / R: the oracle's snapshots are the first nbuf of the full run's (and with
    nbuf > n / R the rows past n / R stay as they were)."""
    for case in (1, 3, 4, 5, 7):
        n, nch, R = M.SHAPES[case]
        full, _ = M.oracle(case)
        nb = max(1, (n // R) // 2)
        assert nb < n // R
        x, x0, rv = M.channels(case)
        for c in (0, nch - 1):
            np.testing.assert_array_equal(S.c_states(cl, x[c], x0[c], rv[c], S.QD0, R, nb), full[c, :nb])
            more = S.c_states(cl, x[c], x0[c], rv[c], S.QD0, R, n // R + 2)
            np.testing.assert_array_equal(more[:n // R], full[c])
            assert (more[n // R:] == 0).all()


def test_expected_kernel_names():
    """The dispatch rule the GPU tests assert against (ekf_impl / ekf_seq_launch), on a 256-CU
    device."""
    t = M.tuning
    assert M.expected_kernel(130, 1607, 16, t("row_rot"), 256) == "ekf_rot_kernel"
    assert M.expected_kernel(130, 1607, 16, t("row"), 256) == "ekf_row_kernel"
    assert M.expected_kernel(130, 1607, 16, t("lane_rot"), 256) == "ekf_lane_rot_kernel"
    assert M.expected_kernel(130, 1607, 16, t("lane"), 256) == "ekf_kernel"
    assert M.expected_kernel(5, 4133, 7, t("row_rot"), 256) == "ekf_row_kernel"
    assert M.expected_kernel(4097, 100, 4, t("row_rot"), 256) == "ekf_lane_rot_kernel"
    assert M.expected_kernel(5, 4099, 1024, t("pit"), 256) == "ekf_pit (B=16, nb=257)"
    assert M.expected_kernel(5, 4099, 1024, t("pit", ekf_pit_block=49), 256) == "ekf_pit (B=49, nb=84)"
    assert M.expected_kernel(4, 9000, 3000, t("pit"), 256) == "ekf_pit (B=16, nb=563)"
    assert M.expected_kernel(5, 4095, 1024, t("pit"), 256) == "ekf_rot_kernel"
    assert M.expected_kernel(64, 400000, 4000, t("pit"), 256) == "ekf_pit (B=391, nb=1024)"
