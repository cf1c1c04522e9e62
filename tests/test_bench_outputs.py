"""bench.py's plain run and --dump-outputs: a plain run prints the headline line only
(everything that takes runs of its own is behind --full) and --dump-outputs DIR writes
what the last timed step returned, one .npy per result column, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "kernels_ms", "window_breakdown", "per_rank_kernels_ms", "batch_status0_frac", "batch_m_mean",
             "scaling_anchor", "extra_configs", "cpu_baseline", "cpu_baseline_c", "parity")


def test_dump_outputs_columns_and_fixed_sample(tmp_path, monkeypatch):
    """The six columns in float64 and the status in float32, one file each; beyond
    DUMP_MAX_SEGMENTS a sample of the segments that is the same at every call, ascending,
    with its positions beside it."""
    torch = pytest.importorskip("torch")
    import bench
    n = 37
    out = torch.arange(6 * n, dtype=torch.float64).reshape(6, n)
    ok = (torch.arange(n, dtype=torch.int32) % 3)
    bench.dump_outputs(str(tmp_path / "all"), out, ok)
    assert sorted(os.listdir(tmp_path / "all")) == sorted([c + ".npy" for c in bench.DUMP_COLUMNS] + ["fitok.npy"])
    for c, name in enumerate(bench.DUMP_COLUMNS):
        a = np.load(tmp_path / "all" / (name + ".npy"))
        assert a.dtype == np.float64 and np.array_equal(a, out[c].numpy())
    st = np.load(tmp_path / "all" / "fitok.npy")
    assert st.dtype == np.float32 and np.array_equal(st, ok.numpy().astype(np.float32))
    monkeypatch.setattr(bench, "DUMP_MAX_SEGMENTS", 5)
    bench.dump_outputs(str(tmp_path / "s1"), out, ok)
    bench.dump_outputs(str(tmp_path / "s2"), out, ok)
    idx = np.load(tmp_path / "s1" / "segment_index.npy")
    assert idx.shape == (5,) and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    for f in os.listdir(tmp_path / "s1"):
        assert np.array_equal(np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f)), f
    assert np.array_equal(np.load(tmp_path / "s1" / "m.npy"), out[1].numpy()[idx.astype(int)])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    """`bench.py --gpus 1 --steps 3 --warmup 1` on 3,000 segments: the headline keys, none of
    --full's, ms_per_step consistent with value, and the dumped columns are the fit of the
    batch (every status 0, m = 6 to 1e-3 in the mean, as the --full line's own check asks)."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nseg = 3000
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--segments", str(nseg), "--dump-outputs", str(tmp_path / "dump")]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [v for v in p.stdout.strip().splitlines() if v.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert all(k in line for k in HEADLINE) and not [k for k in FULL_ONLY if k in line], sorted(line)
    assert line["steps"] == 3 and line["unit"] == "segments/s" and line["dtype"] == "f64" and line["higher_is_better"]
    assert line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / nseg - 1.0) < 1e-2  # both rounded to 4 digits at least
    cols = {f[:-4]: np.load(tmp_path / "dump" / f) for f in os.listdir(tmp_path / "dump")}
    assert sorted(cols) == sorted(("amp", "m", "phi", "psi", "dc", "ssq", "fitok"))
    assert all(v.shape == (nseg,) for v in cols.values())
    assert cols["fitok"].dtype == np.float32 and np.all(cols["fitok"] == 0)
    assert all(cols[k].dtype == np.float64 and np.all(np.isfinite(cols[k])) for k in ("amp", "m", "phi", "psi", "dc", "ssq"))
    assert abs(cols["m"].mean() - 6.0) < 1e-3
