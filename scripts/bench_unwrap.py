"""Times dfmi_unwrap's two geometries beside a plain device copy of the same x -> y bytes.

Every shape is device resident. Per shape, in one process and alternating within each round:
  copy     y.copy_(x): the floor, 8 B read + 8 B written per point
  series   unwrap_path = 1, one workgroup per series
  tiled    unwrap_path = 2, three launches over tiles of 1,024 points
  default  unwrap_path = 0, what the host picks
Times are device events around `inner` back-to-back calls, the median over the rounds, after a
warm-up round of every variant. One JSON line per shape: ms, points per second and the ratio to
the copy. The second block sweeps the series count at N = 100k: the smallest count from which
the series kernel is no slower than the tiled path is the crossover the default rule states.
usage: python scripts/bench_unwrap.py [--out profiles/unwrap_bench.jsonl] [--rounds 7]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 100_000), (3, 100_000), (1, 1_250_000), (3, 1_250_000), (1, 10_000_000), (3, 10_000_000),
          (1024, 100_000)]
SWEEP = [(n, 100_000) for n in (16, 32, 64, 128, 256, 512)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unwrap_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    from deepfmkit_amd import _lib, unwrap
    if not torch.cuda.is_available():
        raise SystemExit("bench_unwrap needs a GPU: nothing is measured without one")
    lib = _lib.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def run(variant, x, y):
        if variant == "copy":
            y.copy_(x)
            return
        _lib.check(lib.dfmi_unwrap(x.data_ptr(), x.shape[0], x.shape[1], x.shape[1], 2 * np.pi, None, 0, 1, 0,
                                   y.data_ptr(), x.shape[1], None, 0, _lib.DFMI_MEM_DEVICE,
                                   torch.cuda.current_stream().cuda_stream), "dfmi_unwrap")

    paths = {"series": 1, "tiled": 2, "default": 0}
    with open(args.out, "w") as f:
        for block, shapes in (("shape", SHAPES), ("sweep", SWEEP)):
            for nser, N in shapes:
                g = torch.Generator(device="cuda").manual_seed(nser * 31 + N)
                ramp = 2.1 * torch.arange(N, device="cuda", dtype=torch.float64)
                x = torch.remainder(ramp + 0.1 * torch.randn((nser, N), generator=g, device="cuda", dtype=torch.float64)
                                    + np.pi, 2 * np.pi) - np.pi
                y = torch.empty_like(x)
                inner = max(3, int(1e9 // (nser * N)))  # about 16 GB of traffic per timing
                times = {v: [] for v in ["copy"] + list(paths)}
                for rnd in range(args.rounds + 1):
                    for v in times:
                        _lib.check(lib.dfmi_set_tuning(b"unwrap_path", paths.get(v, 0)), "dfmi_set_tuning")
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(inner):
                            run(v, x, y)
                        e1.record()
                        e1.synchronize()
                        if rnd:  # round 0 warms every variant up
                            times[v].append(e0.elapsed_time(e1) / inner)
                lib.dfmi_set_tuning(b"unwrap_path", 0)
                ref = unwrap(x[:1, :4096].contiguous())  # the timed output is an unwrapped ramp
                assert float((y[0, :4096] - ref[0]).abs().max()) == 0.0
                ms = {v: float(np.median(t)) for v, t in times.items()}
                rec = {"block": block, "nser": nser, "N": N, "inner": inner, "rounds": args.rounds,
                       "ms": ms, "spread_ms": {v: [float(min(t)), float(max(t))] for v, t in times.items()},
                       "gpoints_per_s": {v: nser * N / m / 1e6 for v, m in ms.items()},
                       "copy_gb_per_s": 16e-6 * nser * N / ms["copy"],
                       "ratio_to_copy": {v: ms[v] / ms["copy"] for v in paths}}
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec))
                del x, y
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
