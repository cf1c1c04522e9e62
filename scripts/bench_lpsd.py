"""What the log-frequency spectral density costs (dfmi_lpsd); one JSON line per point.

  device   deepfmkit_amd.lpsd.lpsd on device-resident white noise of N = 100,000 and 1,250,000
           samples, default settings (Jdes 500, Kdes 100, Kaiser 200 dB, order 0), 1 and 3
           series: HIP events around each warm call, the median of `--runs` calls (the call
           includes the host plan and the upload of its tables)
  numpy    the numpy restatement of the definition (tests/helpers/lpsd_ref.py) at N = 100,000
           on one host core, and the largest relative difference of the device's Sxx from it

usage: python scripts/bench_lpsd.py [--runs 7] [--warmup 2] [--sizes 100000 1250000] [--no-numpy]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
FS = 50.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_250_000])
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()

    import torch

    from deepfmkit_amd import lpsd as M

    if not torch.cuda.is_available():
        raise SystemExit("bench_lpsd.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream()
    for N in args.sizes:
        host = 1e-3 * np.random.RandomState(N % 1000).randn(3, N)
        x = torch.from_numpy(host).to(dev)
        p = M.plan(N, FS)
        for nser in (1, 3):
            xs = x[0] if nser == 1 else x
            for _ in range(args.warmup):
                r = M.lpsd(xs, FS)
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                r = M.lpsd(xs, FS)
                e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            level = float(np.median(r.Sxx.cpu().numpy() / (2 * 1e-6 / FS)))
            print(json.dumps({"bench": "lpsd", "part": "device", "N": N, "nser": nser, "J": int(p.f.size),
                              "window_samples": int(p.L.sum()), "segments": int(p.K.sum()),
                              "sample_products": int((p.L * p.K).sum()) * nser, "runs": args.runs,
                              "warmup": args.warmup, "ms_median": round(float(np.median(ms)), 4),
                              "ms_min": round(min(ms), 4), "ms_all": [round(v, 4) for v in ms],
                              "gproducts_per_s": round(int((p.L * p.K).sum()) * nser / np.median(ms) / 1e6, 2),
                              "median_Sxx_over_white_level": round(level, 4)}), flush=True)
        if N == 100_000 and not args.no_numpy:
            import lpsd_ref as R
            t0 = time.perf_counter()
            ref = R.lpsd(host[0], FS)
            t_np = time.perf_counter() - t0
            ours = M.lpsd(x[0], FS).Sxx.cpu().numpy()
            print(json.dumps({"bench": "lpsd", "part": "numpy", "N": N, "nser": 1,
                              "numpy_restatement_one_core_s": round(t_np, 3),
                              "max_rel_diff_device_vs_numpy": float(np.max(np.abs(ours / ref["Sxx"] - 1)))}),
                  flush=True)
        del x


if __name__ == "__main__":
    main()
