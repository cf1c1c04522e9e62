"""What the log-frequency cross-spectral density costs (dfmi_lcsd) beside dfmi_lpsd on the same
two series stacked (nser = 2); one JSON line per size, printed and written to --out.

Device-resident white noise of N = 100,000 and 1,250,000 samples, default settings (Jdes 500,
Kdes 100, Kaiser 200 dB, order 0). Both C-ABI calls are timed on device memory with outputs
allocated beforehand and the plan made once (each call includes the sort and upload of its
table): HIP events around each warm call, the median of `--runs` calls after `--warmup`. The pair
call evaluates one sincos per sample product where the two-series call evaluates two, so it
should cost less; `lcsd_python_ms` is deepfmkit_amd.lpsd.lcsd as users call it (plan, outputs,
complex results, H and the residual included).

usage: python scripts/bench_lcsd.py [--runs 7] [--warmup 2] [--sizes 100000 1250000] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS = 50.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_250_000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lcsd", "bench_lcsd.jsonl"))
    args = ap.parse_args()

    import torch

    from deepfmkit_amd import _lib
    from deepfmkit_amd import lpsd as M

    if not torch.cuda.is_available():
        raise SystemExit("bench_lcsd.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream()
    lib = _lib.load()

    def timed(call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    lines = []
    for N in args.sizes:
        xy = torch.from_numpy(1e-3 * np.random.RandomState(N % 1000).randn(2, N)).to(dev)
        p = M.plan(N, FS)
        J = int(p.f.size)
        plan_args = (N, FS, _lib.ptr(p.b), _lib.ptr(p.L), _lib.ptr(p.K), J, 0, 200.0)
        out = torch.empty((5, J), dtype=torch.float64, device=dev)
        sxx2 = torch.empty((2, J), dtype=torch.float64, device=dev)
        enbw = torch.empty(J, dtype=torch.float64, device=dev)

        def pair():
            _lib.check(lib.dfmi_lcsd(xy[0].data_ptr(), N, xy[1].data_ptr(), N, 1, *plan_args,
                                     *(out[i].data_ptr() for i in range(5)), enbw.data_ptr(), _lib.DFMI_MEM_DEVICE,
                                     stream.cuda_stream), "dfmi_lcsd")

        def two_series():
            _lib.check(lib.dfmi_lpsd(xy.data_ptr(), 2, N, *plan_args, sxx2.data_ptr(), enbw.data_ptr(),
                                     _lib.DFMI_MEM_DEVICE, stream.cuda_stream), "dfmi_lpsd")

        t_lpsd, t_pair = timed(two_series), timed(pair)
        t_py = timed(lambda: M.lcsd(xy[0], xy[1], FS))
        same = bool(torch.equal(out[0], sxx2[0]) and torch.equal(out[1], sxx2[1]))
        med = {k: float(np.median(v)) for k, v in (("lpsd2", t_lpsd), ("lcsd", t_pair), ("py", t_py))}
        lines.append(json.dumps({
            "bench": "lcsd", "N": N, "J": J, "segments": int(p.K.sum()), "sample_products": int((p.L * p.K).sum()),
            "runs": args.runs, "warmup": args.warmup,
            "lcsd_pair_ms": round(med["lcsd"], 4), "lcsd_pair_ms_all": [round(v, 4) for v in t_pair],
            "lpsd_two_series_ms": round(med["lpsd2"], 4), "lpsd_two_series_ms_all": [round(v, 4) for v in t_lpsd],
            "pair_over_two_series": round(med["lcsd"] / med["lpsd2"], 4), "lcsd_python_ms": round(med["py"], 4),
            "sxx_syy_bits_equal_lpsd": same, "median_coh": round(float(out[4].median()), 5)}))
        print(lines[-1], flush=True)
        del xy
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
