"""Windowed demodulation (dfmi_demod_window: demod_window_kernel) against the rectangular call
(dfmi_demod_typed, the bin kernels) on the same device-resident record in the same process: 100k segments of
R = 4000 at 1 kHz / 200 kS/s, ndata 10, float64 / float32 / int16, Hann (K = 1) and Blackman-Harris (K = 3).
Timed as scripts/bench_nonperiodic.py times its demodulation (warm-up, then HIP events over --steps whole calls,
best of --runs windows, the ways in turn inside every round). One JSON line per (type, window) with the ratio to
the rectangular call and the fraction of 8 TB/s. usage: python scripts/bench_window.py [--tag NAME] [--steps 10]
[--warmup 3] [--runs 3] [--segments 100000] >> profiles/window_bench.jsonl"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, the figure bench.py's roofline uses
F_SAMP, F_MOD, R, ND, SCALE = 200000.0, 1000.0, 4000, 10, 4096.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="head")
    ap.add_argument("--types", default="float64,float32,int16")
    ap.add_argument("--windows", default="hann,blackmanharris")
    ap.add_argument("--segments", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()

    import torch

    from deepfmkit_amd import _lib
    from deepfmkit_amd.fitters import _xtype, w0_of
    from deepfmkit_amd.physics import SnrSpec, synth_snr

    lib = _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("bench_window.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream()
    st, D, nseg, w0 = stream.cuda_stream, _lib.DFMI_MEM_DEVICE, args.segments, w0_of(F_MOD, F_SAMP)

    def window(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            f()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    xd = torch.empty(nseg * R, dtype=torch.float64, device=dev)
    synth_snr(SnrSpec(seed=1234, f_samp=F_SAMP, f_mod=F_MOD, m=6.0, snr_db=40.0), 0, nseg * R, out=xd)
    qi = torch.empty((2 * ND, nseg), dtype=torch.float64, device=dev)
    dc = torch.empty(nseg, dtype=torch.float64, device=dev)
    for dtype in args.types.split(","):
        x = (torch.clamp(torch.round(SCALE * xd), -32768, 32767).to(torch.int16) if dtype == "int16"
             else xd.to(getattr(torch, dtype)))
        xt = _xtype(x.dtype)
        coef = {w: _lib.window_coefficients(w) for w in args.windows.split(",")}

        def call(way):
            if way == "rect":
                _lib.check(lib.dfmi_demod_typed(x.data_ptr(), xt, nseg, R, R, ND, w0, 0, qi.data_ptr(), dc.data_ptr(), D,
                                                st), "demod")
            else:
                a = coef[way]
                _lib.check(lib.dfmi_demod_window(x.data_ptr(), xt, nseg, R, R, ND, w0, 0, _lib.ptr(a), a.size,
                                                 qi.data_ptr(), dc.data_ptr(), D, st), "demod_window")

        ways = ["rect"] + list(coef)
        kern, runs = {}, {w: [] for w in ways}
        for w in ways:
            for _ in range(args.warmup):
                call(w)
            torch.cuda.synchronize()
            kern[w] = lib.dfmi_last_demod_kernel().decode()
        for _ in range(args.runs):  # the ways in turn inside every round
            for w in ways:
                runs[w].append(window(lambda: call(w)))
        torch.cuda.synchronize()
        nbytes = nseg * R * x.element_size() + nseg * 8 * (2 * ND + 1)  # every sample once + the outputs
        for w in ways:
            print(json.dumps({"bench": "window", "tag": args.tag, "dtype": dtype, "window": w, "R": R, "ndata": ND,
                              "segments": nseg, "steps": args.steps, "warmup": args.warmup,
                              "demod_ms": round(min(runs[w]), 4), "demod_ms_runs": [round(v, 4) for v in runs[w]],
                              "ratio_to_rect": round(min(runs[w]) / min(runs["rect"]), 4), "demod_kernel": kern[w],
                              "demod_algorithmic_bytes": nbytes,
                              "demod_frac_of_8TBps": round(nbytes / (min(runs[w]) * 1e-3) / HBM_PEAK, 4)}), flush=True)
        del x


if __name__ == "__main__":
    main()
