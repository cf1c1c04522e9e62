"""dfmi_residual on device-resident records, 100k segments: the 1 kHz / R = 4000 record as float64, float32 and
int16 with and without the residual record, and the 997 Hz / R = 4012 record (no integer period: the rotating
evaluator) as float64. Beside every time: its algorithmic bytes (every sample once, the parameters, the outputs)
over 8 TB/s, and dfmi_demod_typed's time on the same record (same bytes read: the yardstick the project has).
HIP events over --steps whole calls, best of --runs windows after warm-up, the ways in turn inside every round.
One JSON line per (record, type, way). usage: python scripts/bench_residual.py [--tag NAME] [--steps 10]
[--warmup 3] [--runs 3] [--segments 100000]"""
import argparse
import json
import os
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, the figure bench.py's roofline uses
F_SAMP, SCALE, NDATA = 200000.0, 4096.0, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="head")
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
        raise SystemExit("bench_residual.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream()
    st, D, nseg = stream.cuda_stream, _lib.DFMI_MEM_DEVICE, args.segments

    def window(f, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(steps):
            f()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    for f_mod, R, dtypes in ((1000.0, 4000, ("float64", "float32", "int16")), (997.0, 4012, ("float64",))):
        w0 = w0_of(f_mod, F_SAMP)
        xd = torch.empty(nseg * R, dtype=torch.float64, device=dev)
        synth_snr(SnrSpec(seed=1234, f_samp=F_SAMP, f_mod=f_mod, m=6.0, snr_db=40.0), 0, nseg * R, out=xd)
        resid = torch.empty((nseg, R), dtype=torch.float64, device=dev)
        for dtype in dtypes:
            i16 = dtype == "int16"
            x = torch.clamp(torch.round(SCALE * xd), -32768, 32767).to(torch.int16) if i16 else xd.to(getattr(torch, dtype))
            xt = _xtype(x.dtype)
            # parameters near the record's: the arithmetic does not depend on how well they fit
            blk = torch.empty((5, nseg), dtype=torch.float64, device=dev)
            blk[:4] = torch.tensor([1.6 * (SCALE if i16 else 1.0), 6.0, 0.3, 0.1], dtype=torch.float64, device=dev)[:, None]
            qi = torch.empty((2 * NDATA, nseg), dtype=torch.float64, device=dev)
            out3 = torch.empty((2, nseg), dtype=torch.float64, device=dev)
            ip = torch.empty(nseg, dtype=torch.int32, device=dev)

            def demod():
                _lib.check(lib.dfmi_demod_typed(x.data_ptr(), xt, nseg, R, R, NDATA, w0, 0, qi.data_ptr(),
                                                blk[4].data_ptr(), D, st), "demod")

            def residual(with_resid):
                _lib.check(lib.dfmi_residual(x.data_ptr(), xt, nseg, R, R, w0, 0, blk.data_ptr(), nseg, blk[4].data_ptr(),
                                             out3[0].data_ptr(), out3[1].data_ptr(), ip.data_ptr(),
                                             resid.data_ptr() if with_resid else None, R, D, st), "residual")

            ways = {"demod_typed": demod, "residual": lambda: residual(False), "residual+resid": lambda: residual(True)}
            read = nseg * R * x.element_size()
            nbytes = {"demod_typed": read + nseg * 8 * (2 * NDATA + 1), "residual": read + nseg * (5 * 8 + 20),
                      "residual+resid": read + nseg * (5 * 8 + 20) + nseg * R * 8}
            runs = {w: [] for w in ways}
            for f in ways.values():
                for _ in range(args.warmup):
                    f()
            torch.cuda.synchronize()
            for _ in range(args.runs):
                for w, f in ways.items():
                    runs[w].append(window(f, args.steps))
            torch.cuda.synchronize()
            rms = float(torch.sqrt(out3[0] / R).median())
            for w in ways:
                best = min(runs[w])
                print(json.dumps({"bench": "residual", "tag": args.tag, "dtype": dtype, "f_mod": f_mod, "R": R, "way": w,
                                  "segments": nseg, "steps": args.steps, "warmup": args.warmup, "ms_best": round(best, 4),
                                  "ms_runs": [round(v, 4) for v in runs[w]], "algorithmic_bytes": nbytes[w],
                                  "ms_at_8TBps": round(nbytes[w] / HBM_PEAK * 1e3, 4),
                                  "frac_of_8TBps": round(nbytes[w] / (best * 1e-3) / HBM_PEAK, 4),
                                  "demod_kernel": lib.dfmi_last_demod_kernel().decode() if w == "demod_typed" else None,
                                  "median_rms": rms}), flush=True)
            del x, blk, qi, out3, ip
        del xd, resid


if __name__ == "__main__":
    main()
