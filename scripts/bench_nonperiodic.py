"""Records without a usable integer modulation period (dfmi_detect_period = 0), 100k segments, device-resident:
demod_blocks_kernel (tuning key "demod_blocks" = 1, the default) against the per-sample-sincos route
("demod_blocks" = 0: demod_direct_kernel, behind widen_rows for float32 / int16), and the 1 kHz / R = 4000 call of
the same ndata and type (the periodic kernels: the roofline to compare with). Shapes: f_mod 997 Hz, n = 20
(R = 4012) at ndata 10 / 30 / 62 for float64, float32 and int16; f_mod 100 Hz, n = 2 (R = 4000, period 2000) at
ndata 10. Timed as scripts/bench_hop.py times its step (warm-up, then HIP events over --steps whole calls, best of
--runs windows, the ways in turn inside every round), for the demodulation alone and for the nls_records step.
One JSON line per (shape, type, way). usage: python scripts/bench_nonperiodic.py [--tag NAME] [--steps 10]
[--warmup 3] [--runs 3] [--segments 100000]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, the figure bench.py's roofline uses
F_SAMP, SCALE = 200000.0, 4096.0
SHAPES = [(997.0, 20, 10), (997.0, 20, 30), (997.0, 20, 62), (100.0, 2, 10)]  # (f_mod, n, ndata)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="head")
    ap.add_argument("--types", default="float64,float32,int16")
    ap.add_argument("--segments", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--direct-steps", type=int, default=2, help="calls per window of the (slow) demod_blocks = 0 way")
    args = ap.parse_args()

    import torch

    from deepfmkit_amd import _lib
    from deepfmkit_amd import fit as F
    from deepfmkit_amd.fitters import _xtype, w0_of
    from deepfmkit_amd.physics import SnrSpec, synth_snr

    lib = _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nonperiodic.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream()
    st, D, thr0, nseg = stream.cuda_stream, _lib.DFMI_MEM_DEVICE, F.FITOK_THRESHOLD, args.segments

    def window(f, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(steps):
            f()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    for f_mod, n_per, nd in SHAPES:
        R = int(F_SAMP / f_mod * n_per)
        # way -> (f_mod, R, demod_blocks, calls per window)
        ways = {"blocks": (f_mod, R, 1, args.steps), "direct": (f_mod, R, 0, args.direct_steps),
                "periodic_1kHz": (1000.0, 4000, 1, args.steps)}
        xd = {}
        for fm, r in {(v[0], v[1]) for v in ways.values()}:
            xd[fm] = torch.empty(nseg * r, dtype=torch.float64, device=dev)
            synth_snr(SnrSpec(seed=1234, f_samp=F_SAMP, f_mod=fm, m=6.0, snr_db=40.0), 0, nseg * r, out=xd[fm])
        for dtype in args.types.split(","):
            if f_mod == 100.0 and dtype != "float64":
                continue
            i16 = dtype == "int16"
            cast = (lambda v: torch.clamp(torch.round(SCALE * v), -32768, 32767).to(torch.int16)) if i16 else (
                lambda v: v.to(getattr(torch, dtype)))
            x = {fm: cast(v) for fm, v in xd.items()}
            F.FITOK_THRESHOLD = thr0 * (SCALE ** 2 if i16 else 1.0)  # stated in counts, as bench_hop.py does
            cfg0, xt = F.lm_config(), _xtype(x[f_mod].dtype)
            g = np.array([[1.6 * (SCALE if i16 else 1.0), 6.0, 0.0, 0.0]])
            out = torch.empty((6, nseg), dtype=torch.float64, device=dev)
            ok = torch.empty(nseg, dtype=torch.int32, device=dev)
            qi = torch.empty((2 * nd, nseg), dtype=torch.float64, device=dev)
            dc = torch.empty(nseg, dtype=torch.float64, device=dev)

            def call(way, step):
                fm, r, key, _ = ways[way]
                _lib.check(lib.dfmi_set_tuning(b"demod_blocks", key), "tune")
                w0 = w0_of(fm, F_SAMP)
                if step:
                    _lib.check(lib.dfmi_nls_record_typed(x[fm].data_ptr(), xt, 1, nseg * r, nseg, r, nd, w0, 0, _lib.ptr(g),
                                                         1, nseg - 1, cfg0, out.data_ptr(), ok.data_ptr(), D, st), "record")
                else:
                    _lib.check(lib.dfmi_demod_typed(x[fm].data_ptr(), xt, nseg, r, r, nd, w0, 0, qi.data_ptr(),
                                                    dc.data_ptr(), D, st), "demod")

            kern, runs, druns = {}, {w: [] for w in ways}, {w: [] for w in ways}
            for w in ways:
                for _ in range(args.warmup if ways[w][2] else 1):
                    call(w, True)
                    call(w, False)
                torch.cuda.synchronize()
                kern[w] = lib.dfmi_last_demod_kernel().decode()
            for _ in range(args.runs):  # the ways in turn inside every round
                for w in ways:
                    runs[w].append(window(lambda: call(w, True), ways[w][3]))
                    druns[w].append(window(lambda: call(w, False), ways[w][3]))
            torch.cuda.synchronize()
            _lib.check(lib.dfmi_set_tuning(b"demod_blocks", 1), "tune")
            for w in ways:
                r = ways[w][1]
                nbytes = nseg * r * x[f_mod].element_size() + nseg * 8 * (2 * nd + 1)  # every sample once + the outputs
                print(json.dumps({"bench": "nonperiodic", "tag": args.tag, "dtype": dtype, "f_mod": ways[w][0], "R": r,
                                  "ndata": nd, "way": w, "segments": nseg, "steps": ways[w][3], "warmup": args.warmup,
                                  "ms_per_step_best": round(min(runs[w]), 4),
                                  "ms_per_step_runs": [round(v, 4) for v in runs[w]],
                                  "demod_ms": round(min(druns[w]), 4), "demod_ms_runs": [round(v, 4) for v in druns[w]],
                                  "demod_kernel": kern[w], "demod_algorithmic_bytes": nbytes,
                                  "demod_frac_of_8TBps": round(nbytes / (min(druns[w]) * 1e-3) / HBM_PEAK, 4)}), flush=True)
            del out, ok, qi, dc, x
        F.FITOK_THRESHOLD = thr0
        del xd


if __name__ == "__main__":
    main()
