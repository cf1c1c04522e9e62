"""Overlapped-segment readout (dfmi_nls_record_hop / dfmi_demod_hop) on a config-2 record (100k x R = 4000
samples, L = 200, ndata 10), device-resident, int16 and float64, V = R / hop = 2, 4, 8. Per (type, V) three ways
to the same points, each timed as scripts/bench_frames.py times its step (warm-up, then HIP events over --steps
whole calls, best of --runs windows, the ways in turn inside every round), for the step and the demodulation alone:
  native    the hop calls at the default tuning (demod_hop_kernel where it applies)
  inplace   "demod_hop" = 0: the planar kernels at seg_stride = hop
  gathered  what a caller without the hop entry points does: the windows gathered (unfold + contiguous), then
            the planar typed call on the copy
and `disjoint`: the non-overlapped step on the same record (hop = R, the planar call: the parent's step).
One JSON line per (type, V, way). usage: python scripts/bench_hop.py [--tag NAME] [--steps 10] [--warmup 3] [--runs 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, the figure bench.py's roofline uses
F_SAMP, F_MOD, SCALE = 200000.0, 1000.0, 4096.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="head")
    ap.add_argument("--types", default="int16,float64")
    ap.add_argument("--V", default="2,4,8")
    ap.add_argument("--segments", type=int, default=100_000)
    ap.add_argument("--R", type=int, default=4000)
    ap.add_argument("--ndata", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()

    import torch

    from deepfmkit_amd import _lib
    from deepfmkit_amd import fit as F
    from deepfmkit_amd.fitters import _xtype, w0_of
    from deepfmkit_amd.physics import SnrSpec, synth_snr

    lib = _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hop.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    R, nd, w0, n = args.R, args.ndata, w0_of(F_MOD, F_SAMP), args.segments * args.R
    cfg0, thr0 = None, F.FITOK_THRESHOLD
    stream = torch.cuda.current_stream()
    st, D = stream.cuda_stream, _lib.DFMI_MEM_DEVICE
    xd = torch.empty(n, dtype=torch.float64, device=dev)
    synth_snr(SnrSpec(seed=1234, f_samp=F_SAMP, f_mod=F_MOD, m=6.0, snr_db=40.0), 0, n, out=xd)

    def window(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            f()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    for dtype in args.types.split(","):
        i16 = dtype == "int16"
        x = torch.clamp(torch.round(SCALE * xd), -32768, 32767).to(torch.int16) if i16 else xd
        F.FITOK_THRESHOLD = thr0 * (SCALE ** 2 if i16 else 1.0)  # stated in counts, as bench_frames.py does
        cfg0, xt = F.lm_config(), _xtype(x.dtype)
        g = np.array([[1.6 * (SCALE if i16 else 1.0), 6.0, 0.0, 0.0]])
        for V in [1] + [int(v) for v in args.V.split(",")]:  # V = 1: the disjoint step
            hop = R // V
            nseg = (n - R) // hop + 1
            out = torch.empty((6, nseg), dtype=torch.float64, device=dev)
            ok = torch.empty(nseg, dtype=torch.int32, device=dev)
            qi = torch.empty((2 * nd, nseg), dtype=torch.float64, device=dev)
            dc = torch.empty(nseg, dtype=torch.float64, device=dev)

            def tune(v):
                _lib.check(lib.dfmi_set_tuning(b"demod_hop", v), "tune")

            def hop_step(v):
                tune(v)
                _lib.check(lib.dfmi_nls_record_hop(x.data_ptr(), xt, 1, n, nseg, R, hop, nd, w0, 0, _lib.ptr(g), 1, nseg - 1,
                                                   cfg0, out.data_ptr(), ok.data_ptr(), D, st), "dfmi_nls_record_hop")

            def hop_demod(v):
                tune(v)
                _lib.check(lib.dfmi_demod_hop(x.data_ptr(), xt, 1, n, nseg, R, hop, nd, w0, 0, qi.data_ptr(), dc.data_ptr(),
                                              D, st), "dfmi_demod_hop")

            def gathered(step):
                y = x.unfold(0, R, hop).contiguous()
                if step:
                    _lib.check(lib.dfmi_nls_record_typed(y.data_ptr(), xt, 1, nseg * R, nseg, R, nd, w0, 0, _lib.ptr(g), 1,
                                                         nseg - 1, cfg0, out.data_ptr(), ok.data_ptr(), D, st), "record")
                else:
                    _lib.check(lib.dfmi_demod_typed(y.data_ptr(), xt, nseg, R, R, nd, w0, 0, qi.data_ptr(), dc.data_ptr(), D,
                                                    st), "demod")

            if V == 1:
                ways = {"disjoint": (lambda: hop_step(1), lambda: hop_demod(1))}
            else:
                ways = {"native": (lambda: hop_step(1), lambda: hop_demod(1)),
                        "inplace": (lambda: hop_step(0), lambda: hop_demod(0)),
                        "gathered": (lambda: gathered(True), lambda: gathered(False))}
            kern, runs, druns = {}, {w: [] for w in ways}, {w: [] for w in ways}
            for w, (fs, fd) in ways.items():
                for _ in range(args.warmup):
                    fs()
                    fd()
                torch.cuda.synchronize()
                kern[w] = lib.dfmi_last_demod_kernel().decode()
            for _ in range(args.runs):  # the ways in turn inside every round
                for w, (fs, fd) in ways.items():
                    runs[w].append(window(fs))
                    druns[w].append(window(fd))
            torch.cuda.synchronize()
            tune(1)
            nbytes = n * x.element_size() + nseg * 8 * (2 * nd + 1)  # every sample once + the outputs
            for w in ways:
                print(json.dumps({"bench": "hop", "tag": args.tag, "dtype": dtype, "V": V, "hop": hop, "way": w,
                                  "segments": nseg, "R": R, "ndata": nd, "steps": args.steps, "warmup": args.warmup,
                                  "ms_per_step_best": round(min(runs[w]), 4),
                                  "ms_per_step_runs": [round(v, 4) for v in runs[w]],
                                  "demod_ms": round(min(druns[w]), 4), "demod_ms_runs": [round(v, 4) for v in druns[w]],
                                  "demod_kernel": kern[w], "demod_algorithmic_bytes": nbytes,
                                  "demod_frac_of_8TBps": round(nbytes / (min(druns[w]) * 1e-3) / HBM_PEAK, 4)}), flush=True)
            del out, ok, qi, dc


if __name__ == "__main__":
    main()
