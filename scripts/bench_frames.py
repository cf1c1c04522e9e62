"""Frame-interleaved int16 records against the planar int16 path: config-2-sized (100k buffers
x R = 4000 in total, ndata 10), split over nch = 2 / 4 / 8 channels of one (N, nch) int16 frames
tensor on the device. Per nch, three ways to the same fits, each timed as
scripts/bench_sample_dtype.py times its step (warm-up, then HIP events over --steps whole calls,
best of --runs windows; the three are timed in turn inside every window round, and the script
is run once per process: three processes give the alternating process triples):
  planar     dfmi_nls_record_typed on an already de-interleaved (nch, N) record: the byte floor
  transpose  what a caller without the frame entry points does: frames.T.contiguous() + planar
             (existing API only, so this row can be timed on an earlier tree too)
  frames     dfmi_nls_record_frames on the frames as they lie
and the demodulation alone (dfmi_demod_typed / dfmi_demod_frames) for its fraction of HBM peak.
FITOK_THRESHOLD and the amplitude guess are stated in counts, as bench_sample_dtype.py does.
One JSON line per (nch, way); `equal_to_planar_bits` compares the six columns and fitok.
usage: python scripts/bench_frames.py [--tag NAME] [--nch 2,4,8] [--steps 20] [--warmup 5] [--runs 3]"""
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
    ap.add_argument("--nch", default="2,4,8")
    ap.add_argument("--segments", type=int, default=100_000)
    ap.add_argument("--R", type=int, default=4000)
    ap.add_argument("--ndata", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()

    import torch

    from deepfmkit_amd import _lib
    from deepfmkit_amd import fit as F
    from deepfmkit_amd.fitters import w0_of
    from deepfmkit_amd.physics import SnrSpec, synth_snr

    lib = _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames.py needs a GPU")
    has_frames = "dfmi_nls_record_frames" in _lib.SYMBOLS  # an earlier tree: planar and transpose only
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    R, nd, w0 = args.R, args.ndata, w0_of(F_MOD, F_SAMP)
    F.FITOK_THRESHOLD *= SCALE ** 2
    cfg = F.lm_config()
    stream = torch.cuda.current_stream()
    st, D, I16 = stream.cuda_stream, _lib.DFMI_MEM_DEVICE, _lib.DFMI_I16

    for nch in [int(v) for v in args.nch.split(",")]:
        nbuf = args.segments // nch
        n, nseg = nbuf * R, nch * nbuf
        fr = torch.empty((n, nch), dtype=torch.int16, device=dev)
        x = torch.empty(n, dtype=torch.float64, device=dev)
        for c in range(nch):
            synth_snr(SnrSpec(seed=1234 + c, f_samp=F_SAMP, f_mod=F_MOD, m=6.0, phi=0.3 * c, snr_db=40.0), 0, n, out=x)
            fr[:, c] = torch.clamp(torch.round(SCALE * x), -32768, 32767).to(torch.int16)
        del x
        planar = fr.T.contiguous()
        g = np.tile([1.6 * SCALE, 6.0, 0.0, 0.0], (nch, 1))
        out = {w: torch.empty((6, nseg), dtype=torch.float64, device=dev) for w in ("planar", "transpose", "frames")}
        ok = {w: torch.empty(nseg, dtype=torch.int32, device=dev) for w in out}
        qi = torch.empty((2 * nd, nseg), dtype=torch.float64, device=dev)
        dc = torch.empty(nseg, dtype=torch.float64, device=dev)

        def planar_call(xp, w):
            _lib.check(lib.dfmi_nls_record_typed(xp.data_ptr(), I16, nch, n, nbuf, R, nd, w0, 0, _lib.ptr(g), 1, nbuf - 1,
                                                 cfg, out[w].data_ptr(), ok[w].data_ptr(), D, st), "dfmi_nls_record_typed")

        def frames_call():
            _lib.check(lib.dfmi_nls_record_frames(fr.data_ptr(), I16, nch, nch, nbuf, R, nd, w0, 0, _lib.ptr(g), 1,
                                                  nbuf - 1, cfg, out["frames"].data_ptr(), ok["frames"].data_ptr(), D, st),
                       "dfmi_nls_record_frames")

        steps = {"planar": lambda: planar_call(planar, "planar"),
                 "transpose": lambda: planar_call(fr.T.contiguous(), "transpose")}
        demods = {"planar": lambda: _lib.check(lib.dfmi_demod_typed(planar.data_ptr(), I16, nseg, R, R, nd, w0, 0,
                                                                    qi.data_ptr(), dc.data_ptr(), D, st), "demod")}
        if has_frames:
            steps["frames"] = frames_call
            demods["frames"] = lambda: _lib.check(lib.dfmi_demod_frames(fr.data_ptr(), I16, nch, nch, nbuf, R, nd, w0, 0,
                                                                        qi.data_ptr(), dc.data_ptr(), D, st), "demod")

        def window(f):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                f()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / args.steps

        kern, runs, druns = {}, {w: [] for w in steps}, {w: [] for w in demods}
        for w, f in list(steps.items()) + list(demods.items()):
            for _ in range(args.warmup):
                f()
            torch.cuda.synchronize()
            kern.setdefault(w, lib.dfmi_last_demod_kernel().decode())
        for _ in range(args.runs):  # the ways in turn inside every round
            for w, f in steps.items():
                runs[w].append(window(f))
            for w, f in demods.items():
                druns[w].append(window(f))
        torch.cuda.synchronize()
        ref = (out["planar"].cpu().numpy(), ok["planar"].cpu().numpy())
        nbytes = nseg * (R * 2 + 8 * (2 * nd + 1))
        for w in steps:
            line = {"bench": "frames", "tag": args.tag, "nch": nch, "way": w, "segments": nseg, "R": R, "ndata": nd,
                    "steps": args.steps, "warmup": args.warmup, "ms_per_step_best": round(min(runs[w]), 4),
                    "ms_per_step_runs": [round(v, 4) for v in runs[w]], "kernel": kern[w],
                    "ratio_to_planar": round(min(runs[w]) / min(runs["planar"]), 4),
                    "equal_to_planar_bits": bool(np.array_equal(out[w].cpu().numpy(), ref[0])
                                                 and np.array_equal(ok[w].cpu().numpy(), ref[1]))}
            if w in druns:
                line.update(demod_ms=round(min(druns[w]), 4), demod_ms_runs=[round(v, 4) for v in druns[w]],
                            demod_algorithmic_bytes=nbytes,
                            demod_frac_of_8TBps=round(nbytes / (min(druns[w]) * 1e-3) / HBM_PEAK, 4))
            print(json.dumps(line), flush=True)
        del fr, planar, out, ok, qi, dc


if __name__ == "__main__":
    main()
