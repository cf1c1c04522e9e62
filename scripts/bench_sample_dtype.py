"""float32 and int16 against float64 sample records on the headline step: config 2 (100k
segments x R = 4000 @ 200 kS/s) at ndata 10, 30 and 62, the SAME values as float64 and as float32
(the record is generated, cast to float32 once, and the float64 copy is that cast widened
back, so both dtypes fit the same numbers and their results must be equal bit for bit).
The int16 rows fit the same record quantised as a 12-bit-scale ADC would,
clamp(round(4096 x), -32768, 32767), from an amplitude guess of 1.6 * 4096 counts and with
FITOK_THRESHOLD stated in counts^2 (1e-3 * 4096^2: ssq is in counts^2, and at the volts-scale
threshold every segment would take the m-grid retry, a different LM workload), and are
compared bit for bit with one (untimed) float64 call on the widened counts: "int16" is the
default path, "int16-ldsbins" the same call with the tuning key demod_i16_int = 0 (the
float kernels' LDS-bin fold instead of the integer-accumulating fold of the bin kernels).

Device-resident (timed as bench.py times its step: warm-up, then HIP events over --steps
whole dfmi_nls_record(_typed) calls, repeated --runs times; dfmi_step_timing gives the
demodulation / LM split where the pipeline is the fused one, otherwise the demodulation is
timed alone through dfmi_demod(_typed)) and host-resident (pinned host buffers through
DFMI_MEM_HOST, PCIe-inclusive, as scripts/bench_host_input.py). One JSON line per point.

Copied into a checkout from before the typed entry points, the script times that tree's
float64 points only (--tag names the tree in the output lines).
usage: python scripts/bench_sample_dtype.py [--tag NAME] [--ndata 10,30,62] [--steps 20] [--warmup 5]
                                            [--runs 3] [--no-host] [--dtypes float64,float32,int16,int16-ldsbins]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, the figure bench.py's roofline uses
F_SAMP, F_MOD = 200000.0, 1000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="head")
    ap.add_argument("--ndata", default="10,30,62")
    ap.add_argument("--segments", type=int, default=100_000)
    ap.add_argument("--R", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--dtypes", default="float64,float32,int16,int16-ldsbins")
    args = ap.parse_args()

    import torch

    from deepfmkit_amd import _lib
    typed = "dfmi_nls_record_typed" in _lib.SYMBOLS  # a tree from before the typed calls: float64 only
    from deepfmkit_amd import fit as F
    from deepfmkit_amd.fitters import w0_of
    from deepfmkit_amd.physics import SnrSpec, synth_snr

    lib = _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample_dtype.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    nseg, R = args.segments, args.R
    x = torch.empty(nseg * R, dtype=torch.float64, device=dev)
    synth_snr(SnrSpec(seed=1234, f_samp=F_SAMP, f_mod=F_MOD, m=6.0, snr_db=40.0), 0, nseg * R, out=x)
    x32 = x.float()
    x64 = x32.double()
    i16 = typed and hasattr(_lib, "DFMI_I16")  # a tree from before int16 records: the float points only
    x16 = torch.clamp(torch.round(4096.0 * x), -32768, 32767).to(torch.int16) if i16 else None
    del x
    want = args.dtypes.split(",")
    # name -> (samples, sample type or None for the untyped call, demod_i16_int, scale of amp and sqrt(ssq))
    variants = [("float64", x64, None, None, 1.0)]
    if typed:
        variants.append(("float32", x32, _lib.DFMI_F32, None, 1.0))
    if i16:
        variants += [("int16", x16, _lib.DFMI_I16, 1, 4096.0), ("int16-ldsbins", x16, _lib.DFMI_I16, 0, 4096.0)]
    variants = [v for v in variants if v[0] in want]
    w0 = w0_of(F_MOD, F_SAMP)
    thr0 = F.FITOK_THRESHOLD
    cfg = F.lm_config()
    g = np.array([[1.6, 6.0, 0.0, 0.0]])

    def select(scale, key):
        nonlocal cfg
        g[0, 0] = 1.6 * scale
        F.FITOK_THRESHOLD = thr0 * scale ** 2
        cfg = F.lm_config()
        if key is not None:
            _lib.check(lib.dfmi_set_tuning(b"demod_i16_int", key), "dfmi_set_tuning")
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    out = torch.empty((6, nseg), dtype=torch.float64, device=dev)
    ok = torch.empty(nseg, dtype=torch.int32, device=dev)

    def record_call(xp, xtype, nd, o, k, mem):
        if xtype is not None:
            rc = lib.dfmi_nls_record_typed(xp, xtype, 1, nseg * R, nseg, R, nd, w0, 0, _lib.ptr(g), 1, nseg - 1,
                                           cfg, o, k, mem, st if mem == _lib.DFMI_MEM_DEVICE else None)
        else:
            rc = lib.dfmi_nls_record(xp, 1, nseg * R, nseg, R, nd, w0, 0, _lib.ptr(g), 1, nseg - 1, cfg, o, k, mem,
                                     st if mem == _lib.DFMI_MEM_DEVICE else None)
        _lib.check(rc, "dfmi_nls_record")

    results = {}
    for nd in [int(v) for v in args.ndata.split(",")]:
        qi = torch.empty((2 * nd, nseg), dtype=torch.float64, device=dev)
        dc = torch.empty(nseg, dtype=torch.float64, device=dev)
        for name, xt, xtype, key, scale in variants:
            select(scale, key)
            if name == "int16" or (name == "int16-ldsbins" and (nd, "counts") not in results):
                # the comparand of the int16 rows: the float64 fit of the widened counts, untimed
                xw = xt.double()
                record_call(xw.data_ptr(), None, nd, out.data_ptr(), ok.data_ptr(), _lib.DFMI_MEM_DEVICE)
                torch.cuda.synchronize()
                results[(nd, "counts")] = (out.cpu().numpy().copy(), ok.cpu().numpy().copy())
                del xw

            def step():
                record_call(xt.data_ptr(), xtype, nd, out.data_ptr(), ok.data_ptr(), _lib.DFMI_MEM_DEVICE)

            def demod_only():
                if xtype is not None:
                    rc = lib.dfmi_demod_typed(xt.data_ptr(), xtype, nseg, R, R, nd, w0, 0, qi.data_ptr(),
                                              dc.data_ptr(), _lib.DFMI_MEM_DEVICE, st)
                else:
                    rc = lib.dfmi_demod(xt.data_ptr(), nseg, R, R, nd, w0, 0, qi.data_ptr(), dc.data_ptr(),
                                        _lib.DFMI_MEM_DEVICE, st)
                _lib.check(rc, "dfmi_demod")

            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            kname = lib.dfmi_last_demod_kernel().decode()
            runs = []
            for _ in range(args.runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                _lib.check(lib.dfmi_step_timing(1), "dfmi_step_timing")
                e0.record(stream)
                for _ in range(args.steps):
                    step()
                e1.record(stream)
                e1.synchronize()
                _lib.check(lib.dfmi_step_timing(0), "dfmi_step_timing")
                td, tl, tn = np.zeros(1), np.zeros(1), np.zeros(1, dtype=np.int64)
                _lib.check(lib.dfmi_step_timing_read(_lib.ptr(td), _lib.ptr(tl), _lib.ptr(tn)), "dfmi_step_timing_read")
                run = {"ms_per_step": e0.elapsed_time(e1) / args.steps}
                if int(tn[0]) == args.steps:  # the fused pipeline marks its two launches
                    run["demod_ms"], run["lm_ms"] = float(td[0]) / args.steps, float(tl[0]) / args.steps
                    run["demod_timing"] = "dfmi_step_timing (events around the step's own launch)"
                else:
                    for _ in range(args.warmup):
                        demod_only()
                    e0.record(stream)
                    for _ in range(args.steps):
                        demod_only()
                    e1.record(stream)
                    e1.synchronize()
                    run["demod_ms"] = e0.elapsed_time(e1) / args.steps
                    run["demod_timing"] = "the demodulation launched alone (dfmi_demod), events over the window"
                    run["demod_kernel"] = lib.dfmi_last_demod_kernel().decode()
                runs.append(run)
            best = min(runs, key=lambda r: r["ms_per_step"])
            bytes_demod = nseg * (R * xt.element_size() + 8 * (2 * nd + 1))
            torch.cuda.synchronize()
            results[(nd, name)] = (out.cpu().numpy().copy(), ok.cpu().numpy().copy())
            line = {"bench": "sample_dtype", "tag": args.tag, "residency": "device", "dtype": name, "ndata": nd,
                    "segments": nseg, "R": R, "steps": args.steps, "warmup": args.warmup,
                    "ms_per_step_best": round(best["ms_per_step"], 4),
                    "ms_per_step_runs": [round(r["ms_per_step"], 4) for r in runs],
                    "segments_per_s": round(nseg / (best["ms_per_step"] * 1e-3), 1), "kernel": kname,
                    "demod_ms": round(best["demod_ms"], 4), "lm_ms": round(best["lm_ms"], 4) if "lm_ms" in best else None,
                    "demod_ms_runs": [round(r["demod_ms"], 4) for r in runs], "demod_timing": best["demod_timing"],
                    "demod_kernel": best.get("demod_kernel", kname), "demod_algorithmic_bytes": bytes_demod,
                    "demod_GBps": round(bytes_demod / (best["demod_ms"] * 1e-3) / 1e9, 1),
                    "demod_frac_of_8TBps": round(bytes_demod / (best["demod_ms"] * 1e-3) / HBM_PEAK, 4)}
            ref = (nd, "float64") if name == "float32" else (nd, "counts") if name.startswith("int16") else None
            if ref in results:
                a, b = results[ref], results[(nd, name)]
                line["equal_to_float64_bits"] = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
            print(json.dumps(line), flush=True)
        del qi, dc

    if args.no_host:
        return
    nd = 10
    for name, xt, xtype, key, scale in variants:
        select(scale, key)
        xh = xt.cpu().pin_memory()
        oh = np.empty((6, nseg))
        kh = np.empty(nseg, dtype=np.int32)

        def call():
            record_call(xh.data_ptr(), xtype, nd, _lib.ptr(oh), _lib.ptr(kh), _lib.DFMI_MEM_HOST)

        call()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            call()  # returns after the results are back on the host (the library synchronises)
            ts.append(time.perf_counter() - t0)
        t = float(np.median(ts))
        nbytes = nseg * R * xh.element_size()
        ref = results.get((nd, name))
        print(json.dumps({"bench": "sample_dtype", "tag": args.tag, "residency": "host (pinned), PCIe-inclusive",
                          "dtype": name, "ndata": nd, "segments": nseg, "R": R, "calls": 5,
                          "seconds_median": round(t, 6), "seconds_all": [round(v, 6) for v in ts],
                          "segments_per_s": round(nseg / t, 1), "bytes_h2d": nbytes,
                          "h2d_GBps_effective": round(nbytes / t / 1e9, 2),
                          "equal_to_device_path": None if ref is None else bool(np.array_equal(oh, ref[0]))}), flush=True)
        del xh


if __name__ == "__main__":
    main()
