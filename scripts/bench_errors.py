"""What the per-segment standard errors cost (dfmi_fisher, fit(errors=True)); one JSON line per
point, HIP events over timed windows after a warm-up as scripts/bench_sample_dtype.py.

  fisher   dfmi_fisher alone (sigma only, and all four outputs) on the device-resident result
           block of a config-2 record call (100k segments x R = 4000 @ 200 kS/s, 40 dB) at
           ndata 10, 30, 62, beside the LM's time of the same call (dfmi_step_timing)
  facade   DeepFitFramework.fit on the device-resident record with and without errors=True
           (wall clock, median)
  crlb     helpers.calculate_m_precision over the notebook grid (ndata 3..30 x 500 values of
           m, 80 dB) against the same loop in numpy / scipy on one core

usage: python scripts/bench_errors.py [--segments 100000] [--steps 20] [--warmup 5] [--runs 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F_SAMP, F_MOD = 200000.0, 1000.0


def numpy_m_precision(m_range, ndata, snr_db):
    """calculate_m_precision as a point-by-point numpy loop (the CPU cost being replaced)."""
    from deepfmkit_amd.helpers import calculate_jacobian
    var = (1.0 / 10 ** (snr_db / 20.0)) ** 2
    out = []
    for m in m_range:
        J = calculate_jacobian(ndata, np.array([1.0, m, np.pi / 4, 0.0]))
        try:
            out.append(np.sqrt(var * np.linalg.inv(J.T @ J)[1, 1]))
        except np.linalg.LinAlgError:
            out.append(np.inf)
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=100_000)
    ap.add_argument("--R", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()

    import torch

    import deepfmkit_amd as dfm
    from deepfmkit_amd import _lib, helpers
    from deepfmkit_amd import fit as F
    from deepfmkit_amd.fitters import w0_of
    from deepfmkit_amd.physics import SnrSpec, synth_snr

    lib = _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("bench_errors.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    nseg, R = args.segments, args.R
    x = torch.empty(nseg * R, dtype=torch.float64, device=dev)
    synth_snr(SnrSpec(seed=1234, f_samp=F_SAMP, f_mod=F_MOD, m=6.0, snr_db=40.0), 0, nseg * R, out=x)
    w0 = w0_of(F_MOD, F_SAMP)
    cfg = F.lm_config()
    g = np.array([[1.6, 6.0, 0.0, 0.0]])
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    out = torch.empty((6, nseg), dtype=torch.float64, device=dev)
    ok = torch.empty(nseg, dtype=torch.int32, device=dev)
    jtj = torch.empty((10, nseg), dtype=torch.float64, device=dev)
    cov = torch.empty((10, nseg), dtype=torch.float64, device=dev)
    sig = torch.empty((4, nseg), dtype=torch.float64, device=dev)
    fok = torch.empty(nseg, dtype=torch.int32, device=dev)

    def window(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / args.steps)
        return ms

    for nd in (10, 30, 62):
        def record():
            _lib.check(lib.dfmi_nls_record(x.data_ptr(), 1, nseg * R, nseg, R, nd, w0, 0, _lib.ptr(g), 1, nseg - 1, cfg,
                                           out.data_ptr(), ok.data_ptr(), _lib.DFMI_MEM_DEVICE, st), "dfmi_nls_record")

        def fisher(all_outputs):
            o = out.data_ptr()
            _lib.check(lib.dfmi_fisher(o, nseg, nseg, nd, o + 5 * nseg * 8, 1.0 / (2 * nd - 4),
                                       jtj.data_ptr() if all_outputs else None, cov.data_ptr() if all_outputs else None,
                                       sig.data_ptr(), fok.data_ptr() if all_outputs else None,
                                       _lib.DFMI_MEM_DEVICE, st), "dfmi_fisher")

        for _ in range(args.warmup):
            record()
        torch.cuda.synchronize()
        _lib.check(lib.dfmi_step_timing(1), "dfmi_step_timing")
        rec_ms = window(record)
        _lib.check(lib.dfmi_step_timing(0), "dfmi_step_timing")
        td, tl, tn = np.zeros(1), np.zeros(1), np.zeros(1, dtype=np.int64)
        _lib.check(lib.dfmi_step_timing_read(_lib.ptr(td), _lib.ptr(tl), _lib.ptr(tn)), "dfmi_step_timing_read")
        lm_ms, lm_src = (float(tl[0]) / int(tn[0]), "dfmi_step_timing") if int(tn[0]) else (None, None)
        if lm_ms is None:
            # not the fused pipeline: no marks. The demodulation launched alone (dfmi_demod) over the
            # same window; the LM (with the seed) is the rest of the step
            qi = torch.empty((2 * nd, nseg), dtype=torch.float64, device=dev)
            dc = torch.empty(nseg, dtype=torch.float64, device=dev)

            def demod_only():
                _lib.check(lib.dfmi_demod(x.data_ptr(), nseg, R, R, nd, w0, 0, qi.data_ptr(), dc.data_ptr(),
                                          _lib.DFMI_MEM_DEVICE, st), "dfmi_demod")

            lm_ms, lm_src = min(rec_ms) - min(window(demod_only)), "step minus dfmi_demod alone (seed included)"
            del qi, dc
        sig_ms = window(lambda: fisher(False))
        all_ms = window(lambda: fisher(True))
        torch.cuda.synchronize()
        print(json.dumps({"bench": "errors", "part": "fisher", "ndata": nd, "points": nseg, "steps": args.steps,
                          "warmup": args.warmup, "fisher_sigma_ms_runs": [round(v, 4) for v in sig_ms],
                          "fisher_sigma_ms_best": round(min(sig_ms), 4),
                          "fisher_all_outputs_ms_best": round(min(all_ms), 4),
                          "record_step_ms_best": round(min(rec_ms), 4),
                          "lm_ms_per_step": round(lm_ms, 4), "lm_timing": lm_src,
                          "demod_ms_per_step": round(float(td[0]) / int(tn[0]), 4) if int(tn[0]) else None,
                          "not_ok_points": int((fok == 0).sum()), "sigma_m_median": float(sig[1].median())}),
              flush=True)

    # the facade on the device-resident record
    dff = dfm.DeepFitFramework()
    raw = dfm.DeepRawObject()
    raw.data, raw.label, raw.f_samp, raw.f_mod, raw.t0 = x, "rec", F_SAMP, F_MOD, 0.0
    dff.raws["rec"] = raw
    wall = {}
    for name, kw in (("plain", {}), ("errors", {"errors": True})):
        ts = []
        for k in range(2 + 7):
            t0 = time.perf_counter()
            dff.fit("rec", n=20, **kw)
            if k >= 2:
                ts.append(time.perf_counter() - t0)
        wall[name] = ts
    print(json.dumps({"bench": "errors", "part": "facade", "segments": nseg, "R": R, "ndata": 10, "calls": 7,
                      "fit_ms_median": round(1e3 * float(np.median(wall["plain"])), 3),
                      "fit_errors_ms_median": round(1e3 * float(np.median(wall["errors"])), 3),
                      "fit_ms_all": [round(1e3 * v, 3) for v in wall["plain"]],
                      "fit_errors_ms_all": [round(1e3 * v, 3) for v in wall["errors"]]}), flush=True)
    del x, dff, raw

    # the CRLB sweep of the reference's notebook: 28 values of ndata x 500 values of m
    m = np.linspace(0.1, 30, 500)
    nds = list(range(3, 31))
    helpers.calculate_m_precision(m, 10, 80.0)
    t0 = time.perf_counter()
    ours = [helpers.calculate_m_precision(m, nd, 80.0) for nd in nds]
    t_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = [numpy_m_precision(m, nd, 80.0) for nd in nds]
    t_np = time.perf_counter() - t0
    rel = max(float(np.max(np.abs(a - b) / b)) for a, b in zip(ours, ref))
    print(json.dumps({"bench": "errors", "part": "crlb", "grid": [len(nds), len(m)], "calls": len(nds),
                      "calculate_m_precision_s": round(t_gpu, 5), "numpy_one_core_s": round(t_np, 4),
                      "speedup": round(t_np / t_gpu, 1), "max_rel_diff_vs_numpy": rel}), flush=True)


if __name__ == "__main__":
    main()
