"""Coloured asd-mode trial synthesis on the GPU (dfmi_synth_asd_coloured) in trials per second
at N = 4000 and N = 200,000 samples per trial, against two baselines:
  (a) the host generator (numpy + scipy.signal.lfilter, SignalGenerator.generate) on one core;
  (b) the white-only dfmi_synth_asd at the same N (the same trials without f_n / arml_mod_n).
Also the bare basis series (dfmi_plnoise). One JSON line per N, appended to --out
(default profiles/plnoise/bench_plnoise.jsonl).

  python scripts/bench_plnoise.py [--out FILE] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _cfg(dfm, coloured):
    laser = dfm.LaserConfig()
    laser.amp_n = 1e-4
    ifo = dfm.InterferometerConfig()
    if coloured:
        laser.f_n = 1e6
        ifo.arml_mod_n = 1e-12
    dfm.set_laser_df_for_effect(laser, ifo, 6.0)
    return dfm.DFMIObject("main", laser, ifo)


def _median_s(fn, reps):
    import torch
    fn()  # warm-up: workspaces, code objects
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plnoise", "bench_plnoise.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    import deepfmkit_amd as dfm
    from deepfmkit_amd import physics as P
    assert torch.cuda.is_available(), "bench_plnoise.py needs a GPU"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for n, ntrial, nhost in ((4000, 2048, 8), (200000, 256, 2)):
        n_seconds = n / 200000.0
        col, white = _cfg(dfm, True), _cfg(dfm, False)
        tns = list(range(ntrial))
        t_col = _median_s(lambda: P.synthesize_asd_trials([col] * ntrial, tns, n_seconds), a.reps)
        t_white = _median_s(lambda: P.synthesize_asd_trials([white] * ntrial, tns, n_seconds), a.reps)
        t_basis = _median_s(lambda: P.alpha_noise(200000.0, n, 2.0, tns, device="cuda"), a.reps)
        P.SignalGenerator().generate(col, n_seconds, mode="asd", trial_num=0)  # warm-up: imports, the design
        t0 = time.perf_counter()
        for t in range(nhost):
            P.SignalGenerator().generate(col, n_seconds, mode="asd", trial_num=t)
        t_host = (time.perf_counter() - t0) / nhost
        row = {"n": n, "ntrial": ntrial, "nsec": int(len(P.alpha_noise_design(200000.0, n, 2.0)[0])),
               "device": torch.cuda.get_device_name(0),
               "coloured_trials_per_s": ntrial / t_col[0], "coloured_s": t_col,
               "white_trials_per_s": ntrial / t_white[0], "white_s": t_white,
               "basis_series_per_s": ntrial / t_basis[0], "basis_s": t_basis,
               "host_trials_per_s": 1.0 / t_host, "host_trials_timed": nhost,
               "coloured_vs_host": (ntrial / t_col[0]) * t_host, "coloured_vs_white": t_white[0] / t_col[0]}
        print(json.dumps(row))
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
