"""Workgroup prologue of the bin demodulation (csrc/demod.h bins_kernel_body) from the probe
buffer, at the benchmark's step (config 2: dfmi_nls_record over NSEG segments of R = 4000,
ndata 10): per workgroup the time from entry to the first sample load issued and to the first
contraction begun, the workgroup's life, and the spread of the wave exits, for demod_spw in SPW
(default 0,1,2). Workgroups of the first generation (all resident slots start at once) and the
later ones (dispatched into a saturated memory system) are reported apart.
DFMI_LIB=path measures another build of the library (an A/B build with
-DDFMI_BINS_LATE_STAGE=0 stages the basis at entry). One JSON line per setting."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from deepfmkit_amd import _lib  # noqa: E402
from deepfmkit_amd import fit as F  # noqa: E402
from deepfmkit_amd.fitters import w0_of  # noqa: E402

if os.environ.get("DFMI_LIB"):
    _lib.LIB_PATH = os.environ["DFMI_LIB"]
KW, WPB = 16384, 4
KG = KW // WPB
STAMPS = 16 + 2 * KW
N = STAMPS + 3 * KG
lib = _lib.load()
dev = torch.device("cuda", 0)
nseg, R, nd = int(os.environ.get("NSEG", 100000)), 4000, 10
x = bench.gen_shard(torch, dev, 0, nseg, R, seed=bench.SEED)
st = torch.cuda.current_stream()
out = torch.empty((6, nseg), dtype=torch.float64, device=dev)
ok = torch.empty(nseg, dtype=torch.int32, device=dev)
cfg = F.lm_config()
g = np.array([1.6, 6.0, 0.0, 0.0])
slots = 3 * torch.cuda.get_device_properties(0).multi_processor_count


def step():
    _lib.check(lib.dfmi_nls_record(x.data_ptr(), 1, nseg * R, nseg, R, nd, w0_of(1000.0, 200000.0), 0, g.ctypes.data,
                                   1, nseg - 1, cfg, out.data_ptr(), ok.data_ptr(), _lib.DFMI_MEM_DEVICE,
                                   st.cuda_stream), "step")


def pct(v):
    return {"n": int(v.size), "median": round(float(np.median(v)), 3), "p10": round(float(np.percentile(v, 10)), 3),
            "p90": round(float(np.percentile(v, 90)), 3), "max": round(float(v.max()), 3)} if v.size else {"n": 0}


for spw in [int(s) for s in os.environ.get("SPW", "0,1,2").split(",")]:
    _lib.check(lib.dfmi_set_tuning(b"demod_spw", spw), "spw")
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(50):
        step()
    e1.record(st)
    e1.synchronize()
    ms = e0.elapsed_time(e1) / 50
    _lib.check(lib.dfmi_set_tuning(b"probe", 0), "p")
    _lib.check(lib.dfmi_set_tuning(b"probe", 1), "p")
    step()
    torch.cuda.synchronize()
    pr = (ctypes.c_int64 * N)()
    _lib.check(lib.dfmi_probe_read(pr, N), "read")
    _lib.check(lib.dfmi_set_tuning(b"probe", 0), "p")
    a = np.frombuffer(pr, dtype=np.int64)
    t0 = a[3]
    ex = a[16:16 + KW]
    fin = (ex[ex > 0] - t0) / 100.0  # us (100 MHz counter)
    ent, ld, con = (a[STAMPS + k * KG: STAMPS + (k + 1) * KG] for k in range(3))
    m = (ent > 0) & (con > 0)
    wg = np.arange(KG)
    last = ex[:KW].reshape(KG, WPB).max(axis=1)  # the workgroup's last wave out
    res = {"lib": os.environ.get("DFMI_LIB", "default"), "kernel": lib.dfmi_last_demod_kernel().decode(),
           "nseg": nseg, "demod_spw": spw, "step_ms": round(ms, 4), "probed_workgroups": int(m.sum()),
           "wave_exit_us": {"min": round(float(fin.min()), 1), "median": round(float(np.median(fin)), 1),
                            "max": round(float(fin.max()), 1)}}
    for name, sel in (("first_generation", m & (wg < slots)), ("later", m & (wg >= slots))):
        have_ld = sel & (ld > 0)
        res[name] = {"entry_to_first_load_us": pct((ld[have_ld] - ent[have_ld]) / 100.0),
                     "entry_to_first_contraction_us": pct((con[sel] - ent[sel]) / 100.0),
                     "workgroup_life_us": pct((last[sel & (last > 0)] - ent[sel & (last > 0)]) / 100.0)}
    print(json.dumps(res), flush=True)
