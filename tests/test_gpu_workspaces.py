"""Per-stream workspaces of libdfmi.so (dfmi_capi.hip workspace()): a call from one more caller
stream than "ws_streams" (default 4) waits for the device, frees the least recently used stream's
set and allocates its own; dfmi_release_workspaces frees every set. Neither may change a result:
one device record fitted by dfmi_nls_record on the default stream, then on six non-default streams
in turn for two rounds (every call of the second round evicts), then once more after a release;
every output and fitok is compared bit for bit with the first call's."""
import numpy as np
import pytest

from deepfmkit_amd import _lib
from deepfmkit_amd import fit as _fit

pytestmark = pytest.mark.gpu

NBUF, R, NDATA, PERIOD = 8, 400, 10, 200
W0 = 2.0 * np.pi / PERIOD
NSTREAM, ROUNDS = 6, 2
SENT = -7.25e77  # sentinel (exactly representable, never a result)


def record(torch):
    """One float64 device record of NBUF segments: the reference signal model at slowly drifting
    parameters plus seeded noise."""
    rng = np.random.RandomState(20260)
    t = np.arange(NBUF * R, dtype=np.float64)
    seg = np.floor(t / R)
    m = 6.0 + 0.02 * seg
    phi = 0.3 + 0.05 * seg
    x = 0.2 + 1.6 * np.cos(phi + m * np.cos(W0 * t + 0.1)) + 1e-3 * rng.standard_normal(t.size)
    return torch.from_numpy(x).cuda()


def fit(lib, x, guess, cfg, stream, out, ok):
    """dfmi_nls_record (DFMI_MEM_DEVICE) on `stream` (None: the default stream) into out / ok."""
    _lib.check(lib.dfmi_nls_record(x.data_ptr(), 1, NBUF * R, NBUF, R, NDATA, W0, 0, _lib.ptr(guess), 1, NBUF - 1, cfg,
                                   out.data_ptr(), ok.data_ptr(), _lib.DFMI_MEM_DEVICE,
                                   None if stream is None else stream.cuda_stream), "dfmi_nls_record")
    return out, ok


def test_stream_eviction_and_release_keep_results():
    import torch
    lib = _lib.load()
    val = np.zeros(1, dtype=np.int64)
    _lib.check(lib.dfmi_get_tuning(b"ws_streams", _lib.ptr(val)), "dfmi_get_tuning")
    assert val[0] == 4  # the default: six streams in turn evict on every call of the second round
    x = record(torch)
    guess = np.array([[1.6, 6.0, 0.0, 0.0]])
    cfg = _fit.lm_config()
    # every call's own sentinel-filled outputs, filled before any call: the fills run on the default
    # stream, which the other streams do not wait for
    ncall = 1 + NSTREAM * ROUNDS + 1
    outs = torch.full((ncall, 6, NBUF), SENT, dtype=torch.float64, device=x.device)
    oks = torch.full((ncall, NBUF), -5, dtype=torch.int32, device=x.device)
    torch.cuda.synchronize()
    ref_out, ref_ok = fit(lib, x, guess, cfg, None, outs[0], oks[0])
    torch.cuda.synchronize()
    ref_out, ref_ok = ref_out.cpu().numpy(), ref_ok.cpu().numpy()
    assert ref_ok.min() >= 0 and np.isfinite(ref_out).all() and (ref_out != SENT).all()  # no sentinel left
    streams = [torch.cuda.Stream() for _ in range(NSTREAM)]
    assert len({s.cuda_stream for s in streams} | {0}) == NSTREAM + 1  # distinct, none the default
    got = []
    for rnd in range(ROUNDS):
        for k, s in enumerate(streams):
            i = 1 + rnd * NSTREAM + k
            got.append((f"round {rnd} stream {k}",) + fit(lib, x, guess, cfg, s, outs[i], oks[i]))
    _lib.check(lib.dfmi_release_workspaces(), "dfmi_release_workspaces")
    got.append(("after release",) + fit(lib, x, guess, cfg, None, outs[-1], oks[-1]))
    torch.cuda.synchronize()
    for what, out, ok in got:
        o, k = out.cpu().numpy(), ok.cpu().numpy()
        assert np.array_equal(k, ref_ok), what
        assert np.array_equal(o.view(np.uint64), ref_out.view(np.uint64)), \
            f"{what}: max |diff| {np.max(np.abs(o - ref_out)):.3e}"
