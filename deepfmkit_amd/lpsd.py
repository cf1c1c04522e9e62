"""Log-frequency spectral density (LPSD) of a series on the GPU.

The reference computes the spectrum of the fitted phase with `spectools.lpsd`
(data.py:239-244, core.py:590-609). Here the estimator is the project's own definition
(after Tröbs & Heinzel 2006 and LTPDA's ltf_plan): parity with spectools is
NOT pinned, because that package is not available to test against.

  plan(N, fs, ...)     the frequency plan, on the host (dfmi_lpsd_plan): f, fres, b, L, K
  lpsd(x, fs, ...)     the spectrum of one series or of (nser, N) series that share the plan,
                       one dfmi_lpsd call (windows, per-segment DFT bins and sums in HIP)
  lcsd(x, y, fs, ...)  the cross-spectral density, coherence, transfer estimate and residual of
                       two series (or of one x against many y) on the same plan, one dfmi_lcsd
                       call

Only the Kaiser window (win=np.kaiser or 'kaiser') and order 0 (segment mean removed) or -1
(nothing removed) are supported; anything else raises ValueError. There is no CPU fallback:
without a GPU lpsd raises DFMIError.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import _lib

LPSDResult = namedtuple("LPSDResult", "f Sxx asd enbw L K b")
LPSDPlan = namedtuple("LPSDPlan", "f fres b L K")
LCSDResult = namedtuple("LCSDResult", "f Sxx Syy Sxy coh H resid enbw L K b")


def kaiser_alpha(psll):
    """The Kaiser parameter alpha of a peak side-lobe level of `psll` dB (window beta = pi alpha)."""
    p = float(psll) / 100.0
    return ((0.0889732 * p - 0.493285) * p + 4.71469) * p - 0.0821377


def default_olap(psll):
    """olap='default': the recommended overlap (a fraction) of the Kaiser window of `psll` dB."""
    a = kaiser_alpha(psll)
    return (100.0 - 1.0 / (((4.42204e-05 * a - 0.000925946) * a + 0.00912223) * a + 0.0061076)) / 100.0


def _olap(olap, psll):
    if isinstance(olap, str):
        if olap != "default":
            raise ValueError(f"olap: a fraction in [0, 1) or 'default', got {olap!r}")
        return default_olap(psll)
    return float(olap)


def _check_settings(order, win, psll):
    if not (win is np.kaiser or (isinstance(win, str) and win.lower() == "kaiser")):
        raise ValueError("lpsd: only the Kaiser window is supported (win=np.kaiser or 'kaiser')")
    if order not in (0, -1):
        raise ValueError("lpsd: order must be 0 (segment mean removed) or -1 (nothing removed)")
    pa = np.pi * kaiser_alpha(psll)
    if not 0.0 < pa <= 64.0:
        raise ValueError(f"lpsd: psll = {psll} is outside the Kaiser fit's range (0 < pi alpha <= 64)")


def plan(N, fs, olap="default", bmin=1, Lmin=0, Jdes=500, Kdes=100, psll=200):
    """The frequency plan of a series of N samples at rate fs (host only)."""
    lib = _lib.load()
    args = (int(N), float(fs), _olap(olap, psll), float(bmin), int(Lmin), int(Jdes), int(Kdes))
    J = lib.dfmi_lpsd_plan(*args, None, None, None, None, None, 0)
    if J < 0:
        raise ValueError("lpsd plan: need N >= 8, fs > 0, 0 <= olap < 1, bmin > 0, Jdes >= 1, Kdes >= 1 "
                         f"(N={args[0]}, fs={args[1]}, olap={args[2]}, bmin={args[3]}, Jdes={args[5]}, Kdes={args[6]})")
    f, fres, b = np.empty(J), np.empty(J), np.empty(J)
    L, K = np.empty(J, dtype=np.int64), np.empty(J, dtype=np.int64)
    got = lib.dfmi_lpsd_plan(*args, _lib.ptr(f), _lib.ptr(fres), _lib.ptr(b), _lib.ptr(L), _lib.ptr(K), J)
    if got != J:
        raise _lib.DFMIError(f"dfmi_lpsd_plan returned {got} after counting {J}")
    return LPSDPlan(f, fres, b, L, K)


def _is_device_tensor(x):
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def lpsd(x, fs, olap="default", bmin=1, Lmin=0, Jdes=500, Kdes=100, order=0, win=np.kaiser, psll=200):
    """LPSD of x: a numpy array or a CUDA float64 tensor, 1-D or (nser, N).

    Returns LPSDResult(f, Sxx, asd, enbw, L, K, b): Sxx is the one-sided power spectral density
    (shape (J,) for 1-D input, (nser, J) otherwise), asd = sqrt(Sxx), enbw the equivalent
    noise bandwidth per frequency; f, L, K, b are the plan (numpy). For device input Sxx, asd
    and enbw are tensors on the input's device, enqueued on its current stream."""
    _check_settings(order, win, psll)
    lib = _lib.load()
    one = x.dim() == 1 if _is_device_tensor(x) else np.ndim(x) == 1
    if _is_device_tensor(x):
        import torch
        if x.dtype != torch.float64:
            raise ValueError("device series must be float64")
        x2 = x.reshape(1, -1) if one else x
        if x2.dim() != 2:
            raise ValueError("x must be 1-D or (nser, N)")
        if x2.stride(1) != 1 or (x2.shape[0] > 1 and x2.stride(0) < x2.shape[1]):
            x2 = x2.contiguous()
    else:
        x2 = np.ascontiguousarray(x, dtype=np.float64)
        x2 = x2.reshape(1, -1) if one else x2
        if x2.ndim != 2:
            raise ValueError("x must be 1-D or (nser, N)")
    nser, N = int(x2.shape[0]), int(x2.shape[1])
    if nser < 1:
        raise ValueError("x holds no series")
    p = plan(N, fs, olap, bmin, Lmin, Jdes, Kdes, psll)
    J = p.f.size
    if _is_device_tensor(x):
        import torch
        Sxx = torch.empty((nser, J), dtype=torch.float64, device=x2.device)
        enbw = torch.empty(J, dtype=torch.float64, device=x2.device)
        with torch.cuda.device(x2.device):
            rc = lib.dfmi_lpsd(x2.data_ptr(), nser, int(x2.stride(0)) if nser > 1 else N, N, float(fs), _lib.ptr(p.b),
                               _lib.ptr(p.L), _lib.ptr(p.K), J, int(order), float(psll), Sxx.data_ptr(),
                               enbw.data_ptr(), _lib.DFMI_MEM_DEVICE, torch.cuda.current_stream(x2.device).cuda_stream)
        _lib.check(rc, "dfmi_lpsd")
        asd = torch.sqrt(Sxx)
    else:
        Sxx, enbw = np.empty((nser, J)), np.empty(J)
        rc = lib.dfmi_lpsd(_lib.ptr(x2), nser, N, N, float(fs), _lib.ptr(p.b), _lib.ptr(p.L), _lib.ptr(p.K), J,
                           int(order), float(psll), _lib.ptr(Sxx), _lib.ptr(enbw), _lib.DFMI_MEM_HOST, None)
        _lib.check(rc, "dfmi_lpsd")
        asd = np.sqrt(Sxx)
    if one:
        Sxx, asd = Sxx[0], asd[0]
    return LPSDResult(p.f, Sxx, asd, enbw, p.L, p.K, p.b)


def _series_2d(x, name):
    """x as (nser, N) rows the C ABI can read (a device tensor's row stride may exceed N), and
    whether it came 1-D."""
    if _is_device_tensor(x):
        import torch
        if x.dtype != torch.float64:
            raise ValueError("device series must be float64")
        one = x.dim() == 1
        x2 = x.reshape(1, -1) if one else x
        if x2.dim() != 2:
            raise ValueError(f"{name} must be 1-D or (nser, N)")
        if x2.stride(1) != 1 or (x2.shape[0] > 1 and x2.stride(0) < x2.shape[1]):
            x2 = x2.contiguous()
    else:
        one = np.ndim(x) == 1
        x2 = np.ascontiguousarray(x, dtype=np.float64)
        x2 = x2.reshape(1, -1) if one else x2
        if x2.ndim != 2:
            raise ValueError(f"{name} must be 1-D or (nser, N)")
    if x2.shape[0] < 1:
        raise ValueError(f"{name} holds no series")
    return x2, one


def lcsd(x, y, fs, olap="default", bmin=1, Lmin=0, Jdes=500, Kdes=100, order=0, win=np.kaiser, psll=200):
    """Cross-spectral density and coherence of x and y on lpsd's frequency plan:
    numpy arrays or CUDA float64 tensors (both the same kind), 1-D, or (nser, N) with both 2-D of
    equal shape, or a 1-D x against a 2-D y (one x shared by every row of y). One dfmi_lcsd call.

    Returns LCSDResult(f, Sxx, Syy, Sxy, coh, H, resid, enbw, L, K, b): Sxy = 2 mean conj(A) B /
    (fs sum w^2) (complex, scipy.signal.csd's convention), coh = |Sxy|^2 / (Sxx Syy) (not
    clamped; NaN where Sxx Syy = 0), H = Sxy / Sxx the x -> y transfer estimate, resid =
    Syy (1 - coh) the density of y without its x-coherent part. Shapes (J,) for two 1-D inputs,
    (nser, J) otherwise; for device input the spectra are tensors on the input's device,
    enqueued on its current stream. f, L, K, b are the plan (numpy)."""
    _check_settings(order, win, psll)
    lib = _lib.load()
    dev = _is_device_tensor(x)
    if dev != _is_device_tensor(y) or (dev and x.device != y.device):
        raise ValueError("lcsd: x and y must both be numpy arrays or both be tensors on one device")
    x2, xone = _series_2d(x, "x")
    y2, yone = _series_2d(y, "y")
    npair, N = int(y2.shape[0]), int(y2.shape[1])
    if int(x2.shape[1]) != N:
        raise ValueError(f"lcsd: x and y differ in length ({int(x2.shape[1])} and {N})")
    if not (xone or int(x2.shape[0]) == npair) or (yone and not xone):
        raise ValueError("lcsd: x and y must have equal shapes, or x must be 1-D against a 2-D y")
    p = plan(N, fs, olap, bmin, Lmin, Jdes, Kdes, psll)
    J = p.f.size
    plan_args = (N, float(fs), _lib.ptr(p.b), _lib.ptr(p.L), _lib.ptr(p.K), J, int(order), float(psll))
    if dev:
        import torch
        out = torch.empty((5, npair, J), dtype=torch.float64, device=y2.device)
        enbw = torch.empty(J, dtype=torch.float64, device=y2.device)
        xs = 0 if xone else (int(x2.stride(0)) if npair > 1 else N)
        ys = int(y2.stride(0)) if npair > 1 else N
        with torch.cuda.device(y2.device):
            rc = lib.dfmi_lcsd(x2.data_ptr(), xs, y2.data_ptr(), ys, npair, *plan_args,
                               *(out[i].data_ptr() for i in range(5)), enbw.data_ptr(), _lib.DFMI_MEM_DEVICE,
                               torch.cuda.current_stream(y2.device).cuda_stream)
        _lib.check(rc, "dfmi_lcsd")
        cplx = torch.complex
    else:
        out, enbw = np.empty((5, npair, J)), np.empty(J)
        rc = lib.dfmi_lcsd(_lib.ptr(x2), 0 if xone else N, _lib.ptr(y2), N, npair, *plan_args,
                           *(_lib.ptr(out[i]) for i in range(5)), _lib.ptr(enbw), _lib.DFMI_MEM_HOST, None)
        _lib.check(rc, "dfmi_lcsd")

        def cplx(re, im):
            z = np.empty(re.shape, dtype=np.complex128)
            z.real, z.imag = re, im
            return z
    Sxx, Syy, coh = out[0], out[1], out[4]
    with np.errstate(divide="ignore", invalid="ignore"):  # Sxx = 0 or NaN is no error: H is inf or NaN there
        Sxy, H = cplx(out[2], out[3]), cplx(out[2] / Sxx, out[3] / Sxx)  # componentwise: the same bits on both paths
    resid = Syy * (1.0 - coh)
    if xone and yone:
        Sxx, Syy, Sxy, coh, H, resid = Sxx[0], Syy[0], Sxy[0], coh[0], H[0], resid[0]
    return LCSDResult(p.f, Sxx, Syy, Sxy, coh, H, resid, enbw, p.L, p.K, p.b)
