"""Operations on fitted series on the GPU.

  unwrap(x, period, status, ...)   removes the jumps of a multiple of `period` from one series or
                                   from (nser, N) series, stepping over invalid points (failed
                                   fits, non-finite samples): one dfmi_unwrap call, an exact
                                   integer scan in HIP

`fit()` returns phi wrapped to (-pi, pi] (reference fit.py:359-360); a record that moves more
than half a wavelength gives a sawtooth, and this is the step between the fit and its spectrum.
There is no CPU fallback: without a GPU unwrap raises DFMIError.
"""
from __future__ import annotations

import numpy as np

from . import _lib

FILLS = {"nan": 0, "hold": 1}


def _is_device_tensor(x):
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def _rows(a, dev, np_dtype, name):
    """a as (nser, N) rows of np_dtype that the C ABI can read in place where their layout is
    legal (unit element stride, a row stride of at least N elements), a contiguous copy
    otherwise: (rows, row stride in elements, came 1-D)."""
    if dev:
        import torch
        if not _is_device_tensor(a):
            raise ValueError(f"unwrap: {name} must be a tensor on x's device")
        a = a.to(getattr(torch, np.dtype(np_dtype).name))
        one = a.dim() == 1
        a2 = a.reshape(1, -1) if one else a
        if a2.dim() != 2:
            raise ValueError(f"{name} must be 1-D or (nser, N)")
        if a2.stride(1) != 1 or (a2.shape[0] > 1 and a2.stride(0) < a2.shape[1]):
            a2 = a2.contiguous()
        return a2, int(a2.stride(0)), one
    if _is_device_tensor(a):
        raise ValueError(f"unwrap: {name} must be a numpy array, as x is")
    a = np.asarray(a, dtype=np_dtype)
    one = a.ndim == 1
    a2 = a.reshape(1, -1) if one else a
    if a2.ndim != 2:
        raise ValueError(f"{name} must be 1-D or (nser, N)")
    item = a2.itemsize
    unit = a2.shape[1] <= 1 or a2.strides[1] == item
    rows = a2.shape[0] <= 1 or (a2.strides[0] % item == 0 and a2.strides[0] >= a2.shape[1] * item)
    if not (unit and rows):
        a2 = np.ascontiguousarray(a2)
    return a2, a2.strides[0] // item, one


def unwrap(x, period=2 * np.pi, status=None, max_status=1, fill="nan", cycles=False):
    """x with its jumps of a multiple of `period` removed: a numpy array or a CUDA float64 tensor,
    1-D or (nser, N); rows with a stride are read in place.

    A point is valid when x is finite and, with `status` (integers of x's shape, a fit's fitok),
    0 <= status <= max_status. The first valid point keeps its value; every later valid point is
    moved by the whole number of periods that brings it within period / 2 of the valid point
    before it, so invalid points are stepped over. At invalid points y is NaN (fill="nan") or
    holds the last valid y, the first valid y before any (fill="hold"). y - x is an exact
    multiple of period: y = fma(cycles, period, x).

    Returns y, or (y, cycles) with cycles=True (int64). Device input gives tensors on the same
    device, enqueued on its current stream."""
    if fill not in FILLS:
        raise ValueError(f"fill: one of {sorted(FILLS)}, got {fill!r}")
    lib = _lib.load()
    dev = _is_device_tensor(x)
    if dev and str(x.dtype) != "torch.float64":
        raise ValueError("device series must be float64")
    x2, xs, one = _rows(x, dev, np.float64, "x")
    nser, N = int(x2.shape[0]), int(x2.shape[1])
    s2, ss = None, 0
    if status is not None:
        s2, ss, _ = _rows(status, dev, np.int32, "status")
        if tuple(s2.shape) != (nser, N):
            raise ValueError(f"status has shape {tuple(s2.shape)}, x has {(nser, N)}")
    if dev:
        import torch
        y = torch.empty((nser, N), dtype=torch.float64, device=x2.device)
        c = torch.empty((nser, N), dtype=torch.int64, device=x2.device) if cycles else None
        with torch.cuda.device(x2.device):
            rc = lib.dfmi_unwrap(x2.data_ptr(), nser, xs, N, float(period), _lib.ptr(s2), ss, int(max_status),
                                 FILLS[fill], y.data_ptr(), N, _lib.ptr(c), N, _lib.DFMI_MEM_DEVICE,
                                 torch.cuda.current_stream(x2.device).cuda_stream)
    else:
        y = np.empty((nser, N))
        c = np.empty((nser, N), dtype=np.int64) if cycles else None
        rc = lib.dfmi_unwrap(_lib.ptr(x2), nser, xs, N, float(period), _lib.ptr(s2), ss, int(max_status),
                             FILLS[fill], _lib.ptr(y), N, _lib.ptr(c), N, _lib.DFMI_MEM_HOST, None)
    _lib.check(rc, "dfmi_unwrap")
    if one:
        y, c = y[0], (c[0] if cycles else None)
    return (y, c) if cycles else y
