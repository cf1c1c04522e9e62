"""numpy restatement of the project's cross-spectral density and coherence,
written from the definition and sharing no code with the product. The plan, the window and the
Kaiser polynomial are lpsd_ref's, and Sxx goes through lpsd_ref.lpsd's own operations in its
order, so it equals lpsd_ref.lpsd's exactly. `dtype` is the type of the estimate's arithmetic
(np.float64, or np.longdouble for the twin that measures the restatement's own rounding)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lpsd_ref import _pi, kaiser_alpha, plan, window  # noqa: E402


def lcsd(x, y, fs, olap="default", bmin=1, Lmin=0, Jdes=500, Kdes=100, order=0, psll=200, dtype=np.float64):
    """dict(f, Sxx, Syy, Sxy, coh, H, resid, enbw, L, K, b) for one pair of series."""
    if order not in (0, -1):
        raise ValueError("order")
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError("x and y: two 1-D series of equal length")
    N = x.size
    f, fres, b, L, K = plan(N, fs, olap, bmin, Lmin, Jdes, Kdes, psll)
    alpha = kaiser_alpha(psll)
    xd, yd = x.astype(dtype), y.astype(dtype)
    two_pi = dtype(2) * _pi(dtype)
    ctype = np.complex128 if dtype is np.float64 else np.clongdouble
    Sxx = np.empty(f.size, dtype=dtype)
    Syy = np.empty(f.size, dtype=dtype)
    Sxy = np.empty(f.size, dtype=ctype)
    enbw = np.empty(f.size, dtype=dtype)
    wcache = {}
    for j in range(f.size):
        Lj, Kj = int(L[j]), int(K[j])
        if Lj not in wcache:
            wcache[Lj] = window(Lj, alpha, dtype)
        w = wcache[Lj]
        n = np.arange(Lj).astype(dtype)
        t = dtype(b[j]) * n / dtype(Lj)
        t = t - np.floor(t)
        ph = two_pi * t
        e = np.cos(ph) - 1j * np.sin(ph)
        we = w * e
        axx, ayy, are, aim = dtype(0), dtype(0), dtype(0), dtype(0)
        for k in range(Kj):
            s = int(np.floor(np.float64(k) * np.float64(N - Lj) / np.float64(Kj - 1) + 0.5)) if Kj > 1 else 0
            sx, sy = xd[s:s + Lj], yd[s:s + Lj]
            if order == 0:
                sx = sx - sx.mean()
                sy = sy - sy.mean()
            A = np.sum(we * sx)
            B = np.sum(we * sy)
            axx = axx + (A.real * A.real + A.imag * A.imag)
            ayy = ayy + (B.real * B.real + B.imag * B.imag)
            are = are + (A.real * B.real + A.imag * B.imag)  # conj(A) B
            aim = aim + (A.real * B.imag - A.imag * B.real)
        s2 = np.sum(w * w)
        s1 = np.sum(w)
        Sxx[j] = dtype(2) * (axx / dtype(Kj)) / (dtype(fs) * s2)
        Syy[j] = dtype(2) * (ayy / dtype(Kj)) / (dtype(fs) * s2)
        Sxy[j] = (dtype(2) * (are / dtype(Kj)) / (dtype(fs) * s2)) + 1j * (dtype(2) * (aim / dtype(Kj)) / (dtype(fs) * s2))
        enbw[j] = dtype(fs) * s2 / (s1 * s1)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = Sxx * Syy
        coh = np.where(den > 0, (Sxy.real * Sxy.real + Sxy.imag * Sxy.imag) / den, dtype(np.nan))
        H = Sxy / Sxx
    resid = Syy * (dtype(1) - coh)
    return dict(f=f, Sxx=Sxx, Syy=Syy, Sxy=Sxy, coh=coh, H=H, resid=resid, enbw=enbw, L=L, K=K, b=b)
