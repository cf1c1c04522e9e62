"""numpy restatement of the project's LPSD definition, written from the
definition and sharing no code with the product: the Kaiser polynomials, the frequency plan
and the estimate, segment by segment. `dtype` is the type of the estimate's arithmetic
(np.float64, or np.longdouble for the twin that measures the restatement's own rounding); the
plan is always float64, as the product's host plan is, so both twins see the same (b, L, K)."""
import numpy as np


def kaiser_alpha(psll):
    p = psll / 100.0
    return ((0.0889732 * p - 0.493285) * p + 4.71469) * p - 0.0821377


def default_olap(alpha):
    return (100.0 - 1.0 / (((4.42204e-05 * alpha - 0.000925946) * alpha + 0.00912223) * alpha + 0.0061076)) / 100.0


def plan(N, fs, olap="default", bmin=1, Lmin=0, Jdes=500, Kdes=100, psll=200, literal=False):
    """(f, fres, b, L, K) of the plan: float64 arrays f, fres, b and int64 arrays L, K.
    literal=True leaves out the bin floor: the plan loop alone, in which the
    emitted b can fall below bmin when L is rounded."""
    if isinstance(olap, str):
        olap = default_olap(kaiser_alpha(psll))
    N = int(N)
    fs, olap, bmin = float(fs), float(olap), float(bmin)
    xov = 1.0 - olap
    fresmin = fs / N
    freslim = fresmin * (1.0 + xov * (Kdes - 1))
    logfact = (N / 2.0) ** (1.0 / Jdes) - 1.0
    f, fr, bb, LL, KK = [], [], [], [], []
    fi = fresmin * bmin
    while fi < fs / 2.0:
        fres = fi * logfact
        if fres <= freslim:
            fres = np.sqrt(fres * freslim)
        if fres < fresmin:
            fres = fresmin
        b = fi / fres
        if b < bmin:
            b = bmin
            fres = fi / b
        L = int(np.floor(fs / fres + 0.5))
        L = min(max(L, int(Lmin), 1), N)
        K = int(np.floor((N - L) / (xov * L) + 1.0 + 0.5))
        if K == 1:
            L = N
        fres = fs / L
        b = fi / fres
        if b < bmin and not literal:
            # the bin floor: rounding L moved b = fi L / fs below bmin; take the shortest
            # segment that keeps it (N at most), and K, fres, b again
            L = min(N, max(int(np.ceil(bmin * fs / fi)), int(Lmin), 1))
            while fi / (fs / L) < bmin and L < N:
                L += 1
            K = int(np.floor((N - L) / (xov * L) + 1.0 + 0.5))
            if K == 1:
                L = N
            fres = fs / L
            b = fi / fres
            if b < bmin:  # L = N and fi = fresmin bmin: b is bmin but for the rounding of the quotient
                b = bmin
        f.append(fi), fr.append(fres), bb.append(b), LL.append(L), KK.append(K)
        fi = fi + fres
    return (np.array(f), np.array(fr), np.array(bb), np.array(LL, dtype=np.int64), np.array(KK, dtype=np.int64))


def _pi(dtype):
    return dtype(np.pi) if dtype is np.float64 else dtype(4) * np.arctan(dtype(1))


def _i0(x, dtype):
    """I0 by its power series (all terms positive) in `dtype`."""
    x = np.asarray(x, dtype=dtype)
    q = x * x / dtype(4)
    term = np.ones_like(q)
    s = np.ones_like(q)
    for k in range(1, 400):
        term = term * q / dtype(k * k)
        s = s + term
    return s


def window(L, alpha, dtype=np.float64):
    n = np.arange(L).astype(dtype)
    z = dtype(2) * n / dtype(L) - dtype(1)
    pa = _pi(dtype) * dtype(alpha)
    arg = pa * np.sqrt(np.maximum(dtype(1) - z * z, dtype(0)))
    return _i0(arg, dtype) / _i0(pa, dtype)


def lpsd(x, fs, olap="default", bmin=1, Lmin=0, Jdes=500, Kdes=100, order=0, psll=200, dtype=np.float64):
    """dict(f, Sxx, enbw, L, K, b) for one series x."""
    if order not in (0, -1):
        raise ValueError("order")
    x = np.asarray(x, dtype=np.float64)
    N = x.size
    f, fres, b, L, K = plan(N, fs, olap, bmin, Lmin, Jdes, Kdes, psll)
    alpha = kaiser_alpha(psll)
    xd = x.astype(dtype)
    two_pi = dtype(2) * _pi(dtype)
    Sxx = np.empty(f.size, dtype=dtype)
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
        acc = dtype(0)
        for k in range(Kj):
            s = int(np.floor(np.float64(k) * np.float64(N - Lj) / np.float64(Kj - 1) + 0.5)) if Kj > 1 else 0
            seg = xd[s:s + Lj]
            if order == 0:
                seg = seg - seg.mean()
            A = np.sum(we * seg)
            acc = acc + (A.real * A.real + A.imag * A.imag)
        s2 = np.sum(w * w)
        s1 = np.sum(w)
        Sxx[j] = dtype(2) * (acc / dtype(Kj)) / (dtype(fs) * s2)
        enbw[j] = dtype(fs) * s2 / (s1 * s1)
    return dict(f=f, Sxx=Sxx, enbw=enbw, L=L, K=K, b=b)
