"""Independent numpy restatement of the coloured-noise definition:
the design, the cascade as a scalar loop in float64 and in longdouble, the analytic
response and the noise arrays. It shares no code with deepfmkit_amd."""
import math

import numpy as np


def sections_between(fs, lw0, lw1, nsec, alpha):
    """nsec pole-zero sections spaced evenly in log10(omega) over [lw0, lw1]: (nsec, 3)."""
    dp = (lw1 - lw0) / nsec
    rows = []
    for i in range(nsec):
        lp = lw0 + dp * 0.5 * ((2 * i + 1) - alpha / 2)
        f0 = 10 ** lp / (2 * np.pi)
        f1 = 10 ** (lp + dp * alpha / 2) / (2 * np.pi)
        rows.append(((fs + np.pi * f1) / (fs + np.pi * f0), -(fs - np.pi * f1) / (fs + np.pi * f0),
                     (fs - np.pi * f0) / (fs + np.pi * f0)))
    return np.array(rows, dtype=np.float64).reshape(nsec, 3)


def design(fs, N, alpha):
    """(sections (nsec, 3), scale) of the definition."""
    if N < 4 or not 0 < alpha <= 2:
        raise ValueError("design: N >= 4, 0 < alpha <= 2")
    f_min, f_max = fs / N, fs / 2
    # the C library's log10 (math.log10), not np.log10: numpy's own log10 differs from it in
    # the last place at some arguments (2 pi 0.02 is one), and the section frequencies
    # 10^lp magnify one ulp of lw0 up to ~80 ulp of a coefficient near fs = pi f1
    lw0, lw1 = math.log10(2 * np.pi * f_min), math.log10(2 * np.pi * f_max)
    nsec = int(np.ceil(4.5 * (lw1 - lw0)))
    if nsec > 64:
        raise ValueError("design: more than 64 sections")
    return sections_between(fs, lw0, lw1, nsec, alpha), f_max ** (-alpha / 2)


def table(nsec, fs=200000.0, alpha=2.0):
    """A stable table of exactly nsec sections (over the band of a 2^20-sample record):
    what a caller of dfmi_plnoise may pass beside the designed ones."""
    lw0, lw1 = math.log10(2 * np.pi * fs / 2 ** 20), math.log10(2 * np.pi * fs / 2)
    return sections_between(fs, lw0, lw1, nsec, alpha), (fs / 2) ** (-alpha / 2)


def cascade(sections, x, dtype=np.float64):
    """Every section in turn over x, zero initial state, a scalar loop in `dtype`
    (each operation rounded): y[k] = a0 x[k] + z; z = a1 x[k] + b1 y[k]."""
    v = np.array(x, dtype=dtype)
    for a0, a1, b1 in np.asarray(sections, dtype=np.float64):
        a0, a1, b1 = dtype(a0), dtype(a1), dtype(b1)
        z = dtype(0.0)
        for k in range(v.size):
            xk = v[k]
            y = a0 * xk + z
            z = a1 * xk + b1 * y
            v[k] = y
    return v


def cascade_many(sections, X, dtype=np.float64):
    """cascade() over the rows of X (nser, T) at once: the scalar loop over samples with one
    numpy operation per step across the series (elementwise: each series' own arithmetic)."""
    V = np.array(X, dtype=dtype)
    for a0, a1, b1 in np.asarray(sections, dtype=np.float64):
        a0, a1, b1 = dtype(a0), dtype(a1), dtype(b1)
        z = np.zeros(V.shape[0], dtype=dtype)
        for k in range(V.shape[1]):
            xk = V[:, k]
            y = a0 * xk + z
            z = a1 * xk + b1 * y
            V[:, k] = y
    return V


def gaussians(seed, sigma, count):
    return np.random.RandomState(seed).normal(scale=sigma, size=count)


def series(sections, scale, sigma, seed, n_warm, n, dtype=np.float64):
    """basis = scale * cascade(x)[n_warm:], x the legacy RandomState normal stream."""
    y = cascade(sections, gaussians(seed, sigma, n_warm + n), dtype)
    return dtype(scale) * y[n_warm:]


def response2(sections, scale, fs, f):
    """|H(f)|^2 of scale * cascade (analytic, one-sided PSD of the series for unit-ASD white
    input of variance fs/2: PSD(f) = |H|^2)."""
    zinv = np.exp(-2j * np.pi * np.asarray(f, dtype=np.float64) / fs)
    h = np.full(zinv.shape, scale, dtype=np.complex128)
    for a0, a1, b1 in sections:
        h = h * (a0 + a1 * zinv) / (1 - b1 * zinv)
    return np.abs(h) ** 2


def noise_arrays(fs, n, trial_num, f_n, amp_n, df_n, arml_mod_n):
    """The four asd-mode sources in the reference's order (physics.py:578-611)."""
    rng = np.random.RandomState(1 + 4 * trial_num)
    out, basis = {}, None
    for name, asd, white in (("laser_frequency", f_n, False), ("amplitude", amp_n, True), ("df", df_n, True),
                             ("armlength", arml_mod_n, False)):
        if asd == 0.0:
            out[name] = 0.0
        elif white:
            out[name] = rng.normal(scale=asd * np.sqrt(fs / 2.0), size=n)
        else:
            if basis is None:
                sec, scale = design(fs, n, 2.0)
                basis = series(sec, scale, np.sqrt(fs / 2.0), 2 + 4 * trial_num, 2 * n, n)
            out[name] = asd / np.sqrt(2) * basis
    return out
