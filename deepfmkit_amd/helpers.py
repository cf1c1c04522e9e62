"""Statistical helpers (mirror of the reference helpers.py module surface).

The reference's CRLB functions invert the Fisher matrix J^T J of the DFMI model point by
point in numpy (helpers.py:16-45, 98-132). The Jacobian depends on (a, m, phi, psi) alone,
so here every such function is ONE dfmi_fisher call over all of its points (csrc/fisher.h:
the J^T J of fit.py:68-150 and its inverse, one GPU lane per point); the same entry point
gives the per-segment standard errors of a fit (fitters.nls_records(errors=True)).
There is no CPU fallback: without a GPU these raise DFMIError.

  fisher(params, ndata, var, var_mul, want)          the thin binding of dfmi_fisher
  calculate_m_precision(m_range, ndata, snr_db)      helpers.py:98-132
  calculate_crlb_for_m(m_true, ndata, snr_db, R)     helpers.py:16-45
  calculate_jacobian(ndata, param)                   helpers.py:60-96 (host: one point)
  snr_to_asd(snr_db, f_samp)                         helpers.py:47-58 (host)
  set_laser_df_for_effect(laser, ifo, m)             helpers.py:10-14 (physics.py here)
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .physics import set_laser_df_for_effect  # noqa: F401

# order of the ten upper-triangle entries of jtj / cov (include/dfmi.h dfmi_fisher)
UPPER = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))
_ROWS = {"jtj": 10, "cov": 10, "sigma": 4}


def _is_device_tensor(x):
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def fisher(params, ndata, var=None, var_mul=1.0, want=("sigma",)):
    """dfmi_fisher at n parameter points.

    params: (4, n) component-major [amp, m, phi, psi] or (n, 4), a numpy array or a CUDA
    float64 tensor (a (4, 4) input is read as component-major; a 1-D input of four values is
    one point). var: None or (n,) per-point
    variance factors, multiplied by var_mul. want: any of 'jtj' (10, n), 'cov' (10, n),
    'sigma' (4, n), at least one. Returns a dict of the wanted arrays plus 'ok' (n,) int32:
    numpy arrays for host input, tensors on the input's device (enqueued on its current
    stream, not synchronised) for device input."""
    lib = _lib.load()
    want = tuple(want)
    if not want or any(w not in _ROWS for w in want):
        raise ValueError(f"want: one or more of {tuple(_ROWS)}, got {want}")
    ndata = int(ndata)
    if _is_device_tensor(params):
        import torch
        p = params.reshape(4, 1) if params.dim() == 1 and params.numel() == 4 else params
        if p.dim() != 2 or 4 not in p.shape:
            raise ValueError("params must be (4, n) or (n, 4)")
        if p.shape[0] != 4:
            p = p.t()
        if p.dtype != torch.float64:
            raise ValueError("device params must be float64")
        n = int(p.shape[1])
        if p.stride(1) != 1 or p.stride(0) < n:
            p = p.contiguous()
        ld = int(p.stride(0))
        v = None
        if var is not None:
            v = var.to(device=p.device, dtype=torch.float64).contiguous()
            if v.numel() != n:
                raise ValueError("var must have one entry per point")
        out = {w: torch.empty((_ROWS[w], n), dtype=torch.float64, device=p.device) for w in want}
        out["ok"] = torch.empty(n, dtype=torch.int32, device=p.device)
        with torch.cuda.device(p.device):
            rc = lib.dfmi_fisher(p.data_ptr(), n, max(ld, n), ndata, None if v is None else v.data_ptr(),
                                 float(var_mul), *[out[w].data_ptr() if w in out else None for w in _ROWS],
                                 out["ok"].data_ptr(), _lib.DFMI_MEM_DEVICE,
                                 torch.cuda.current_stream(p.device).cuda_stream)
        _lib.check(rc, "dfmi_fisher")
        return out
    p = np.asarray(params, dtype=np.float64)
    if p.ndim == 1 and p.size == 4:
        p = p.reshape(4, 1)
    if p.ndim != 2 or 4 not in p.shape:
        raise ValueError("params must be (4, n) or (n, 4)")
    p = np.ascontiguousarray(p if p.shape[0] == 4 else p.T)
    n = p.shape[1]
    v = None
    if var is not None:
        v = np.ascontiguousarray(var, dtype=np.float64).ravel()
        if v.size != n:
            raise ValueError("var must have one entry per point")
    out = {w: np.empty((_ROWS[w], n)) for w in want}
    out["ok"] = np.empty(n, dtype=np.int32)
    rc = lib.dfmi_fisher(_lib.ptr(p), n, n, ndata, _lib.ptr(v), float(var_mul),
                         *[_lib.ptr(out.get(w)) for w in _ROWS], _lib.ptr(out["ok"]), _lib.DFMI_MEM_HOST, None)
    _lib.check(rc, "dfmi_fisher")
    return out


def _noise_power(snr_db):
    """Variance of white noise `snr_db` below a unit-amplitude cosine (mean square 1/2)."""
    return 0.5 / 10 ** (snr_db / 10.0)


def _points(m, phi):
    """(4, n) component-major points (1, m, phi, 0) for dfmi_fisher."""
    p = np.zeros((4, m.size))
    p[0] = 1.0
    p[1] = m
    p[2] = phi
    return p


def calculate_crlb_for_m(m_true, ndata, snr_db, buffer_size):
    """helpers.py:16-45: the Cramér-Rao lower bound of m at (a, phi, psi) = (1, 0, 0) for
    white noise of `snr_db` on a unit cosine, each quadrature a mean over `buffer_size`
    samples (variance noise/(2 buffer_size)). m_true may be an array (one GPU call for all of
    it); np.nan where J^T J has no inverse."""
    m = np.atleast_1d(np.asarray(m_true, dtype=np.float64))
    r = fisher(_points(m.ravel(), 0.0), ndata, var_mul=_noise_power(snr_db) / (2 * buffer_size), want=("sigma",))
    crlb = np.where(r["ok"] != 0, r["sigma"][1], np.nan).reshape(m.shape)
    return crlb if np.ndim(m_true) else float(crlb[0])


def snr_to_asd(snr_db, f_samp):
    """helpers.py:47-58: the amplitude noise ASD that gives `snr_db` on a unit cosine: white
    noise of variance s^2 has the one-sided density s^2 / (f_samp / 2)."""
    return np.sqrt(_noise_power(snr_db) / (f_samp / 2.0))


def _harmonic_factors(ndata, m, phi, psi):
    """Per-harmonic factors of the model for j = 1..ndata, named as csrc/lm.h harmonic_term
    names them: j, pt = cos(phi + j pi/2), ptd = cos(phi + j pi/2 + pi/2), Jj = J_j(m),
    dJ = J_j'(m) = (J_{j-1} - J_{j+1})/2, cj = cos(j psi), sj = sin(j psi)."""
    from scipy.special import jv
    j = np.arange(1, ndata + 1)
    quarter = j * np.pi / 2.0
    return (j, np.cos(phi + quarter), np.cos(phi + quarter + np.pi / 2.0), jv(j, m),
            0.5 * (jv(j - 1, m) - jv(j + 1, m)), np.cos(j * psi), np.sin(j * psi))


def calculate_jacobian(ndata, param):
    """helpers.py:60-96: the model Jacobian (2*ndata, 4) at one point, on the host. Rows
    0..ndata-1 are the Q residuals, the rest the I residuals; a column with per-harmonic
    amplitude u is [u cj | -u sj] (the model is Q_j = u cj, I_j = -u sj with u = a pt Jj),
    the psi column its derivative [-u sj j | -u cj j]. Column 0 is model/a and stays zero at
    a == 0 (fit.py:126-128). The operations and their order are the reference's."""
    a, m, phi, psi = param
    j, pt, ptd, Jj, dJ, cj, sj = _harmonic_factors(ndata, m, phi, psi)

    def rotated(u):
        return np.concatenate([u * cj, -u * sj])

    u = a * pt * Jj
    J = np.zeros((2 * ndata, 4))
    if a != 0:
        J[:, 0] = rotated(u) / a
    J[:, 1] = rotated(a * pt * dJ)
    J[:, 2] = rotated(a * ptd * Jj)
    J[:, 3] = np.concatenate([u * -sj * j, -u * cj * j])
    return J


def calculate_m_precision(m_range, ndata, snr_db):
    """helpers.py:98-132: the statistical uncertainty of m over m_range at
    (a, phi, psi) = (1, pi/4, 0) for I/Q noise of amplitude 10^(-snr_db/20); np.inf where
    J^T J has no inverse."""
    m = np.asarray(m_range, dtype=np.float64).ravel()
    if m.size == 0:
        return np.array([])
    r = fisher(_points(m, np.pi / 4), ndata, var_mul=(1.0 / 10 ** (snr_db / 20.0)) ** 2, want=("sigma",))
    return np.where(r["ok"] != 0, r["sigma"][1], np.inf)
