"""Raw and fit containers (reference data.py:16-309, hot-path subset).

`DeepRawObject.data` keeps the reference's shape — a pandas DataFrame with one
float64 column `ch0` — so code written against the reference keeps working. A
torch tensor already resident on the GPU is also accepted as `data` (the
device-resident path used by bench.py); `samples()` hands either form to the
engine without a copy.
"""
from __future__ import annotations

import numpy as np
import pandas as pd


class DeepRawObject:
    """One raw channel plus metadata (reference data.py:16-42)."""

    def __init__(self, data=None):
        self.raw_file = None
        self.label = None
        self.t0 = None
        self.f_samp = None
        self.f_mod = None
        self.sim = None
        self.data = pd.DataFrame()
        self.phi = None
        self.phi_sim = None
        self.phi_sim_downsamp = None
        self.f_noise = None
        self.l_noise = None
        self.a_noise = None
        self.df_noise = None
        if data is not None:
            if isinstance(data, np.ndarray):
                data = pd.DataFrame(np.asarray(data, dtype=np.float64).reshape(-1), columns=["ch0"])
            self.data = data

    def samples(self):
        """The channel's samples as a 1-D float64 array or device tensor (no copy)."""
        d = self.data
        if isinstance(d, pd.DataFrame):
            return d["ch0"].to_numpy() if "ch0" in d.columns else d.iloc[:, 0].to_numpy()
        if isinstance(d, pd.Series):
            return d.to_numpy()
        return d  # numpy array or torch tensor

    def n_samples(self):
        d = self.data
        return int(d.shape[0])


class DeepFitObject:
    """Fit results of one channel (reference data.py:121-208, 239-244)."""

    # LPSD results and settings (reference data.py:147-156). Class-level defaults: an
    # instance carries its own only once calc_lpsd ran or the user set one.
    f = None
    Sxx = None
    olap = "default"
    bmin = 1
    Lmin = 0
    Jdes = 500
    Kdes = 100
    order = 0
    win = staticmethod(np.kaiser)
    psll = 200

    def __init__(self):
        self.fit_file = None
        self.label = None
        self.n = None
        self.t0 = None
        self.R = None
        self.fs = None
        self.f_samp = None
        self.f_mod = None
        self.ndata = 10
        self.init_a = 1.6
        self.init_m = 6.0
        self.nbuf = None
        self.time = np.array([])
        self.ssq = np.array([])
        self.amp = np.array([])
        self.m = np.array([])
        self.tau = np.array([])
        self.phi = np.array([])
        self.psi = np.array([])
        self.dc = np.array([])

    def to_txt(self, filename):
        """fit_data text format (reference data.py:178-208), written by libdfmi's
        host writer in the reference's exact bytes (textio.write_fit)."""
        from . import textio
        textio.write_fit(self, filename)

    def lpsd_settings(self):
        """The LPSD settings of this fit as keyword arguments of deepfmkit_amd.lpsd.lpsd."""
        return dict(olap=self.olap, bmin=self.bmin, Lmin=self.Lmin, Jdes=self.Jdes, Kdes=self.Kdes, order=self.order,
                    win=self.win, psll=self.psll)

    def calc_lpsd(self, which="phi"):
        """LPSD of a fitted parameter (the reference's calc_lpsd takes phi, data.py:239-244) at
        the fit data rate fs with this object's settings: sets f and Sxx, on the GPU
        (deepfmkit_amd.lpsd; the estimator is the project's own definition)."""
        from .lpsd import lpsd
        r = lpsd(np.asarray(getattr(self, which), dtype=np.float64), self.fs, **self.lpsd_settings())
        self.f, self.Sxx = r.f, r.Sxx
