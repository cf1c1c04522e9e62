"""Shared cases of the coloured-noise tests (CPU and GPU): the configurations of the whole-trial
checks and the known answer of frequency noise through a fit."""
import numpy as np
import scipy.constants as sc

# (f_n, arml_mod_n, amp_n, df_n): f_n only; arml_mod_n only; both; both with white amp_n and df_n
COLOUR_CASES = [(1e6, 0.0, 0.0, 0.0), (0.0, 1e-12, 0.0, 0.0), (1e6, 1e-12, 0.0, 0.0), (1e6, 1e-12, 1e-4, 2e3)]


def configs(f_n, arm_n, amp_n, df_n, m=6.0):
    import deepfmkit_amd as dfm
    laser = dfm.LaserConfig()
    laser.f_n, laser.amp_n, laser.df_n = f_n, amp_n, df_n
    ifo = dfm.InterferometerConfig()
    ifo.arml_mod_n = arm_n
    ifo.arml_mod_amp = 1e-7
    dfm.set_laser_df_for_effect(laser, ifo, m)
    cfg = dfm.DFMIObject("main_trial", laser, ifo)
    wit_ifo = dfm.InterferometerConfig()
    wit_ifo.meas_arml = 0.15
    wit_ifo.arml_mod_n = arm_n  # a witness sees no arm-length noise whatever its own setting
    return cfg, dfm.DFMIObject("witness_trial", laser, wit_ifo)


def known_answer(fit_rows, cfg, noise_f, R_buf):
    """(residual std, excursion std) of the fitted phi against -2 pi (c/lambda + mean noise per
    buffer) (meas_arml - ref_arml) / c modulo 2 pi, up to a constant (the fit's cos(-x) branch)."""
    nbar = np.asarray(noise_f).reshape(-1, R_buf).mean(axis=1)
    tau = (cfg.ifo.meas_arml - cfg.ifo.ref_arml) / sc.c
    want = -2 * np.pi * (sc.c / cfg.laser.wavelength + nbar) * tau
    d = (fit_rows - want + np.pi) % (2 * np.pi) - np.pi
    d0 = np.angle(np.mean(np.exp(1j * d)))
    resid = (d - d0 + np.pi) % (2 * np.pi) - np.pi
    return float(np.std(resid)), float(np.std(2 * np.pi * nbar * tau))


def quickstart_config():
    import deepfmkit_amd as dfm
    laser = dfm.LaserConfig()
    laser.f_n = 1e6
    ifo = dfm.InterferometerConfig()
    dfm.set_laser_df_for_effect(laser, ifo, 6.0)
    return dfm.DFMIObject("main", laser, ifo)
