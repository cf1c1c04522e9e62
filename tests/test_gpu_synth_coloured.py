"""Coloured asd-mode trials on the GPU (dfmi_synth_asd_coloured: csrc/plnoise.hip feeding
csrc/synth.hip) against the host generator, the new entry without colour against
dfmi_synth_asd, an Experiment over a frequency-noise axis on the device path, and the known
answer of frequency noise through DeepFitFramework.simulate + fit."""
import os
import sys

import numpy as np
import pytest
import scipy.constants as sc

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import experiment_spec as S  # noqa: E402
import plnoise_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

WHITE_TOL = 1e-9  # tests/test_gpu_workers.py: a few ulps of the phase upstream of the cos


def _signal_tol(cfg):
    """One-ulp differences in the noise (the device's log) can flip the rounding of
    c / lambda + n_f (ulp 0.0625 Hz): 4 x amp vis 2 pi spacing(c / lambda) |tau_m - tau_r|."""
    laser, ifo = cfg.laser, cfg.ifo
    tau = abs(ifo.meas_arml / sc.c - ifo.ref_arml / sc.c)
    return 4 * laser.amp * laser.visibility * 2 * np.pi * np.spacing(sc.c / laser.wavelength) * tau + WHITE_TOL


@pytest.mark.parametrize("case", C.COLOUR_CASES)
def test_coloured_trials_match_host_generator(case):
    from deepfmkit_amd import physics as P
    runs = [(0, 0.02), (3, 0.02)] + ([(1, 0.005)] if case == C.COLOUR_CASES[3] else [])
    for ns in sorted({r[1] for r in runs}):
        tns = [t for t, s in runs if s == ns]
        pairs = [C.configs(*case) for _ in tns]
        hosts = [P.SignalGenerator().generate(c, ns, mode="asd", trial_num=t, witness_config=w)
                 for (c, w), t in zip(pairs, tns)]
        dm = P.synthesize_asd_trials([c for c, _ in pairs], tns, ns, dynamic=True).cpu().numpy()
        dw = P.synthesize_asd_trials([w for _, w in pairs], tns, ns, dynamic=False).cpu().numpy()
        for k, ((c, w), h) in enumerate(zip(pairs, hosts)):
            em = np.max(np.abs(dm[k] - np.asarray(h["main"].samples())))
            ew = np.max(np.abs(dw[k] - np.asarray(h["witness"].samples())))
            print(f"case {case} trial {tns[k]} {ns} s: main {em:.3g} (tol {_signal_tol(c):.3g}) "
                  f"witness {ew:.3g} (tol {_signal_tol(w):.3g})")
            assert em <= _signal_tol(c) and ew <= _signal_tol(w)


def test_mixed_batch_white_rows_keep_their_bits():
    """White-only trials inside a coloured batch are dfmi_synth_asd's bits; colour == NULL and
    all-zero gains through the new entry are too."""
    import torch
    from deepfmkit_amd import _lib, physics as P
    from deepfmkit_amd.fitters import _torch_stream
    white = [C.configs(0.0, 0.0, 1e-4, 2e3)[0], C.configs(0.0, 0.0, 0.0, 0.0, m=8.0)[0]]
    col = C.configs(1e6, 1e-12, 1e-4, 0.0)[0]
    tns = [3, 5]
    ref = P.synthesize_asd_trials(white, tns, 0.02).cpu().numpy()
    mixed = P.synthesize_asd_trials([white[0], col, white[1]], [3, 4, 5], 0.02).cpu().numpy()
    np.testing.assert_array_equal(mixed[[0, 2]], ref)
    assert not np.array_equal(mixed[1], ref[0])
    lib = _lib.load()
    tab = P.synth_trial_table(white, tns)
    ctab = P.synth_colour_table(white, tns)
    assert np.all(ctab["g_freq"] == 0) and np.all(ctab["g_arm"] == 0)
    sec, scale = P.alpha_noise_design(200000.0, 4000, 2.0)
    for colour in (None, ctab.ctypes.data):
        out = torch.zeros((2, 4000), dtype=torch.float64, device="cuda")
        _lib.check(lib.dfmi_synth_asd_coloured(tab.ctypes.data, colour, sec.ctypes.data, len(sec), scale, 8000, 2,
                                               4000, 200000.0, out.data_ptr(), _lib.DFMI_MEM_DEVICE,
                                               _torch_stream()), "dfmi_synth_asd_coloured")
        np.testing.assert_array_equal(out.cpu().numpy(), ref)
    host = np.zeros((2, 4000))  # host memory, no table at all: colour == NULL needs none
    _lib.check(lib.dfmi_synth_asd_coloured(tab.ctypes.data, None, None, 0, 0.0, 0, 2, 4000, 200000.0,
                                           host.ctypes.data, _lib.DFMI_MEM_HOST, None), "dfmi_synth_asd_coloured")
    np.testing.assert_array_equal(host, ref)


FN_KEYS = {"m_main", "f_noise", "phi"}


def _fn_factory():
    from deepfmkit_amd import factories, physics

    class FnFactory(factories.ExperimentFactory):
        def _get_expected_params_keys(self):
            return set(FN_KEYS)

        def __call__(self, params):
            cfg = S.noisy_config(physics, {"m_main": params["m_main"], "amp_noise": 1e-4, "phi": params["phi"]})
            cfg["laser_config"].f_n = params["f_noise"]
            return cfg
    return FnFactory()


def _fn_experiment():
    from deepfmkit_amd.experiments import Experiment
    exp = Experiment("fn")
    exp.set_config_factory(_fn_factory())
    exp.add_axis("m_main", np.array([5.0, 7.5]))
    exp.add_axis("f_noise", np.array([0.0, 1e5, 1e6]))
    exp.add_stochastic_variable("phi", S.phi_generator)
    exp.n_trials = 2
    exp.add_analysis("NLS", "nls", fitter_kwargs={"ndata": 10})
    np.random.seed(S.SEED)
    return exp


def test_experiment_over_a_frequency_noise_axis_runs_on_the_device(monkeypatch):
    """An f_n axis stays on the device generator (the host generator is never called) and
    agrees with the same experiment forced onto the host generator at the tolerances
    tests/test_gpu_experiments.py uses between those paths."""
    from deepfmkit_amd import experiments
    with monkeypatch.context() as mp:
        mp.setattr(experiments, "device_synth_supported", lambda cfg: False)
        host = S.flatten(_fn_experiment().run(engine="gpu"))

    class NoHost:
        def generate(self, *a, **k):
            raise AssertionError("host generator called for a coloured configuration")
    monkeypatch.setattr(experiments, "SignalGenerator", NoHost)
    dev = S.flatten(_fn_experiment().run(engine="gpu"))
    fitok = {k.rsplit("/", 1)[0]: v for k, v in host.items() if k.endswith("/fitok")}
    assert sorted(dev) == sorted(host)
    for k, a in dev.items():
        b = host[k]
        ok = fitok.get(k.rsplit("/", 1)[0])
        tol = np.where(ok != 0, 1e-7, 1e-9) if ok is not None else 1e-9
        if k.endswith("/fitok"):
            np.testing.assert_array_equal(a, b, err_msg=k)
        elif k.endswith("/ssq"):
            np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-300, err_msg=k)
        elif k.endswith("/phi"):
            d = np.abs((a - b + np.pi) % (2 * np.pi) - np.pi)
            print(f"{k}: max |d| {d.max():.3g}")
            assert (d <= tol).all(), (k, d.max())
        else:
            print(f"{k}: max |d| {np.abs(a - b).max():.3g}")
            assert (np.abs(a - b) <= tol).all(), (k, np.abs(a - b).max())


def test_known_answer_through_simulate_and_fit():
    """The quickstart's settings through DeepFitFramework.simulate(mode='asd') and the GPU fit:
    residual std <= 1e-2 x excursion std, every fitok 0 (the bound of the CPU test)."""
    import deepfmkit_amd as dfm
    from deepfmkit_amd import physics as P
    cfg = C.quickstart_config()
    dff = dfm.DeepFitFramework()
    dff.load_sim(cfg)
    dff.simulate("main", n_seconds=1.0, mode="asd", trial_num=0)
    fit = dff.fit("main", n=20)
    noise = P.asd_noise_arrays(cfg, 200000, 0)["laser_frequency"]
    resid, exc = C.known_answer(np.asarray(fit.phi), cfg, noise, 4000)
    print(f"known answer (GPU fit): residual std {resid:.3e} rad, excursion std {exc:.3e} rad")
    df = list(dff.fits_df.values())[0]
    assert len(fit.phi) == 50 and np.all(np.asarray(df["fitok"]) == 0)
    assert resid <= 1e-2 * exc
