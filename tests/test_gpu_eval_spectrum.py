"""The spectrogram and Welch spectrum of recorder columns (evaluate.spectrum_device -> irrl_eval_spectrum) on the MI355X: the device against the
numpy twin on the generated cases of tests/eval_spectrum_lib.py, run-to-run bits, `work` given or not, the spectrograms on or off, the refusals,
and robustness_sweep(spectrum=...) against the twin on the downloaded recorders for the LSTM actor in both forms of the loop and for MlpPolicy.

`segments` must be equal, a NaN must sit in the same places, and every other word lies within the bound of tests/eval_spectrum_lib.py:
32 n 2^-53 g_k density (sum |a_n|)^2 per bin and segment, derived there, not measured.  Bit equality with the twin is not asked of the device:
its compiler fuses the accumulation s + a * t where numpy does not."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_spectrum_lib as L
import test_gpu_eval_mlp as TM
import test_gpu_eval_persistent as TP
from conftest import load_env_cfg
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV
from high_speed_quadrupedal_locomotion_by_irrl_amd.helper import obs_normalisation

FF, FE = L.FRAME_FIRST, L.FRAME_EVERY
DEV = torch.device("cuda")


def _device(x, done):
    return torch.from_numpy(x.copy()).to(DEV), None if done is None else torch.from_numpy(done.copy()).to(DEV)     # (the cases are read-only)


# ---- (a) the generated cases ----
@pytest.mark.parametrize("nperseg,hop,T,conditions,detrend,window", L.cases())
def test_device_against_the_twin(nperseg, hop, T, conditions, detrend, window):
    """all three outputs against the twin, with and without rec_done; a second run gives the same bytes; the spectrograms off leave the rest
    unchanged; with one robot per condition a call without `work` gives the same bytes as one with it, with more it is refused"""
    x, done = L.case(nperseg, T)
    s = L.spec(nperseg, hop, detrend)
    win, tw = L.tables(nperseg, window)
    xd, dd = _device(x, done)
    kw = dict(conditions=conditions, frame_first=FF, frame_every=FE, frames=T)
    worst = 0.0
    for with_done in (True, False):
        want = L.twin(nperseg, hop, T, conditions, detrend, window, with_done)
        got = EV.spectrum_to_numpy(EV.spectrum_device(xd, dd if with_done else None, s, win, tw, **kw))
        worst = max(worst, L.within(got, want, L.bounds(want, nperseg, window, conditions), (nperseg, hop, T, conditions, detrend, window, with_done)))
    print("largest |device - twin| / bound: %.3g" % worst)
    first = EV.spectrum_to_numpy(EV.spectrum_device(xd, dd, s, win, tw, **kw))
    again = EV.spectrum_to_numpy(EV.spectrum_device(xd, dd, s, torch.from_numpy(win.copy()).to(DEV), torch.from_numpy(tw.copy()).to(DEV), **kw))
    for k in ("segments", "psd_sum", "sxx"):
        assert first[k].tobytes() == again[k].tobytes(), ("second run", k)
    off = EV.spectrum_to_numpy(EV.spectrum_device(xd, dd, s, win, tw, sxx=False, **kw))
    assert off["sxx"] is None and off["segments"].tobytes() == first["segments"].tobytes() and off["psd_sum"].tobytes() == first["psd_sum"].tobytes()
    if conditions == L.N:
        work = torch.full((EV.spectrum_work(L.N, s),), float("nan"), device=DEV, dtype=torch.float64)
        for w in (work, None):
            res = EV.spectrum_to_numpy(EV.spectrum_device(xd, dd, s, win, tw, work=w, **kw))
            for k in ("segments", "psd_sum", "sxx"):
                assert first[k].tobytes() == res[k].tobytes(), ("work", w is None, k)
    else:
        with pytest.raises(RuntimeError, match="irrl_eval_spectrum: .*work"):
            EV.spectrum_device(xd, dd, s, win, tw, work=None, **kw)
        with pytest.raises(ValueError, match="work"):
            EV.spectrum_device(xd, dd, s, win, tw, work=torch.zeros(3, device=DEV, dtype=torch.float64), **kw)


def test_device_refusals():
    x, done = L.case(16, 61)
    xd, dd = _device(x, done)
    s = L.spec(16, 5, 1)
    win, tw = L.tables(16, "hann")
    kw = dict(frame_first=FF, frame_every=FE, frames=61)
    with pytest.raises(ValueError, match="conditions"):
        EV.spectrum_device(xd, dd, s, win, tw, conditions=4, **kw)
    with pytest.raises(ValueError):
        EV.spectrum_device(xd, dd, s, win, tw, frame_first=FF, frame_every=FE, frames=63)          # past the recorder's rows
    with pytest.raises(ValueError, match="float32"):
        EV.spectrum_device(xd.double(), dd, s, win, tw, **kw)
    with pytest.raises(ValueError, match="rec_done"):
        EV.spectrum_device(xd, dd[:-1], s, win, tw, **kw)
    with pytest.raises(ValueError, match="spectrum_tables"):
        EV.spectrum_device(xd, dd, s, win[:-1], tw, **kw)
    with pytest.raises(ValueError, match="spectrum_tables"):
        EV.spectrum_device(xd, dd, s, win, tw.astype(np.float32), **kw)
    with pytest.raises(RuntimeError, match="irrl_eval_spectrum: .*matrix_env"):
        EV.spectrum_device(xd, dd, dict(s, matrix_env=(6,)), win, tw, **kw)
    with pytest.raises(ValueError, match="nperseg"):
        EV.spectrum_device(xd, dd, dict(s, nperseg=7), win, tw, **kw)


# ---- (b) the sweep ----
MUS, DELAYS, CMDS, WARM, STEPS = (0.8, 0.1), (0, 1, 2, 3), (1.0, 2.0), 20, 80
VIB = dict(nperseg=16, hop=8, window="hann", band_hz=100.0)        # (control_dt 0.002 s: fs = 500 Hz, 31.25 Hz per bin)


def _sweep_against_the_twin(policy, persistent, cfg, walkers):
    kw = dict(warm_steps=WARM, steps=STEPS, persistent=persistent, **TP.HZ)
    rows = EV.robustness_sweep(policy, cfg, MUS, DELAYS, CMDS, spectrum=VIB, record_spectrum=True, **kw)
    off = EV.robustness_sweep(policy, cfg, MUS, DELAYS, CMDS, **kw)
    assert len(rows) == len(off) == 16
    _, obs_std, _, act_std = obs_normalisation(cfg)
    fs = 1.0 / float(cfg["control_dt"])
    win, tw = EV.spectrum_tables(16, "hann")
    new = set(EV.spectrum_table_keys()) | {"spectrum", "sxx", "spec_x", "rec_done"}
    K, S_max = 9, (STEPS - 16) // 8 + 1
    seen = 0
    for i, (r, o) in enumerate(zip(rows, off)):
        assert set(r) - set(o) == (new if i < 8 else new - {"sxx"}) and {k: r[k] for k in o} == o, i
        assert np.array_equal(r["spectrum"]["freqs"], np.arange(K) * fs / 16) and r["rec_done"].shape == (STEPS,)
        for name, (rec, c0, cn) in EV.SPECTRUM_SOURCES.items():
            xs = r["spec_x"][name]
            assert xs.shape == (STEPS, 12) and xs.dtype == np.float32 and np.abs(xs).max() > 0
            std = (obs_std if rec == "obs_cond" else act_std)[c0:c0 + cn]
            s = EV.spectrum_spec(12, 0, 12, 16, 8, fs, scale=std, matrix_env=(0,))
            want = EV.spectrum_numpy(xs[:, None, :], r["rec_done"][:, None], s, win, tw, windowed=True)
            per = L.segment_bounds(want["a"], win, fs)                                  # [1, S_max, 12, K]
            assert r["spectrum"]["segments"] == int(want["segments"][0])
            got, b = r["spectrum"][name], per.sum(1)[0]
            assert got.shape == (12, K) and np.all(np.isfinite(got)) and np.all(np.abs(got - want["psd_sum"][0]) <= b), (i, name)
            if i < 8:
                gx, bx = r["sxx"][name], np.transpose(per[0], (1, 0, 2))
                assert gx.shape == (12, S_max, K) and np.all(np.abs(gx - want["sxx"][0]) <= bx), (i, name)
                assert np.all(gx[:, int(want["segments"][0]):] == 0.0)
            row = EV.spectrum_row({name: got}, r["spectrum"]["segments"], fs, (name,), VIB["band_hz"], nperseg=16)
            assert all(r[k] == v or (np.isnan(r[k]) and np.isnan(v)) for k, v in row.items()), (i, name, row)
            if r["spectrum"]["segments"] > 0 and got[:, 1:].sum() > 0:                  # (a column that never moves has no peak: NaN)
                assert 0.0 < r["vib_peak_hz_" + name] <= fs / 2 and 0.0 <= r["vib_frac_" + name] <= 1.0
                seen += 1
    assert seen >= 3 * walkers                                                         # that many robots lived to fill a segment
    return rows


def test_robustness_sweep_with_spectrum_lstm_both_forms():
    """16 robots (2 frictions x 4 delays x 2 commands), 20 warm-up + 80 measured steps, nperseg 16, hop 8, Hann: every row's sums and the first
    eight rows' spectrograms lie within the bound of the twin on the downloaded recorder words, the other keys equal the sweep without
    `spectrum`; the five-launch and the persistent form of the loop give the same bytes"""
    cfg = load_env_cfg("bp5_manual_eval.yaml", num_envs=4)
    per_step = _sweep_against_the_twin(TP.ACTOR, False, cfg, 1)
    persistent = _sweep_against_the_twin(TP.ACTOR, True, cfg, 1)
    for a, b in zip(per_step, persistent):
        for name in EV.SPECTRUM_SOURCES:
            assert a["spectrum"][name].tobytes() == b["spectrum"][name].tobytes() and a["spec_x"][name].tobytes() == b["spec_x"][name].tobytes()
    print(EV.sweep_table(per_step, spectrum=True))
    for name in EV.SPECTRUM_SOURCES:                                                   # the first condition's Welch spectra, for the record
        print("%-10s %s" % (name, " ".join("%.3e" % v for v in per_step[0]["spectrum"][name].sum(0) / max(per_step[0]["spectrum"]["segments"], 1))))
    with pytest.raises(KeyError, match="spectrum source"):
        EV.robustness_sweep(TP.ACTOR, cfg, MUS, DELAYS, CMDS, spectrum=dict(VIB, sources=("torque",)), warm_steps=0, steps=20)
    with pytest.raises(ValueError, match="unknown keys"):
        EV.robustness_sweep(TP.ACTOR, cfg, MUS, DELAYS, CMDS, spectrum=dict(VIB, overlap=3), warm_steps=0, steps=20)
    with pytest.raises(ValueError, match="record_spectrum"):
        EV.robustness_sweep(TP.ACTOR, cfg, MUS, DELAYS, CMDS, record_spectrum=True, warm_steps=0, steps=20)
    short = EV.robustness_sweep(TP.ACTOR, cfg, (0.8,), (0,), (1.0,), spectrum=VIB, warm_steps=0, steps=10)      # fewer frames than a segment
    assert short[0]["spectrum"]["segments"] == 0 and np.all(short[0]["spectrum"]["joint"] == 0.0) and np.isnan(short[0]["vib_peak_hz_joint"])
    assert short[0]["sxx"]["joint"].shape == (12, 0, 9)


def test_robustness_sweep_with_spectrum_mlp():
    cfg = load_env_cfg("bp5_manual_eval.yaml", num_envs=4)
    _sweep_against_the_twin(TM._mlp(), "auto", cfg, 0)
