"""The analyses of a gait recorder (evaluate.footfall_device -> irrl_eval_footfall: one workgroup per robot keeps the four legs' flags in LDS as
64-frame bit words; evaluate.motor_plane_device -> irrl_eval_motor_plane: one workgroup per (condition, joint)) on the MI355X against the numpy
twins (evaluate.footfall_numpy, evaluate.motor_plane_numpy), and the robustness sweep that carries them.

(a) the generated recorders of tests/eval_footfall_lib.py, uploaded: [rows, 5, 32] with frame_first = 3, frame_every = 2 and T = 1, 2, 4, 5, 11,
    12, 13, 63, 64, 65, 257, 1000 (the filter's borders, the word, wave and workgroup edges) and [rows, 2, 32] with T = 16384 (the 256-thread
    form), with and without rec_done.
(b) the motor plane on a generated [rows, 6, 32] recorder as 2 x 3 and on RaiSim's torques and rates as a [1000, 1, 32] recorder.
(c) the closed loop: robustness_sweep on frictions 0.8 / 0.1 x delays 0 / 3 at 2 m/s, 300 warm-up + 500 steps, footfall= and motor= on.
Everything is integers, or f64 sums added in one stated order: device == twin bit for bit, a second run gives the same bits, and an optional
output that is off leaves the others unchanged."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_footfall_lib as L
import test_gpu_eval_persistent as TP
from conftest import load_env_cfg
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV

SPEC = L.SPEC
FKEYS, MKEYS = ("counts", "support", "phase", "pattern"), ("counts", "hist", "fold")


def _up(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _footfall(rec, done, spec=SPEC, **kw):
    return EV.footfall_to_numpy(EV.footfall_device(_up(rec), _up(done), spec, **kw))


def _motor(rec, done, spec, conditions, **kw):
    return EV.motor_plane_to_numpy(EV.motor_plane_device(_up(rec), _up(done), spec, conditions, **kw))


def _same_bits(a, b, keys, what):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
        else:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


# ---- (a) generated recorders, footfall ----
@pytest.mark.parametrize("T", L.TS + (L.T_BIG,))
def test_footfall_device_equals_the_twin_bit_for_bit(T):
    """counts, support, phase and pattern == footfall_numpy with and without rec_done; a second run gives the same bits; every optional
    output off leaves the others unchanged"""
    N = 2 if T == L.T_BIG else 5
    rec, done = L.footfall_case(T, N)
    kw = dict(frame_first=L.FRAME_FIRST, frame_every=L.FRAME_EVERY, frames=T)
    for dn in (done, None):
        want = EV.footfall_numpy(rec, dn, SPEC, **kw)
        got = _footfall(rec, dn, **kw)
        print("T = %d, done %s: counts of robot 0, leg 0 %s" % (T, dn is not None, got["counts"][0, 0].tolist()))
        _same_bits(got, want, FKEYS, "T = %d" % T)
        _same_bits(_footfall(rec, dn, **kw), got, FKEYS, "second run")
    full = got
    bare = _footfall(rec, None, support=False, phase=False, pattern=False, **kw)
    assert bare["support"] is None and bare["phase"] is None and bare["pattern"] is None and bare["counts"].tobytes() == full["counts"].tobytes()
    for off in ("support", "phase", "pattern"):
        part = _footfall(rec, None, **dict(kw, **{off: False}))
        assert part[off] is None
        _same_bits(part, full, [k for k in FKEYS if k != off], off + " off")
    nobins = _footfall(rec, None, spec=dict(SPEC, phase_bins=0), **kw)
    assert nobins["phase"] is None
    _same_bits(nobins, full, ("counts", "support", "pattern"), "phase_bins = 0")


@pytest.mark.parametrize("spec", [dict(reach=0, hold=0, phase_bins=1), dict(reach=8, hold=64, phase_bins=64), dict(reach=1, hold=63, phase_bins=7),
                                  dict(reach=4, hold=19, phase_bins=16)])
def test_footfall_other_specs_and_hand_made_diagrams(spec):
    """the limits of reach, hold and phase_bins on T = 257 and T = 1000, and the four hand-made gaits as one recorder [1000, 4, 32]"""
    for T in (257, 1000):
        rec, done = L.footfall_case(T)
        kw = dict(frame_first=L.FRAME_FIRST, frame_every=L.FRAME_EVERY, frames=T)
        _same_bits(_footfall(rec, done, spec, **kw), EV.footfall_numpy(rec, done, spec, **kw), FKEYS, (T, spec))
    rng = np.random.RandomState(3)
    lags = ((0.0, 0.5, 0.5, 0.0), (0.0, 0.5, 0.0, 0.5), (0.0, 0.0, 0.5, 0.5), (0.0, 0.0, 0.0, 0.0))
    flags = np.stack([L.gait_flags(1000, 100, 0.4, lg, rng, dropouts=2, start=-10) for lg in lags], 1)
    rec, done = L.diagram_recorder(flags)
    got = _footfall(rec, done, spec)
    _same_bits(got, EV.footfall_numpy(rec, done, spec), FKEYS, "diagrams")
    if spec["reach"] == 4:
        names = [EV.footfall_row(got["counts"][i], got["support"][i], got["phase"][i], 0.01)["gait"] for i in range(4)]
        assert names == ["trot", "pace", "bound", "pronk"] and np.all(got["counts"][:, :, 4] == 10)


# ---- (b) the motor plane ----
@pytest.mark.parametrize("period,bins", [(7, 40), (1, 1), (100, 64), (1024, 64)])
def test_motor_plane_device_equals_the_twin_bit_for_bit(period, bins):
    """2 conditions x 3 robots with different T_e, samples on the envelope, NaN and inf words: counts and hist as integers, fold as f64 bytes;
    a second run gives the same bits; hist / fold off leave the others unchanged; 70 robots in one condition (more than one chunk of 64)"""
    spec = dict(L.MOTOR_SPEC, period=period, t_bins=bins, w_bins=bins if bins != 40 else 45)
    rec, done = L.motor_case(61)
    kw = dict(frame_first=L.FRAME_FIRST, frame_every=L.FRAME_EVERY, frames=61)
    for dn in (done, None):
        want = EV.motor_plane_numpy(rec, dn, spec, 2, **kw)
        got = _motor(rec, dn, spec, 2, **kw)
        _same_bits(got, want, MKEYS, (period, bins, dn is not None))
        _same_bits(_motor(rec, dn, spec, 2, **kw), got, MKEYS, "second run")
    bare = _motor(rec, None, spec, 2, hist=False, fold=False, **kw)
    assert bare["hist"] is None and bare["fold"] is None and bare["counts"].tobytes() == got["counts"].tobytes()
    for off, spec_off in (("hist", dict(spec, t_bins=0)), ("fold", dict(spec, period=0))):
        part = _motor(rec, None, spec_off, 2, **kw)
        assert part[off] is None
        _same_bits(part, got, [k for k in MKEYS if k != off], off + " off")
    _same_bits(_motor(rec, done, spec, None, **kw), EV.motor_plane_numpy(rec, done, spec, None, **kw), MKEYS, "one robot per condition")
    if period == 7:
        many, mdone = L.motor_case(33, conditions=1, robots=70)
        kw = dict(frame_first=L.FRAME_FIRST, frame_every=L.FRAME_EVERY, frames=33)
        _same_bits(_motor(many, mdone, spec, 1, **kw), EV.motor_plane_numpy(many, mdone, spec, 1, **kw), MKEYS, "70 robots")


def test_motor_plane_on_raisims_torques_and_rates():
    rec, d = L.raisim_motor_recorder()
    spec = EV.motor_spec(None, tau_max=18.0, w_crit=14.2, w_max=40.0, sat=float(d["sat"]))
    got = _motor(rec, None, spec, 1)
    _same_bits(got, EV.motor_plane_numpy(rec, None, spec), MKEYS, "fixture")
    assert np.array_equal(got["counts"][0], d["counts"]) and np.all(got["counts"][0, :, 3] == 0) and np.all(got["fold"][0, 7, :, 0] == 10.0)


# ---- (c) the closed loop ----
MUS, DELAYS, CMD, WARM, STEPS = (0.8, 0.1), (0, 3), 2.0, 300, 500
NEW_KEYS = {"footfall", "motor", "pattern", "hist", "rec_gait", "rec_done"}
OUTSIDE_SAT = 0.01     # the test's saturation band: evaluate.motor_spec's default (see the docstring below)


def _same_numbers(a, b):
    return set(a) == set(b) and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


def test_robustness_sweep_footfall_and_motor():
    """robustness_sweep(footfall=, motor=) on frictions 0.8 / 0.1 x delays 0 / 3 at 2 m/s, 300 warm-up + 500 steps, persistent where it exists:
    every row's device results equal the twins run on the row's own downloaded gait recorder bit for bit (both are pure functions of the same f32
    words); TOUCHDOWNS <= RAW_TOUCHDOWNS on every leg; OUTSIDE == 0 at the default sat = 0.01, because the engine clamps to this envelope;
    without the keywords the rows have today's keys and bits.
    Measured on one MI355X (the figures are printed): at 2 m/s no sample of the four conditions comes nearer than 3.0 N m to the envelope (its
    largest "excess" is -3.03 N m) and no joint is saturated, so no sample lands outside by rounding and the band was not widened; raw
    touchdown rate 21.5 .. 23.5 per second and leg, debounced stride frequency 4.99 .. 5.06 Hz, duty 0.50 .. 0.53, a trot.  (At 5 m/s, which
    this test does not run, the recorder's pairs do leave the envelope, by up to 0.9 N m: HISTORY.md says why.)"""
    cfg = load_env_cfg("bp5_manual_eval.yaml", num_envs=4)
    mspec = EV.motor_spec(cfg, sat=OUTSIDE_SAT)
    sweep = lambda **kw: EV.robustness_sweep(TP.ACTOR, cfg, MUS, DELAYS, [CMD], warm_steps=WARM, steps=STEPS, persistent="auto", **kw)
    rows = sweep(footfall=SPEC, motor=mspec, record_gait=True)
    assert len(rows) == 4
    dt = float(cfg["control_dt"])
    worst = 0.0
    for r in rows:
        assert NEW_KEYS <= set(r) and r["rec_gait"].shape == (STEPS, 32) and r["pattern"].shape == (STEPS,) and r["hist"].shape == (12, 40, 45)
        rec, done = r["rec_gait"][:, None, :], r["rec_done"][:, None]
        f = EV.footfall_numpy(rec, done, SPEC)
        assert r["footfall"]["counts"].tobytes() == f["counts"][0].tobytes() and r["footfall"]["support"].tobytes() == f["support"][0].tobytes()
        assert r["footfall"]["phase"].tobytes() == f["phase"][0].tobytes() and r["pattern"].tobytes() == f["pattern"][:, 0].tobytes()
        want = EV.footfall_row(f["counts"][0], f["support"][0], f["phase"][0], dt)
        assert _same_numbers({k: v for k, v in r["footfall"].items() if k not in ("counts", "support", "phase")}, want)
        m = EV.motor_plane_numpy(rec, done, mspec)
        assert r["motor"]["counts"].tobytes() == m["counts"][0].tobytes() and r["motor"]["fold"].tobytes() == m["fold"][0].tobytes()
        assert r["hist"].tobytes() == m["hist"][0].tobytes()
        c = f["counts"][0].astype(np.int64)
        assert np.all(c[:, 4] <= c[:, 2]), c[:, (2, 4)]
        mm, ww, kept = EV.motor_samples(rec[:int(c[0, 0]), 0], mspec)
        up, low = EV.motor_up(ww, mspec), -EV.motor_up(-ww, mspec)
        excess = float(np.max(np.where(kept, np.maximum(mm - up, low - mm), -np.inf))) if kept.any() else 0.0
        worst = max(worst, excess)
        print("mu %g delay %d: frames %d, raw touchdown rate %.2f Hz, debounced stride %.2f Hz, duty %.3f, gait %s, largest excess over the envelope %.3e N m, "
              "saturated %.4f" % (r["mu"], r["delay"], c[0, 0], r["footfall"]["raw_hz"], r["footfall"]["stride_hz"], r["footfall"]["duty"], r["footfall"]["gait"],
                                  excess, float(np.nanmax(r["motor"]["saturated"]))))
    print("largest excess over the envelope: %.6e N m" % worst)
    print(EV.sweep_table(rows, footfall=True))
    for r in rows:
        assert np.all(r["motor"]["counts"][:, 3] == 0), (r["mu"], r["delay"], r["motor"]["counts"][:, 3].tolist())
    plain, again = sweep(), sweep()
    old = set(rows[0]) - NEW_KEYS
    for p, a, r in zip(plain, again, rows):
        assert set(p) == old and _same_numbers(p, a) and _same_numbers(p, {k: r[k] for k in old})
