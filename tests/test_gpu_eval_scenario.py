"""The evaluation loop with a scenario -- command schedule, heading hold, statistics buckets (PolicyEvaluator.set_scenario ->
irrl_lstm_eval_scenario[_persistent]) -- on the MI355X: the two device forms against each other bit for bit, a neutral scenario against no
scenario, split invariance, the schedule's routing, the heading element against a float64 PI, the buckets against body_statistics, and the closed
loop against the host-driven twin.

Pool and actor as tests/test_gpu_eval_persistent.py builds them (its helpers are used): bp5_manual_eval.yaml, N = 19 (a ragged last wave), D = 6 with
delays e % 6, frictions 0.05 .. 0.8, filters at 1 / 50 / 30 Hz, the bp5_155 actor, 60 steps as 20 + 40 with envs 3 and 17 dropped to z = 0.14 between
the calls.  The scenario: S = 5 command rows held 7 steps, B = 3 buckets of 16 steps, t0 = 4 -- schedule and bucket boundaries fall inside both calls
and the call boundary falls mid-segment --, heading hold with per-env references and gains, off on the envs e % 5 == 4."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import parity_lib as PL
import test_gpu_eval_persistent as TP
from conftest import load_env_cfg
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV
from high_speed_quadrupedal_locomotion_by_irrl_amd.checkpoint import NumpyLstmActor
from high_speed_quadrupedal_locomotion_by_irrl_amd.helper import obs_normalisation

N, D, T, T1, HZ, ALL, ACTOR, FALLERS = TP.N, TP.D, TP.T, TP.T1, TP.HZ, TP.ALL, TP.ACTOR, TP.FALLERS
S, CMD_EVERY, B, STAT_EVERY, T0 = 5, 7, 3, 16, 4


@pytest.fixture(scope="module")
def policy():
    return EV.load_policy(ACTOR, torch.device("cuda"))


def _table(n):
    return np.stack([(r + 1) / S * np.linspace(0.5, 5.0, n)[:, None] * np.array([1.0, 0.1, -0.05])[None] for r in range(S)], 0)


def _heading(n):
    off = np.arange(n) % 5 == 4
    return dict(ref=np.linspace(-0.8, 0.8, n), kp=np.where(off, 0.0, np.linspace(0.5, 1.5, n)), ki=np.where(off, 0.0, 0.1 + 0.05 * (np.arange(n) % 3)), windup=0.004)


def _install(ev):
    """(windup 0.004: an env 0.5 rad off its reference for 60 steps of 2 ms integrates 0.06, so the clamp engages on most envs)"""
    ev.set_scenario(cmd_schedule=_table(ev.n), cmd_every=CMD_EVERY, heading=_heading(ev.n), stat_buckets=B, stat_every=STAT_EVERY, t0=T0)
    return ev


def _same(a, b, n):
    TP._assert_same_buffers(a, b, n)
    assert a.stats.shape == b.stats.shape and torch.equal(a.heading_int, b.heading_int)


def _run(ev, calls, persistent, drop_at=None):
    parts = []
    for s in calls:
        if drop_at is not None and ev.t == drop_at:
            TP._drop(ev.env)
        parts.append(ev.run(s, record=ALL, persistent=persistent))
    return TP._cat(parts)


@pytest.fixture(scope="module")
def scene(policy):
    """the shared scenario in the five-launch form, 20 + 40 with the drop: records, the state in front of the run, the evaluator"""
    ev = _install(TP._evaluator(policy, N, **HZ))
    state0 = ev.env.get_state()
    rec = _run(ev, (T1, T - T1), False, drop_at=T1)
    torch.cuda.synchronize()
    return dict(ev=ev, rec=rec, np={k: v.cpu().numpy() for k, v in rec.items()}, state0=state0)


@pytest.mark.parametrize("over, variant", [({}, "shipped_flat"), ({"ContactExit": 0}, "md")])
def test_the_scenario_in_both_forms_is_bit_identical(policy, scene, over, variant):
    """test 1: every recorder, stats [B, 18, N], ring, cmd, both histories, heading_int, done, obs, the actor's half of lstm_state, get_state and
    GetJointEffort, for the shipped solver settings and for the run-time-solver kernel (`md`)"""
    a = _install(TP._evaluator(policy, N, over, **HZ))
    ra = _run(a, (T1, T - T1), True, drop_at=T1)
    if over:
        b = _install(TP._evaluator(policy, N, over, **HZ))
        rb = _run(b, (T1, T - T1), False, drop_at=T1)
    else:
        b, rb = scene["ev"], scene["rec"]
    assert a.env.kernel_variant == variant and a.persistent_supported
    done = ra["done"].cpu().numpy()
    assert sorted(np.flatnonzero(done[T1])) == FALLERS and int(done.sum()) == 2
    TP._assert_same_records(ra, rb)
    _same(a, b, N)
    assert a.stats.shape == (B, len(EV.STAT_SLOTS), N)
    frames = a.stats[:, 0].cpu().numpy()
    assert np.array_equal(frames, np.repeat(np.array([T0 + STAT_EVERY, STAT_EVERY, T - T0 - 2 * STAT_EVERY], float)[:, None], N, 1))
    assert float(a.heading_int.abs().max()) > 0.0


@pytest.mark.parametrize("persistent", [False, True])
def test_a_neutral_scenario_equals_no_scenario(policy, persistent):
    """test 2: one row equal to cmd_target, B = 1, gains zero -- through the scenario entry point -- against the old entry point, both forms"""
    a, b = TP._evaluator(policy, N, **HZ), TP._evaluator(policy, N, **HZ)
    a.set_scenario(heading=dict(ref=0.3, kp=0.0, ki=0.0))
    assert a.scenario is not None and b.scenario is None and a.stats.shape == (1, len(EV.STAT_SLOTS), N)
    ra, rb = _run(a, (T1, T - T1), persistent, drop_at=T1), _run(b, (T1, T - T1), persistent, drop_at=T1)
    TP._assert_same_records(ra, rb)
    a.stats = a.stats[0]
    _same(a, b, N)
    assert float(a.heading_int.abs().max()) == 0.0


@pytest.mark.parametrize("n", [N, 1, 16])
def test_split_invariance(policy, n):
    """test 3: 60 steps as one call, as 20 + 40 and as 1 + 0 + 59 (a single-step launch, a call that launches nothing, a resume) in the persistent
    form, and as 20 + 40 in the five-launch form, leave identical records and buffers; N = 19, 1 and 16"""
    runs = []
    for calls in ((T,), (T1, T - T1), (1, 0, T - 1)):
        ev = _install(TP._evaluator(policy, n, **HZ))
        runs.append((ev, _run(ev, calls, True)))
    five = _install(TP._evaluator(policy, n, **HZ))
    runs.append((five, _run(five, (T1, T - T1), False)))
    for ev, rec in runs[1:]:
        TP._assert_same_records(runs[0][1], rec)
        _same(runs[0][0], ev, n)


def test_the_two_forms_alternate_mid_scenario(policy, scene):
    """test 4: 20 persistent + 20 five-launch + 20 persistent on one evaluator == the shared five-launch scene (the drop at step 20 included)"""
    a = _install(TP._evaluator(policy, N, **HZ))
    parts = [a.run(T1, record=ALL, persistent=True)]
    TP._drop(a.env)
    parts += [a.run(20, record=ALL, persistent=False), a.run(20, record=ALL, persistent=True)]
    TP._assert_same_records(TP._cat(parts), scene["rec"])
    _same(a, scene["ev"], N)


def test_schedule_routing_and_heading_element(policy):
    """test 5, command filter off: recorded obs_cond[:, :, 0:3] ARE the scaled table rows bit for bit (element 2 on the heading-off envs); element 2
    of the heading-on envs equals the float64 PI recomputed from the recorded body rows (step t reads row t - 1, step 0 get_state in front of the
    run) within 2e-5 -- tests/test_eval_scenario_host.py measures 7.7e-7 for the same arithmetic on the host --; heading_int of the dropped envs is
    zero right behind their `done`"""
    ev = _install(TP._evaluator(policy, N, cmd_hz=None, vel_hz=50.0, act_hz=30.0))
    q0 = ev.env.get_state()[:, 3:7]
    first = ev.run(T1, record=("obs_cond", "body", "done"), persistent=True)
    TP._drop(ev.env)
    step = ev.run(1, record=("obs_cond", "body", "done"), persistent=True)
    torch.cuda.synchronize()
    integ_after_done = ev.heading_int.cpu().numpy().copy()
    rest = ev.run(T - T1 - 1, record=("obs_cond", "body", "done"), persistent=True)
    rec = {k: v.cpu().numpy() for k, v in TP._cat([first, step, rest]).items()}
    assert sorted(np.flatnonzero(rec["done"][T1])) == FALLERS
    assert np.all(integ_after_done[FALLERS] == 0.0) and np.abs(integ_after_done).max() > 0.0
    cfg = load_env_cfg("bp5_manual_eval.yaml")
    mean, std, _, _ = obs_normalisation(cfg)
    rows = np.array([EV.schedule_row(t, T0, CMD_EVERY, S) for t in range(T)])
    scaled = (_table(N).astype(np.float32) - np.asarray(mean[0:3], np.float32)) / np.asarray(std[0:3], np.float32)
    h = EV.heading_parameters(_heading(N), N, float(cfg["Omega"]), float(cfg["control_dt"]))
    on = (h["kp"] != 0) | (h["ki"] != 0)
    assert on.sum() == N - len(range(4, N, 5))
    assert np.array_equal(rec["obs_cond"][:, :, 0:2].view(np.uint32), scaled[rows][:, :, 0:2].view(np.uint32))
    assert np.array_equal(rec["obs_cond"][:, ~on, 2].view(np.uint32), scaled[rows][:, ~on, 2].view(np.uint32))
    # the device's parameters are the f32 roundings of these; the recomputation runs in f64 from them
    f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    ref, kp, ki, w, dt = f32(h["ref"]), f32(h["kp"]), f32(h["ki"]), float(np.float32(h["windup"])), float(np.float32(h["dt"]))
    quat = np.concatenate([q0[None], rec["body"][:-1, :, 3:7]], 0).astype(np.float64)
    integ, worst, clamped = np.zeros(N), 0.0, 0
    for t in range(T):
        err = EV.wrap_angle(ref - EV.yaw_from_quaternion(quat[t]))
        assert np.abs(err).max() < 3.0
        integ = np.clip(integ + err * dt, -w, w)
        clamped += int((np.abs(integ[on]) == w).sum())
        want = ((kp * err + ki * integ) - mean[2]) / std[2]
        worst = max(worst, np.abs(want[on] - rec["obs_cond"][t, on, 2]).max())
        integ[rec["done"][t]] = 0.0
    print("max |device - float64 PI| heading element: %.3g; env-steps on the clamp: %d" % (worst, clamped))
    assert worst <= 2e-5 and clamped > 0
    assert np.abs(np.where(on, integ, 0.0) - ev.heading_int.cpu().numpy()).max() <= 1e-7


def test_bucket_statistics_equal_the_body_log_statistics_per_bucket(scene):
    """test 6: per bucket and env, against evaluate.body_statistics of the recorded body rows of that bucket's steps: means 1e-9 absolute,
    standard deviations 1e-6 relative (the bounds of tests/test_gpu_eval_rollout.py); frames and falls exact; statistics() is the whole window"""
    got = scene["ev"].bucket_statistics()
    buckets = np.array([EV.schedule_row(t, T0, STAT_EVERY, B) for t in range(T)])
    worst = {}
    for b in range(B):
        sel = buckets == b
        for e in range(N):
            for k, v in EV.body_statistics(scene["np"]["body"][sel, e]).items():
                if k == "vx_body":
                    continue
                err = abs(got[k][b, e] - v) if k.endswith("_mean") else abs(got[k][b, e] - v) / abs(v)
                worst[k] = max(worst.get(k, 0.0), err)
        assert np.all(got["frames"][b] == sel.sum()) and np.array_equal(got["falls"][b], scene["np"]["done"][sel].sum(0))
    print("worst |device - body_statistics| per bucket (means absolute, stds relative):", {k: "%.2e" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= (1e-9 if k.endswith("_mean") else 1e-6), (k, v)
    whole = scene["ev"].statistics()
    assert np.all(whole["frames"] == T) and np.array_equal(whole["falls"], scene["np"]["done"].sum(0))
    for e in range(N):
        assert abs(whole["vx_body_mean"][e] - EV.body_statistics(scene["np"]["body"][:, e])["vx_body_mean"]) <= 1e-9


LEVELS, LEVEL_STEPS = 4, 600


def test_staircase_sweep_with_heading_hold_agrees_with_the_host_driven_twin():
    """test 7: mu 0.8 x delays 0, 1 x commands 5, 4 m/s, the four-level staircase of 600 steps per level with the heading hold on, no warm-up: ONE
    persistent launch of 2400 steps through evaluate.robustness_sweep against evaluate.reference_rollout on HipVecEnv (same GPU) with the same
    schedule and heading.  Per level, over its second half (300 frames, three gait periods): v_x, height and mean pitch inside
    parity_lib.RAISIM_LOG_TOL, the project's bound for this device-against-host comparison at constant command; no falls on either side.
    Margin, measured before anything else the way the constant-command sweep test's was: this twin on the f64 oracle on the CPU with N(0, 2e-5)
    noise on the actions, three seeds against the noise-free run, worst of the four envs per level --
        level 1 (1.25 / 1.0 m/s): v_x 4.7e-4 relative (4.9e-4 m/s), z 1.9e-5 m, pitch 5.8e-5 rad
        level 2:                  v_x 2.0e-4 relative,              z 2.9e-5 m, pitch 1.8e-4 rad
        level 3:                  v_x 3.7e-4 relative,              z 1.0e-4 m, pitch 1.9e-4 rad
        level 4 (5 / 4 m/s):      v_x 4.5e-4 relative,              z 7.9e-5 m, pitch 1.5e-4 rad
    against the bounds 2 %, 4 mm and 0.004 rad: every level, level 1 included, stays a factor of 20 or more inside on the oracle alone, so all
    four levels are compared relatively under RAISIM_LOG_TOL as it stands."""
    from hip_env import HipVecEnv
    grid = [(0.8, d, c) for d in (0, 1) for c in (5.0, 4.0)]
    n = len(grid)
    cfg = load_env_cfg("bp5_manual_eval.yaml", num_envs=n)
    rows = EV.robustness_sweep(ACTOR, cfg, [0.8], [0, 1], [5.0, 4.0], warm_steps=0, levels=LEVELS, level_steps=LEVEL_STEPS, heading=EV.heading_hold(n))
    assert len(rows) == n * LEVELS and [r["level"] for r in rows[:LEVELS]] == [1, 2, 3, 4]
    rec = EV.reference_rollout(HipVecEnv(cfg), NumpyLstmActor.from_npz(ACTOR), cfg, [g[1] for g in grid],
                               [g[2] for g in grid], LEVELS * LEVEL_STEPS, cmd_schedule=EV.staircase_schedule([g[2] for g in grid], LEVELS),
                               cmd_every=LEVEL_STEPS, heading=EV.heading_hold(n), mu=[g[0] for g in grid])
    assert int(rec["falls"].sum()) == 0
    tol = PL.RAISIM_LOG_TOL
    print()
    for i, g in enumerate(grid):
        for l in range(LEVELS):
            r = rows[i * LEVELS + l]
            h = EV.body_statistics(rec["body"][l * LEVEL_STEPS + LEVEL_STEPS // 2:(l + 1) * LEVEL_STEPS, i])
            assert (r["mu"], r["delay"], r["cmd"], r["level"]) == (g[0], g[1], g[2], l + 1) and r["cmd_level"] == (l + 1) / LEVELS * g[2]
            print("delay %d cmd %.1f level %d (%.2f m/s): device vx %.4f z %.4f pitch %+.4f | host vx %.4f z %.4f pitch %+.4f" % (
                g[1], g[2], l + 1, r["cmd_level"], r["vx_body_mean"], r["z_mean"], r["pitch_mean"], h["vx_body_mean"], h["z_mean"], h["pitch_mean"]))
            assert r["falls"] == 0 and r["frames"] == LEVEL_STEPS // 2
            assert abs(r["vx_body_mean"] - h["vx_body_mean"]) / abs(h["vx_body_mean"]) < tol["vx_rel"], (g, l, r["vx_body_mean"], h["vx_body_mean"])
            assert abs(r["z_mean"] - h["z_mean"]) < tol["z_abs"], (g, l, r["z_mean"], h["z_mean"])
            assert abs(r["pitch_mean"] - h["pitch_mean"]) < tol["pitch_mean_abs"], (g, l, r["pitch_mean"], h["pitch_mean"])


def test_capability_and_refusals_with_a_scenario(policy):
    """test 8: a Crutial pool and a (32, 32) policy are refused by the persistent scenario call with the condition named; the five-launch
    scenario call runs on them"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import CustomLSTMPolicy
    torch.manual_seed(5)
    small = CustomLSTMPolicy(n_lstm=(32, 32)).to(torch.device("cuda"))
    small.prepare()
    n = 6
    for over, pol, word in (({"Crutial": True}, policy, "crutial"), ({}, small, "hid 48")):
        a = _install(TP._evaluator(pol, n, over, **HZ))
        assert a.persistent_supported is False
        with pytest.raises(RuntimeError, match=word) as info:
            a.run(3, persistent=True)
        assert "irrl_lstm_eval_scenario_persistent" in str(info.value) and a.t == 0
        rec = a.run(12, record=ALL, persistent=False)
        torch.cuda.synchronize()
        assert rec["body"].shape == (12, n, 13) and a.t == 12 and float(a.stats[:, 0].sum()) == 12.0 * n
        assert float(a.heading_int.abs().max()) > 0.0


def test_reset_rebases_the_scenario_origin(policy):
    """a scenario installed mid-run (t0 = the then-current t) starts at its first row again after reset(): 20 steps, install, reset, 30 steps ==
    a fresh evaluator with the scenario installed at t = 0"""
    a, b = TP._evaluator(policy, 6, **HZ), TP._evaluator(policy, 6, **HZ)
    a.run(T1)
    a.set_scenario(cmd_schedule=_table(6), cmd_every=CMD_EVERY, heading=_heading(6), stat_buckets=B, stat_every=STAT_EVERY)
    assert a.scenario["t0"] == T1
    a.reset()
    assert a.t == 0 and a.scenario["t0"] == 0
    b.set_scenario(cmd_schedule=_table(6), cmd_every=CMD_EVERY, heading=_heading(6), stat_buckets=B, stat_every=STAT_EVERY)
    ra, rb = a.run(30, record=ALL, persistent=True), b.run(30, record=ALL, persistent=True)
    TP._assert_same_records(ra, rb)       # (the pools' full states are not compared: a pool that ran before its reset keeps counters of its own)
    torch.cuda.synchronize()
    for k in ("stats", "ring", "cmd", "vel_his", "act_his", "heading_int", "done", "obs"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    c = TP._evaluator(policy, 6, **HZ)
    c.set_scenario(t0=1000)
    c.run(5)
    c.reset()
    assert c.scenario["t0"] == 1000
