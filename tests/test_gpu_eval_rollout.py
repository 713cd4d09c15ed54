"""The device-resident evaluation loop (evaluate.PolicyEvaluator -> irrl_lstm_eval_rollout, kernels csrc/eval_rollout.hpp) on the MI355X, piece by
piece against what already exists: the numpy conditioning, the policy-step kernel, the float64 action filter, a second pool replaying the applied
actions, get_state, evaluate.body_statistics, and the host-driven closed loop.

One scenario is computed once and shared: bp5_manual_eval.yaml with N = 19 envs (ragged against the 16-env policy workgroup and the
4-robots-per-wave env layout), the bp5_155 actor (hid 48), D = 6 with delays e % 6, commands 0.5 .. 5 m/s, frictions 0.05 .. 0.8, command / rate /
action low-passes at 1 / 50 / 30 Hz, T = 60 steps issued as 20 + 40, and between the two calls the base of envs 3 and 17 is put at 0.14 m (below the
0.15 m termination height): exactly those two terminate at step 20."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

import parity_lib as PL
from conftest import GOLDEN, load_env_cfg
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV
from high_speed_quadrupedal_locomotion_by_irrl_amd.helper import obs_normalisation

N, D, T, T1 = 19, 6, 60, 20
FALLERS = [3, 17]
DELAYS = np.arange(N) % D
CMDS = np.linspace(0.5, 5.0, N)
MUS = np.linspace(0.05, 0.8, N)
HZ = dict(cmd_hz=1.0, vel_hz=50.0, act_hz=30.0)
ALL = tuple(EV.RECORDERS)
ACTOR = os.path.join(GOLDEN, "actor_bp5_155.npz")      # the reference's trained bp5_155 actor


def _cfg(n=N):
    return load_env_cfg("bp5_manual_eval.yaml", num_envs=n)


def _pool(n=N, mus=MUS):
    import high_speed_quadrupedal_locomotion_by_irrl_amd as pkg
    from high_speed_quadrupedal_locomotion_by_irrl_amd.flexible_robot import FlexibleGymEnv
    env = FlexibleGymEnv(pkg.__BLACKPANTHER_V55_RESOURCE_DIRECTORY__, yaml.safe_dump(_cfg(n), default_flow_style=False, width=float("inf")))
    env.init()
    env.SetContactCoefficient(EV.contact_material(mus))
    return env


def _drop(env):
    st = env.get_state()
    st[FALLERS, 2] = 0.14
    env.set_state(st)


def _cat(a, b):
    return {k: torch.cat([a[k], b[k]], 0) for k in a}


@pytest.fixture(scope="module")
def scene():
    pol = EV.load_policy(ACTOR, torch.device("cuda"))
    env = _pool()
    ev = EV.PolicyEvaluator(env, pol, DELAYS, CMDS, depth=D, **HZ)
    ob_reset = ev.obs.clone()
    first = ev.run(T1, record=ALL)
    _drop(env)
    rec = _cat(first, ev.run(T - T1, record=ALL))
    torch.cuda.synchronize()
    effort = np.zeros((N, 12), np.float32)
    env.GetJointEffort(effort)
    out = dict(pol=pol, ev=ev, ob_reset=ob_reset, rec=rec, np={k: v.cpu().numpy() for k, v in rec.items()}, final=env.get_state(), effort=effort,
               stats=ev.statistics())
    # the same pool once more with the rate filter off: the delay line alone
    ev2 = EV.PolicyEvaluator(env, pol, DELAYS, CMDS, depth=D, cmd_hz=1.0, vel_hz=None, act_hz=30.0)
    out["ob_reset2"] = ev2.obs.cpu().numpy()
    out["routing"] = {k: v.cpu().numpy() for k, v in ev2.run(15, record=("obs_cond", "obs_raw")).items()}
    return out


def test_exactly_the_two_dropped_envs_terminate(scene):
    done = scene["np"]["done"]
    assert done.shape == (T, N) and sorted(np.flatnonzero(done[T1])) == FALLERS and int(done.sum()) == 2


def test_conditioning_equals_the_numpy_twin(scene):
    """numpy condition() applied to the device's own raw observations and done flags.  f32 rounding of a convex low-pass: at most 2 ulp per step,
    summing to 2 ulp / alpha -- 2e-5 on elements 3-34 (alpha_vel 0.386, |o| <~ 10), 2e-4 on the command elements (alpha_cmd 0.0124, |cmd| <= 5)."""
    raw, done, cond = scene["np"]["obs_raw"], scene["np"]["done"], scene["np"]["obs_cond"]
    cfg = _cfg()
    mean, std, _, _ = obs_normalisation(cfg)
    dt = float(cfg["control_dt"])
    a_cmd, a_vel = EV.lowpass_alpha(dt, HZ["cmd_hz"]), EV.lowpass_alpha(dt, HZ["vel_hz"])
    target = np.stack([CMDS, np.zeros(N), np.zeros(N)], 1)
    st = EV.condition_state(scene["ob_reset"].cpu().numpy(), D)
    worst = [0.0, 0.0]
    for t in range(T):
        o = EV.condition(st, t, scene["ob_reset"].cpu().numpy() if t == 0 else raw[t - 1], DELAYS, target, a_cmd, a_vel, mean[0:3], std[0:3])
        worst = [max(worst[0], np.abs(o[:, 3:] - cond[t, :, 3:]).max()), max(worst[1], np.abs(o[:, 0:3] - cond[t, :, 0:3]).max())]
        st["cmd"][done[t]] = 0.0
    print("max |device - numpy| conditioned observation: elements 3-34 %.3g, command elements %.3g" % tuple(worst))
    assert worst[0] <= 2e-5 and worst[1] <= 2e-4


def test_delay_line_routes_bit_for_bit(scene):
    """rate filter off: rec_obs_cond[t, e, 3:] IS rec_obs_raw[max(t - delay_e, 0) - 1, e, 3:] (index -1: the reset observation)"""
    cond, raw = scene["routing"]["obs_cond"], scene["routing"]["obs_raw"]
    src = np.concatenate([scene["ob_reset2"][None], raw], 0)          # src[k + 1] = raw[k]
    for t in range(cond.shape[0]):
        want = src[np.maximum(t - DELAYS, 0), np.arange(N)]
        assert np.array_equal(cond[t, :, 3:].view(np.uint32), want[:, 3:].view(np.uint32)), t


def test_actor_is_the_policy_step_kernel(scene):
    """policy.fused_step replayed deterministically over the recorded conditioned observations and done flags gives rec_act_clipped bit for bit,
    LSTM resets of envs 3 and 17 included"""
    pol, rec = scene["pol"], scene["rec"]
    st = pol.initial_state(N, rec["obs_cond"].device)
    done = torch.zeros(N, dtype=torch.bool, device=st.device)
    for t in range(T):
        _, clipped, _, _, st = pol.fused_step(rec["obs_cond"][t].contiguous(), st, done, noise=None)
        assert torch.equal(clipped, rec["act_clipped"][t]), t
        done = rec["done"][t].contiguous()
    assert torch.equal(st, scene["ev"].lstm_state)


def test_action_filter(scene):
    """rec_act_applied against the float64 low-pass of rec_act_clipped: |a| <= 1, alpha_act 0.274 -> 2 ulp / alpha < 1e-5"""
    a = EV.lowpass_alpha(float(_cfg()["control_dt"]), HZ["act_hz"])
    y = np.zeros((N, 12))
    worst = 0.0
    for t in range(T):
        y = (1 - a) * y + a * scene["np"]["act_clipped"][t].astype(np.float64)
        worst = max(worst, np.abs(y - scene["np"]["act_applied"][t]).max())
    print("max |device - float64| applied action: %.3g" % worst)
    assert worst <= 1e-5
    assert np.array_equal(scene["np"]["act_applied"][-1], scene["ev"].act_his.cpu().numpy())


def test_env_steps_equal_a_second_pool_replaying_the_applied_actions(scene):
    """an identical pool stepped through rec_act_applied by the existing step_rows (one launch per step), with the same set_state after step 20,
    reproduces rec_obs_raw, rec_reward and rec_done bit for bit and ends in the identical pool state"""
    env = _pool()
    dev = scene["rec"]["act_applied"].device
    ob0 = torch.zeros(N, 35, device=dev)
    env.reset(ob0)
    assert torch.equal(ob0, scene["ob_reset"])
    rows = scene["rec"]["act_applied"].contiguous()
    ob, rew = torch.zeros(T, N, 35, device=dev), torch.zeros(T, N, device=dev)
    done, extra = torch.zeros(T, N, dtype=torch.bool, device=dev), torch.zeros(T, N, 6, device=dev)
    env.step_rows(T1, rows, 0, ob[:T1], rew[:T1], done[:T1], extra[:T1], persistent=False)
    _drop(env)
    env.step_rows(T - T1, rows, T1, ob[T1:], rew[T1:], done[T1:], extra[T1:], persistent=False)
    assert torch.equal(ob, scene["rec"]["obs_raw"]) and torch.equal(rew, scene["rec"]["reward"]) and torch.equal(done, scene["rec"]["done"])
    assert np.array_equal(env.get_state(), scene["final"])


def test_recorders_show_the_pool(scene):
    """last row of rec_body = gc[0:7] | gv[0:6] of get_state, last row of rec_torque = GetJointEffort, as f32"""
    fin = scene["final"]
    want = np.concatenate([fin[:, 0:7], fin[:, 19:25]], 1).astype(np.float32)
    assert np.array_equal(scene["np"]["body"][-1], want)
    assert np.array_equal(scene["np"]["torque"][-1], scene["effort"])
    assert np.array_equal(scene["np"]["obs_raw"][-1], scene["ev"].obs.cpu().numpy())


def test_statistics_equal_the_body_log_statistics_of_the_recorded_rows(scene):
    """per env over the 60 rows (accumulated over the two calls): means to 1e-9 absolute, standard deviations to 1e-6 relative (f64 accumulation
    of f32 samples of O(1) on both sides); falls = rec_done.sum(0) exactly"""
    st = scene["stats"]
    worst = {}
    for e in range(N):
        want = EV.body_statistics(scene["np"]["body"][:, e])
        for k, v in want.items():
            if k == "vx_body":
                continue
            err = abs(st[k][e] - v) if k.endswith("_mean") else abs(st[k][e] - v) / abs(v)
            worst[k] = max(worst.get(k, 0.0), err)
    print("worst |device - body_statistics| (means absolute, stds relative):", {k: "%.2e" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= (1e-9 if k.endswith("_mean") else 1e-6), (k, v)
    assert np.array_equal(st["falls"], scene["np"]["done"].sum(0)) and np.all(st["frames"] == T)


def test_filters_off_is_the_plain_loop_of_the_existing_calls():
    """a_cmd = a_vel = a_act = 1 and no delay: rec_obs_raw, rec_act_applied and the final pool state are bit-identical to a host-driven loop of
    the existing calls (command written into obs[:, 0:3] in torch, policy step, env.step on the clipped action)"""
    steps = 30
    pol = EV.load_policy(ACTOR, torch.device("cuda"))
    env = _pool()
    ev = EV.PolicyEvaluator(env, pol, np.zeros(N, int), CMDS, cmd_hz=None, vel_hz=None, act_hz=None)
    assert ev.depth == 1 and ev.a_cmd == ev.a_vel == ev.a_act == 1.0
    rec = ev.run(steps, record=("obs_raw", "act_applied", "act_clipped"))
    assert torch.equal(rec["act_applied"], rec["act_clipped"])
    env2 = _pool()
    dev = ev.obs.device
    mean, std, _, _ = obs_normalisation(_cfg())
    scaled = (torch.from_numpy(np.stack([CMDS, np.zeros(N), np.zeros(N)], 1).astype(np.float32)).to(dev)
              - torch.tensor(mean[0:3], dtype=torch.float32, device=dev)) / torch.tensor(std[0:3], dtype=torch.float32, device=dev)
    obs, rew = torch.zeros(N, 35, device=dev), torch.zeros(N, device=dev)
    done, extra = torch.zeros(N, dtype=torch.bool, device=dev), torch.zeros(N, 6, device=dev)
    env2.reset(obs)
    st = pol.initial_state(N, dev)
    for t in range(steps):
        o = obs.clone()
        o[:, 0:3] = scaled
        _, clipped, _, _, st = pol.fused_step(o, st, done, noise=None)
        assert torch.equal(clipped, rec["act_applied"][t]), t
        env2.step(clipped, obs, rew, done, extra)
        assert torch.equal(obs, rec["obs_raw"][t]), t
    assert np.array_equal(env2.get_state(), env.get_state())


def test_sweep_agrees_with_the_host_driven_loop():
    """the four steady_2s RaiSim conditions with delays 0-3 (mu 0.8, 5 m/s, 1000 warm-up + 1000 recorded frames) once through
    evaluate.robustness_sweep and once through parity_lib.closed_loop_log_conditions on HipVecEnv, same GPU.  The two loops differ by f32 against
    f64 actor arithmetic and diverge chaotically, so statistics are compared, under the project's own RAISIM_LOG_TOL (the RaiSim logs' repeat
    scatter).  Margin, from the f64 oracle with N(0, 2e-5) noise on the actions, three seeds: v_x moved <= 8.3e-4 relative (bound 2 %), z <= 1.2e-4 m
    (4 mm), pitch <= 1.7e-4 rad (0.004); delays 4-5 moved up to 1.6 % and are left out."""
    from hip_env import HipVecEnv
    with open(os.path.join(GOLDEN, "raisim_body_logs.json")) as f:
        conds, _ = PL.raisim_log_conditions(json.load(f)["logs"])
    conds = sorted([c for c in conds if c["family"] == "steady_2s" and c["delay"] <= 3 and c["mu"] == 0.8], key=lambda c: c["delay"])
    assert [c["delay"] for c in conds] == [0, 1, 2, 3] and all(c["cmd"] == 5.0 and c["warm"] == 1000 and c["frames"] == 1000 for c in conds)
    cfg = _cfg(4)
    rows = EV.robustness_sweep(ACTOR, cfg, [0.8], [0, 1, 2, 3], [5.0], warm_steps=1000, steps=1000)
    recs, falls = PL.closed_loop_log_conditions(HipVecEnv(cfg), cfg, conds)
    host = [EV.body_statistics(r) for r in recs]
    print("\ndevice evaluator (evaluate.robustness_sweep):\n" + EV.sweep_table(rows))
    print("host-driven loop (closed_loop_log_conditions on HipVecEnv):\n" + EV.sweep_table(
        [dict(mu=c["mu"], delay=c["delay"], cmd=c["cmd"], falls=int(f), **{k: v for k, v in h.items() if k != "vx_body"}) for c, f, h in zip(conds, falls, host)]))
    tol = PL.RAISIM_LOG_TOL
    for r, h, f in zip(rows, host, falls):
        assert r["falls"] == 0 and int(f) == 0 and r["frames"] == 1000
        assert abs(r["vx_body_mean"] - h["vx_body_mean"]) / abs(h["vx_body_mean"]) < tol["vx_rel"], (r["delay"], r["vx_body_mean"], h["vx_body_mean"])
        assert abs(r["z_mean"] - h["z_mean"]) < tol["z_abs"], (r["delay"], r["z_mean"], h["z_mean"])
        assert abs(r["pitch_mean"] - h["pitch_mean"]) < tol["pitch_mean_abs"], (r["delay"], r["pitch_mean"], h["pitch_mean"])
