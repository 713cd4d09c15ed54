"""The persistent single-launch form of the device evaluation loop (PolicyEvaluator.run(persistent=True) -> irrl_lstm_eval_rollout_persistent, kernel
csrc/env_eval_kernels.hpp) on the MI355X: BIT IDENTITY with the five-launch form (persistent=False, tests/test_gpu_eval_rollout.py holds that one
to numpy, the policy-step kernel and a replaying pool).  Two identical pools are built the way that file builds its scene, one per form.

The shared scenario: bp5_manual_eval.yaml with N = 19 envs (ragged against the 16-robot workgroup AND the 4-robot wave), the bp5_155 actor (hid 48),
D = 6 with delays e % 6, commands 0.5 .. 5 m/s, frictions 0.05 .. 0.8, command / rate / action low-passes at 1 / 50 / 30 Hz, T = 60 steps issued as
20 + 40 (the second call starts at ring slot 2), the base of envs 3 and 17 put at 0.14 m between the calls (they terminate at step 20: the reset
path inside the step loop), all eight recorders and the statistics on."""
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

from conftest import GOLDEN, load_env_cfg
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV

N, D, T, T1 = 19, 6, 60, 20
FALLERS = [3, 17]
HZ = dict(cmd_hz=1.0, vel_hz=50.0, act_hz=30.0)
ALL = tuple(EV.RECORDERS)
ACTOR = os.path.join(GOLDEN, "actor_bp5_155.npz")      # the reference's trained bp5_155 actor
HID = 48
# the blocks of the work array both forms write (the persistent form leaves `value` alone), as include/irrl_env.h lays them out one behind the
# other: name -> (offset, width) in units of N floats
WORK = dict(obs_cond=(0, 35), action=(35, 12), clipped=(47, 12), applied=(59, 12), reward=(73, 1), extra=(74, 6))


def _work(ev, name):
    c, w = WORK[name]
    return ev.work.view(-1)[ev.n * c:ev.n * (c + w)]


def _pool(n, **over):
    import high_speed_quadrupedal_locomotion_by_irrl_amd as pkg
    from high_speed_quadrupedal_locomotion_by_irrl_amd.flexible_robot import FlexibleGymEnv
    cfg = load_env_cfg("bp5_manual_eval.yaml", num_envs=n, **over)
    env = FlexibleGymEnv(pkg.__BLACKPANTHER_V55_RESOURCE_DIRECTORY__, yaml.safe_dump(cfg, default_flow_style=False, width=float("inf")))
    env.init()
    env.SetContactCoefficient(EV.contact_material(np.linspace(0.05, 0.8, n)))
    return env


def _evaluator(pol, n, over=None, depth=D, **kw):
    env = _pool(n, **(over or {}))
    return EV.PolicyEvaluator(env, pol, np.arange(n) % depth, np.linspace(0.5, 5.0, n), depth=depth, **kw)


def _drop(env):
    st = env.get_state()
    st[FALLERS, 2] = 0.14
    env.set_state(st)


def _cat(parts):
    return {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}


def _effort(env, n):
    effort = np.zeros((n, 12), np.float32)
    env.GetJointEffort(effort)
    return effort


def _assert_same_buffers(a, b, n, full_state=False):
    """everything the two forms promise to leave identical: evaluator state, the actor's half of the LSTM state (c0, h0, c1, h1 of SD = 8 HID),
    the work columns both write, the pool"""
    torch.cuda.synchronize()
    for k in ("stats", "ring", "cmd", "vel_his", "act_his", "done", "obs"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.lstm_state[:, :4 * HID], b.lstm_state[:, :4 * HID])
    if full_state:
        assert torch.equal(a.lstm_state, b.lstm_state)
    for k in WORK:
        assert torch.equal(_work(a, k), _work(b, k)), k
    assert a.t == b.t
    assert np.array_equal(a.env.get_state(), b.env.get_state())
    assert np.array_equal(_effort(a.env, n), _effort(b.env, n))


def _assert_same_records(ra, rb):
    assert sorted(ra) == sorted(rb)
    for k in ra:
        assert ra[k].shape == rb[k].shape and torch.equal(ra[k], rb[k]), k


@pytest.fixture(scope="module")
def policy():
    return EV.load_policy(ACTOR, torch.device("cuda"))


def _scenario(pol, persistent, over=None):
    ev = _evaluator(pol, N, over, **HZ)
    first = ev.run(T1, record=ALL, persistent=persistent)
    _drop(ev.env)
    rec = _cat([first, ev.run(T - T1, record=ALL, persistent=persistent)])
    return ev, rec


@pytest.mark.parametrize("over, variant", [({}, "shipped_flat"), ({"ContactExit": 0}, "md")])
def test_the_scenario_in_both_forms_is_bit_identical(policy, over, variant):
    """test 1 (the shipped solver settings: irrl_eval_persistent_kernel_l16) and test 2 (ContactExit: 0, variant `md`: its run-time-solver twin
    _rt_l16): every recorder, stats, ring, cmd, vel_his, act_his, done, obs, the actor's half of lstm_state, the six work column groups,
    get_state and GetJointEffort; and the two dropped envs, and only they, are done at row 20"""
    a, ra = _scenario(policy, True, over)
    b, rb = _scenario(policy, False, over)
    assert a.env.kernel_variant == variant and a.persistent_supported and b.persistent_supported
    done = ra["done"].cpu().numpy()
    assert done.shape == (T, N) and sorted(np.flatnonzero(done[T1])) == FALLERS and int(done.sum()) == 2
    _assert_same_records(ra, rb)
    _assert_same_buffers(a, b, N)
    assert torch.equal(a.stats[EV.STAT_SLOTS.index("n")], torch.full((N,), float(T), dtype=torch.float64, device=a.stats.device))


def test_filters_off_no_delay_unclipped_mean(policy):
    """test 3: every filter off (coefficients exactly 1), depth 1, clip=False (the unclipped mean is applied), no recorders, no statistics, 30
    steps: final buffers and pool equal; with the obs_raw recorder alone, its rows equal"""
    kw = dict(depth=1, cmd_hz=None, vel_hz=None, act_hz=None, clip=False)
    a, b = _evaluator(policy, N, **kw), _evaluator(policy, N, **kw)
    assert a.depth == 1 and a.a_cmd == a.a_vel == a.a_act == 1.0
    assert a.run(30, accumulate=False, persistent=True) == {} and b.run(30, accumulate=False, persistent=False) == {}
    _assert_same_buffers(a, b, N)
    assert float(a.stats.abs().sum()) == 0.0
    assert torch.equal(_work(a, "action"), _work(a, "applied"))     # the mean, before the clip, was applied as it is
    print("largest |mean action| of the last step: %.3f (beyond 1: the clip would have acted)" % float(_work(a, "action").abs().max()))
    ra, rb = a.run(7, record=("obs_raw",), accumulate=False, persistent=True), b.run(7, record=("obs_raw",), accumulate=False, persistent=False)
    _assert_same_records(ra, rb)
    _assert_same_buffers(a, b, N)


@pytest.mark.parametrize("n", [1, 16])
def test_single_step_zero_step_and_resume(policy, n):
    """test 4: N = 1 and N = 16, 12 steps with all recorders issued as 1 + 0 + 11: a single-step launch, a call that launches nothing, a resume"""
    a, b = _evaluator(policy, n, **HZ), _evaluator(policy, n, **HZ)
    ra = [a.run(s, record=ALL, persistent=True) for s in (1, 0, 11)]
    rb = [b.run(s, record=ALL, persistent=False) for s in (1, 0, 11)]
    assert all(v.shape[0] == 0 for v in ra[1].values()) and a.t == 12
    _assert_same_records(_cat(ra), _cat(rb))
    _assert_same_buffers(a, b, n)


def test_the_two_forms_may_follow_each_other(policy):
    """test 5: 20 steps persistent, 20 five-launch, 20 persistent on one evaluator == 60 five-launch steps on the other (the persistent form
    leaves the critic's half of the LSTM state alone and the actor never reads it): recorders, statistics, the actor's half of the state"""
    a, b = _evaluator(policy, N, **HZ), _evaluator(policy, N, **HZ)
    ra = _cat([a.run(20, record=ALL, persistent=p) for p in (True, False, True)])
    rb = b.run(60, record=ALL, persistent=False)
    _assert_same_records(ra, rb)
    _assert_same_buffers(a, b, N)


def test_capability_and_refusals(policy):
    """test 6: no persistent kernel for a Crutial pool, a ContactSolver 0 pool (variant `dir`) or a (32, 32) policy: `persistent_supported` is
    False, persistent=True raises with the condition named, persistent="auto" runs and equals persistent=False"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import CustomLSTMPolicy
    torch.manual_seed(5)
    small = CustomLSTMPolicy(n_lstm=(32, 32)).to(torch.device("cuda"))
    small.prepare()
    n = 6
    for over, pol, word in (({"Crutial": True}, policy, "crutial"), ({"ContactSolver": 0}, policy, "dir"), ({}, small, "hid 48")):
        a, b = _evaluator(pol, n, over, **HZ), _evaluator(pol, n, over, **HZ)
        assert a.persistent_supported is False
        with pytest.raises(RuntimeError, match=word):
            a.run(3, persistent=True)
        assert a.t == 0
        ra, rb = a.run(8, record=ALL, persistent="auto"), b.run(8, record=ALL, persistent=False)
        _assert_same_records(ra, rb)
        assert torch.equal(a.lstm_state, b.lstm_state)                   # "auto" took the five-launch form: the critic's half too
        torch.cuda.synchronize()
        assert torch.equal(a.stats, b.stats) and np.array_equal(a.env.get_state(), b.env.get_state())
    ok = _evaluator(policy, n, **HZ)
    assert ok.persistent_supported is True
    assert set(ok.run(2, record=("body",), persistent="auto")) == {"body"}
