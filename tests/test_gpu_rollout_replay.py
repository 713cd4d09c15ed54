"""The seam between a device rollout and the update, on an MI355X: a real rollout of ppo2.Runner on the HIP engine, then everything it recorded
recomputed in float64 from the recorded observations alone (tests/rollout_replay_lib.py; tests/test_rollout_replay_reference.py checks that
library against the eager runner on the CPU oracle).  The checks themselves are written once, in tests/rollout_checks_lib.py, for this module and
tests/test_gpu_rollout_ragged.py.

Pool: default_cfg.yaml, 40 robots (two full 16-robot workgroups and a ragged one), EnvIdOffset 1000, 24 steps, two consecutive run() calls per
case -- the second starts at rng_base 24 with the carried LSTM state and done flags.  Chosen robots are thrown over the 0.65 m termination
bound so that their episodes end in rows 1, 2, 5, 11, 17, 23 of `masks` and after the last step (`last_dones`), on robots of all three
workgroups; a case whose recorded flags are not exactly the designed ones fails.

Cases: CustomLSTMPolicy in the default mode (one persistent actor-only launch + `_critic_pass`) and step by step (one policy launch + one env
launch per step from Python); MlpPolicy in the default persistent mode and step by step.  One case per policy has logstd spread over [-1, 0.5].
The other rollout modes -- "direct", "one_launch", "persistent" with the critic in the loop, the workgroup-wide actor, hipGraph replay -- are tied
to these bit for bit by test_graph_capture_warmup_leaves_no_trace_and_setters_invalidate_the_graph and
test_mlp_rollout_modes_give_the_same_rollouts_bit_for_bit (tests/test_gpu_ppo.py) and are not run again here.

Per rollout: (2) the exploration noise z = (action - mean64) / exp(logstd) of EVERY row, env and slot against the Philox / Box-Muller reference
at (noise_seed, env + env_id_offset, row + rng_base), within 2e-3; (3) recorded neglogp and values against the float64 replay in the metric and
bounds of lstm_forms_lib.step_errors / STEP_TOL, a tensor over its bound held to 4 x the error of the float32 eager replay of the same batch;
(4) the state and done flags handed to the bootstrap call and its value, likewise; (5) returns and advantages against float64 GAE of the recorded
rewards / values / masks and the float64 bootstrap, within 2e-5 (1 + max |returns|); (6) the same replay with `masks` one row early must miss by
100 x those bounds on every robot whose episode ended (values for the recurrent policy; returns for both -- MlpPolicy uses masks nowhere else).
`clipped` is checked nowhere here: the rewards follow it, and the mode-equality tests cover them.

Then update(batch, 0.0, 0.2) on the recorded batch of the second rollout with the rollout's weights: every parameter bit-identical afterwards,
clipfrac exactly 0, pg / vf / entropy as rollout_replay_lib.expected_stats within (10 tol, tol) for tol = the arithmetic's bound (f32, bf16x6: 2e-5,
i.e. ppo_loss_lib.STATS_RTOL / STATS_ATOL; bf16x3: 1e-4), approxkl <= (d_old + d_new)^2 / 2.

None of these bounds was fitted to a GPU run.  Measured on an MI355X, worst of the two rollouts (every case realised exactly the designed ends):
  lstm default    sampler 1.5e-06  value 1.0e-07  neglogp 8.9e-08  last value 3.2e-07  state (actor | critic) 1.1e-07 | 1.3e-07  returns 2.7e-07
  lstm stepwise   sampler 1.5e-06  value 8.9e-08  neglogp 1.1e-07  last value 2.4e-07  state 8.8e-08 | 9.3e-08  returns 2.8e-07
  mlp default     sampler 1.3e-06  value 2.1e-07  neglogp 9.0e-08  last value 1.9e-07  returns 3.4e-07
  mlp stepwise    sampler 1.4e-06  value 2.5e-07  neglogp 7.5e-08  last value 2.0e-07  returns 3.2e-07
  masks one row early: returns >= 8.6e-02 on every ended robot (bound x 4300); LSTM values, largest over the ended robots, >= 1.7e-02 (bound x 850;
  least single robot 1.3e-03)
  lr-0 update, LSTM: evaluate against float64 (neglogp, value) f32 8.1e-08, 9.6e-07; bf16x6 8.3e-08, 7.9e-07; bf16x3 1.4e-07, 6.1e-06;
  max |ratio - 1| 1.9e-06 / 1.9e-06 / 5.7e-06; approxkl 4.3e-13 / 4.2e-13 / 6.7e-13 (bounds 1.2e-11 / 1.2e-11 / 2.2e-11); |pg| 9.5e-08
  lr-0 update, MlpPolicy: approxkl 5.3e-13 (f32), 3.0e-11 (bf16x3), the same with and without records and for 1 and 4 minibatches; |pg| <= 6.3e-08;
  vf and entropy equal float64 to the 7 digits printed, clipfrac 0, in all 11 update cases.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import ppo_loss_lib as PL
import rollout_checks_lib as K
import rollout_replay_lib as R
from conftest import load_env_cfg

# (policy, mode, logstd range)
CASES = [("lstm", "default", None), ("lstm", "stepwise", (-1.0, 0.5)), ("mlp", "default", (-1.0, 0.5)), ("mlp", "stepwise", None)]
_cache = {}


def _case(kind, mode, logstd_range):
    """-> model, runner, [(batch, last, rng_base)]: two consecutive device rollouts under the scenario (made once, never changed afterwards)"""
    key = (kind, mode)
    if key in _cache:
        return _cache[key]
    import yaml
    import high_speed_quadrupedal_locomotion_by_irrl_amd as pkg
    from high_speed_quadrupedal_locomotion_by_irrl_amd import lstm_fused
    from high_speed_quadrupedal_locomotion_by_irrl_amd.flexible_robot import FlexibleGymEnv
    from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import CustomLSTMPolicy, MlpPolicy
    from high_speed_quadrupedal_locomotion_by_irrl_amd.ppo2 import PPO2, Runner
    from high_speed_quadrupedal_locomotion_by_irrl_amd.vec_env import TorchVecEnv
    cfg = load_env_cfg("default_cfg.yaml", num_envs=R.N_ENVS, EnvIdOffset=R.ENV_ID_OFFSET)
    env = TorchVecEnv(FlexibleGymEnv(pkg.__BLACKPANTHER_V55_RESOURCE_DIRECTORY__, yaml.safe_dump(cfg)))
    lstm = kind == "lstm"
    model = PPO2(policy=CustomLSTMPolicy if lstm else MlpPolicy, env=env, n_steps=R.T_STEPS, nminibatches=1, noptepochs=2, gamma=R.GAMMA, lam=R.LAM, seed=3)
    assert model.env_id_offset == R.ENV_ID_OFFSET and next(model.policy.parameters()).is_cuda
    R.perturb_(model.policy, 11, logstd_range)
    runner = Runner(env, model, R.T_STEPS, R.GAMMA, R.LAM, use_graph=False if mode == "stepwise" else None)
    # conditions: the exploration noise of every training run, and the mode the case is about
    assert runner.noise_source == "kernel" and runner._fused and runner.rollout_launch == "direct"
    if mode == "stepwise":
        runner.rollout_launch = "graph"                 # with use_graph off: one Python call per launch (`_fused_step`)
    else:
        assert runner.rollout_one_launch_per_step == 3 and lstm_fused.MLP_ROLLOUT == "persistent"
        assert runner._actor_only_supported() == lstm
    rollouts = R.collect(runner, R.PLAN, cfg["control_dt"])
    assert runner._graph is None and not runner._fallback_noted and runner.noise_all is None
    assert [b for _, _, b in rollouts] == [0, R.T_STEPS] and int(runner.rng_base) == 2 * R.T_STEPS
    _cache[key] = (model, runner, rollouts)
    return _cache[key]


@pytest.mark.parametrize("kind,mode,logstd_range", CASES, ids=["%s-%s" % c[:2] for c in CASES])
def test_device_rollout_is_what_a_float64_replay_of_its_observations_gives(kind, mode, logstd_range):
    model, runner, rollouts = _case(kind, mode, logstd_range)
    plan, T = R.PLAN, R.T_STEPS
    # the designed ends are the ones this test is about (rollout_checks_lib.check_replay asserts that they are exactly the realised ones)
    rows = set(plan.values())
    assert len(rows) >= 4 and {1, T - 1, T} <= rows and any(i >= 32 for i in plan) and len({i // 16 for i in plan}) == 3
    assert rollouts[0][0]["masks"].shape[1] == R.N_ENVS
    K.check_replay(model, rollouts, plan, (kind, mode), logstd_range)


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16x6"])
def test_zero_learning_rate_update_of_the_lstm_policy_sees_ratio_one(prec, monkeypatch):
    from high_speed_quadrupedal_locomotion_by_irrl_amd import lstm_fused
    model, runner, rollouts = _case(*CASES[0])
    batch, last, _ = rollouts[1]
    monkeypatch.setattr(lstm_fused, "PRECISION", prec)
    K.lstm_zero_lr_check(model, batch, last, prec)


@pytest.mark.parametrize("nminibatches", [1, 4])
@pytest.mark.parametrize("prec,records", [("f32", False), ("f32", True), ("bf16x3", False), ("bf16x3", True)])
def test_zero_learning_rate_update_of_the_mlp_policy_sees_ratio_one(prec, records, nminibatches, monkeypatch):
    from high_speed_quadrupedal_locomotion_by_irrl_amd import ppo2 as P2
    model, runner, rollouts = _case(*CASES[2])
    batch, last, _ = rollouts[1]
    monkeypatch.setattr(P2, "MLP_PRECISION", prec)
    monkeypatch.setattr(P2, "MLP_RECORDS", records)
    monkeypatch.setattr(model, "nminibatches", nminibatches)
    assert model.fused_mlp and P2.mlp_ppo_grads_supported(model.policy, batch["obs"].reshape(-1, 35))
    rep = R.replay(model.policy, batch, last)
    shuffles = model._shuffles
    print("\n[lr-0 update, mlp, %s, records %s, %d minibatches]" % (prec, records, nminibatches), end=" ")
    K.zero_lr_update(model, batch, last, rep, PL.BOUNDS[prec])
    assert model._shuffles - shuffles == model.noptepochs
