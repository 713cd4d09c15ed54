"""The persistent multi-step and rollout kernels for pools whose solver settings are read at RUN TIME (kernel variants "md" and "dir"): a config
without the build-defined Contact* keys (the reference's own YAMLs), ContactSolver 1 / 2, another sweep cap, a tolerance of zero, a control step
of other than eight substeps.  Such pools used to fall back to one launch per step (two per rollout step) silently; now they run the single
launch, bit-identical to the per-step kernel of the same rule, and the pool says which kernels it runs (kernel_variant / kernel_name /
persistent_supported).  Pools that still fall back (Crutial; 4-lane pools for the rollout kernels) say so too."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import load_env_cfg
from rollout_checks_lib import assert_actor_only_equals as _assert_actor_only_equals

CONTACT_KEYS = ("ContactSolver", "ContactExit", "ContactTolerance", "ContactIterations")
LAYOUTS = {"l16": ("16", "1", "_l16"), "l4": ("4", "1", "_l4"), "l4w2": ("4", "2", "_l4w2")}    # IRRL_LANES_PER_ROBOT, IRRL_L4_WAVES, kernel suffix


def _cfg(kind, n):
    """the issue's five run-time-solver configurations -> (environment mapping, variant the pool must report)"""
    if kind == "no_contact_keys":        # what a user of the reference's unmodified YAML passes: ContactTolerance defaults to 0.0
        cfg = load_env_cfg("default_cfg.yaml", num_envs=n)
        return {k: v for k, v in cfg.items() if k not in CONTACT_KEYS}, "md"
    if kind == "terrain_tol0":
        return load_env_cfg("bp5_terrain.yaml", num_envs=n, ContactTolerance=0.0), "md"
    over, variant = {"solver1": ({"ContactSolver": 1}, "md"), "iters5": ({"ContactIterations": 5}, "md"), "solver2": ({"ContactSolver": 2}, "dir")}[kind]
    return load_env_cfg("default_cfg.yaml", num_envs=n, **over), variant


def _layout(monkeypatch, layout):
    lanes, waves, suffix = LAYOUTS[layout]
    monkeypatch.setenv("IRRL_LANES_PER_ROBOT", lanes)
    monkeypatch.setenv("IRRL_L4_WAVES", waves)
    return int(lanes), int(waves), suffix


def _torch_env(cfg):
    import yaml
    import high_speed_quadrupedal_locomotion_by_irrl_amd as pkg
    from high_speed_quadrupedal_locomotion_by_irrl_amd.flexible_robot import FlexibleGymEnv
    from high_speed_quadrupedal_locomotion_by_irrl_amd.vec_env import TorchVecEnv
    return TorchVecEnv(FlexibleGymEnv(pkg.__BLACKPANTHER_V55_RESOURCE_DIRECTORY__, yaml.safe_dump(cfg, default_flow_style=False, width=float("inf"))))


def _outs(lead, n):
    return (torch.full(lead + (n, 35), float("nan"), device="cuda"), torch.full(lead + (n,), float("nan"), device="cuda"),
            torch.zeros(lead + (n,), dtype=torch.bool, device="cuda"), torch.full(lead + (n, 6), float("nan"), device="cuda"))


def _steps_one_by_one(env, table, first, K):
    """K step() calls -> the [K, N, .] rows they returned"""
    n = env.n
    one, want = _outs((), n), _outs((K,), n)
    for k in range(K):
        env.impl.step(table[(first + k) % table.shape[0]], *one)
        for w, o in zip(want, one):
            w[k].copy_(o)
    return want


@pytest.mark.parametrize("layout", ["l16", "l4", "l4w2"])
@pytest.mark.parametrize("kind", ["no_contact_keys", "solver1", "iters5", "solver2", "terrain_tol0"])
def test_run_time_solver_pools_run_the_multi_step_kernel_bit_for_bit(monkeypatch, kind, layout):
    """N = 90 (the last wave and, with several waves per workgroup, the last workgroup ragged in every layout), K = 120 steps from an action
    table of 32 rows that wraps, five robots below the termination height first (in-step resets at step 0): the pool reports the single launch,
    names a multi-step kernel of its layout, and the rows and the final state equal those of K step() calls."""
    from hip_env import HipVecEnv
    lanes, waves, suffix = _layout(monkeypatch, layout)
    n, K, rows = 90, 120, 32
    cfg, variant = _cfg(kind, n)
    a, b = HipVecEnv(cfg), HipVecEnv(cfg)
    assert a.impl.lanes_per_robot == lanes and a.impl.waves_per_simd == waves
    assert a.impl.kernel_variant == variant
    assert a.impl.persistent_supported == 1
    name = a.impl.kernel_name(1)
    assert "steps_persistent" in name and name.endswith(suffix), name
    assert name == "irrl_steps_persistent_kernel_%s%s" % ("rt" if variant == "md" else "dir", suffix)
    assert a.impl.kernel_name(0) == "irrl_step_kernel_%s%s" % (variant, suffix) and a.impl.kernel_name(2) == ""
    g = torch.Generator(device="cuda").manual_seed(9)
    table = (0.6 * torch.randn(rows, n, 12, device="cuda", generator=g)).clamp(-1, 1)
    for env in (a, b):
        st = env.get_state()
        st[:5, 2] = 0.1
        env.set_state(st)
    pers = _outs((K,), n)
    a.impl.step_rows(K, table, 5, *pers, persistent=True)
    want = _steps_one_by_one(b, table, 5, K)
    torch.cuda.synchronize()
    for what, p, w in zip(("ob", "reward", "done", "extraInfo"), pers, want):
        assert torch.equal(p, w), "persistent launch: %s rows differ from K step() calls" % what
    assert want[2][0, :5].all(), "the forced terminations of step 0 are missing from row 0"
    np.testing.assert_array_equal(a.get_state(), b.get_state())


def test_time_step_setter_moves_a_pool_to_the_run_time_kernels_and_keeps_the_single_launch():
    from hip_env import HipVecEnv
    n, K, rows = 90, 60, 16
    cfg = load_env_cfg("default_cfg.yaml", num_envs=n)
    a, b = HipVecEnv(cfg), HipVecEnv(cfg)
    assert a.impl.kernel_variant == "shipped_flat" and a.impl.persistent_supported == 1
    assert a.impl.kernel_name(1) == "irrl_steps_persistent_kernel_flat_l16"
    for env in (a, b):
        env.impl.setControlTimeStep(0.001)        # 4 substeps of 0.25 ms: not the count compiled into the shipped kernels
    assert a.impl.kernel_variant == "md" and a.impl.persistent_supported == 1
    assert a.impl.kernel_name(1) == "irrl_steps_persistent_kernel_rt_l16" and a.impl.kernel_name(0) == "irrl_step_kernel_md_l16"
    g = torch.Generator(device="cuda").manual_seed(3)
    table = (0.6 * torch.randn(rows, n, 12, device="cuda", generator=g)).clamp(-1, 1)
    pers = _outs((K,), n)
    a.impl.step_rows(K, table, 0, *pers, persistent=True)
    want = _steps_one_by_one(b, table, 0, K)
    torch.cuda.synchronize()
    for what, p, w in zip(("ob", "reward", "done", "extraInfo"), pers, want):
        assert torch.equal(p, w), what
    np.testing.assert_array_equal(a.get_state(), b.get_state())


def _three_rollouts(runner, env):
    b1 = {k: v.clone() for k, v in runner.run().items() if torch.is_tensor(v)}
    env.wrapper.setSeed(77)                       # new noise / command streams from the next reset on
    b2 = {k: v.clone() for k, v in runner.run().items() if torch.is_tensor(v)}
    b3 = {k: v.clone() for k, v in runner.run().items() if torch.is_tensor(v)}
    return b1, b2, b3


@pytest.mark.parametrize("kind,modes", [("no_contact_keys", ("direct", "one_launch", "persistent", "persistent_actor", "persistent_actor_wg")),
                                        ("terrain_tol0", ("persistent", "persistent_actor"))])
def test_lstm_rollout_modes_on_a_run_time_solver_pool(monkeypatch, kind, modes):
    """64 envs, 20 steps, three rollouts with a reseed behind the first: every way to issue the LSTM rollout gives the eager runner's buffers --
    bit for bit, but for the actor-only modes' values / returns / critic state (the sequence kernels' f32 level) -- and the pool HAS the combined
    kernels: irrl_lstm_rollout_supports says 1 for fuse 1, 2 and 3."""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib
    from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import CustomLSTMPolicy
    from high_speed_quadrupedal_locomotion_by_irrl_amd.ppo2 import PPO2, Runner
    lib = _lib.load()
    cfg, variant = _cfg(kind, 64)
    out = {}
    for mode in ("eager",) + tuple(modes):
        monkeypatch.delenv("IRRL_ACTOR_WAVES", raising=False)
        if mode == "persistent_actor_wg":
            monkeypatch.setenv("IRRL_ACTOR_WAVES", "0")
        env = _torch_env(cfg)
        assert env.wrapper.lanes_per_robot == 16 and env.wrapper.kernel_variant == variant
        assert [lib.irrl_lstm_rollout_supports(env.wrapper._h, 48, f) for f in (0, 1, 2, 3)] == [1, 1, 1, 1]
        model = PPO2(policy=CustomLSTMPolicy, env=env, n_steps=20, nminibatches=1, noptepochs=1, seed=9)
        runner = Runner(env, model, 20, 0.99, 0.998, use_graph=False)
        assert runner.rollout_launch == "direct"
        runner.rollout_launch = "graph" if mode == "eager" else "direct"      # "graph" without a graph: one Python call per launch
        runner.rollout_one_launch_per_step = {"one_launch": 1, "persistent": 2, "persistent_actor": 3, "persistent_actor_wg": 3}.get(mode, 0)
        out[mode] = _three_rollouts(runner, env)
        assert runner._actor_only_supported()
    monkeypatch.delenv("IRRL_ACTOR_WAVES", raising=False)
    assert not torch.equal(out["eager"][1]["obs"], out["eager"][0]["obs"])
    for mode in modes:
        for i in range(3):
            if mode.startswith("persistent_actor"):
                _assert_actor_only_equals(out[mode][i], out["eager"][i], (mode, i))
            else:
                for k in ("obs", "actions", "values", "true_reward", "masks", "neglogpacs", "returns", "states"):
                    assert torch.equal(out[mode][i][k], out["eager"][i][k]), (mode, i, k)


def test_runner_asks_again_after_a_time_step_setter():
    """the answer of `Runner._actor_only_supported()` depends on the substep count: a runner that ran on a default pool keeps working after
    setControlTimeStep moved the pool to the run-time-solver kernels, and its rollout is the eager runner's over the same sequence"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import CustomLSTMPolicy
    from high_speed_quadrupedal_locomotion_by_irrl_amd.ppo2 import PPO2, Runner
    cfg = load_env_cfg("default_cfg.yaml", num_envs=64)
    out = {}
    for mode in ("default", "eager"):
        env = _torch_env(cfg)
        assert env.wrapper.lanes_per_robot == 16 and env.wrapper.kernel_variant == "shipped_flat"
        model = PPO2(policy=CustomLSTMPolicy, env=env, n_steps=20, nminibatches=1, noptepochs=1, seed=4)
        runner = Runner(env, model, 20, 0.99, 0.998, use_graph=False)
        if mode == "eager":
            runner.rollout_launch = "graph"
        else:
            assert runner.rollout_launch == "direct" and runner.rollout_one_launch_per_step == 3
        b1 = {k: v.clone() for k, v in runner.run().items() if torch.is_tensor(v)}
        env.wrapper.setControlTimeStep(0.001)
        assert env.wrapper.kernel_variant == "md"
        b2 = {k: v.clone() for k, v in runner.run().items() if torch.is_tensor(v)}      # (a RuntimeError here: a stale capability answer)
        out[mode] = (b1, b2)
        assert mode == "eager" or runner._actor_only_supported()
    for i in range(2):
        _assert_actor_only_equals(out["default"][i], out["eager"][i], i)


def test_mlp_rollout_modes_on_a_run_time_solver_pool(monkeypatch):
    """96 envs, 40 steps, ContactIterations 5: the persistent MlpPolicy rollout exists for the pool and equals the two-launch and the eager forms"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib, lstm_fused
    from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import MlpPolicy
    from high_speed_quadrupedal_locomotion_by_irrl_amd.ppo2 import PPO2, Runner
    lib = _lib.load()
    cfg, variant = _cfg("iters5", 96)
    out = {}
    for mode in ("persistent", "direct", "eager"):
        monkeypatch.setattr(lstm_fused, "MLP_ROLLOUT", "direct" if mode == "direct" else "persistent")
        env = _torch_env(cfg)
        assert env.wrapper.kernel_variant == variant
        assert lib.irrl_mlp_rollout_supports(env.wrapper._h, 64, 2) == 1 and lib.irrl_mlp_rollout_supports(env.wrapper._h, 64, 0) == 1
        assert lib.irrl_mlp_rollout_supports(env.wrapper._h, 48, 2) == 0 and lib.irrl_mlp_rollout_supports(env.wrapper._h, 64, 3) == 0
        model = PPO2(policy=MlpPolicy, env=env, n_steps=40, nminibatches=1, noptepochs=1, seed=9)
        runner = Runner(env, model, 40, 0.99, 0.998, use_graph=False)
        assert runner.rollout_launch == "direct"
        runner.rollout_launch = "graph" if mode == "eager" else "direct"
        out[mode] = _three_rollouts(runner, env)
    for mode in ("persistent", "direct"):
        for i in range(3):
            for k in ("obs", "actions", "values", "true_reward", "masks", "neglogpacs", "returns"):
                assert torch.equal(out[mode][i][k], out["eager"][i][k]), (mode, i, k)


def test_pools_that_still_fall_back_say_so(monkeypatch, capsys):
    from hip_env import HipVecEnv
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib
    from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import CustomLSTMPolicy
    from high_speed_quadrupedal_locomotion_by_irrl_amd.ppo2 import PPO2, Runner
    lib = _lib.load()
    cr = HipVecEnv(load_env_cfg("default_cfg.yaml", num_envs=64, Crutial=True))
    assert cr.impl.kernel_variant == "crutial_md" and cr.impl.persistent_supported == 0
    assert cr.impl.kernel_name(1) == cr.impl.kernel_name(0) == "irrl_step_kernel_crutial_md_l16"
    assert [lib.irrl_lstm_rollout_supports(cr.impl._h, 48, f) for f in (0, 1, 2, 3)] == [1, 0, 0, 0]
    assert lib.irrl_mlp_rollout_supports(cr.impl._h, 64, 2) == 0
    # the runner says once, and only once, why such a pool's rollout is two launches per step; a pool with the kernels prints nothing
    for over, lines in (({"Crutial": True}, 1), ({}, 0)):
        env = _torch_env(load_env_cfg("default_cfg.yaml", num_envs=64, **over))
        model = PPO2(policy=CustomLSTMPolicy, env=env, n_steps=6, nminibatches=1, noptepochs=1, seed=2)
        runner = Runner(env, model, 6, 0.99, 0.998, use_graph=False)
        capsys.readouterr()
        runner.run()
        runner.run()
        notes = [l for l in capsys.readouterr().out.splitlines() if l.startswith("[PPO2] rollout runs as two launches per step")]
        assert len(notes) == lines, notes
        assert not notes or ("crutial_md" in notes[0] and "Crutial" in notes[0])
    monkeypatch.setenv("IRRL_LANES_PER_ROBOT", "4")
    env4 = HipVecEnv(_cfg("no_contact_keys", 64)[0])
    assert env4.impl.lanes_per_robot == 4 and env4.impl.kernel_variant == "md"
    assert env4.impl.persistent_supported == 1 and env4.impl.kernel_name(1) == "irrl_steps_persistent_kernel_rt_l4"
    assert lib.irrl_lstm_rollout_supports(env4.impl._h, 48, 3) == 0 and lib.irrl_lstm_rollout_supports(env4.impl._h, 48, 0) == 1
    assert lib.irrl_mlp_rollout_supports(env4.impl._h, 64, 2) == 0


def _fallback_notes(capsys):
    return [l for l in capsys.readouterr().out.splitlines() if l.startswith("[PPO2] rollout runs as two launches per step")]


@pytest.mark.parametrize("policy,lanes,over,variant,reason", [
    ("lstm", "16", {"ContactSolver": 2}, "dir", "ContactSolver 0 / 2"), ("mlp", "16", {"ContactSolver": 0}, "dir", "ContactSolver 0 / 2"),
    ("lstm", "4", {}, "shipped_flat", "16-lane layout only (this pool: 4 lanes per robot)"), ("mlp", "4", {"ContactTolerance": 0.0}, "md", "16-lane layout only"),
    ("mlp", "16", {"Crutial": True}, "crutial_md", "Crutial")])
def test_the_runner_names_variant_and_reason_once_where_a_pool_has_no_rollout_kernel(monkeypatch, capsys, policy, lanes, over, variant, reason):
    """every reason the note can give (first per-contact rule, 4-lane layout, the meteorite), for both policies: one line at the first run(), none later"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import CustomLSTMPolicy, MlpPolicy
    from high_speed_quadrupedal_locomotion_by_irrl_amd.ppo2 import PPO2, Runner
    monkeypatch.setenv("IRRL_LANES_PER_ROBOT", lanes)
    env = _torch_env(load_env_cfg("default_cfg.yaml", num_envs=64, **over))
    assert env.wrapper.lanes_per_robot == int(lanes) and env.wrapper.kernel_variant == variant
    model = PPO2(policy=CustomLSTMPolicy if policy == "lstm" else MlpPolicy, env=env, n_steps=6, nminibatches=1, noptepochs=1, seed=2)
    runner = Runner(env, model, 6, 0.99, 0.998, use_graph=False)
    assert runner.rollout_launch == "direct"
    capsys.readouterr()
    runner.run()
    notes = _fallback_notes(capsys)
    assert len(notes) == 1 and ("'%s'" % variant) in notes[0] and reason in notes[0], notes
    runner.run()
    assert _fallback_notes(capsys) == []


def test_the_note_waits_for_the_first_run_that_asks_for_a_persistent_rollout(capsys):
    """a run() in a mode that asks for two launches per step anyway says nothing and uses nothing up: the line comes with the first run() whose
    persistent rollout the pool cannot give, once"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import CustomLSTMPolicy
    from high_speed_quadrupedal_locomotion_by_irrl_amd.ppo2 import PPO2, Runner
    env = _torch_env(load_env_cfg("default_cfg.yaml", num_envs=64, Crutial=True))
    model = PPO2(policy=CustomLSTMPolicy, env=env, n_steps=6, nminibatches=1, noptepochs=1, seed=2)
    runner = Runner(env, model, 6, 0.99, 0.998, use_graph=False)
    runner.rollout_one_launch_per_step = 0
    capsys.readouterr()
    runner.run()
    assert _fallback_notes(capsys) == []
    runner.rollout_one_launch_per_step = 3
    runner.run()
    assert len(_fallback_notes(capsys)) == 1
    runner.run()
    assert _fallback_notes(capsys) == []
