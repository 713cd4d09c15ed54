"""The edge scenarios of test_kernel_source_edges_emulated.py through the C-ABI on an MI355X: the HIP kernels against the f64 oracle at
long episode clocks, on the rim of the height field, on the sloped and crossed parts of the motor envelope, at the z > 0.65 m and tilt
terminations, in the contact regimes (friction caps mixed inside one wave, 3-6 m/s slides, bouncing landings) and in the gait generator's
regimes (legs beyond reach, failing IK slots chained across legs and passes, lateral commands with lean) -- both lane layouts, and for the scenarios on flat ground also a ContactSolver 1 pool (the run-time-solver kernels, variant
"md", instead of "shipped_flat").  Then the multi-step kernel's bit-identity with one launch per step, started FROM those states.
Scenario hooks, witnesses and tolerances: parity_lib.py; nothing here is fitted to a GPU run."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import parity_lib as PL
import test_kernel_source_edges_emulated as EDGES

N = 16                                     # one 16-lane wave holds four robots, one 4-lane wave sixteen
POOLS = [(16, {}, "shipped_flat"), (4, {}, "shipped_flat"), (16, {"ContactSolver": 1}, "md"), (4, {"ContactSolver": 1}, "md")]
POOL_IDS = ["l16", "l4", "l16-solver1", "l4-solver1"]


def _hip(cfg):
    from hip_env import HipVecEnv
    return HipVecEnv(cfg)


def _maker(monkeypatch, lanes, variant):
    monkeypatch.setenv("IRRL_LANES_PER_ROBOT", str(lanes))

    def make(cfg):
        env = _hip(cfg)
        assert env.impl.lanes_per_robot == lanes and env.impl.kernel_variant == variant, (env.impl.lanes_per_robot, env.impl.kernel_variant)
        return env
    return make


@pytest.mark.parametrize("lanes,over,variant", POOLS, ids=POOL_IDS)
@pytest.mark.parametrize("frame0", [6390, 10000, EDGES.HORIZON_FRAMES])
@pytest.mark.parametrize("cfg_key", sorted(EDGES.CLOCK_CFGS))
def test_long_episode_clock_on_gpu(monkeypatch, cfg_key, frame0, lanes, over, variant):
    EDGES.clock_case(_maker(monkeypatch, lanes, variant), cfg_key, frame0, n=N, **over)


@pytest.mark.parametrize("lanes", [16, 4])
@pytest.mark.parametrize("axis", ["y", "x", "corner"])
def test_rim_of_the_height_field_on_gpu(monkeypatch, axis, lanes):
    EDGES.field_edge_case(_maker(monkeypatch, lanes, "shipped"), axis, n=N)


@pytest.mark.parametrize("lanes,over,variant", POOLS, ids=POOL_IDS)
@pytest.mark.parametrize("crossed", [False, True], ids=["to_1.3_w_max", "crossed"])
def test_motor_envelope_slopes_and_crossed_bounds_on_gpu(monkeypatch, crossed, lanes, over, variant):
    EDGES.motor_envelope_case(_maker(monkeypatch, lanes, variant), n=12, crossed=crossed, **over)


@pytest.mark.parametrize("lanes,over,variant", POOLS, ids=POOL_IDS)
def test_height_and_tilt_terminations_on_gpu(monkeypatch, lanes, over, variant):
    EDGES.terminations_case(_maker(monkeypatch, lanes, variant), n=13, **over)


@pytest.mark.parametrize("lanes,over,variant", POOLS, ids=POOL_IDS)
def test_friction_caps_on_gpu(monkeypatch, lanes, over, variant):
    """16 envs: one 4-lane wave holds all nine frictions, the 16-lane waves hold four robots each -- envs 4..7 with mu 1.3, 2, 3 and 0."""
    EDGES.friction_caps_case(_maker(monkeypatch, lanes, variant), n=N, **over)


@pytest.mark.parametrize("lanes", [16, 4])
@pytest.mark.parametrize("solver", [2, 0])
def test_friction_caps_first_rule_on_gpu(monkeypatch, solver, lanes):
    EDGES.friction_caps_case(_maker(monkeypatch, lanes, "dir"), n=N, ContactSolver=solver)


@pytest.mark.parametrize("lanes", [16, 4])
def test_friction_caps_on_rough_ground_on_gpu(monkeypatch, lanes):
    EDGES.friction_caps_case(_maker(monkeypatch, lanes, "shipped"), n=N, terrain=True)


@pytest.mark.parametrize("lanes,over,variant", POOLS, ids=POOL_IDS)
def test_fast_slide_on_gpu(monkeypatch, lanes, over, variant):
    EDGES.fast_slide_case(_maker(monkeypatch, lanes, variant), n=N, **over)


@pytest.mark.parametrize("lanes", [16, 4])
def test_fast_slide_on_rough_ground_on_gpu(monkeypatch, lanes):
    EDGES.fast_slide_case(_maker(monkeypatch, lanes, "shipped"), n=N, terrain=True)


@pytest.mark.parametrize("lanes,over,variant", POOLS, ids=POOL_IDS)
def test_bouncing_landings_on_gpu(monkeypatch, lanes, over, variant):
    EDGES.bouncing_landings_case(_maker(monkeypatch, lanes, variant), n=N, **over)


@pytest.mark.parametrize("lanes,over,variant", POOLS, ids=POOL_IDS)
@pytest.mark.parametrize("wildcat", [True, False], ids=["wildcat", "forward"])
@pytest.mark.parametrize("key", sorted(EDGES.GAIT_REACH_CFGS))
def test_gait_reach_on_gpu(monkeypatch, key, wildcat, lanes, over, variant):
    """The task state (JR, JRL, JDR, EER, CMD, CMDF, UPH, T0, CONTACT) behind every step, legs beyond max_len in a quarter of the env-steps."""
    EDGES.gait_reach_case(_maker(monkeypatch, lanes, variant), key, wildcat, n=N, **over)


@pytest.mark.parametrize("lanes,over,variant", POOLS, ids=POOL_IDS)
@pytest.mark.parametrize("gait_type", sorted(EDGES.LOW_STANCE_CFGS))
def test_gait_low_stance_on_gpu(monkeypatch, gait_type, lanes, over, variant):
    """Failing asin / acos slots: the shared temp[3] chain is three legs_bcast hand-offs (DPP) in the kernels."""
    EDGES.gait_low_stance_case(_maker(monkeypatch, lanes, variant), gait_type, n=N, **over)


@pytest.mark.parametrize("lanes,over,variant", POOLS, ids=POOL_IDS)
def test_gait_lateral_on_gpu(monkeypatch, lanes, over, variant):
    EDGES.gait_lateral_case(_maker(monkeypatch, lanes, variant), n=N, **over)


@pytest.mark.parametrize("lanes", [16, 4])
@pytest.mark.parametrize("scenario", ["clock", "corner", "motor"] + sorted(EDGES.CONTACT_SCENARIOS) + sorted(EDGES.GAIT_SCENARIOS))
def test_multi_step_kernel_equals_one_launch_per_step_from_edge_states(monkeypatch, scenario, lanes):
    """No new code runs here: the multi-step kernel's bit-identity with K step() calls (test_gpu_runtime_solver_persistent.py, from fresh
    pools) is started from states that claim has not seen -- frame 24 990, robots over the corner of the height field, joint rates beyond
    the motor's no-load speed, and the step-0 states of the three contact scenarios.  16 steps, every step's outputs and the final pool."""
    import torch
    monkeypatch.setenv("IRRL_LANES_PER_ROBOT", str(lanes))
    n, K = (12 if scenario == "motor" else N), 16
    cfg, st = EDGES.edge_state(scenario, n)
    a, b = _hip(cfg), _hip(cfg)
    assert a.impl.lanes_per_robot == lanes and a.impl.persistent_supported == 1 and "steps_persistent" in a.impl.kernel_name(1)
    a.set_state(st)
    b.set_state(st)
    np.testing.assert_array_equal(a.get_state(), b.get_state())
    if scenario == "clock":
        assert a.get_state()[:, PL.S["FRAME"]].min() == EDGES.HORIZON_FRAMES - 10
    rng = np.random.RandomState(8)
    acts = np.stack([PL.random_actions(rng, n, 0.5) for _ in range(K)])
    table = torch.from_numpy(acts).cuda()
    ob = torch.full((K, n, 35), float("nan"), device="cuda"); rew = torch.full((K, n), float("nan"), device="cuda")
    done = torch.zeros(K, n, dtype=torch.bool, device="cuda"); ext = torch.full((K, n, 6), float("nan"), device="cuda")
    a.impl.step_rows(K, table, 0, ob, rew, done, ext, persistent=True)
    torch.cuda.synchronize()
    want = [b.step(acts[k]) for k in range(K)]
    for j, (name, got) in enumerate((("ob", ob), ("reward", rew), ("done", done), ("extraInfo", ext))):
        w = np.stack([x[j] for x in want])
        assert np.array_equal(w, got.cpu().numpy(), equal_nan=True), "%s rows of the multi-step launch differ from %d step() calls" % (name, K)
    sa = a.get_state()
    np.testing.assert_array_equal(sa, b.get_state())
    print("[multi-step from %s, %d lanes] %d steps bit-identical; frames end at %d .. %d, base |x| up to %.1f m, |y| up to %.1f m"
          % (scenario, lanes, K, sa[:, PL.S["FRAME"]].min(), sa[:, PL.S["FRAME"]].max(), np.abs(sa[:, 0]).max(), np.abs(sa[:, 1]).max()))
