"""The kernel source (csrc/env_core.hpp, through the host lane emulation, both lane layouts) against the f64 oracle in the regions
that random actions from a fresh reset never reach -- long episode clocks, the rim of the height field, the sloped and crossed parts
of the motor's torque-speed envelope, the z > 0.65 m and tilt terminations, and the contact regimes: the caps of the per-contact
rules (frictionless, jamming corner) mixed with ordinary robots in one wave, slides at 3-6 m/s, landings that bounce, and the gait
generator's regimes (legs beyond reach, failing IK slots chained across legs, lateral commands with lean), where the task state the step
leaves for the next one is compared too.  Scenario hooks
and their witnesses: parity_lib.py ("Edge scenarios"); the same scenarios through the C-ABI on an MI355X: test_gpu_parity_edges.py.  Tolerances: the unchanged TOL_STEP,
TERRAIN_MAX_FACTOR on rough ground, and the derived 4 f32 ulps on base x / y where robots are moved to x = +-250 m."""
import numpy as np
import pytest

import oracle as O
import parity_lib as PL
from conftest import load_env_cfg
from host_emulation import emu as E

EMUS = [E.EmuVecEnv, E.EmuVecEnv16]
STEPS = 40
# The supported horizon of an episode: 25 000 control steps (50 s, 2.5 times the longest RaiSim recording).  The episode clock
# t0 + frame * control_dt is f32 in the kernels; its rounding reaches the observation through the gait phase, and the error grows
# linearly with the frame (it meets the 5e-4 observation tolerance near 100 000 frames: DESIGN.md section 5).
HORIZON_FRAMES = 25000
CLOCK_CFGS = {"eval": ("bp5_manual_eval.yaml", {}), "eval_time_based_contact": ("bp5_manual_eval.yaml", {"TimeBasedContact": True}),
              "train": ("default_cfg.yaml", {})}


def clock_case(make_cand, cfg_key, frame0, n=8, **over):
    name, extra = CLOCK_CFGS[cfg_key]
    cfg = load_env_cfg(name, num_envs=n, **dict(extra, **over))
    orc, cand = O.OracleVecEnv(cfg), make_cand(cfg)
    hook = PL.long_clock(orc, frame0)
    worst, n_done = PL.check_teacher_forced(orc, cand, steps=STEPS, seed=1, perturb=hook)
    hook.witness()
    return worst


def field_edge_case(make_cand, axis, n=8, **over):
    cfg = load_env_cfg("bp5_terrain.yaml", num_envs=n, **over)
    orc, cand = O.OracleVecEnv(cfg), make_cand(cfg)
    hook = PL.field_edge(orc, axis)
    worst, n_done = PL.check_teacher_forced(orc, cand, steps=STEPS, seed=2, perturb=hook, max_factor=PL.TERRAIN_MAX_FACTOR,
                                            pos_xy_ulps=0 if axis == "y" else 4)
    hook.witness()
    return worst


def motor_envelope_case(make_cand, n=12, crossed=False, **over):
    cfg = load_env_cfg("bp5_manual_eval.yaml", num_envs=n, **over)
    assert (cfg["MotorCriticalSpeed"], cfg["MotorMaxSpeed"]) == (14.2, 40)
    orc, cand = O.OracleVecEnv(cfg), make_cand(cfg)
    hook = PL.motor_envelope(orc, cand, cfg["MotorCriticalSpeed"], cfg["MotorMaxSpeed"], crossed=crossed)
    worst, n_done = PL.check_teacher_forced(orc, cand, steps=STEPS, seed=3, action_scale=1.0, perturb=hook, after_step=hook.after_step)
    hook.witness(n_done)
    assert worst["threshold_events"] == 0           # airborne: there is no threshold to straddle
    return worst


def terminations_case(make_cand, n=13, **over):
    cfg = load_env_cfg("bp5_imitation.yaml", num_envs=n, **over)      # (no observation noise: ENV:1560 tests the NOISY observation's tilt entry)
    orc, cand = O.OracleVecEnv(cfg), make_cand(cfg)
    hook = PL.other_terminations()
    worst, n_done = PL.check_teacher_forced(orc, cand, steps=STEPS, seed=4, perturb=hook, after_step=hook.after_step)
    hook.witness()
    assert n_done >= STEPS // 2
    return worst


def friction_caps_case(make_cand, n=16, terrain=False, **over):
    cfg = load_env_cfg("bp5_terrain.yaml" if terrain else "bp5_imitation.yaml", num_envs=n, **over)
    orc, cand = O.OracleVecEnv(cfg), make_cand(cfg)
    hook = PL.friction_caps(orc, cfg, first_rule=not (cfg["ContactSolver"] & 1))
    worst, n_done = PL.check_teacher_forced(orc, cand, steps=STEPS, seed=5, perturb=hook, after_step=hook.after_step,
                                            max_factor=PL.TERRAIN_MAX_FACTOR if terrain else 10.0)
    hook.witness()
    return worst


def fast_slide_case(make_cand, n=16, terrain=False, **over):
    cfg = load_env_cfg("bp5_terrain.yaml" if terrain else "bp5_imitation.yaml", num_envs=n, **over)
    orc, cand = O.OracleVecEnv(cfg), make_cand(cfg)
    hook = PL.fast_slide(orc, cfg)
    worst, n_done = PL.check_teacher_forced(orc, cand, steps=STEPS, seed=6, perturb=hook, after_step=hook.after_step,
                                            max_factor=PL.TERRAIN_MAX_FACTOR if terrain else 10.0)
    hook.witness()
    return worst


def bouncing_landings_case(make_cand, n=16, **over):
    cfg = load_env_cfg("bp5_imitation.yaml", num_envs=n, **over)
    orc, cand = O.OracleVecEnv(cfg), make_cand(cfg)
    hook = PL.bouncing_landings(orc, cfg)
    worst, n_done = PL.check_teacher_forced(orc, cand, steps=STEPS, seed=7, perturb=hook, after_step=hook.after_step)
    hook.witness()
    return worst


# ---- the gait generator's regimes (parity_lib.py "The task state"): n = 16, 40 steps, a forced reset every third step so that the
# reset's two-pass call -- temp[] carried from the pass at t - control_dt into the pass at t -- is in every case ----
GAIT_REACH_CFGS = {"Vx7.5": {"Vx": 7.5}, "period0.3": {"period": 0.3}}
# GaitType -> (stand_height, lean front and hind, the chain length its witness asks for)
LOW_STANCE_CFGS = {0: (0.11, 0.03, 2), 1: (0.12, 0.025, 2), 2: (0.115, 0.03, 1), 3: (0.11, 0.025, 4)}
GAIT_LATERAL_CFG = dict(Vy=1.0, LeanFront=0.03, LeanHind=-0.02, HeightVariable=True, WILDCAT=False, Manual=False)


def gait_reach_cfg(key, wildcat, n, **over):
    return load_env_cfg("default_cfg.yaml", num_envs=n, **dict(GAIT_REACH_CFGS[key], WILDCAT=wildcat, **over))


def gait_low_stance_cfg(gait_type, n, **over):
    stand, lean, _ = LOW_STANCE_CFGS[gait_type]
    return load_env_cfg("default_cfg.yaml", num_envs=n, **dict(dict(stand_height=stand, LeanFront=lean, LeanHind=lean, GaitType=gait_type), **over))


def _gait_case(make_cand, cfg, hook_of, seed, name):
    orc, cand = O.OracleVecEnv(cfg), make_cand(cfg)
    hook = hook_of(orc, cand, cfg)
    try:
        worst, n_done = PL.check_teacher_forced(orc, cand, steps=STEPS, seed=seed, force_terminal_every=3, perturb=hook, after_step=hook.after_step)
    finally:
        if hook.task.env_steps:
            hook.task.report(name)
    hook.witness()
    assert n_done >= STEPS // 3
    return hook


def gait_reach_case(make_cand, key, wildcat, n=16, assert_bounds=True, **over):
    cfg = gait_reach_cfg(key, wildcat, n, **over)
    return _gait_case(make_cand, cfg, lambda o, c, g: PL.gait_reach(o, c, g, assert_bounds), 8, "gait_reach %s WILDCAT %s" % (key, wildcat))


def gait_low_stance_case(make_cand, gait_type, n=16, assert_bounds=True, **over):
    cfg = gait_low_stance_cfg(gait_type, n, **over)
    return _gait_case(make_cand, cfg, lambda o, c, g: PL.gait_low_stance(o, c, g, LOW_STANCE_CFGS[gait_type][2], assert_bounds), 9,
                      "gait_low_stance GaitType %d" % gait_type)


def gait_lateral_case(make_cand, n=16, assert_bounds=True, **over):
    cfg = load_env_cfg("default_cfg.yaml", num_envs=n, **dict(GAIT_LATERAL_CFG, **over))
    return _gait_case(make_cand, cfg, lambda o, c, g: PL.gait_lateral(o, c, g, assert_bounds), 10, "gait_lateral")


CONTACT_SCENARIOS = {"friction_caps": PL.friction_caps, "fast_slide": PL.fast_slide, "bouncing_landings": PL.bouncing_landings}
GAIT_SCENARIOS = ("gait_lateral", "gait_low_stance", "gait_reach")


def edge_state(scenario, n):
    """-> (config, the f32-rounded state of an oracle pool after the scenario's step-0 perturbation): where the multi-step tests start"""
    if scenario in GAIT_SCENARIOS:
        if scenario == "gait_reach":
            cfg = gait_reach_cfg("Vx7.5", True, n)
            hook = PL.gait_reach(None, None, cfg)
        elif scenario == "gait_low_stance":
            cfg = gait_low_stance_cfg(3, n)
            hook = PL.gait_low_stance(None, None, cfg, 4)
        else:
            cfg = load_env_cfg("default_cfg.yaml", num_envs=n, **GAIT_LATERAL_CFG)
            hook = PL.gait_lateral(None, None, cfg)
        orc = O.OracleVecEnv(cfg)
        return cfg, PL.f32_round_state(hook(PL.f32_round_state(orc.get_state()), 0, None))
    if scenario in CONTACT_SCENARIOS:
        cfg = load_env_cfg("bp5_imitation.yaml", num_envs=n)
        orc = O.OracleVecEnv(cfg)
        hook = CONTACT_SCENARIOS[scenario](orc, cfg)
        return cfg, PL.f32_round_state(hook(PL.f32_round_state(orc.get_state()), 0, np.random.RandomState(0)))
    if scenario == "clock":
        cfg = load_env_cfg("default_cfg.yaml", num_envs=n)
        orc = O.OracleVecEnv(cfg)
        hook = PL.long_clock(orc, HORIZON_FRAMES - 10)            # 16 steps from here cross the horizon
    elif scenario == "corner":
        cfg = load_env_cfg("bp5_terrain.yaml", num_envs=n)
        orc = O.OracleVecEnv(cfg)
        hook = PL.field_edge(orc, "corner")
    else:
        cfg = load_env_cfg("bp5_manual_eval.yaml", num_envs=n)
        orc = O.OracleVecEnv(cfg)
        hook = PL.motor_envelope(orc, None, cfg["MotorCriticalSpeed"], cfg["MotorMaxSpeed"])
    return cfg, PL.f32_round_state(hook(PL.f32_round_state(orc.get_state()), 0, None))


@pytest.mark.parametrize("emu", EMUS)
@pytest.mark.parametrize("frame0", [6390, 10000, HORIZON_FRAMES])        # 6390: two_pi_over_period * t passes 2^8 pi / 2 inside the 40 steps
@pytest.mark.parametrize("cfg_key", sorted(CLOCK_CFGS))
def test_long_episode_clock(emu, frame0, cfg_key):
    clock_case(emu, cfg_key, frame0)


@pytest.mark.parametrize("emu", EMUS)
@pytest.mark.parametrize("axis", ["y", "x", "corner"])
def test_rim_of_the_height_field(emu, axis):
    field_edge_case(emu, axis)


@pytest.mark.parametrize("emu", EMUS)
@pytest.mark.parametrize("crossed", [False, True], ids=["to_1.3_w_max", "crossed"])
def test_motor_envelope_slopes_and_crossed_bounds(emu, crossed):
    motor_envelope_case(emu, crossed=crossed)


@pytest.mark.parametrize("emu", EMUS)
def test_height_and_tilt_terminations(emu):
    terminations_case(emu)


@pytest.mark.parametrize("emu", EMUS)
@pytest.mark.parametrize("solver", [3, 1, 2, 0])
def test_friction_caps_frictionless_ordinary_and_jammed_robots_side_by_side(emu, solver):
    """ContactSolver 3 / 1: the published rule in both sweep orders (jamming cap, frictionless path, the wave-level skips around them);
    2 / 0: the first rule and its own cap."""
    friction_caps_case(emu, ContactSolver=solver)


@pytest.mark.parametrize("emu", EMUS)
def test_friction_caps_on_rough_ground(emu):
    friction_caps_case(emu, terrain=True)


@pytest.mark.parametrize("emu", EMUS)
@pytest.mark.parametrize("terrain", [False, True], ids=["flat", "rough"])
def test_fast_slide(emu, terrain):
    fast_slide_case(emu, terrain=terrain)


@pytest.mark.parametrize("emu", EMUS)
@pytest.mark.parametrize("solver", [3, 2])
def test_bouncing_landings(emu, solver):
    bouncing_landings_case(emu, ContactSolver=solver)


@pytest.mark.parametrize("emu", EMUS)
@pytest.mark.parametrize("wildcat", [True, False], ids=["wildcat", "forward"])
@pytest.mark.parametrize("key", sorted(GAIT_REACH_CFGS))
def test_gait_reach_legs_beyond_max_len(emu, key, wildcat):
    """Targets beyond reach are rescaled to max_len - 1e-5: JR and JDR there are held to the same bound as in reach.  Before the
    constants of the straight leg (csrc/env_core.hpp IRRL_IK_REACH_*) the kernel source missed it several times over: JR 4.6e-5 to
    6.6e-5 rad against a bound near 8e-6 there, from acos at 1 - 3.5e-5 in f32 (the oracle's own f32 build: 5.7e-5 rad); now 6.4e-7 rad."""
    gait_reach_case(emu, key, wildcat)


@pytest.mark.parametrize("emu", EMUS)
@pytest.mark.parametrize("gait_type", sorted(LOW_STANCE_CFGS))
def test_gait_low_stance_failing_slots_inherit_the_previous_leg(emu, gait_type):
    gait_low_stance_case(emu, gait_type)


@pytest.mark.parametrize("emu", EMUS)
def test_gait_lateral_commands_lean_and_variable_swing_height(emu):
    gait_lateral_case(emu)


@pytest.mark.parametrize("scenario", ["clock", "corner", "motor"] + sorted(CONTACT_SCENARIOS) + sorted(GAIT_SCENARIOS))
def test_carried_lane_context_equals_store_and_load_from_edge_states(scenario):
    """The host counterpart of test_multi_step_kernel_equals_one_launch_per_step_from_edge_states (test_gpu_parity_edges.py): 16 steps with
    the lane context carried in registers (sub-lanes 1-3 poisoned behind every step) == 16 step() calls, from frame 24 990, from over the
    corner of the height field, from joint rates beyond the motor's no-load speed and from the step-0 states of the three contact
    scenarios (mixed friction, 3-6 m/s slides, landings) -- every step's outputs and the final pool, bit for bit."""
    n, K = (16 if scenario in CONTACT_SCENARIOS or scenario in GAIT_SCENARIOS else 12), 16
    cfg, st = edge_state(scenario, n)
    a, b = E.EmuVecEnv16(cfg), E.EmuVecEnv16(cfg)
    a.set_state(st)
    b.set_state(st)
    rng = np.random.RandomState(8)
    acts = np.stack([PL.random_actions(rng, n, 0.5) for _ in range(K)])
    got = a.steps_carried(acts, poison=True)
    want = [b.step(acts[k]) for k in range(K)]
    for j, name in enumerate(("ob", "reward", "done", "extraInfo")):
        assert np.array_equal(np.stack([w[j] for w in want]), got[j], equal_nan=True), name
    np.testing.assert_array_equal(a.get_state(), b.get_state())


def test_base_xy_allowance_is_off_by_default_and_scales_only_x_and_y():
    """pos_xy_ulps: with the default 0 a base 5.8e-5 m off at x = 250 m (4 f32 ulps there are 6.1e-5 m) fails the position check as before;
    with 4 it passes under 2e-5 + 6.1e-5 m; the same offset on z (entry 2) fails either way."""
    cfg = load_env_cfg("bp5_imitation.yaml", num_envs=4)

    class Shifted(O.OracleVecEnv):
        entry, shift = 0, 5.8e-5

        def get_state(self):
            st = O.OracleVecEnv.get_state(self)
            st[:, self.entry] += self.shift
            return st

    def far_out(st, k, rng):
        st[:, 0] = 250.0
        return st

    for entry, ulps, passes in ((0, 0, False), (0, 4, True), (2, 4, False)):
        orc, cand = O.OracleVecEnv(cfg), Shifted(cfg)
        cand.entry = entry
        try:
            PL.check_teacher_forced(orc, cand, steps=3, perturb=far_out, pos_xy_ulps=ulps)
            ok = True
        except AssertionError:
            ok = False
        assert ok == passes, (entry, ulps)
    assert 4 * np.spacing(np.float32(250.0)) == pytest.approx(6.1e-5, rel=0.01)
