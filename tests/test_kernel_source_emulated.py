"""CPU-side checks of the KERNEL SOURCE (csrc/env_core.hpp) through the host lane emulation
(tests/host_emulation): the same Schur-complement dynamics, quad reductions and masked reset the GPU
runs, compared with the f64 oracle.  The real parity tests (HIP through the C-ABI) are in
test_gpu_parity.py and need an MI355X; these run in the build container."""
import numpy as np
import pytest

import oracle as O
import parity_lib as PL
from conftest import load_env_cfg
from host_emulation import emu as E


# the shipped kernels use 16 lanes per robot (lanes_hip16.hpp); the 4-lanes-per-robot layout of the same source
# (lanes_hip.hpp) is kept as a second instantiation and checked on the core cases
EMU = E.EmuVecEnv16


def _pair(cfg, emu=None):
    return O.OracleVecEnv(cfg), (emu or EMU)(cfg)


@pytest.mark.parametrize("emu", [E.EmuVecEnv, E.EmuVecEnv16])
def test_both_lane_layouts_match_oracle(emu):
    orc, cand = _pair(load_env_cfg("default_cfg.yaml", num_envs=8), emu)
    PL.check_init(orc, cand)
    PL.check_teacher_forced(orc, cand, steps=60, force_terminal_every=7)
    orc, cand = _pair(load_env_cfg("bp5_terrain.yaml", num_envs=4), emu)
    PL.check_teacher_forced(orc, cand, steps=40, force_terminal_every=9, max_factor=PL.TERRAIN_MAX_FACTOR)


@pytest.mark.parametrize("emu", [E.EmuVecEnv, E.EmuVecEnv16])
def test_trunk_box_corners_collide_like_the_oracle(emu):
    """ENV:242 / URDF:26: the trunk's collision box.  Robots tilted onto a bottom corner at 0.15-0.17 m: the corner contacts of
    the kernel source (both lane layouts) against the oracle's, teacher-forced; the oracle's statistic proves corners did touch."""
    orc, cand = _pair(load_env_cfg("bp5_imitation.yaml", num_envs=8), emu)
    h0 = orc.box_hits()
    worst, n_done = PL.check_teacher_forced(orc, cand, steps=40, seed=3, perturb=PL.tilt_onto_box_corner, max_factor=PL.CORNER_MAX_FACTOR, cap_factor=PL.CORNER_CAP_FACTOR)
    assert orc.box_hits() - h0 > 8 * 40 * 4          # on average more than half a corner-substep pair per env-substep
    assert n_done < 8 * 40 // 4                      # most steps stay inside the episode: the physics is what is compared
    # rough ground brings corners down at small tilts too
    orc, cand = _pair(load_env_cfg("bp5_terrain.yaml", num_envs=4), emu)
    PL.check_teacher_forced(orc, cand, steps=30, seed=5, perturb=lambda st, k, rng: PL.tilt_onto_box_corner(st, k, rng, 0.16, 0.30, 20.0, 55.0),
                            max_factor=PL.TERRAIN_MAX_FACTOR)


@pytest.mark.parametrize("emu", [E.EmuVecEnv, E.EmuVecEnv16])
def test_crutial_meteorite_matches_the_oracle(emu):
    """Crutial: True (ENV:273-284, 731-740, 815-861): the schedule (parked at reset and every 5 periods, released a step later)
    free-running from init, then teacher-forced steps with a sphere dropped onto the trunk / the ground before every step."""
    cfg = load_env_cfg("bp5_imitation.yaml", num_envs=24, Crutial=True, CubeNum=6, period=0.05)   # K = 125 control steps
    orc, cand = _pair(cfg, emu)                    # (24 envs x 40 steps: the 0.5 % event budget is 4 env-steps, not 1)
    k = PL.S["SPHERE"]
    assert np.abs(orc.get_state()[:, k:k + 9] - cand.get_state()[:, k:k + 9]).max() < 1e-6
    st = orc.get_state()
    st[:, PL.S["FRAME"]] = 110
    orc.set_state(st)
    PL.check_teacher_forced(orc, cand, steps=30, seed=2, force_terminal_every=11)       # crosses frame 125: park + release
    s = orc.get_state()
    assert (s[:, k + 8] == 1).any() and orc.sphere_hits() == 0
    h0 = orc.sphere_hits()
    worst, n_done = PL.check_teacher_forced(orc, cand, steps=40, seed=4, perturb=PL.drop_meteorite, max_factor=PL.CORNER_MAX_FACTOR, cap_factor=PL.CORNER_CAP_FACTOR)
    assert orc.sphere_hits() - h0 > 120                                                 # the spheres did hit trunks (1-2 substeps of contact per impact)
    # rough ground under the sphere
    orc, cand = _pair(load_env_cfg("bp5_terrain.yaml", num_envs=3, Crutial=True, CubeNum=2), emu)
    PL.check_teacher_forced(orc, cand, steps=24, seed=6, perturb=PL.drop_meteorite, max_factor=PL.TERRAIN_MAX_FACTOR)


@pytest.mark.parametrize("emu", [E.EmuVecEnv, E.EmuVecEnv16])
def test_gauss_seidel_contact_order_is_still_available(emu):
    """ContactSolver: 0 (sequential Gauss-Seidel over FR, FL, HR, HL, then the box corners) -- the default is 2 (simultaneous
    updates); both orders exist in the oracle and in the kernel source and agree with each other pairwise."""
    orc, cand = _pair(load_env_cfg("default_cfg.yaml", num_envs=8, ContactSolver=0), emu)
    PL.check_teacher_forced(orc, cand, steps=60, force_terminal_every=7)
    orc, cand = _pair(load_env_cfg("bp5_imitation.yaml", num_envs=8, ContactSolver=0), emu)
    PL.check_teacher_forced(orc, cand, steps=30, seed=3, perturb=PL.tilt_onto_box_corner, max_factor=PL.CORNER_MAX_FACTOR, cap_factor=PL.CORNER_CAP_FACTOR)


@pytest.mark.parametrize("solver", [1, 3])
@pytest.mark.parametrize("emu", [E.EmuVecEnv, E.EmuVecEnv16])
def test_published_contact_rule_kernel_source_matches_the_oracle(emu, solver):
    """ContactSolver 1 (the published method: Gauss-Seidel + the exact maximum-dissipation single-contact solve of RaiSim's solver,
    Hwangbo et al. 2018) and 3 (same rule, simultaneous sweeps): kernel source (solve_contact_md in csrc/env_core.hpp) against the
    oracle's solve_contact_md, both lane layouts -- training config with noise / randomised friction / resets, robots tilted onto
    a trunk-box corner (the corners use the same rule), rough ground, the meteorite."""
    orc, cand = _pair(load_env_cfg("default_cfg.yaml", num_envs=8, ContactSolver=solver), emu)
    PL.check_init(orc, cand)
    PL.check_teacher_forced(orc, cand, steps=60, force_terminal_every=7)
    orc, cand = _pair(load_env_cfg("bp5_imitation.yaml", num_envs=8, ContactSolver=solver), emu)
    h0 = orc.box_hits()
    PL.check_teacher_forced(orc, cand, steps=30, seed=3, perturb=PL.tilt_onto_box_corner, max_factor=PL.CORNER_MAX_FACTOR, cap_factor=PL.CORNER_CAP_FACTOR)
    assert orc.box_hits() - h0 > 8 * 30 * 4
    orc, cand = _pair(load_env_cfg("bp5_terrain.yaml", num_envs=4, ContactSolver=solver), emu)
    PL.check_teacher_forced(orc, cand, steps=40, force_terminal_every=9, max_factor=PL.TERRAIN_MAX_FACTOR)
    orc, cand = _pair(load_env_cfg("bp5_imitation.yaml", num_envs=6, Crutial=True, CubeNum=6, period=0.05, ContactSolver=solver), emu)
    h0 = orc.sphere_hits()
    PL.check_teacher_forced(orc, cand, steps=30, seed=4, perturb=PL.drop_meteorite, max_factor=PL.CORNER_MAX_FACTOR, cap_factor=PL.CORNER_CAP_FACTOR)
    assert orc.sphere_hits() - h0 > 20


def test_init_matches_oracle_train_cfg():
    PL.check_init(*_pair(load_env_cfg("default_cfg.yaml", num_envs=24)))


def test_init_matches_oracle_imitation_cfg():
    PL.check_init(*_pair(load_env_cfg("bp5_imitation.yaml", num_envs=8)))


def test_dynamics_probe_matches_oracle():
    orc, cand = _pair(load_env_cfg("default_cfg.yaml", num_envs=12))
    rng = np.random.RandomState(0)
    for _ in range(5):
        a = PL.random_actions(rng, 12)
        orc.step(a)
    cand.set_state(PL.f32_round_state(orc.get_state()))
    orc.set_state(PL.f32_round_state(orc.get_state()))
    PL.check_probe(orc, cand)


def test_teacher_forced_train_cfg_with_noise_randomisation_and_resets():
    cfg = load_env_cfg("default_cfg.yaml", num_envs=8)
    orc, cand = _pair(cfg)
    task = PL.task_state_check(orc, cand, cfg)        # what the step's closing task logic leaves for the NEXT step
    worst, n_done = PL.check_teacher_forced(orc, cand, steps=120, force_terminal_every=7, after_step=task.after_step)
    task.report("train config")
    assert n_done >= 10  # the masked in-step reset path was exercised


def test_teacher_forced_eval_style_cfg():
    cfg = load_env_cfg("bp5_imitation.yaml", num_envs=4, GaitType=0, WILDCAT=False, HeightVariable=True,
                       MotorCriticalSpeed=14.2, MotorMaxSpeed=40, stand_height=0.30, ObsFilter=True, Filter=True,
                       TimeBasedContact=True, ActionNoise=0.1, SharedNoiseScalar=False)
    orc, cand = _pair(cfg)
    task = PL.task_state_check(orc, cand, cfg)
    PL.check_teacher_forced(orc, cand, steps=60, seed=2, force_terminal_every=9, after_step=task.after_step)
    task.report("eval-style config")


def test_free_running_horizons():
    cfg = load_env_cfg("bp5_imitation.yaml", num_envs=8)
    PL.check_free_running(O.OracleVecEnv, EMU, cfg)


def test_invariants_small():
    cand = EMU(load_env_cfg("default_cfg.yaml", num_envs=16))
    PL.check_invariants(cand, steps=30)


def test_config_parser_matches_pyyaml():
    import yaml
    cfg = load_env_cfg("default_cfg.yaml")
    text = yaml.safe_dump(cfg)
    cand = EMU(dict(cfg, num_envs=2))
    assert cand.n == 2
    # missing mandatory key -> error naming the key (reference: RSFATAL "Node ... doesn't exist")
    bad = dict(cfg)
    del bad["Stiffness"]
    with pytest.raises(RuntimeError, match="Stiffness"):
        E.EmuVecEnv(bad)
    assert EMU(dict(cfg, num_envs=2, Crutial=True)).n == 2         # the meteorite pool builds (test_crutial_meteorite_matches_the_oracle)
    assert "seedd" in text


def test_terrain_heightfield_and_teacher_forced_parity():
    """Terrain: True (Environment.hpp:254-264).  The product's generator (csrc/irrl_terrain.hpp) and the oracle's
    independent restatement must produce the same table; stepping on it must agree like on the plane."""
    cfg = load_env_cfg("default_cfg.yaml", num_envs=8, Terrain=True)
    orc, cand = _pair(cfg)
    Ho, Hc = orc.heightfield(), cand.heightfield()
    assert Ho.shape == (5000, 500) and np.abs(Ho - Hc).max() < 1e-7
    assert 0.02 < np.abs(Ho).max() < 0.2 and abs(float(Ho.mean())) < 0.02          # zScale 0.1 relief
    h, nx, ny, nz = orc.terrain_sample(1.234, -3.21)
    assert abs(nx * nx + ny * ny + nz * nz - 1) < 1e-12 and nz > 0.7
    # the bilinear field has a different normal in every cell: a toe within rounding distance of a cell edge lands in
    # the neighbouring cell in one precision (a discontinuity like the contact threshold), so only the 99th percentile
    # is held to the stated tolerance here
    worst, n_done = PL.check_teacher_forced(orc, cand, steps=140, force_terminal_every=11, max_factor=PL.TERRAIN_MAX_FACTOR)
    # the robots really stand on the relief: toes rest at the local terrain height, not at z = 0
    import _np_robot as R
    st = orc.get_state()
    toes = R.toe_positions(st[0, :19])
    hs = np.array([orc.terrain_sample(t[0], t[1])[0] for t in toes])
    assert np.all(toes[:, 2] - 0.0275 - hs > -5e-3)


@pytest.mark.parametrize("cand", [E.EmuVecEnv, E.EmuVecEnv16])
def test_reference_trajectory_mode(cand):
    """ManualTraj: False: command, joint reference and phase come from row frame_idx of the table, episodes
    start at a random frame; oracle and kernel source agree teacher-forced, and the observation really shows the table."""
    tab = PL.ref_table()
    cfg = load_env_cfg("default_cfg.yaml", num_envs=16, ManualTraj=False, max_time=0.4)
    cfg["_ref_table"] = tab
    orc, c = O.OracleVecEnv(cfg), cand(cfg)
    PL.check_init(orc, c)
    st = orc.get_state()
    frames = st[:, PL.S["FRAME"]].astype(int)
    span = 900 // 2 - int(0.4 / 0.002) - 10
    assert frames.min() >= 1 and frames.max() <= span and len(set(frames.tolist())) > 4   # random start frames (ENV:571), +1 after reset
    ob = orc.observe()
    mean, std = O.obs_scaling(cfg)
    raw = ob * std + mean
    # obs[0:3] = cmd columns, obs[3:5] = phase columns of the row the reset's command update used (frame - 1 ... ) / observed
    for i in range(16):
        f = frames[i] - 1                                   # the observation was built before frame_idx++ (ENV:624-630)
        assert np.abs(raw[i, 3:5] - tab[f, 25:27]).max() < 1e-5
        assert np.abs(raw[i, 0:3] - tab[f, 27:30]).max() < 1e-5
    PL.check_teacher_forced(orc, c, steps=30, seed=4)


@pytest.mark.parametrize("cand", [E.EmuVecEnv, E.EmuVecEnv16])
def test_manual_eval_mode_with_state_disturbance(cand):
    """The evaluation configuration (Manual: True = bp5_test.yaml: fixed start pose, no command process, t0 = 0) with
    ForceDisturbance: the base state is kicked every 10 gait periods (ENV:912-940); period 0.02 s makes that every 100 steps."""
    cfg = load_env_cfg("default_cfg.yaml", num_envs=6, Manual=True, ForceDisturbance=True, period=0.02, ObsNoise=0.0, ActionNoise=0.0)
    orc, c = O.OracleVecEnv(cfg), cand(cfg)
    PL.check_init(orc, c)
    st0 = orc.get_state()
    assert np.allclose(st0[:, 0:2], 0.0) and np.allclose(st0[:, PL.S["T0"]], 0.0)       # Manual: origin start, t0 = 0
    rng = np.random.RandomState(3)
    K = int(0.02 / 0.002 * 10)          # evaluated in double like ENV:747 (in f32 it would be 99)
    assert K == 100
    plain = O.OracleVecEnv(dict(cfg, ForceDisturbance=False))
    kicked = []
    for k in range(210):
        a = PL.random_actions(rng, 6, 0.1)
        before = orc.get_state()
        plain.set_state(before)
        orc.step(a)
        plain.step(a)
        if np.abs(orc.get_state()[:, 0:37] - plain.get_state()[:, 0:37]).max() > 1e-3:
            kicked.append(int(before[0, PL.S["FRAME"]]))
    assert kicked == [100, 200], kicked
    orc2, c2 = O.OracleVecEnv(cfg), cand(cfg)
    PL.check_teacher_forced(orc2, c2, steps=120, seed=9, action_scale=0.1)


@pytest.mark.parametrize("make", [O.OracleVecEnv, E.EmuVecEnv16])
def test_raisim_trained_policy_trots_at_the_commanded_speed(make):
    """Sim-to-sim: the controller the reference authors trained in RaiSim (bp5_155) runs this build's physics closed loop in
    the reference's evaluation configuration (rsc/bp5_manual_eval.yaml) -- no fall, and the commanded 1.5 m/s is tracked within
    10 % (f64 oracle and the f32 kernel source)."""
    cfg = load_env_cfg("bp5_manual_eval.yaml")
    vx, falls = PL.closed_loop_reference_policy(make(cfg), cfg, 1.5, 700)
    assert falls == 0
    assert abs(vx[350:].mean() - 1.5) < 0.15, vx[350:].mean()


def test_reference_trajectory_csv_reader(tmp_path):
    """csrc/irrl_csv.hpp restates VectorizedEnvironment.hpp:33-76 `readCSV_m`: comma separated, no header, one row per line;
    CRLF line ends, blank lines and short rows (zero padded) are tolerated, a missing file is an error."""
    import ctypes as C
    l = E.lib(16)
    l.emu_read_csv.restype = C.c_int
    l.emu_read_csv.argtypes = [C.c_char_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    tab = PL.ref_table(rows=7)
    path = tmp_path / "a b ref.csv"
    lines = [",".join("%.9g" % v for v in r) for r in tab]
    lines[2] = ",".join(lines[2].split(",")[:25])                    # short row
    path.write_bytes(("\r\n".join(lines[:4]) + "\r\n\r\n" + "\n".join(lines[4:]) + "\n").encode())
    r, c = C.c_int(0), C.c_int(0)
    assert l.emu_read_csv(str(path).encode(), None, C.byref(r), C.byref(c)) == 0 and (r.value, c.value) == (7, 30)
    out = np.zeros((7, 30), np.float32)
    assert l.emu_read_csv(str(path).encode(), out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(r), C.byref(c)) == 0
    want = tab.copy()
    want[2, 25:] = 0.0
    assert np.allclose(out, want, rtol=1e-6, atol=1e-7)
    assert l.emu_read_csv(b"/nonexistent/ref.csv", None, C.byref(r), C.byref(c)) != 0


@pytest.mark.parametrize("make", [O.OracleVecEnv, E.EmuVecEnv16])
def test_policy_trained_on_the_hip_engine_trots_in_the_oracle(make):
    """Policy-level parity of engine and oracle: an actor trained for 2000 PPO updates ON THE MI355X ENGINE (f32 HIP kernels,
    `scripts/run_bp_v5.py --train`, 200 envs; tests/golden/actor_trained_on_hip_engine.npz via tools/export_actor_fixture.py)
    drives the f64 oracle and the emulated kernel source closed loop in Manual mode with its own training config: no fall,
    commanded 1.5 m/s tracked (the training config has WILDCAT: True -> the robot runs in -x)."""
    cfg = load_env_cfg("default_cfg.yaml", num_envs=1, Manual=True, ObsNoise=0.0, ActionNoise=0.0, StochasticDynamics=False)
    vx, falls = PL.closed_loop_reference_policy(make(cfg), cfg, 1.5, 900, fixture="actor_trained_on_hip_engine.npz")
    assert falls == 0
    assert -1.75 < vx[450:].mean() < -1.2, vx[450:].mean()


@pytest.mark.parametrize("width", [4, 16])
@pytest.mark.parametrize("cfg_name,over", [("default_cfg.yaml", {}), ("bp5_terrain.yaml", {}), ("bp5_manual_eval.yaml", {"ObsFilter": True})])
def test_lane_context_carried_in_registers_equals_store_and_load(width, cfg_name, over):
    """Round 5: the multi-step kernels (env_kernels.hip: `irrl_steps_persistent_kernel`, the persistent rollout kernels) keep a robot's lane
    context in registers from one control step to the next -- load_lane once, { step_compute; lane_carry } per step, store_lane once -- instead
    of storing and re-loading it around every step.  The same kernel source on the host: K steps carried == K `step_body` calls (store + load
    every step), EVERY step's outputs and the final pool bit for bit -- with in-step resets, noise, per-episode model randomisation (terrain
    config), the observation filter's history -- and, in the 16-lane layout, with the context of sub-lanes 1-3 POISONED behind every step: on the
    GPU those lanes skip the epilogue, so every word the next step reads must come back from sub-lane 0 (`lane_carry`)."""
    from host_emulation.emu import EmuVecEnv
    n, K = 6, 60
    cfg = load_env_cfg(cfg_name, num_envs=n, **over)
    a, b = EmuVecEnv(cfg, width=width), EmuVecEnv(cfg, width=width)
    rng = np.random.default_rng(7)
    acts = np.clip(0.6 * rng.standard_normal((K, n, 12)), -1, 1).astype(np.float32)
    st = a.get_state()
    st[:2, 2] = 0.1                    # two robots start below the termination height: an in-step reset in the very first step
    a.set_state(st); b.set_state(st)
    want = [a.step(acts[k]) for k in range(K)]
    got = b.steps_carried(acts, poison=(width == 16))
    for j, name in enumerate(("ob", "reward", "done", "extraInfo")):
        w = np.stack([x[j] for x in want])
        assert np.array_equal(w, got[j], equal_nan=True), "%s differs at step %d" % (name, int(np.argwhere(w != got[j])[0][0]))
    assert np.stack([x[2] for x in want]).sum() >= 2
    np.testing.assert_array_equal(a.get_state(), b.get_state())
