#!/usr/bin/env python3
"""run_bp_v5.py -- train branch of the reference's experiment script (IRRL/script/run_bp_v5.py:196-259) on the
MI355X engine.  Same construction order and hyper-parameters (run_bp_v5.py:227-242); the import block is the
reference's own (run_bp_v5.py:8-13), resolved by the compat packages at the repo root.

    python scripts/run_bp_v5.py --train --max_iter 6144000                 # imitation stage
    python scripts/run_bp_v5.py --train --load data/..._Iteration_100.pkl  # relaxation stage (new reward coeffs in --cfg)
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 scripts/run_bp_v5.py --train   # 8 x 4096 envs, RCCL grads

    python scripts/run_bp_v5.py --test --model data/..._final.pkl --cmd 1.5 --steps 2000   # headless evaluation
    python scripts/run_bp_v5.py --test --sweep --model data/..._final.pkl --sweep_mu 0.05,0.4,0.8 --sweep_delay 0,1,2,3,4,5 --sweep_cmd 1,2,3,4,5 \
        --warm 1000 --steps 2000 --out table.json                                          # robustness grid, device-resident
    python scripts/run_bp_v5.py --test --sweep --model data/..._final.pkl --sweep_mu 0.8,0.1 --sweep_delay 0,1,2,3,4,5 --cmd 5 \
        --perturb z=0.02,roll=0.25,pitch=0.25,z_dot=1,roll_dot=1,pitch_dot=1 --explorations 10000 --perturb_at 1000 --steps 1000 \
        --out explorations.npz                                                             # perturbation exploration, device-resident
    ... --perturb ... --entropy [--entropy_chunk 100]                                      # + entropy, cells, histograms per frame (Figure3/4.py)
    python scripts/run_bp_v5.py --test --sweep --model data/..._final.pkl --sweep_cmd 5 --recurrence [--recurrence_frames 800 --recurrence_radius 10] \
        --out sweep.json                                                                   # + recurrence rate, determinism, longest line and stride
                                                                                           # period per condition; the matrices of the first 8 to --out
    python scripts/run_bp_v5.py --test --sweep --model data/..._final.pkl --sweep_cmd 2,5 --footfall [--motor] --out sweep.json
                                                                                           # + debounced stride frequency, duty, the gait's name
                                                                                           # [+ motor saturation]; gait diagrams and maps to --out
    python scripts/run_bp_v5.py --test --sweep --model data/..._final.pkl --sweep_cmd 2,5 --corr [--corr_x contact --corr_y lstm] --out sweep.json
                                                                                           # + the largest correlation of a foot-contact flag with
                                                                                           # an LSTM unit, its leg and unit; the matrices to --out
    python scripts/run_bp_v5.py --test --sweep --model data/..._final.pkl --sweep_cmd 2,5 --vibration [--vib_nperseg 256 --vib_hop 224 --vib_window tukey \
        --vib_band 50] --out sweep.json                                                    # + the Welch spectrum's peak frequency and the share of
                                                                                           # power above the band for joint angles, joint rates and
                                                                                           # actions; spectra and spectrograms to --out
    python scripts/run_bp_v5.py --test --sweep --step --gait --model data/..._final.pkl --persistent on   # cost of transport, duty factors and
                                                                                           # touchdown rate per (friction, command level)

`--test` keeps the evaluation LOOP of the reference (run_bp_v5.py:353-470: Manual-mode env, externally supplied command in
obs[0:3], observation delay line, velocity / action low-pass filters, numpy LSTM actor, per-step records of joint state,
posture, effort and the true simulator state) with a fixed command (`--cmd`, the reference's `flag_fix_cmd`) instead of
the gamepad, and writes the records to an .npz instead of the ~700 lines of matplotlib analysis (run_bp_v5.py:471-1121),
which stay out of scope.  `--o` (CSV export of the actor) is kept.
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import yaml  # noqa: E402

from flex_gym.env.RaisimGymVecEnv import TorchVecEnv as Environment  # noqa: E402  (device-resident VecEnv)
from flex_gym.env.env.BlackPanther_V55 import __BLACKPANTHER_V55_RESOURCE_DIRECTORY__ as __RSCDIR__  # noqa: E402
from flex_gym.algo.ppo2 import PPO2  # noqa: E402
from flex_gym.archi.policies import CustomLSTMPolicy, MlpPolicy  # noqa: E402
from flex_gym.helper.raisim_gym_helper import ConfigurationSaver, TensorboardLauncher  # noqa: E402
from _flexible_robot import FlexibleGymEnv  # noqa: E402

N_LSTM = [48, 48]  # run_bp_v5.py:111


def parse_args(argv):
    p = argparse.ArgumentParser(description="Train control policies (MI355X engine).")
    p.add_argument("--train", dest="train", action="store_true", default=True)
    p.add_argument("--test", dest="train", action="store_false")
    p.add_argument("--cfg", type=str, default=os.path.abspath(__RSCDIR__ + "/default_cfg.yaml"), help="configuration file")
    p.add_argument("--max_iter", dest="max_iter", type=int, default=200000000, help="total timesteps (all GPUs)")
    p.add_argument("--save", dest="save_flag", type=lambda s: str(s).lower() not in ("0", "false", "no"), default=True)
    p.add_argument("--l", dest="learn_rate", type=float, default=1e-3)
    p.add_argument("--load", dest="pre_trained_model", type=str, default=None, help="warm start (IRRL relaxation stage)")
    p.add_argument("--model", dest="trained_model", type=str, default=None)
    p.add_argument("--o", dest="flag_output", action="store_true", default=False, help="export the actor to CSV")
    p.add_argument("--policy", choices=["lstm", "mlp"], default="lstm", help="lstm = CustomLSTMPolicy (bp5), mlp = MlpPolicy")
    p.add_argument("--num_envs", type=int, default=None, help="override environment.num_envs (per GPU)")
    p.add_argument("--eval_every_n", type=int, default=100)
    p.add_argument("--seed", type=int, default=None, help="override the yaml's seeds: `seed` (policy init, sampling noise) and environment.seedd (env RNG)")
    # --test (run_bp_v5.py:61-108 flag_fix_cmd, delay, vel_filter_freq, act_filter_freq)
    p.add_argument("--cmd", dest="flag_fix_cmd", type=float, default=1.0, help="fixed forward-velocity command of --test [m/s]")
    p.add_argument("--steps", type=int, default=1500, help="control steps of --test")
    p.add_argument("--delay", type=int, default=0, help="observation delay in control steps (DelayTool)")
    p.add_argument("--vel_filter_freq", type=float, default=1.0e6, help="low-pass on the joint-rate / omega observations [Hz]")
    p.add_argument("--act_filter_freq", type=float, default=1.0e6, help="low-pass on the action [Hz]")
    p.add_argument("--cmd_filter_freq", type=float, default=1.0, help="low-pass on the command [Hz] (GaitGenerator command_filter_freq)")
    p.add_argument("--out", type=str, default=None, help="--test: .npz with the per-step records; --sweep: .json with the table")
    # --test --sweep: the robustness grid of the paper (friction x observation delay x command) in one device-resident pool
    floats = lambda s: [float(v) for v in str(s).split(",") if v != ""]
    p.add_argument("--sweep", action="store_true", default=False, help="--test: run the friction x delay x command grid on the device (evaluate.robustness_sweep)")
    p.add_argument("--sweep_mu", type=floats, default=[0.05, 0.4, 0.8], help="friction coefficients, comma separated")
    p.add_argument("--sweep_delay", type=lambda s: [int(v) for v in str(s).split(",") if v != ""], default=[0, 1, 2, 3, 4, 5], help="observation delays [control steps]")
    p.add_argument("--sweep_cmd", type=floats, default=[1.0, 2.0, 3.0, 4.0, 5.0], help="forward-velocity commands [m/s]")
    p.add_argument("--persistent", choices=["auto", "on", "off"], default=None,
                   help="--sweep: the whole run as one persistent launch (on; refused where the kernel does not exist), where it exists (auto), or five "
                        "launches per control step (off); same table bit for bit.  Default: evaluate.PERSISTENT_DEFAULT")
    p.add_argument("--warm", type=int, default=1000, help="--sweep: control steps on friction 0.8 before the condition's own friction is installed")
    # the reference's own names (run_bp_v5.py:383-388 and :308-315 / :400-406), for --test and --test --sweep
    p.add_argument("--step", dest="flag_step", action="store_true", default=False,
                   help="--test: the command staircase, (t // step_steps + 1) / 4 of the command, four levels (--sweep: --steps is replaced by 4 x "
                        "--step_steps and the table has one row per condition and level, over the second half of the level)")
    p.add_argument("--step_steps", type=int, default=5000, help="--step: control steps per level (even)")
    p.add_argument("--gait", dest="flag_gait", action="store_true", default=False,
                   help="--sweep: measure joint power, cost of transport, duty factors and stride frequency on the device as well (with --step: per "
                        "command level, the table behind the reference's Figure 2 bar chart); --gait_mass / --gait_g as in that figure")
    p.add_argument("--gait_mass", type=float, default=None, help="--gait: the mass of the cost of transport [kg] (default: each robot's own total)")
    p.add_argument("--gait_g", type=float, default=9.81, help="--gait: the gravity of the cost of transport [m/s^2]")
    p.add_argument("--dir_fd", dest="flag_dir_fd", action="store_true", default=False,
                   help="--test: direction feedback, a PI loop (kp 1, ki 0.1, clamp Omega) on the base yaw replaces the yaw-rate command")
    # --test --sweep --perturb: the perturbation exploration of the reference's Exp_Raw_Data/Param-*.txt
    def noise(s):
        out = {}
        for item in str(s).split(","):
            if item == "":
                continue
            k, _, v = item.partition("=")
            out[k.strip() + "_noise"] = float(v)
        return out
    p.add_argument("--perturb", type=noise, default=None,
                   help="--sweep: random base-state kicks, amplitudes as key=value out of z, roll, pitch, x_dot, y_dot, z_dot, roll_dot, pitch_dot, yaw_dot "
                        "(the Param files' *_noise keys): --explorations robots per (--sweep_mu, --sweep_delay) at the command --cmd, one kick each at step "
                        "--perturb_at, then --steps control steps; one row per (mu, delay), kicks and statistics to the .npz --out")
    p.add_argument("--explorations", type=int, default=1000, help="--perturb: explorations per condition (the Param files' NoE)")
    p.add_argument("--perturb_at", type=int, default=1000, help="--perturb: the control step of the kick (the warm-up in front of it runs on friction 0.8)")
    p.add_argument("--perturb_seed", type=int, default=0, help="--perturb: seed of the kicks")
    p.add_argument("--entropy", dest="flag_entropy", action="store_true", default=False,
                   help="--perturb: the reference's ensemble analysis per post-kick frame on the device (evaluate.ENSEMBLE_SPEC_REFERENCE: state-space entropy, "
                        "occupied cells, per-feature histograms, mean and standard deviation); the table gains H0, H_last, kappa and t_floor, --out the arrays")
    p.add_argument("--entropy_chunk", type=int, default=None,
                   help="--entropy: run the post-kick frames in calls of at most this many steps, so that the body recorder on the device holds that many rows")
    p.add_argument("--recurrence", dest="flag_recurrence", action="store_true", default=False,
                   help="--sweep: the reference's recurrence plot in numbers, per robot on the device (evaluate.RECURRENCE_SPEC_REFERENCE): the table gains "
                        "RR, DET, LMAX and period_s (--perturb: their medians over the survivors); --out also gets the level matrices of the first 8 conditions")
    p.add_argument("--footfall", dest="flag_footfall", action="store_true", default=False,
                   help="--sweep: the reference's debounced contact flags per robot on the device (evaluate.FOOTFALL_SPEC_REFERENCE): the table gains "
                        "stride_hz_db, duty_db and gait; --out also gets the gait diagrams (`pattern`) of the first 8 conditions")
    p.add_argument("--motor", dest="flag_motor", action="store_true", default=False,
                   help="--footfall: the motor's torque-speed plane per condition and joint on the device (evaluate.motor_spec of the config): the table "
                        "gains sat_max; --out also gets the folded loops and the 2-D maps (`hist`) of the first 8 conditions")
    p.add_argument("--corr", dest="flag_corr", action="store_true", default=False,
                   help="--sweep: the reference's --corr -- the Pearson correlation of two recorded quantities per robot on the device over the measured "
                        "steps (evaluate.CORR_SOURCES; by default the four foot-contact flags against every LSTM cell and hidden unit, recorded after "
                        "each policy step): the table gains corr_max, corr_leg and corr_unit; --out also gets the matrices of the first 8 conditions. "
                        "The measured steps run in the five-launch form (the LSTM state's recorder is steps x robots x 4 hid x 4 B)")
    p.add_argument("--corr_x", type=str, default="contact", help="--corr: the x source, one of contact, torque, joint_rate, body, obs, action, lstm, value")
    p.add_argument("--corr_y", type=str, default="lstm", help="--corr: the y source (an MlpPolicy checkpoint has no recurrent state: choose another than lstm)")
    p.add_argument("--vibration", dest="flag_vibration", action="store_true", default=False,
                   help="--sweep: the reference's --virba -- scipy.signal.spectrogram of the joint angles, joint rates and applied actions per robot on the "
                        "device over the measured steps (evaluate.SPECTRUM_SOURCES, in rad, rad/s, rad): the table gains vib_peak_hz and vib_frac per "
                        "source; --out also gets the Welch spectra of all conditions and the spectrograms (`sxx`) of the first 8")
    p.add_argument("--vib_nperseg", type=int, default=256, help="--vibration: frames per segment, 8 .. 1024 (scipy's default 256)")
    p.add_argument("--vib_hop", type=int, default=224, help="--vibration: frames between the starts of two segments (scipy's default nperseg - nperseg // 8)")
    p.add_argument("--vib_window", choices=["boxcar", "hann", "tukey"], default="tukey", help="--vibration: the window (tukey: alpha 0.25, scipy's default)")
    p.add_argument("--vib_band", type=float, default=50.0, help="--vibration: vib_frac is the share of power above this frequency [Hz] (the reference's set_ylim)")
    p.add_argument("--recurrence_frames", type=int, default=None, help="--recurrence: the last so many frames of the run are analysed (default: min(steps, 800))")
    p.add_argument("--recurrence_radius", type=int, default=None, help="--recurrence: the recurrence radius in levels of 0.001 (default 10)")
    return p.parse_args(argv)


def recurrence_keywords(args):
    """--recurrence [--recurrence_frames T --recurrence_radius r] -> the keywords of robustness_sweep / perturbation_study"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd.evaluate import RECURRENCE_SPEC_REFERENCE
    if not args.flag_recurrence:
        return {}
    spec = dict(RECURRENCE_SPEC_REFERENCE)
    if args.recurrence_radius is not None:
        spec["radius"] = args.recurrence_radius
    return dict(recurrence=spec, recurrence_frames=args.recurrence_frames)


def footfall_keywords(args, env_cfg):
    """--footfall [--motor] -> the keywords of robustness_sweep"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd.evaluate import FOOTFALL_SPEC_REFERENCE, motor_spec
    if args.flag_motor and not args.flag_footfall:
        raise SystemExit("--motor goes with --footfall")
    if not args.flag_footfall:
        return {}
    return dict(footfall=dict(FOOTFALL_SPEC_REFERENCE), motor=motor_spec(env_cfg) if args.flag_motor else None)


def correlation_keywords(args):
    """--corr [--corr_x NAME --corr_y NAME] -> the keywords of robustness_sweep"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd.evaluate import CORR_SOURCES
    if not args.flag_corr:
        return {}
    for k in (args.corr_x, args.corr_y):
        if k not in CORR_SOURCES:
            raise SystemExit("--corr_x / --corr_y: %r is none of %s" % (k, ", ".join(sorted(CORR_SOURCES))))
    if args.persistent == "on":
        raise SystemExit("--corr records inside the policy, which only the five-launch form of the loop can: --persistent auto or off")
    return dict(correlation=dict(x=args.corr_x, y=args.corr_y))


def vibration_keywords(args):
    """--vibration [--vib_nperseg P --vib_hop H --vib_window NAME --vib_band HZ] -> the keywords of robustness_sweep"""
    if not args.flag_vibration:
        return {}
    return dict(spectrum=dict(nperseg=args.vib_nperseg, hop=args.vib_hop, window=args.vib_window, band_hz=args.vib_band))


def plain(v):
    """a row's value for json: arrays as nested lists, dicts of them too"""
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    return v.tolist() if hasattr(v, "tolist") else v


def run_test(args, cfg):
    """Headless evaluation loop (run_bp_v5.py:300-470 without gamepad, window and plots).  One Manual-mode env on the
    numpy boundary (testStep-style single env), the trained actor as a numpy LSTM (CustomerLstmNN twin) or, for an MlpPolicy checkpoint, its
    numpy MLP twin -- picked by the checkpoint's kind."""
    import numpy as np
    from flex_gym.env.RaisimGymVecEnv import RaisimGymVecEnv
    from high_speed_quadrupedal_locomotion_by_irrl_amd.checkpoint import numpy_actor, read_checkpoint
    from high_speed_quadrupedal_locomotion_by_irrl_amd.evaluate import (condition, condition_state, contact_material, heading_hold, heading_parameters,
                                                                        lowpass_alpha, staircase_schedule, yaw_from_quaternion)
    from high_speed_quadrupedal_locomotion_by_irrl_amd.helper import obs_normalisation
    if args.trained_model is None:
        raise SystemExit("model path can't be ignored during test mode (--model)")
    ecfg = dict(cfg["environment"])
    ecfg["num_envs"] = 1
    if not ecfg.get("Manual"):
        print("*" * 50 + "\nMake sure the Manual flag is opened!!! (forcing Manual: True for this run)\n" + "*" * 50)
        ecfg["Manual"] = True
    env = RaisimGymVecEnv(FlexibleGymEnv(__RSCDIR__, yaml.safe_dump(ecfg)))
    _, params = read_checkpoint(args.trained_model)
    ctrl = numpy_actor(params)
    obs_mean, obs_std, action_mean, action_std = obs_normalisation(ecfg)
    dt = float(ecfg["control_dt"])
    # the default 1e6 Hz of --vel_filter_freq / --act_filter_freq goes THROUGH the filters here (alpha ~ 0.99992) as in the reference's loop,
    # while --sweep maps >= 1e6 to "off" (run_sweep): a known difference between the two branches, kept as it is.
    # The command low-pass is the reference's GaitGenerator filtering the gamepad / fixed command at 1 Hz.
    a_cmd, a_vel, a_act = (lowpass_alpha(dt, f) for f in (args.cmd_filter_freq, args.vel_filter_freq, args.act_filter_freq))
    env.SetContactCoefficient(contact_material(0.8))                                # run_bp_v5.py:317-318
    obs = env.reset()
    st = condition_state(obs, args.delay + 1)                                       # delay line (DelayTool), command and rate history
    act_his = np.zeros(12)
    action_total = np.zeros([env.num_envs, env.num_acts], dtype=np.float32)
    rec = {k: [] for k in ("joint", "joint_dot", "posture", "omega", "phase", "act", "oss", "contact", "joint_effort", "cmd", "reward")}
    cmd_target = np.array([[args.flag_fix_cmd, 0.0, 0.0]])
    n_done = 0
    # --step: the command staircase, four levels of --step_steps control steps; --dir_fd: the PI loop on the base yaw (the evaluator's scenario)
    schedule = staircase_schedule(cmd_target, 4) if args.flag_step else None
    heading = heading_parameters(heading_hold(1), 1, float(ecfg["Omega"]), dt) if args.flag_dir_fd else None
    for t in range(args.steps):
        state = env.OriginState()[0, :]
        yaw = yaw_from_quaternion(state[None, 3:7]) if heading is not None else None
        o = condition(st, t, obs, [args.delay], cmd_target, a_cmd, a_vel, obs_mean[0:3], obs_std[0:3], cmd_schedule=schedule, cmd_every=args.step_steps,
                      heading=heading, yaw=yaw)[0]                                              # Manual: the script owns obs[0:3]
        action = ctrl.predict(o)
        action = (1 - a_act) * act_his + a_act * action
        act_his = action
        action_total[0, :] = action
        ob_double = o * obs_std + obs_mean
        rec["joint"].append(ob_double[5:17]); rec["joint_dot"].append(ob_double[17:29]); rec["posture"].append(ob_double[29:32])
        rec["omega"].append(ob_double[32:35]); rec["phase"].append(ob_double[3:5]); rec["act"].append(action * action_std + action_mean)
        rec["oss"].append(state[0:37]); rec["contact"].append(state[37:41]); rec["joint_effort"].append(env.GetJointEffort()[0, :])
        rec["cmd"].append(st["cmd"][0].copy())
        obs, reward, done, _ = env.step(action_total, visualize=False)
        rec["reward"].append(float(reward[0]))
        if done[0]:
            n_done += 1
            ctrl.reset()
            st["cmd"][:] = 0.0                  # the env restarted from rest
            st["heading_int"][:] = 0.0
    out = {k: np.asarray(v) for k, v in rec.items()}
    vx = out["oss"][:, 19]
    print("test: %d steps (%.2f s), command %.2f m/s, mean forward velocity %.3f m/s (last half %.3f), falls %d, mean reward %.4f"
          % (args.steps, args.steps * dt, args.flag_fix_cmd, float(vx.mean()), float(vx[len(vx) // 2:].mean()), n_done,
             float(np.mean(out["reward"]))))
    if args.out:
        np.savez_compressed(args.out, **out)
        print("records written to", args.out)
    return out


def run_sweep(args, cfg):
    """--test --sweep: every (friction, delay, command) condition is one env of ONE Manual-mode pool; the loop of `run_test` runs on the device
    (evaluate.PolicyEvaluator), `--warm` steps on the script's default material, then `--steps` on the condition's own over which the
    statistics are taken.  Prints the table, writes it to --out as JSON."""
    import json
    from high_speed_quadrupedal_locomotion_by_irrl_amd.evaluate import PERSISTENT_DEFAULT, heading_hold, robustness_sweep, sweep_table
    if args.trained_model is None:
        raise SystemExit("model path can't be ignored during test mode (--model)")
    none_if_off = lambda f: None if f >= 1.0e6 else f
    n = len(args.sweep_mu) * len(args.sweep_delay) * len(args.sweep_cmd)
    # --step: four levels of --step_steps steps in place of --steps, one row per condition and level; --dir_fd: the heading hold on every env.
    # Still one pool and one call per run: with --persistent on, one launch (two with a warm-up).
    gait = dict(gait=True, mass=args.gait_mass, g=args.gait_g) if args.flag_gait else {}
    keywords = dict(warm_steps=args.warm, steps=args.steps, cmd_hz=args.cmd_filter_freq, vel_hz=none_if_off(args.vel_filter_freq),
                    act_hz=none_if_off(args.act_filter_freq), persistent=PERSISTENT_DEFAULT if args.persistent is None else args.persistent,
                    levels=4 if args.flag_step else None, level_steps=args.step_steps if args.flag_step else None,
                    heading=heading_hold(n) if args.flag_dir_fd else None, **gait, **recurrence_keywords(args),
                    **footfall_keywords(args, cfg["environment"]), **correlation_keywords(args), **vibration_keywords(args))
    try:
        rows = robustness_sweep(args.trained_model, cfg["environment"], args.sweep_mu, args.sweep_delay, args.sweep_cmd, **keywords)
    except ValueError as e:
        if args.flag_corr and "no recurrent state" in str(e):      # an MlpPolicy checkpoint with --corr_y lstm (or --corr_x lstm)
            raise SystemExit("--corr: %s" % e)
        raise
    print(sweep_table(rows, gait=args.flag_gait, recurrence=args.flag_recurrence, footfall=args.flag_footfall, correlation=args.flag_corr,
                      spectrum=args.flag_vibration))
    if args.out:
        with open(args.out, "w") as f:                                 # (--recurrence: the level matrices of the first 8 conditions as nested lists)
            json.dump([{k: plain(v) for k, v in r.items()} for r in rows], f, indent=1)   # (--footfall / --motor: the patterns and the maps too)
        print("table written to", args.out)
    return rows


def run_perturb(args, cfg):
    """--test --sweep --perturb: the perturbation exploration (evaluate.perturbation_study) -- every (friction, delay) condition x --explorations is
    one env of ONE Manual-mode pool.  Prints one row per (mu, delay); writes the kicks and the per-bucket statistics to --out (.npz)."""
    import numpy as np
    from high_speed_quadrupedal_locomotion_by_irrl_amd.evaluate import ENSEMBLE_SPEC_REFERENCE, PERSISTENT_DEFAULT, perturbation_study, perturbation_table
    if args.trained_model is None:
        raise SystemExit("model path can't be ignored during test mode (--model)")
    none_if_off = lambda f: None if f >= 1.0e6 else f
    bucket = min(args.perturb_at, args.steps)
    entropy = dict(ensemble=ENSEMBLE_SPEC_REFERENCE, frame_chunk=args.entropy_chunk) if args.flag_entropy else {}
    rows = perturbation_study(args.trained_model, cfg["environment"], args.sweep_mu, args.sweep_delay, args.flag_fix_cmd, args.explorations, args.perturb,
                              warm_steps=args.perturb_at, frames=args.steps, seed=args.perturb_seed, bucket_steps=bucket, cmd_hz=args.cmd_filter_freq,
                              vel_hz=none_if_off(args.vel_filter_freq), act_hz=none_if_off(args.act_filter_freq),
                              persistent=PERSISTENT_DEFAULT if args.persistent is None else args.persistent,
                              **(dict(gait=True, mass=args.gait_mass, g=args.gait_g) if args.flag_gait else {}), **entropy, **recurrence_keywords(args))
    print(perturbation_table(rows, gait=args.flag_gait, ensemble=args.flag_entropy, recurrence=args.flag_recurrence))
    if args.out:
        out = dict(mu=np.array([r["mu"] for r in rows]), delay=np.array([r["delay"] for r in rows]), cmd=np.array([r["cmd"] for r in rows]),
                   surviving=np.array([r["surviving"] for r in rows]), falls=np.stack([r["falls"] for r in rows]), kicks=np.stack([r["kicks"] for r in rows]))
        for k in rows[0]["stats"]:
            out["stat_" + k] = np.stack([r["stats"][k] for r in rows])        # [condition, bucket, exploration]
        for k in (rows[0]["gait"] if args.flag_gait else ()):
            out["gait_" + k] = np.stack([r["gait"][k] for r in rows])
        for k in (rows[0]["ensemble"] if args.flag_entropy else ()):
            if rows[0]["ensemble"][k] is not None:
                out["ensemble_" + k] = np.stack([r["ensemble"][k] for r in rows])  # [condition, frame, ...]
        for k in (rows[0]["recurrence"] if args.flag_recurrence else ()):
            out["recurrence_" + k] = np.stack([r["recurrence"][k] for r in rows])  # [condition, exploration]
        np.savez_compressed(args.out, **out)
        print("kicks and statistics written to", args.out)
    return rows


def main(argv=None):
    import torch
    args = parse_args(argv)
    cfg = yaml.safe_load(open(args.cfg, "r"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # under a launcher (complete env:// rendezvous: WORLD_SIZE, RANK, MASTER_PORT), also with one rank: the collectives run over RCCL.
    # A shell that merely exports WORLD_SIZE=1 stays single-process.
    launched = all(k in os.environ for k in ("WORLD_SIZE", "RANK", "MASTER_PORT"))
    if world > 1 and not launched:
        raise SystemExit("WORLD_SIZE=%d but RANK / MASTER_PORT are not set: start the ranks with torch.distributed.run" % world)
    if launched:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("IRRL_BACKEND", "nccl")          # "gloo": CPU-side collectives (tests, one-device multi-rank runs)
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
            torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local_rank))  # RCCL over xGMI
        else:
            torch.distributed.init_process_group(backend)
    if not args.train and not args.flag_output:
        if args.sweep and args.perturb is not None:
            return run_perturb(args, cfg)
        return run_sweep(args, cfg) if args.sweep else run_test(args, cfg)
    if args.num_envs:
        cfg["environment"]["num_envs"] = args.num_envs
    if args.seed is not None:
        cfg["seed"] = int(args.seed)
        cfg["environment"]["seedd"] = int(args.seed)
    # rank r owns the global env ids r * num_envs .. of the one big pool: same seed everywhere, results independent of the GPU count
    cfg["environment"]["EnvIdOffset"] = rank * int(cfg["environment"]["num_envs"])
    # run_bp_v5.py:205-207: the environment sub-tree is dumped to a string and parsed again on the native side
    env = Environment(FlexibleGymEnv(__RSCDIR__, yaml.safe_dump(cfg["environment"]), device=local_rank))

    if args.flag_output:
        model = PPO2.load(args.trained_model, env=env)
        from high_speed_quadrupedal_locomotion_by_irrl_amd.checkpoint import export_actor_csv
        name = os.path.splitext(os.path.basename(args.trained_model))[0]
        print("exported to", export_actor_csv(model, os.path.join(os.getcwd(), "model", name)))
        return


    saver = None
    if args.save_flag and rank == 0:
        saver = ConfigurationSaver(log_dir=os.path.join(ROOT, "data", "black_panther_v5_test"), save_items=[args.cfg])
    log_path = saver.data_dir if saver else ""
    policy = CustomLSTMPolicy if args.policy == "lstm" else MlpPolicy
    kwargs = dict(n_lstm=N_LSTM) if args.policy == "lstm" else {}
    n_steps = math.floor(cfg["environment"]["max_time"] / cfg["environment"]["control_dt"])      # 750
    if args.pre_trained_model is None:
        model = PPO2(tensorboard_log=log_path, policy=policy, policy_kwargs=kwargs, env=env, gamma=0.99, n_steps=n_steps,
                     ent_coef=0.000, learning_rate=args.learn_rate, vf_coef=0.5, max_grad_norm=0.5, lam=0.998,
                     nminibatches=1 if args.policy == "lstm" else 4, noptepochs=10, cliprange=0.2, verbose=1,
                     seed=int(cfg.get("seed", 1)))
    else:
        model = PPO2.load(args.pre_trained_model, env=env, verbose=1)      # run_bp_v5.py:244-248
        model.tensorboard_log = log_path
        model.learning_rate = args.learn_rate
    if saver:
        TensorboardLauncher(saver.data_dir + "/PPO2_1")
    model.learn(total_timesteps=args.max_iter, eval_every_n=args.eval_every_n, log_dir=log_path,
                record_video=bool(cfg.get("record_video", False)))
    if rank == 0 and log_path:
        print("final checkpoint:", model.save(log_path + "_final"))
    if launched:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
