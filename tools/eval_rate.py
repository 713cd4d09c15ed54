"""Control steps per second of the policy evaluation loop at 4096 envs: the device-resident evaluator (evaluate.PolicyEvaluator: five launches per
step, no host round trip) and the host-driven loop it replaces (evaluate.reference_rollout, reached through tests/parity_lib.closed_loop_log_conditions,
on HipVecEnv: numpy boundary, float64 numpy actor, get_state and every record on every step).  Same pool size, same actor, same conditions; wall
clock around work that ends in a device synchronise.

    python tools/eval_rate.py [--envs 4096] [--steps 2000] [--host-steps 200]

--ab: the persistent single-launch form (PolicyEvaluator.run(persistent=True), kernel csrc/env_eval_kernels.hpp) against the five-launch form, same
process, same pool, interleaved A, B, A, B (A = five launches per step), statistics only and all recorders; the host-driven leg is skipped.

    python tools/eval_rate.py --ab [--envs 4096 | --envs 90] [--steps 2000] [--scenario]

--scenario (with --ab): every leg runs with a scenario installed (PolicyEvaluator.set_scenario: a 5-row command staircase over the timed steps, the
heading hold on every env, 4 statistics buckets) through irrl_lstm_eval_scenario[_persistent].

--kicks K (with --ab): every leg runs with a kick table installed (PolicyEvaluator.set_scenario(kicks=): a tenth of the reference's exploration
amplitudes on every env, one row every K timed steps) through irrl_lstm_eval_perturbed[_persistent].  Another trajectory than the run without
kicks, so only roughly comparable with it.

--gait (with --ab): every leg measures joint power, torque and ground-force sums and the footfall pattern too (PolicyEvaluator.measure_gait) through
irrl_lstm_eval_measured[_persistent]; the same trajectory as the run without, so the difference is the measurements' cost.

--policy mlp: the actor is an MlpPolicy (layers (64, 64); torch.manual_seed(0) initialisation, no trained fixture is needed for a time per step)
through irrl_mlp_eval_measured[_persistent].  With --events the time per control step comes from events on the stream around `--steps` steps
behind a `--warmup`-step warm-up of the same form, the two forms alternating, `--runs` runs each, medians:

    python tools/eval_rate.py --events --policy mlp [--envs 4096 | --envs 90] [--steps 2000] [--warmup 200] [--runs 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

import high_speed_quadrupedal_locomotion_by_irrl_amd as pkg  # noqa: E402
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV  # noqa: E402
from high_speed_quadrupedal_locomotion_by_irrl_amd.flexible_robot import FlexibleGymEnv  # noqa: E402


def ab(args, env, pol, delays, cmds, out):
    """A, B, A, B on one pool: every leg is a fresh evaluator (reset), a 50-step warm-up of its own form, then `steps` steps timed around a
    device synchronise.  The two forms compute the same trajectory bit for bit, so the legs do the same work."""
    n = args.envs
    cases = [("statistics only", (), True), ("all recorders", tuple(EV.RECORDERS), True)] + ([("no statistics", (), False)] if args.no_statistics else [])
    for name, record, acc in cases:
        legs = {False: [], True: []}
        for persistent in (False, True, False, True):
            ev = EV.PolicyEvaluator(env, pol, delays, cmds, cmd_hz=1.0, vel_hz=50.0, act_hz=30.0)
            if args.scenario:
                ev.set_scenario(cmd_schedule=EV.staircase_schedule(cmds, 5), cmd_every=max(args.steps // 5, 1), heading=EV.heading_hold(n), stat_buckets=4,
                                stat_every=max(args.steps // 4, 1), t0=50)
            if args.kicks:
                rows = max(args.steps // args.kicks, 1)
                noise = dict(z_noise=0.002, roll_noise=0.025, pitch_noise=0.025, z_dot_noise=0.1, roll_dot_noise=0.1, pitch_dot_noise=0.1)
                table = EV.exploration_kicks(rows * n, noise, np.random.default_rng(0)).reshape(rows, n, EV.KICK_DIM)
                scn = ev.scenario or {}
                ev.set_scenario(cmd_schedule=None if not args.scenario else EV.staircase_schedule(cmds, 5), cmd_every=scn.get("cmd_every", 1),
                                heading=EV.heading_hold(n) if args.scenario else None, stat_buckets=scn.get("stat_buckets", 1),
                                stat_every=scn.get("stat_every", 1), t0=50, kicks=table, kick_first=args.kicks // 2, kick_every=args.kicks)
            if args.gait:
                ev.measure_gait()
            ev.run(50, record=record, accumulate=acc, persistent=persistent)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.run(args.steps, record=record, accumulate=acc, persistent=persistent)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            legs[persistent].append(1e6 * dt / args.steps)
            print("%-15s %-12s: %d envs x %d steps in %.3f s = %.1f us per step, falls %d"
                  % (name, "persistent" if persistent else "five-launch", n, args.steps, dt, 1e6 * dt / args.steps, int(ev.statistics()["falls"].sum())))
        a, b = min(legs[False]), min(legs[True])
        out[name] = {"steps": args.steps, "five_launch_us_per_step": legs[False], "persistent_us_per_step": legs[True], "persistent_over_five_launch": b / a}
        print("%-15s: five-launch %.1f us, persistent %.1f us per step (best of two each), ratio %.3f" % (name, a, b, b / a))
    print(json.dumps(out))


def events(args, env, pol, delays, cmds, out):
    """per-step form, persistent form, per-step form ... on one pool, `runs` runs each: a fresh evaluator (reset), `warmup` steps of the run's own
    form, then `steps` steps between two events on the stream.  Statistics on, no recorders.  Medians."""
    times = {False: [], True: []}
    for _ in range(args.runs):
        for persistent in (False, True):
            ev = EV.PolicyEvaluator(env, pol, delays, cmds, cmd_hz=1.0, vel_hz=50.0, act_hz=30.0)
            ev.run(args.warmup, persistent=persistent)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ev.run(args.steps, persistent=persistent)
            e1.record()
            e1.synchronize()
            us = 1e3 * e0.elapsed_time(e1) / args.steps
            times[persistent].append(us)
            print("%-10s: %d envs x %d steps, %.2f us per control step, falls %d"
                  % ("persistent" if persistent else "per-step", args.envs, args.steps, us, int(ev.statistics()["falls"].sum())), flush=True)
    a, b = float(np.median(times[False])), float(np.median(times[True]))
    out.update(policy=args.policy, steps=args.steps, warmup=args.warmup, per_step_us=times[False], persistent_us=times[True], per_step_median_us=a,
               persistent_median_us=b, persistent_over_per_step=b / a)
    print("%s policy, %d envs: per-step form %.2f us, persistent form %.2f us per control step (medians of %d), ratio %.3f"
          % (args.policy, args.envs, a, b, args.runs, b / a))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policy", choices=("lstm", "mlp"), default="lstm", help="the actor: the LSTM fixture, or an MlpPolicy (64, 64) as initialised under seed 0")
    ap.add_argument("--events", action="store_true", help="per-step form against persistent form, alternating, timed by stream events; medians of --runs")
    ap.add_argument("--warmup", type=int, default=200, help="--events: control steps of each run's own form in front of the timed ones")
    ap.add_argument("--runs", type=int, default=5, help="--events: runs per form")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--host-steps", type=int, default=200)
    ap.add_argument("--no-statistics", action="store_true", help="--ab: one more pair of legs with neither recorders nor statistics (accumulate=False)")
    ap.add_argument("--scenario", action="store_true", help="--ab: a 5-row command schedule, the heading hold and 4 statistics buckets on every leg")
    ap.add_argument("--kicks", type=int, default=0, help="--ab: a kick table on every leg, one row of small kicks for every env every K timed steps")
    ap.add_argument("--gait", action="store_true", help="--ab: the gait measurements (power, contact statistics) on every leg")
    ap.add_argument("--ab", action="store_true", help="five launches per step (A) against the persistent launch (B), interleaved A, B, A, B")
    args = ap.parse_args()
    n = args.envs
    cfg = yaml.safe_load(open(os.path.join(pkg.__BLACKPANTHER_V55_RESOURCE_DIRECTORY__, "bp5_manual_eval.yaml")))["environment"]
    cfg["num_envs"] = n
    delays, cmds, mus = np.arange(n) % 6, np.linspace(0.5, 5.0, n), np.linspace(0.05, 0.8, n)
    if args.policy == "mlp":
        from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import MlpPolicy
        torch.manual_seed(0)
        pol = EV.load_policy(MlpPolicy(), torch.device("cuda"))
    else:
        pol = EV.load_policy(os.path.join(ROOT, "tests", "golden", "actor_bp5_155.npz"), torch.device("cuda"))
    env = FlexibleGymEnv(pkg.__BLACKPANTHER_V55_RESOURCE_DIRECTORY__, yaml.safe_dump(cfg, default_flow_style=False, width=float("inf")))
    env.init()
    env.SetContactCoefficient(EV.contact_material(mus))
    out = {"envs": n, "scenario": bool(args.scenario), "kicks": int(args.kicks), "gait": bool(args.gait)}
    if args.events:
        return events(args, env, pol, delays, cmds, out)
    if args.ab:
        return ab(args, env, pol, delays, cmds, out)
    for name, record in (("statistics only", ()), ("all recorders", tuple(EV.RECORDERS))):
        ev = EV.PolicyEvaluator(env, pol, delays, cmds, cmd_hz=1.0, vel_hz=50.0, act_hz=30.0)
        ev.run(50, record=record)                                  # code objects loaded, buffers touched
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.run(args.steps, record=record)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        falls = int(ev.statistics()["falls"].sum())
        out[name] = {"steps": args.steps, "seconds": dt, "steps_per_s": args.steps / dt, "env_steps_per_s": args.steps * n / dt, "falls": falls}
        print("device evaluator, %-15s: %d envs x %d steps in %.3f s = %.0f control steps/s (%.1f us per step, %.1f M env-steps/s), falls %d"
              % (name, n, args.steps, dt, args.steps / dt, 1e6 * dt / args.steps, args.steps * n / dt / 1e6, falls))
    import parity_lib as PL
    from hip_env import HipVecEnv
    conds = [dict(cmd=float(cmds[i]), mu=float(mus[i]), delay=int(delays[i]), warm=0, frames=args.host_steps) for i in range(n)]
    host_env = HipVecEnv(cfg)
    t0 = time.perf_counter()
    _, falls = PL.closed_loop_log_conditions(host_env, cfg, conds)
    dt = time.perf_counter() - t0
    out["host-driven"] = {"steps": args.host_steps, "seconds": dt, "steps_per_s": args.host_steps / dt, "env_steps_per_s": args.host_steps * n / dt,
                          "falls": int(np.sum(falls))}
    print("host-driven loop (closed_loop_log_conditions on HipVecEnv): %d envs x %d steps in %.3f s = %.1f control steps/s (%.2f ms per step, %.3f M env-steps/s)"
          % (n, args.host_steps, dt, args.host_steps / dt, 1e3 * dt / args.host_steps, args.host_steps * n / dt / 1e6))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
