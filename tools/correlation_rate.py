"""Times of the correlation moments (evaluate.correlation_device -> irrl_eval_correlation) and of the trace recorders' extra launch in the
five-launch evaluation loop (PolicyEvaluator.run(record=("lstm", "value")) -> irrl_lstm_eval_traced), each taken a few times on one device:

    python tools/correlation_rate.py                         # the moments on generated recorders [1000, 4096, .]: contact x lstm (4 x 192 out of
                                                             # [., 32] and [., 192]) and obs x obs (35 x 35, one buffer), per robot and pooled into 8
                                                             # conditions; the numpy twin on ONE robot on the host; device == twin on 16 robots
    python tools/correlation_rate.py trace ACTOR.npz CONFIG.yaml [N]   # N = 4096 robots in the closed loop, 200 control steps per call: the
                                                             # five-launch loop without a trace (the launches the loop issued before the trace
                                                             # existed), with the value recorder, with both recorders; and the persistent form

Device events around the calls.  profiles/eval_correlation_mi355x.log is its output."""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV

what = sys.argv[1] if len(sys.argv) > 1 else "moments"
print("device:", torch.cuda.get_device_name(0), flush=True)


def timed(fn, reps=3):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out, r


if what == "trace":
    import yaml
    import high_speed_quadrupedal_locomotion_by_irrl_amd as pkg
    from high_speed_quadrupedal_locomotion_by_irrl_amd.flexible_robot import FlexibleGymEnv
    cfg = yaml.safe_load(open(sys.argv[3]))
    cfg = dict(cfg.get("environment", cfg))
    n = int(sys.argv[4]) if len(sys.argv) > 4 else 4096
    cfg["num_envs"], cfg["Manual"] = n, True
    env = FlexibleGymEnv(pkg.__BLACKPANTHER_V55_RESOURCE_DIRECTORY__, yaml.safe_dump(cfg, default_flow_style=False, width=float("inf")))
    env.init()
    pol = EV.load_policy(sys.argv[2], torch.device("cuda"))
    ev = EV.PolicyEvaluator(env, pol, np.arange(n) % 4, np.full(n, 2.0))
    steps = 200
    ev.run(steps)                                                      # (loads the code objects, settles the gait)
    ev.run(2, record=("lstm", "value"))
    print("pool: %d robots, hid %d, %d control steps per call, persistent kernel exists: %s" % (n, ev.hid, steps, ev.persistent_supported), flush=True)
    forms = [("five launches, no trace", dict(persistent=False)), ("five launches + value", dict(persistent=False, record=("value",))),
             ("five launches + lstm + value", dict(persistent=False, record=("lstm", "value")))]
    if ev.persistent_supported:
        forms.append(("persistent launch, no trace", dict(persistent=True)))
    base = None
    for name, kw in forms:
        ms, _ = timed(lambda: ev.run(steps, **kw), reps=5)
        best = min(ms)
        base = best if base is None else base
        print("  %-30s %s ms  (best %.3f ms: %.2f us per control step, %+.2f us against the loop without a trace)"
              % (name + ":", " / ".join("%.2f" % m for m in ms), best, 1e3 * best / steps, 1e3 * (best - base) / steps), flush=True)
    sys.exit(0)


def recorders(T, n, hid, seed):
    """contact flags that follow a stride (gait columns 24:28), an "LSTM state" of which every fourth unit follows a leg's flag with noise, and
    an observation recorder of normal columns; one robot in eight is `done` somewhere"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    gait = torch.randn(T, n, 32, device="cuda", generator=g)
    period = torch.randint(15, 61, (n,), device="cuda", generator=g).float()
    phase = torch.rand(n, device="cuda", generator=g)
    lag = torch.tensor([0.0, 0.5, 0.5, 0.0], device="cuda")
    fr = torch.arange(T, device="cuda", dtype=torch.float32).view(T, 1)
    down = (torch.remainder((fr / period + phase).unsqueeze(-1) - lag, 1.0) < 0.45).float()          # [T, n, 4]
    gait[:, :, 24:28] = down
    lstm = torch.randn(T, n, 4 * hid, device="cuda", generator=g)
    lstm[:, :, 0::4] += down.repeat(1, 1, hid // 4)[:, :, :lstm[:, :, 0::4].shape[2]]
    obs = torch.randn(T, n, 35, device="cuda", generator=g) * 0.5 + 0.2
    done = torch.zeros(T, n, device="cuda", dtype=torch.uint8)
    fallen = torch.arange(0, n, 8, device="cuda")
    done[torch.randint(0, T, (len(fallen),), device="cuda", generator=g), fallen] = 1
    torch.cuda.synchronize()
    return gait, lstm, obs, done


T, n, hid = 1000, 4096, 48
gait, lstm, obs, done = recorders(T, n, hid, 1)
cl = EV.correlation_spec(32, 24, 4, 4 * hid, 0, 4 * hid)
oo = EV.correlation_spec(35, 0, 35, 35, 0, 35)
print("recorders: gait %s %.2f GB, lstm %s %.2f GB, obs %s %.2f GB" % (tuple(gait.shape), gait.numel() * 4 / 1e9, tuple(lstm.shape), lstm.numel() * 4 / 1e9,
                                                                       tuple(obs.shape), obs.numel() * 4 / 1e9), flush=True)
EV.correlation_device(gait, lstm, done, cl)                             # (the first call loads the code object)
EV.correlation_device(gait, lstm, done, cl, conditions=8)
for name, fn, read in (("contact x lstm, per robot", lambda: EV.correlation_device(gait, lstm, done, cl), 4 * (4 + 4 * hid)),
                       ("contact x lstm, per robot, ranges off", lambda: EV.correlation_device(gait, lstm, done, cl, ranges=False), 4 * (4 + 4 * hid)),
                       ("contact x lstm, 8 conditions", lambda: EV.correlation_device(gait, lstm, done, cl, conditions=8), 4 * (4 + 4 * hid)),
                       ("obs x obs, per robot", lambda: EV.correlation_device(obs, obs, done, oo), 4 * 35),
                       ("obs x obs, 8 conditions", lambda: EV.correlation_device(obs, obs, done, oo, conditions=8), 4 * 35)):
    ms, res = timed(fn)
    print("  T = %d, N = %d, %-40s %s ms  (best %.3f ms: %.2f us per robot, %.1f GB/s of analysed recorder columns read once)"
          % (T, n, name + ":", " / ".join("%.3f" % m for m in ms), min(ms), 1e3 * min(ms) / n, T * n * read / min(ms) / 1e6), flush=True)
hx, hy, hd = gait[:, :16].cpu().numpy(), lstm[:, :16].cpu().numpy(), done[:, :16].cpu().numpy()
t0 = time.perf_counter()
EV.correlation_numpy(hx[:, 1:2], hy[:, 1:2], hd[:, 1:2], cl)                # (robot 1 runs the whole window: no `done`)
t1 = time.perf_counter()
print("  the twin on ONE robot at T = 1000 on the host, contact x lstm: %.4f s" % (t1 - t0), flush=True)
sub = [t[:, :16].contiguous() for t in (gait, lstm, done)]
for cond in (16, 2):
    d, w = EV.correlation_to_numpy(EV.correlation_device(sub[0], sub[1], sub[2], cl, conditions=cond)), EV.correlation_numpy(hx, hy, hd, cl, cond)
    print("  16 robots in %d conditions against the twin, every byte equal: %s" % (cond, all(d[k].tobytes() == w[k].tobytes() for k in w)), flush=True)
r = EV.correlation_from_moments(EV.correlation_to_numpy(EV.correlation_device(sub[0], sub[1], sub[2], cl, conditions=1)))["r"][0]
print("  planted units (every fourth follows a leg's flag): largest |r| %.3f, median |r| of the others %.3f" % (np.nanmax(np.abs(r)), np.nanmedian(np.abs(r[:, 1::4]))),
      flush=True)
