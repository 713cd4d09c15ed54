"""Times of the gait recorder's analyses (evaluate.footfall_device -> irrl_eval_footfall, evaluate.motor_plane_device -> irrl_eval_motor_plane),
each taken a few times on one device:

    python tools/footfall_rate.py           # both calls on generated recorders [1000, 4096, 32], [16384, 4096, 32] and [1000, 120000, 32]; the
                                            # numpy twins on ONE robot at T = 1000 on the host; device == twin on 16 robots of the first recorder
    python tools/footfall_rate.py small     # without the 120 000-robot recorder (15 GB)
    python tools/footfall_rate.py sweep ACTOR.npz CONFIG.yaml   # bp5_155 in the closed loop at 2 and 5 m/s: the raw touchdown rate that
                                            # gait_from_sums calls stride_hz beside the debounced stride frequency, and the motor's saturation

Device events around the calls.  profiles/eval_footfall_mi355x.log is its output."""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV

SPEC = EV.FOOTFALL_SPEC_REFERENCE
MOTOR = EV.motor_spec(None, tau_max=18.0, w_crit=14.2, w_max=40.0)
what = sys.argv[1] if len(sys.argv) > 1 else "all"
print("device:", torch.cuda.get_device_name(0), flush=True)

if what == "sweep":
    import yaml
    cfg = yaml.safe_load(open(sys.argv[3]))
    cfg = cfg.get("environment", cfg)
    mspec = EV.motor_spec(cfg)
    rows = EV.robustness_sweep(sys.argv[2], cfg, [0.8], [0], [2.0, 5.0], warm_steps=1000, steps=2000, persistent="auto", gait=True, footfall=SPEC,
                               motor=mspec, record_gait=True)
    print(EV.sweep_table(rows, gait=True, footfall=True))
    for r in rows:
        f = r["footfall"]
        m, w, kept = EV.motor_samples(r["rec_gait"][:f["frames"]], mspec)
        excess = np.where(kept, np.maximum(m - EV.motor_up(w, mspec), -EV.motor_up(-w, mspec) - m), -np.inf).max(0)
        print("cmd %g m/s: largest excess over the envelope per joint (N m, motor side; negative = inside) %s" % (r["cmd"], excess.round(3).tolist()))
        print("cmd %g m/s: raw touchdown rate (gait_from_sums' stride_hz) %s Hz, debounced stride frequency %s Hz, duty %s, stance %s s, swing %s s, "
              "flight %.3f, lags %.3f %.3f %.3f, gait %s; saturated fraction per joint %s, outside %s"
              % (r["cmd"], [round(r["stride_hz%d" % l], 2) for l in range(4)], [round(f["stride_hz%d" % l], 3) for l in range(4)],
                 [round(f["duty%d" % l], 3) for l in range(4)], [round(f["stance_s%d" % l], 3) for l in range(4)], [round(f["swing_s%d" % l], 3) for l in range(4)],
                 f["flight"], f["lag1"], f["lag2"], f["lag3"], f["gait"], r["motor"]["saturated"].round(4).tolist(), r["motor"]["counts"][:, 3].tolist()), flush=True)
    sys.exit(0)


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


def recorder(T, n, seed):
    """a plausible gait per robot: a trot with a stride of 15 .. 60 frames and a duty of 0.3 .. 0.6, a robot's own phase, contact flags that
    chatter (dropouts in the stance), torques and rates that follow the stride with noise; one robot in eight is `done` somewhere"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rec = torch.empty(T, n, 32, device="cuda", dtype=torch.float32)
    period = torch.randint(15, 61, (n,), device="cuda", generator=g).float()
    duty = 0.3 + 0.3 * torch.rand(n, device="cuda", generator=g)
    phase = torch.rand(n, device="cuda", generator=g)
    lag = torch.tensor([0.0, 0.5, 0.5, 0.0], device="cuda")
    amp_t = torch.tensor([4.0, 14.0, 20.0] * 4, device="cuda")
    amp_w = torch.tensor([2.0, 12.0, 14.0] * 4, device="cuda")
    for f0 in range(0, T, 50):
        k = min(50, T - f0)
        fr = torch.arange(f0, f0 + k, device="cuda", dtype=torch.float32).view(k, 1)
        ph = (fr / period + phase).unsqueeze(-1)                                    # [k, n, 1] in strides
        leg = torch.remainder(ph - lag, 1.0)                                        # [k, n, 4]
        down = (leg < duty.view(1, n, 1)) & (torch.rand(k, n, 4, device="cuda", generator=g) > 0.25)
        arg = 6.2831853 * (ph + torch.arange(12, device="cuda").view(1, 1, 12) * 0.13)
        rec[f0:f0 + k, :, 0:12] = torch.sin(arg) * amp_t + torch.randn(k, n, 12, device="cuda", generator=g)
        rec[f0:f0 + k, :, 12:24] = torch.cos(arg) * amp_w + torch.randn(k, n, 12, device="cuda", generator=g)
        rec[f0:f0 + k, :, 24:28] = down.float()
        rec[f0:f0 + k, :, 28:32] = down.float() * 60.0
    done = torch.zeros(T, n, device="cuda", dtype=torch.uint8)
    fallen = torch.arange(0, n, 8, device="cuda")
    done[torch.randint(0, T, (len(fallen),), device="cuda", generator=g), fallen] = 1
    torch.cuda.synchronize()
    return rec, done


shapes = [(1000, 4096), (16384, 4096)] + ([(1000, 120000)] if what != "small" else [])
for T, n in shapes:
    rec, done = recorder(T, n, 1)
    print("recorder: %s, %.2f GB" % (tuple(rec.shape), rec.numel() * 4 / 1e9), flush=True)
    EV.footfall_device(rec, done, SPEC)                                # (the first call loads the code object)
    EV.motor_plane_device(rec, done, MOTOR)
    for name, fn in (("footfall, all outputs", lambda: EV.footfall_device(rec, done, SPEC)),
                     ("footfall, counts only", lambda: EV.footfall_device(rec, done, SPEC, support=False, phase=False, pattern=False)),
                     ("motor plane, one robot per condition", lambda: EV.motor_plane_device(rec, done, MOTOR)),
                     ("motor plane, counts only", lambda: EV.motor_plane_device(rec, done, MOTOR, hist=False, fold=False)),
                     ("motor plane, 8 conditions", lambda: EV.motor_plane_device(rec, done, MOTOR, 8))):
        ms, res = timed(fn)
        print("  T = %d, N = %d, %-38s %s ms  (best %.3f ms: %.2f us per robot, %.1f GB/s of recorder rows)"
              % (T, n, name + ":", " / ".join("%.3f" % m for m in ms), min(ms), 1e3 * min(ms) / n, T * n * 128 / min(ms) / 1e6), flush=True)
    if (T, n) == (1000, 4096):
        host, hdone = rec[:, :16].cpu().numpy(), done[:, :16].cpu().numpy()
        t0 = time.perf_counter()
        EV.footfall_numpy(host[:, 1:2], hdone[:, 1:2], SPEC)                 # (robot 1 runs the whole window: no `done`)
        t1 = time.perf_counter()
        EV.motor_plane_numpy(host[:, 1:2], hdone[:, 1:2], MOTOR)
        t2 = time.perf_counter()
        print("  the twins on ONE robot at T = 1000 on the host: footfall_numpy %.4f s, motor_plane_numpy %.4f s" % (t1 - t0, t2 - t1), flush=True)
        sub, sdone = rec[:, :16].contiguous(), done[:, :16].contiguous()
        f, fw = EV.footfall_to_numpy(EV.footfall_device(sub, sdone, SPEC)), EV.footfall_numpy(host, hdone, SPEC)
        m, mw = EV.motor_plane_to_numpy(EV.motor_plane_device(sub, sdone, MOTOR)), EV.motor_plane_numpy(host, hdone, MOTOR)
        print("  16 robots against the twins, every word equal: footfall %s, motor plane %s"
              % (all(f[k].tobytes() == fw[k].tobytes() for k in f), all(m[k].tobytes() == mw[k].tobytes() for k in m)), flush=True)
        c = f["counts"].astype(np.int64)
        print("  touchdowns raw / debounced of robot 1: %s / %s" % (c[1, :, 2].tolist(), c[1, :, 4].tolist()), flush=True)
    del rec, done
    torch.cuda.empty_cache()
