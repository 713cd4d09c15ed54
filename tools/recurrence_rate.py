"""Times of the recurrence analysis (evaluate.recurrence_device -> irrl_eval_recurrence), each taken a few times on one device:

    python tools/recurrence_rate.py           # recurrence_device on generated recorders [800, 4096, 13], [800, 120000, 13] and [2048, 4096, 13], with
                                              # and without the lag words, and with 8 matrices; recurrence_numpy on ONE robot at T = 800 on the host,
                                              # and device == twin on 16 robots of the first recorder where no pair lies on a level boundary
    python tools/recurrence_rate.py small     # without the 120 000-robot recorder (5 GB)

Device events around the calls.  profiles/eval_recurrence_mi355x.log is its output."""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV

SPEC = EV.RECURRENCE_SPEC_REFERENCE
what = sys.argv[1] if len(sys.argv) > 1 else "all"
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


def recorder(T, n, seed):
    """a plausible gait per robot: a stride of 20 .. 60 frames in height, attitude and rates with a robot's own phase, amplitude and noise level
    (from nearly periodic to irregular), quaternions normalised"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    body = torch.empty(T, n, 13, device="cuda", dtype=torch.float32)
    period = torch.randint(20, 61, (n,), device="cuda", generator=g).float()
    phase = torch.rand(n, device="cuda", generator=g) * 6.2831853
    noise = torch.rand(n, device="cuda", generator=g) ** 3 * 0.02
    scale = torch.tensor([0, 0, 0.004, 0, 0.01, 0.01, 0.0, 0.05, 0.05, 0.2, 0.5, 0.5, 0.1], device="cuda")
    for f0 in range(0, T, 50):
        k = min(50, T - f0)
        fr = torch.arange(f0, f0 + k, device="cuda", dtype=torch.float32).view(k, 1)
        arg = (fr / period + 0.0) * 6.2831853 + phase
        wave = torch.stack([torch.sin(arg * (1 + j % 2) + 0.7 * j) for j in range(13)], -1)
        blk = wave * scale + torch.randn(k, n, 13, device="cuda", generator=g) * noise.view(1, n, 1) * (scale > 0)
        blk[:, :, 2] += 0.3
        blk[:, :, 3] += 1.0
        blk[:, :, 3:7] /= blk[:, :, 3:7].norm(dim=2, keepdim=True)
        blk[:, :, 7] += 4.5
        body[f0:f0 + k] = blk
    torch.cuda.synchronize()
    return body


shapes = [(800, 4096), (2048, 4096)] + ([(800, 120000)] if what != "small" else [])
for T, n in shapes:
    body = recorder(T, n, 1)
    print("recorder: %s, %.2f GB" % (tuple(body.shape), body.numel() * 4 / 1e9), flush=True)
    EV.recurrence_device(body, SPEC)                                   # (the first call loads the code object)
    for name, kw in (("counts + %d lag words" % T, {}), ("counts + %d lag words" % (T // 2 + 1), dict(lags=T // 2 + 1)), ("counts only", dict(lags=0)),
                     ("counts + lag + 8 matrices", dict(matrix_env=tuple(range(8))))):
        ms, res = timed(lambda: EV.recurrence_device(body, SPEC, **kw))
        pairs = 1.5 * T * T * n
        print("  T = %d, N = %d, %-28s %s ms  (best %.3f ms: %.1f us per robot, %.2f G pair evaluations / s)"
              % (T, n, name + ":", " / ".join("%.3f" % m for m in ms), min(ms), 1e3 * min(ms) / n, pairs / min(ms) / 1e6), flush=True)
    if (T, n) == (800, 4096):
        host = body[:, :16].cpu().numpy()
        t0 = time.perf_counter()
        one = EV.recurrence_numpy(host[:, :1], SPEC)
        t1 = time.perf_counter()
        print("  recurrence_numpy on ONE robot at T = 800 on the host: %.3f s" % (t1 - t0), flush=True)
        want = EV.recurrence_numpy(host, SPEC, matrix_env=tuple(range(8)))
        got = EV.recurrence_to_numpy(EV.recurrence_device(body[:, :16].contiguous(), SPEC, matrix_env=tuple(range(8))))
        edges = EV.recurrence_edges(host, SPEC)
        clean = ~edges.any((1, 2))
        same = np.array_equal(got["counts"][clean], want["counts"][clean]) and np.array_equal(got["lag"][clean], want["lag"][clean])
        print("  16 robots against the twin: %d without a pair on a level boundary, counts and lag equal there: %s; matrix entries that differ off the "
              "boundaries: %d" % (clean.sum(), same, int(((got["matrix"] != want["matrix"]) & ~edges[:8]).sum())), flush=True)
        m = EV.recurrence_measures(got["counts"], T, SPEC)
        print("  RR %s\n  DET %s" % (m["RR"].round(4).tolist(), m["DET"].round(4).tolist()), flush=True)
    del body
    torch.cuda.empty_cache()
