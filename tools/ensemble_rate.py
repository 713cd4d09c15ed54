"""Times of the ensemble analysis (evaluate.ensemble_device -> irrl_eval_ensemble) at the reference's shape, each taken a few times on one device:

    python tools/ensemble_rate.py kernel    # ensemble_device on a generated recorder [1000, 120000, 13] (12 conditions x 10000 explorations), with and
                                            # without histograms and moments; a converged ensemble; smaller and larger ensembles; ensemble_numpy on ONE
                                            # condition of the same tensor on the host, and the two compared where no sample lies on a cell edge
    python tools/ensemble_rate.py study     # perturbation_study 2 frictions x 6 delays x 10000 explorations, 1000 + 1000 steps, without and with
                                            # ensemble=ENSEMBLE_SPEC_REFERENCE, frame_chunk=100, twice interleaved; wall clock and peak device memory
    python tools/ensemble_rate.py           # both

Device events around the calls of `kernel`, wall clock around a device synchronise for `study`.  profiles/eval_ensemble_mi355x.log is its output."""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import torch

from conftest import GOLDEN, load_env_cfg
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV

SPEC = EV.ENSEMBLE_SPEC_REFERENCE
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


if what in ("all", "kernel"):
    F, C_, E = 1000, 12, 10000
    n = C_ * E
    g = torch.Generator(device="cuda").manual_seed(1)
    body = torch.empty(F, n, 13, device="cuda", dtype=torch.float32)
    # a plausible ensemble: the spread of every feature grows from nothing over the first 100 frames and shrinks to a few cells over the rest
    for f0 in range(0, F, 50):
        fr = torch.arange(f0, f0 + 50, device="cuda", dtype=torch.float32)
        s = (torch.clamp(fr / 100.0, max=1.0) * torch.exp(-fr / 300.0)).view(50, 1, 1)
        r = torch.randn(50, n, 13, device="cuda", generator=g)
        blk = r * s * torch.tensor([1, 1, 0.03, 0, 0.15, 0.15, 0.3, 1.0, 0.3, 0.5, 1.5, 1.5, 0.5], device="cuda")
        blk[:, :, 2] += 0.3
        blk[:, :, 3] += 1.0
        blk[:, :, 3:7] /= blk[:, :, 3:7].norm(dim=2, keepdim=True)
        blk[:, :, 7] += 4.5
        body[f0:f0 + 50] = blk
    torch.cuda.synchronize()
    print("recorder: %s, %.2f GB" % (tuple(body.shape), body.numel() * 4 / 1e9), flush=True)
    for name, kw in (("entropy + counts + hist + moments", {}), ("entropy + counts only", dict(hist=False, moments=False))):
        ms, res = timed(lambda: EV.ensemble_device(body, C_, SPEC, **kw))
        print("ensemble_device, %s: %s ms (12000 workgroups; %.1f us per (condition, frame))" % (name, ["%.2f" % m for m in ms], min(ms) * 1e3 / 12000), flush=True)
    res = EV.ensemble_to_numpy(EV.ensemble_device(body, C_, SPEC))
    print("H(condition 0) at frames 0, 50, 100, 300, 999: %s; occupied: %s" % (res["entropy"][0, [0, 50, 100, 300, 999]].round(3).tolist(),
                                                                                res["occupied"][0, [0, 50, 100, 300, 999]].tolist()), flush=True)
    # the converged ensemble (every robot of a condition identical: one run of length E) and small ensembles
    same = body[:40, :1].expand(40, n, 13).contiguous()
    ms, r2 = timed(lambda: EV.ensemble_device(same, C_, SPEC))
    print("ensemble_device, 40 frames of ONE run of length 10000: %s ms; largest = %d" % (["%.3f" % m for m in ms], int(r2["largest"].max())), flush=True)
    for e in (16384, 4096, 1024, 256, 24):
        sub = body[:200, :12 * e].contiguous() if 12 * e <= n else body[:200, :7 * e].contiguous()
        cc = sub.shape[1] // e
        ms, _ = timed(lambda: EV.ensemble_device(sub, cc, SPEC))
        print("ensemble_device, [200, %d x %d]: %s ms (%.2f us per workgroup-slot)" % (cc, e, ["%.3f" % m for m in ms], min(ms) * 1e3 / (200 * cc)), flush=True)
    host = body[:, :E].cpu().numpy()
    del body
    t0 = time.time()
    tw = EV.ensemble_numpy(host, 1, SPEC)
    t1 = time.time()
    print("ensemble_numpy, one condition [1000, 10000, 13] on the host: %.1f s (x 12 conditions = %.0f s)" % (t1 - t0, 12 * (t1 - t0)), flush=True)
    x = EV.ensemble_features(host)
    edge = EV.ensemble_edges(x, SPEC).any(1)
    ok = ~edge
    print("frames with a sample on an edge: %d of 1000; elsewhere counters equal: %s, max |H - twin| = %.3g" % (
        edge.sum(), all(np.array_equal(res[k][0][ok], tw[k][0][ok]) for k in ("kept", "occupied", "largest")), np.abs(res["entropy"][0] - tw["entropy"][0])[ok].max()), flush=True)

if what in ("all", "study"):
    mus, delays, E = (0.8, 0.1), (0, 1, 2, 3, 4, 5), 10000
    cfg = load_env_cfg("bp5_manual_eval.yaml", num_envs=len(mus) * len(delays) * E)
    noise = dict(z_noise=0.02, roll_noise=0.25, pitch_noise=0.25, z_dot_noise=1.0, roll_dot_noise=1.0, pitch_dot_noise=1.0)
    actor = os.path.join(GOLDEN, "actor_bp5_155.npz")
    for name, kw in (("without ensemble", {}), ("ensemble, frame_chunk = 100", dict(ensemble=SPEC, frame_chunk=100)), ("without ensemble", {}),
                     ("ensemble, frame_chunk = 100", dict(ensemble=SPEC, frame_chunk=100))):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.time()
        rows = EV.perturbation_study(actor, cfg, mus, delays, 5.0, E, noise, warm_steps=1000, frames=1000, seed=0, persistent="auto", **kw)
        torch.cuda.synchronize()
        t1 = time.time()
        print("perturbation_study 2 x 6 x 10000, 1000 + 1000 steps, %s: %.2f s wall, peak device memory %.2f GB" % (name, t1 - t0, torch.cuda.max_memory_allocated() / 1e9), flush=True)
        if kw:
            print(EV.perturbation_table(rows, ensemble=True), flush=True)
        del rows
