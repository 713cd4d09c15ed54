"""Times of the spectrogram and Welch spectrum of recorder columns (evaluate.spectrum_device -> irrl_eval_spectrum), each taken a few times on
one device:

    python tools/spectrum_rate.py [T N]          # generated recorders [T = 2000, N = 4096, .] at fs = 100 Hz: the sweep's three sources (joint
                                                 # angles and joint rates, 12 columns each out of [., 35], and the applied actions, [., 12]) with the
                                                 # reference's nperseg 256, hop 224, Tukey(0.25), per robot and pooled into 8 conditions, with and
                                                 # without the spectrograms of 8 robots; nperseg 1024 and 64 on one source; the numpy twin on ONE
                                                 # robot on the host; device against twin on 4 robots as a fraction of the tests' bound

Device events around the calls.  The multiply-add count is 2 K nperseg per segment and column (K = nperseg / 2 + 1 bins, Re and Im)."""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV

T = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
FS = 100.0
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


def recorders(seed):
    """joints that swing with each robot's stride (1.5 .. 4 Hz) plus a chatter at 20 .. 45 Hz of a hundredth of the swing, noise on top; one robot
    in eight is `done` somewhere"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(T, device="cuda", dtype=torch.float32).view(T, 1, 1) / FS
    stride = 1.5 + 2.5 * torch.rand(1, n, 1, device="cuda", generator=g)
    chatter = 20.0 + 25.0 * torch.rand(1, n, 1, device="cuda", generator=g)
    phase = 6.2832 * torch.rand(1, n, 35, device="cuda", generator=g)
    obs = torch.sin(6.2832 * stride * t + phase) + 0.01 * torch.sin(6.2832 * chatter * t + 2 * phase) + 0.001 * torch.randn(T, n, 35, device="cuda", generator=g)
    act = obs[:, :, 5:17].clone() * 0.5 + 0.002 * torch.randn(T, n, 12, device="cuda", generator=g)
    done = torch.zeros(T, n, device="cuda", dtype=torch.uint8)
    fallen = torch.arange(0, n, 8, device="cuda")
    done[torch.randint(0, T, (len(fallen),), device="cuda", generator=g), fallen] = 1
    torch.cuda.synchronize()
    return obs, act, done


obs, act, done = recorders(1)
print("recorders: obs %s %.2f GB, act %s %.2f GB" % (tuple(obs.shape), obs.numel() * 4 / 1e9, tuple(act.shape), act.numel() * 4 / 1e9), flush=True)
shown = tuple(range(8))


def run(name, x, first, width, nperseg, hop, conditions, sxx):
    s = EV.spectrum_spec(width, first, 12, nperseg, hop, FS, scale=np.linspace(1.0, 40.0, 12), matrix_env=shown if sxx else ())
    win, tw = (torch.from_numpy(t).cuda() for t in EV.spectrum_tables(nperseg, "tukey", 0.25))
    call = lambda: EV.spectrum_device(x, done, s, win, tw, conditions=conditions)
    call()                                                            # (the first call loads the code object)
    ms, res = timed(call)
    seg = int(res["segments"].sum())
    fma = 2.0 * (nperseg // 2 + 1) * nperseg * 12 * seg
    print("  T = %d, N = %d, %-58s %s ms  (best %.3f ms: %d segments, %.3g f64 multiply-adds, %.2f T multiply-adds/s)"
          % (T, n, name + ":", " / ".join("%.3f" % m for m in ms), min(ms), seg, fma, fma / min(ms) / 1e9), flush=True)
    return min(ms)


total = 0.0
for name, x, first, width in (("joint", obs, 5, 35), ("joint_rate", obs, 17, 35), ("action", act, 0, 12)):
    total += run("%s, nperseg 256, hop 224, per robot, sxx of 8" % name, x, first, width, 256, 224, None, True)
print("  the sweep's three calls (36 columns): %.3f ms" % total, flush=True)
run("joint, nperseg 256, hop 224, per robot, sxx off", obs, 5, 35, 256, 224, None, False)
run("joint, nperseg 256, hop 224, 8 conditions", obs, 5, 35, 256, 224, 8, True)
run("joint, nperseg 1024, hop 896, per robot", obs, 5, 35, 1024, 896, None, True)
run("joint, nperseg 64, hop 56, per robot", obs, 5, 35, 64, 56, None, True)

hx, hd = obs[:, :4].cpu().numpy(), done[:, :4].cpu().numpy()
s = EV.spectrum_spec(35, 5, 12, 256, 224, FS, scale=np.linspace(1.0, 40.0, 12), matrix_env=(0, 1, 2, 3))
win, tw = EV.spectrum_tables(256, "tukey", 0.25)
t0 = time.perf_counter()
EV.spectrum_numpy(hx[:, 1:2], hd[:, 1:2], dict(s, matrix_env=(0,)), win, tw)        # (robot 1 runs the whole window: no `done`)
t1 = time.perf_counter()
print("  the twin on ONE robot at T = %d on the host, 12 columns, nperseg 256: %.3f s" % (T, t1 - t0), flush=True)
want = EV.spectrum_numpy(hx, hd, s, win, tw, windowed=True)
got = EV.spectrum_to_numpy(EV.spectrum_device(obs[:, :4].contiguous(), done[:, :4].contiguous(), s, win, tw))
A = np.abs(want["a"]).sum(-1)                                          # [4, S_max, 12]
k = np.arange(129)
bound = 32.0 * 256 * 2.0 ** -53 / (FS * float((win * win).sum())) * (A * A)[..., None] * np.where((k == 0) | (k == 128), 1.0, 2.0)
err, bound = np.abs(got["sxx"] - want["sxx"]), np.transpose(bound, (0, 2, 1, 3))
print("  4 robots against the twin: segments equal %s, largest |device - twin| / bound over the spectrograms %.3g"
      % (np.array_equal(got["segments"], want["segments"]), float((err[err > 0] / bound[err > 0]).max()) if (err > 0).any() else 0.0), flush=True)
row = EV.spectrum_row(dict(joint=got["psd_sum"][1]), int(got["segments"][1]), FS, ("joint",), 15.0)
print("  robot 1: peak %.2f Hz (its stride), %.2e of the power above 15 Hz (its chatter)" % (row["vib_peak_hz_joint"], row["vib_frac_joint"]), flush=True)
