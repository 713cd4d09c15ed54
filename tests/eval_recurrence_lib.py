"""What tests/test_eval_recurrence_host.py (CPU) and tests/test_gpu_eval_recurrence.py (MI355X) share: the generated body recorders of the
recurrence analysis, the real windows of the fixture and the precondition of the bit-for-bit rule.

recurrence_case(T, N) -> float32 [rows, N, 13], a recorder in the log layout (base x y z | quaternion w x y z | world v | world w) whose analysed
frames are rows FRAME_FIRST + i * FRAME_EVERY, i = 0 .. T - 1 (the rows between them hold other numbers, which no result may depend on):
  robot 0   standing still: every analysed row identical, every pair recurs (d = 0), one line per diagonal, DIAG_MAX = T - w
  robot 1   exactly periodic, 7 frames: rows of equal phase are the same bits (d = 0), rows of different phase lie 85 levels and more apart
  robot 2   drifting upwards by 1.37 levels per frame: pairs up to 7 frames apart recur, none with |i - j| >= w = 10 -- every count but KEPT is 0
  robot 3   a bounded random walk with holds (runs of identical frames: vertical and diagonal lines of every length)
  robot 4   robot 3's kind with another seed, quaternions of both signs of w (q and -q are the same attitude), and frames 0, T - 1 and a few
            between them NaN or inf in one word (dropped)
N = 2 keeps robots 3 and 4 (the T = 2048 case).  The generator asserts that no pair of the case lies within 1e-9 levels of a level boundary
(evaluate.recurrence_edges), so that device, host program and twin must agree as integers."""
import os

import numpy as np

from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV

SPEC = EV.RECURRENCE_SPEC_REFERENCE
W = max(SPEC["theiler"], 1)
FRAME_FIRST, FRAME_EVERY = 3, 2
TS = (1, 2, 63, 64, 65, 257, 800)
T_BIG = 2048
SEED = 11
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raisim_recurrence_windows.npz")


def _rows(z, roll, pitch, yaw, v, w, xy):
    n = len(z)
    body = np.zeros((n, 13))
    body[:, 0:2] = xy
    body[:, 2] = z
    body[:, 3:7] = EV.kick_rows(roll=roll, pitch=pitch, yaw=yaw)[:, 1:5]
    body[:, 7:10] = v
    body[:, 10:13] = w
    return body


def _walk(rng, T):
    """a bounded walk (first-order autoregression, about 18 levels of standard deviation in the normalised state) with holds"""
    s = np.zeros((T, 9))
    x = rng.normal(size=9)
    hold = 0
    for i in range(T):
        if hold > 0:
            hold -= 1
        else:
            x = 0.97 * x + 0.24 * rng.normal(size=9)
            if rng.uniform() < 0.08:
                hold = int(rng.randint(1, 9))
        s[i] = x
    z = 0.3 + 0.002 * s[:, 0]
    return _rows(z, 0.012 * s[:, 1], 0.012 * s[:, 2], 0.3 * s[:, 3], np.array([5.0, 0.0, 0.0]) + 0.06 * s[:, 4:7], 0.06 * s[:, 6:9], np.cumsum(0.01 + 0 * s[:, :2], 0))


def recurrence_case(T, N=5, seed=SEED):
    rng = np.random.RandomState(seed + T)
    rows = FRAME_FIRST + (T - 1) * FRAME_EVERY + 1 + 2
    i = np.arange(T)
    robots = []
    one = np.ones(T)
    robots.append(_rows(0.31 * one, 0.02 * one, -0.03 * one, 0.4 * one, np.tile([5.0, 0.1, -0.2], (T, 1)), np.tile([0.3, -0.2, 0.1], (T, 1)), np.zeros((T, 2))))
    ph = 2 * np.pi * (i % 7) / 7.0
    robots.append(_rows(0.3 + 0.02 * np.sin(ph), 0.05 * np.cos(ph), 0.05 * np.sin(2 * ph), 0 * ph, np.stack([5 + 0 * ph, 0 * ph, np.cos(ph)], 1),
                        np.stack([np.sin(ph), np.cos(2 * ph), 0 * ph], 1), np.zeros((T, 2))))
    robots.append(_rows(0.25 + 0.000274 * i, 0 * one, 0 * one, 0 * one, np.tile([5.0, 0.0, 0.0], (T, 1)), np.zeros((T, 3)), np.stack([0.01 * i, 0 * i], 1)))
    robots.append(_walk(rng, T))
    last = _walk(rng, T)
    last[:, 3:7] *= np.where(rng.uniform(size=T) < 0.5, -1.0, 1.0)[:, None]
    bad = sorted({0, T - 1} | set(rng.randint(0, T, size=max(1, T // 40)).tolist()))
    for k, b in enumerate(bad):
        last[b, (2, 5, 9, 12)[k % 4]] = (np.nan, np.inf, -np.inf)[k % 3]
    robots.append(last)
    robots = robots[-N:] if N < 5 else robots
    body = rng.uniform(-1.0, 1.0, size=(rows, len(robots), 13))        # the rows between the analysed frames: never read
    body[:, :, 3] = 1.0
    for n, r in enumerate(robots):
        body[FRAME_FIRST + i * FRAME_EVERY, n] = r
    body = body.astype(np.float32)
    on = EV.recurrence_edges(body, SPEC, FRAME_FIRST, FRAME_EVERY, T)
    assert not on.any(), "the generated case T = %d has %d pairs on a level boundary: pick another seed" % (T, on.sum())
    return body


def real_windows():
    """the fixture as a recorder [800, 4, 13] (one robot per RaiSim recording) and its Param values"""
    d = np.load(GOLDEN)
    return np.ascontiguousarray(d["body"].transpose(1, 0, 2)), d


def write_case(path, body, spec, frame_first, frame_every, T, lags, matrix_env=()):
    """the case file of tests/eval_recurrence_main.cpp"""
    with open(path, "wb") as f:
        f.write(np.array([body.shape[0], body.shape[1], frame_first, frame_every, T], np.int32).tobytes())
        f.write(np.asarray(spec["lb"], np.float64).tobytes() + np.asarray(spec["ub"], np.float64).tobytes() + np.array([spec["eps"]], np.float64).tobytes())
        f.write(np.array([spec[k] for k in ("steps", "radius", "theiler", "lmin", "vmin")] + [lags, len(matrix_env)], np.int32).tobytes())
        f.write(np.array(list(matrix_env) + [0] * (8 - len(matrix_env)), np.int32).tobytes())
        f.write(np.ascontiguousarray(body, np.float32).tobytes())


def read_result(path, N, T, lags):
    blob = open(path, "rb").read()
    q = np.frombuffer(blob, np.uint8, N * T * T, 0).reshape(N, T, T)
    o = N * T * T
    counts = np.frombuffer(blob, np.uint32, N * 9, o).reshape(N, 9)
    o += N * 36
    lag = np.frombuffer(blob, np.uint32, N * lags, o).reshape(N, lags)
    o += N * lags * 4
    disagree = int(np.frombuffer(blob, np.uint32, 1, o)[0])
    assert o + 4 == len(blob)
    return q, counts, lag, disagree
