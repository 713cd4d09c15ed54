"""What tests/test_eval_correlation_host.py (CPU) and tests/test_gpu_eval_correlation.py (MI355X) share: generated recorder pairs for the
correlation moments (irrl_eval_correlation) and the case files of tests/eval_correlation_main.cpp.

case(T, window, N) -> (x float32 [rows, N, x_dim], y float32 [rows, N, y_dim] -- the SAME array for a window with same=True --, done uint8
[rows, N]): analysed frames are rows FRAME_FIRST + i * FRAME_EVERY (the rows between them hold other numbers and `done` bytes no result may
depend on).  Every column is normal with its own mean and sigma, |mean| <= 10 sigma (what the tolerance of correlation_from_moments is derived
for), apart from, where the x window has three columns or more, analysed x column 1 = 0.0 and column 2 = 0.3 in every frame and robot; the
window "contact_lstm" has 0 / 1 flags in its other x columns.  Robot e's `done` follows e % 5 (a sixth robot, e == 5, is done at T // 3):
  0   never done                      1   done at frame 0: T_e = 0, no sample
  2   done at frame 1: T_e = 1        3   done at a random frame of the second half, and again later (only the first counts)
  4   never done
"""
import numpy as np

from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV

FRAME_FIRST, FRAME_EVERY = 3, 2
TS = (1, 2, 63, 64, 65, 257, 1000)
SEED = 41
# name -> (x_dim, x_first, x_count, y_dim, y_first, y_count, same buffer)
WINDOWS = {"contact_lstm": (32, 24, 4, 192, 0, 192, False),        # the reference's --corr: contact flags x LSTM units
           "obs_obs": (35, 0, 35, 35, 0, 35, True),                # an auto-covariance: x and y are one buffer and one window
           "tiles": (13, 2, 9, 300, 7, 257, False),                # crosses the 8-column x tile and the 256-thread y loop
           "one": (1, 0, 1, 1, 0, 1, False)}
# (N, conditions): per robot, one pooled condition, 2 x 3, 1 x 70
GROUPINGS = ((5, 5), (5, 1), (6, 2), (70, 1))
KEYS = ("count", "sx", "sy", "sxy", "range_x", "range_y")


def spec(window):
    w = WINDOWS[window]
    return EV.correlation_spec(*w[:6])


def cases():
    """(T, window, N, conditions): every T and window per robot and pooled on N = 5; 2 x 3 and 1 x 70 at the sizes around a chunk of 64 frames"""
    out = [(T, w, 5, c) for T in TS for w in WINDOWS for c in (5, 1)]
    out += [(T, w, 6, 2) for T in (2, 65, 257) for w in ("contact_lstm", "tiles")]
    out += [(65, "contact_lstm", 70, 1), (64, "one", 70, 1)]
    return out


def _columns(rng, rows, N, dim):
    sigma = np.exp(rng.uniform(np.log(0.01), np.log(10.0), size=dim))
    mean = rng.uniform(-10.0, 10.0, size=dim) * sigma
    return (mean + sigma * rng.normal(size=(rows, N, dim))).astype(np.float32)


_CACHE = {}


def case(T, window, N=5, seed=SEED):
    key = (T, window, N, seed)
    if key in _CACHE:
        return _CACHE[key]
    xd, xf, cx, yd, yf, cy, same = WINDOWS[window]
    rng = np.random.RandomState(seed + 7 * T + N + sum(map(ord, window)))
    rows = FRAME_FIRST + (T - 1) * FRAME_EVERY + 1 + 2
    sel = FRAME_FIRST + FRAME_EVERY * np.arange(T)
    x = _columns(rng, rows, N, xd)
    if window == "contact_lstm":
        x[:, :, xf:xf + cx] = rng.randint(0, 2, size=(rows, N, cx))
    if cx >= 3:
        x[sel, :, xf + 1] = np.float32(0.0)
        x[sel, :, xf + 2] = np.float32(0.3)
    y = x if same else _columns(rng, rows, N, yd)
    done = (rng.uniform(size=(rows, N)) < 0.3).astype(np.uint8)
    done[sel] = 0
    for e in range(N):
        kind = 5 if e == 5 else e % 5
        if kind == 1:
            done[sel[0], e] = 1
        elif kind == 2 and T >= 2:
            done[sel[1], e] = 1
        elif kind == 3 and T >= 4:
            k = int(rng.randint(T // 2, T - 1))
            done[sel[k], e] = 1
            done[sel[k + 1:], e] = rng.randint(0, 2, size=T - k - 1)
        elif kind == 5:
            done[sel[T // 3], e] = 1
    _CACHE[key] = (x, y, done)
    return _CACHE[key]


def expected_te(done, T):
    dn = done[FRAME_FIRST + FRAME_EVERY * np.arange(T)] != 0
    return np.where(dn.any(0), dn.argmax(0), T)


_TWIN = {}


def twin(T, window, N, conditions, with_done=True):
    """the twin's answer, computed once per case and shared (never written to)"""
    key = (T, window, N, conditions, with_done)
    if key not in _TWIN:
        x, y, done = case(T, window, N)
        _TWIN[key] = EV.correlation_numpy(x, y, done if with_done else None, spec(window), conditions, FRAME_FIRST, FRAME_EVERY, T)
        for v in _TWIN[key].values():
            v.setflags(write=False)
    return _TWIN[key]


def write_case(path, x, y, done, s, conditions, frame_first, frame_every, T):
    same = y is x
    with open(path, "wb") as f:
        np.asarray([x.shape[0], x.shape[1], frame_first, frame_every, T, 0 if done is None else 1, conditions, int(same)], np.int32).tofile(f)
        np.asarray([s[k] for k in ("x_dim", "x_first", "x_count", "y_dim", "y_first", "y_count")], np.int32).tofile(f)
        np.ascontiguousarray(x, np.float32).tofile(f)
        if not same:
            np.ascontiguousarray(y, np.float32).tofile(f)
        if done is not None:
            np.ascontiguousarray(done, np.uint8).tofile(f)


def read_result(path, conditions, s):
    G, cx, cy = conditions, s["x_count"], s["y_count"]
    with open(path, "rb") as f:
        take = lambda dt, shape: np.fromfile(f, dt, int(np.prod(shape))).reshape(shape)
        out = dict(count=take(np.int64, (G,)), sx=take(np.float64, (G, cx, 2)), sy=take(np.float64, (G, cy, 2)), sxy=take(np.float64, (G, cx, cy)),
                   range_x=take(np.float32, (G, cx, 2)), range_y=take(np.float32, (G, cy, 2)))
        out["work_per_env"] = int(take(np.uint64, (1,))[0])
        assert f.read() == b""
    return out


def same_bytes(got, want, what, keys=KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k)


def pooled(x, y, done, s, conditions, g, T):
    """the samples of condition g as float64 [n, cx], [n, cy]: the frames i < T_e of its robots"""
    N = x.shape[1]
    R = N // conditions
    sel = FRAME_FIRST + FRAME_EVERY * np.arange(T)
    te = expected_te(done, T) if done is not None else np.full(N, T)
    xs, ys = [], []
    for e in range(g * R, (g + 1) * R):
        xs.append(x[sel[:te[e]], e, s["x_first"]:s["x_first"] + s["x_count"]])
        ys.append(y[sel[:te[e]], e, s["y_first"]:s["y_first"] + s["y_count"]])
    return np.concatenate(xs).astype(np.float64), np.concatenate(ys).astype(np.float64)
