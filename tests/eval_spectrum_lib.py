"""What tests/test_eval_spectrum_host.py (CPU) and tests/test_gpu_eval_spectrum.py (MI355X) share: generated recorders for the spectrogram
(irrl_eval_spectrum), the twin's answers, the case files of tests/eval_spectrum_main.cpp and THE BOUND.

case(nperseg, T) -> (x float32 [rows, 6, 7], done uint8 [rows, 6]): analysed frames are rows FRAME_FIRST + i * FRAME_EVERY (the rows between them
hold other numbers and `done` bytes no result may depend on).  Of the 7 columns the window 2 .. 6 is analysed (neither the first nor the last
column; five columns: one full block of four for a workgroup and one of a single column):
  0   a sine at the exact bin 3 (3 cycles per nperseg frames) on an offset          1   a sine between the bins 2 and 3 on an offset
  2   the constant 0.3: with the detrend its spectrum is zero up to the bound        3   normal noise around 4 sigma
  4   normal noise; robot 0's sample of frame min(T - 1, 20) is a NaN
Robot e's `done` (only where the frame lies inside T):
  0, 3   never done                                   1   done at frame nperseg - 2: fewer frames than a segment, S_e = 0
  2      done at frame nperseg + 2, in the middle of the segments that follow the first: S_e = 1 (hop >= 3), 2 (hop = 2) or 3 (hop = 1)
  4      done at frame 0: T_e = 0                     5   done at frame T // 2, and again later (only the first counts)
The scale differs per column; fs = 100 Hz.

THE BOUND (derived, not measured).  A length-n f64 dot product in any order, fused or not, errs by at most n u sum |a_n t_n| <= n u A with
u = 2^-53 and A = sum_n |a_n| (|t_n| <= 1); the detrend's mean adds the same order.  With |Re|, |Im| <= A the power errs by at most
|P_dev - P_ref| <= 32 n u g_k density A^2 per bin and segment: 8 from carrying two such errors through Re^2 + Im^2 on both sides, times 4 for the
detrend and the second-order terms.  A is computed in f64 from the twin's windowed segment; for psd_sum the bound is the sum over the
condition's segments.  It is relative to the segment's total energy, not to the bin: it holds the constant column and the empty bins of the
planted sines to zero where a per-bin relative bound would say nothing."""
import numpy as np

from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV

FRAME_FIRST, FRAME_EVERY = 3, 2
N, X_DIM, X_FIRST, X_COUNT = 6, 7, 2, 5
FS = 100.0
SCALE = (1.0, 0.5, 3.0, 35.0, 0.7)
NPERSEGS = (16, 12, 9)                      # even; not a power of two; odd, so that the last bin has a mirror image: g_{K-1} = 2
MATRIX_ENV = (2, 0, 2, 1)                   # robot 2 twice; robot 0 carries the NaN; robot 1 has no segment
GROUPINGS = (6, 2, 1)                       # conditions: 6 x 1, 2 x 3, 1 x 6
WINDOWS = ("boxcar", "hann", "tukey")
SEED = 53
U = 2.0 ** -53


def hops(nperseg):
    return (nperseg, 5, 1)


def lengths(nperseg):
    return (nperseg - 1, nperseg, 61)       # no segment; exactly one; many


def cases():
    """(nperseg, hop, T, conditions, detrend, window): every nperseg x hop x T with the other three cycled through, then every detrend x window x
    grouping at nperseg 16, hop 5, T 61"""
    out, i = [], 0
    for P in NPERSEGS:
        for hop in hops(P):
            for T in lengths(P):
                out.append((P, hop, T, GROUPINGS[i % 3], (i // 3) % 2, WINDOWS[(i + i // 3) % 3]))
                i += 1
    out += [(16, 5, 61, c, d, w) for c in GROUPINGS for d in (0, 1) for w in WINDOWS]
    return list(dict.fromkeys(out))


def spec(nperseg, hop, detrend, matrix_env=MATRIX_ENV):
    return EV.spectrum_spec(X_DIM, X_FIRST, X_COUNT, nperseg, hop, FS, scale=SCALE, detrend=detrend, matrix_env=matrix_env)


_TABLES = {}


def tables(nperseg, window):
    if (nperseg, window) not in _TABLES:
        _TABLES[nperseg, window] = EV.spectrum_tables(nperseg, window, 0.25 if window == "tukey" else 0.0)
        for t in _TABLES[nperseg, window]:
            t.setflags(write=False)
    return _TABLES[nperseg, window]


_CACHE = {}


def case(nperseg, T, seed=SEED):
    key = (nperseg, T, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.RandomState(seed + 11 * nperseg + T)
    rows = FRAME_FIRST + (T - 1) * FRAME_EVERY + 1 + 2
    sel = FRAME_FIRST + FRAME_EVERY * np.arange(T)
    x = rng.normal(size=(rows, N, X_DIM)).astype(np.float32)
    i = np.arange(T, dtype=np.float64)[:, None]
    phase = rng.uniform(0, 2 * np.pi, size=(1, N))
    x[sel, :, X_FIRST + 0] = (0.7 + 1.3 * np.sin(2 * np.pi * 3.0 * i / nperseg + phase)).astype(np.float32)
    x[sel, :, X_FIRST + 1] = (-0.2 + 0.9 * np.sin(2 * np.pi * 2.5 * i / nperseg + phase)).astype(np.float32)
    x[sel, :, X_FIRST + 2] = np.float32(0.3)
    x[sel, :, X_FIRST + 3] = (4.0 + rng.normal(size=(T, N))).astype(np.float32)
    x[sel[min(T - 1, 20)], 0, X_FIRST + 4] = np.float32(np.nan)
    done = (rng.uniform(size=(rows, N)) < 0.3).astype(np.uint8)
    done[sel] = 0
    for e, at in ((1, nperseg - 2), (2, nperseg + 2), (4, 0), (5, T // 2)):
        if at < T:
            done[sel[at], e] = 1
    done[sel[T // 2 + 1:], 5] = rng.randint(0, 2, size=T - T // 2 - 1)
    x.setflags(write=False)
    done.setflags(write=False)
    _CACHE[key] = (x, done)
    return _CACHE[key]


def expected_segments(done, T, nperseg, hop):
    """S_e per robot, from `done` by the stated rule"""
    te = np.full(N, T)
    if done is not None:
        dn = done[FRAME_FIRST + FRAME_EVERY * np.arange(T)] != 0
        te = np.where(dn.any(0), dn.argmax(0), T)
    return np.where(te >= nperseg, (te - nperseg) // hop + 1, 0)


_TWIN = {}


def twin(nperseg, hop, T, conditions, detrend, window, with_done=True):
    """the twin's answer with its windowed segments, computed once per case and shared (never written to)"""
    key = (nperseg, hop, T, conditions, detrend, window, with_done)
    if key not in _TWIN:
        x, done = case(nperseg, T)
        win, tw = tables(nperseg, window)
        _TWIN[key] = EV.spectrum_numpy(x, done if with_done else None, spec(nperseg, hop, detrend), win, tw, conditions, FRAME_FIRST, FRAME_EVERY, T,
                                       windowed=True)
        for v in _TWIN[key].values():
            v.setflags(write=False)
    return _TWIN[key]


def density(window, fs=FS):
    t = 0.0
    for w in window:
        t = t + w * w
    return 1.0 / (fs * t)


def segment_bounds(a, window, fs=FS):
    """the twin's windowed segments a [N, S_max, cx, nperseg] -> 32 n u g_k density A^2 per robot, segment, column and bin [N, S_max, cx, K]; a NaN
    where the segment holds one"""
    nperseg = a.shape[-1]
    k = np.arange(nperseg // 2 + 1)
    g = np.where((k == 0) | (2 * k == nperseg), 1.0, 2.0)
    with np.errstate(invalid="ignore"):
        A = np.abs(a).sum(-1)
        return 32.0 * nperseg * U * density(window, fs) * (A * A)[..., None] * g


def bounds(want, nperseg, window, conditions, matrix_env=MATRIX_ENV):
    """-> dict(psd_sum: its bound [G, cx, K], sxx: its bound [M, cx, S_max, K]) out of the twin's windowed segments `a` [N, S_max, cx, nperseg]"""
    per = segment_bounds(want["a"], tables(nperseg, window)[0])
    with np.errstate(invalid="ignore"):
        psd = per.sum(1).reshape(conditions, N // conditions, X_COUNT, per.shape[-1]).sum(1)
    sxx = np.stack([np.transpose(per[e], (1, 0, 2)) for e in matrix_env]) if matrix_env else None
    return dict(psd_sum=psd, sxx=sxx)


def within(got, want, bound, what):
    """segments equal; NaN in the same places; everything else within the bound; -> the largest error / bound seen (0 / 0 counts as 0)"""
    worst = 0.0
    for key in ("psd_sum", "sxx"):
        if want[key] is None:
            assert got[key] is None, (what, key)
            continue
        g, w, b = got[key], want[key], bound[key]
        assert g.shape == w.shape and g.dtype == w.dtype == np.float64, (what, key)
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), (what, key, "a NaN sits elsewhere")
        err = np.abs(g - w)[~nan]
        assert np.all(err <= b[~nan]), (what, key, float(err.max()), float(b[~nan][err.argmax()]))
        live = err > 0
        if live.any():
            worst = max(worst, float((err[live] / b[~nan][live]).max()))
    assert got["segments"].dtype == np.int64 and np.array_equal(got["segments"], want["segments"]), (what, "segments")
    return worst


def same_bytes(got, want, what, keys=("segments", "psd_sum", "sxx")):
    """equal bits in every word; a NaN for a NaN (its sign and payload are whatever the unit that made it leaves there: x86 and numpy differ)"""
    for k in keys:
        if want[k] is None:
            assert got[k] is None, (what, k)
            continue
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        if g.dtype == np.float64:
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(g), nan), (what, k)
            g, w = np.where(nan, 0.0, g), np.where(nan, 0.0, w)
        assert g.tobytes() == w.tobytes(), (what, k)


def write_case(path, x, done, s, window, tw, conditions, frame_first, frame_every, T):
    with open(path, "wb") as f:
        np.asarray([x.shape[0], x.shape[1], frame_first, frame_every, T, 0 if done is None else 1, conditions], np.int32).tofile(f)
        np.asarray([s[k] for k in ("x_dim", "x_first", "x_count", "nperseg", "hop", "detrend")] + [len(s["matrix_env"])]
                   + list(s["matrix_env"]) + [0] * (8 - len(s["matrix_env"])), np.int32).tofile(f)
        np.asarray([s["fs"]] + list(s["scale"]) + [0.0] * (64 - len(s["scale"])), np.float64).tofile(f)
        np.ascontiguousarray(window, np.float64).tofile(f)
        np.ascontiguousarray(tw, np.float64).tofile(f)
        np.ascontiguousarray(x, np.float32).tofile(f)
        if done is not None:
            np.ascontiguousarray(done, np.uint8).tofile(f)


def read_result(path, conditions, s, T):
    G, cx, P, M = conditions, s["x_count"], s["nperseg"], len(s["matrix_env"])
    K, S_max = P // 2 + 1, ((T - P) // s["hop"] + 1 if T >= P else 0)
    with open(path, "rb") as f:
        take = lambda dt, shape: np.fromfile(f, dt, int(np.prod(shape))).reshape(shape)
        out = dict(segments=take(np.int64, (G,)), psd_sum=take(np.float64, (G, cx, K)), sxx=take(np.float64, (M, cx, S_max, K)) if M else None)
        out["work_per_env"] = int(take(np.uint64, (1,))[0])
        assert f.read() == b""
    return out
