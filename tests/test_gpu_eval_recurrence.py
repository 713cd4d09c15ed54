"""The recurrence analysis of a body recorder (evaluate.recurrence_device -> irrl_eval_recurrence: one workgroup per robot keeps the robot's
normalised states in LDS and walks the time x time matrix of their distances along its diagonals and its columns) on the MI355X against the
float64 twin (evaluate.recurrence_numpy), and the robustness sweep that carries it.

(a) the generated recorders of tests/eval_recurrence_lib.py, uploaded: [rows, 5, 13] with T = 1, 2, 63, 64, 65, 257, 800 (wave and workgroup
    edges) and [rows, 2, 13] with T = 2048 (98 KB of LDS), and the four real windows as a [800, 4, 13] recorder.  No pair lies within 1e-9 levels
    of a level boundary (asserted by the generator and, for the windows, by the host tests), so counts, lag and matrix are the twin's bit for bit.
(b) the closed loop: robustness_sweep on frictions 0.8 / 0.1 x delays 0 / 3 at 2 m/s, 300 warm-up + 256 steps.  These trajectories come from the
    GPU: a pair in which the twin finds d / eps within 1e-9 of a level boundary is left out of the matrix comparison, and the test fails if more
    than 1e-5 of the entries are; counts and lag must equal the integer stage of the twin on the DEVICE's matrix exactly."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_recurrence_lib as L
import test_gpu_eval_persistent as TP
from conftest import load_env_cfg
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV

SPEC = L.SPEC


def _device(body, **kw):
    return EV.recurrence_to_numpy(EV.recurrence_device(torch.from_numpy(np.array(body)).cuda(), kw.pop("spec", SPEC), **kw))


def _same_bits(a, b, what):
    for k in ("counts", "lag", "matrix"):
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
        else:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.fixture(scope="module")
def case257():
    body = L.recurrence_case(257)
    body.setflags(write=False)
    return body, EV.recurrence_numpy(body, SPEC, L.FRAME_FIRST, L.FRAME_EVERY, 257, matrix_env=(0, 1, 2, 3, 4))


# ---- (a) generated recorders and the real windows ----
@pytest.mark.parametrize("T", L.TS + (L.T_BIG,))
def test_device_equals_the_twin_bit_for_bit(T):
    """counts, every lag word and the matrices of all robots == recurrence_numpy; REC_FULL = 2 REC, lag[0] = KEPT, the matrix symmetric; a second
    run gives the same bits"""
    N = 2 if T == L.T_BIG else 5
    body = L.recurrence_case(T, N)
    env = tuple(range(N))
    want = EV.recurrence_numpy(body, SPEC, L.FRAME_FIRST, L.FRAME_EVERY, T, matrix_env=env)
    got = _device(body, frame_first=L.FRAME_FIRST, frame_every=L.FRAME_EVERY, frames=T, matrix_env=env)
    print("T = %d: counts of the last robot %s" % (T, got["counts"][-1].tolist()))
    _same_bits(got, want, "T = %d" % T)
    assert np.array_equal(got["counts"][:, 8], 2 * got["counts"][:, 1]) and np.array_equal(got["lag"][:, 0], got["counts"][:, 0])
    assert np.array_equal(got["matrix"], got["matrix"].transpose(0, 2, 1))
    _same_bits(_device(body, frame_first=L.FRAME_FIRST, frame_every=L.FRAME_EVERY, frames=T, matrix_env=env), got, "second run")


def test_real_windows():
    body, meta = L.real_windows()
    want = EV.recurrence_numpy(body, SPEC, matrix_env=(0, 1, 2, 3))
    got = _device(body, matrix_env=(0, 1, 2, 3))
    _same_bits(got, want, "real windows")
    p = EV.recurrence_period(got["lag"][:, :400], 800, L.W, float(meta["frame_dt"]))
    assert p["lag"][:3].tolist() == [100, 100, 300]


def test_optional_outputs_theiler_and_matrix_lists(case257):
    """matrix_count 0, 1 and 8 with a robot listed twice; lags 0 (lag = NULL), 1 and T; theiler >= T; another radius / lmin / vmin: every output
    that is asked for is the twin's, and the ones that stay are the full call's bits"""
    body, full = case257
    T = 257
    kw = dict(frame_first=L.FRAME_FIRST, frame_every=L.FRAME_EVERY, frames=T)
    a = _device(body, lags=0, **kw)
    assert a["lag"] is None and a["matrix"] is None and a["counts"].tobytes() == full["counts"].tobytes()
    b = _device(body, lags=1, matrix_env=(3,), **kw)
    assert b["lag"].shape == (5, 1) and np.array_equal(b["lag"][:, 0], full["counts"][:, 0]) and b["counts"].tobytes() == full["counts"].tobytes()
    assert b["matrix"].tobytes() == full["matrix"][3:4].tobytes()
    env = (4, 1, 4, 0, 2, 3, 1, 4)                                  # 8 matrices, robots listed twice and three times
    c = _device(body, matrix_env=env, **kw)
    assert c["matrix"].tobytes() == full["matrix"][list(env)].tobytes() and c["lag"].tobytes() == full["lag"].tobytes()
    for spec in (dict(SPEC, theiler=T), dict(SPEC, theiler=T + 5), dict(SPEC, theiler=0), dict(SPEC, radius=40, lmin=1, vmin=5), dict(SPEC, radius=1, lmin=5, vmin=1)):
        want = EV.recurrence_numpy(body, spec, matrix_env=(4,), **kw)
        got = _device(body, spec=spec, matrix_env=(4,), **kw)
        _same_bits(got, want, spec)
        if spec["theiler"] >= T:
            assert np.all(got["counts"][:, 1:] == 0) and got["lag"].tobytes() == full["lag"].tobytes()
    with pytest.raises(ValueError):
        _device(body, lags=T + 1, **kw)
    with pytest.raises(ValueError):
        _device(body, matrix_env=(5,), **kw)


def test_on_a_callers_stream_and_words_of_other_robots_untouched(case257):
    """the launch goes to torch's current stream (a call under torch.cuda.stream(s) behind a copy on s sees the copied recorder); the C entry
    point on a recorder of 3 of the 5 robots, its output buffers placed inside larger ones filled with sentinels, writes its own words alone"""
    import ctypes as C
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib
    body, full = case257
    T = 257
    s = torch.cuda.Stream()
    host = torch.from_numpy(np.array(body)).pin_memory()
    with torch.cuda.stream(s):
        dev = torch.empty(body.shape, device="cuda", dtype=torch.float32)
        dev.copy_(host, non_blocking=True)
        res = EV.recurrence_device(dev, SPEC, L.FRAME_FIRST, L.FRAME_EVERY, T, matrix_env=(0, 1, 2, 3, 4))
    s.synchronize()
    _same_bits(EV.recurrence_to_numpy(res), full, "caller's stream")
    # robots 1 .. 3 as a pool of 3: the words in front of and behind the 3 robots' outputs keep their sentinels
    sub = torch.from_numpy(np.ascontiguousarray(body[:, 1:4])).cuda()
    pad = 64
    counts = torch.full((pad + 3 * 9 + pad,), -7, device="cuda", dtype=torch.int32)
    lag = torch.full((pad + 3 * T + pad,), -7, device="cuda", dtype=torch.int32)
    matrix = torch.full((pad + 2 * T * T + pad,), 0xAB, device="cuda", dtype=torch.uint8)
    st = EV.recurrence_struct(SPEC, T, [2, 0])
    _lib.check(_lib.load().irrl_eval_recurrence(_lib.ptr(sub), int(sub.shape[0]), 3, L.FRAME_FIRST, L.FRAME_EVERY, T, C.cast(C.pointer(st), C.c_void_p),
                                                counts.data_ptr() + 4 * pad, lag.data_ptr() + 4 * pad, matrix.data_ptr() + pad, _lib.stream_ptr(sub.device)))
    torch.cuda.synchronize()
    counts, lag, matrix = counts.cpu().numpy(), lag.cpu().numpy(), matrix.cpu().numpy()
    for buf, n in ((counts, 3 * 9), (lag, 3 * T), (matrix, 2 * T * T)):
        fill = buf[0]
        assert np.all(buf[:pad] == fill) and np.all(buf[pad + n:] == fill)
    assert np.array_equal(counts[pad:pad + 27].view(np.uint32).reshape(3, 9), full["counts"][1:4])
    assert np.array_equal(lag[pad:pad + 3 * T].view(np.uint32).reshape(3, T), full["lag"][1:4])
    assert np.array_equal(matrix[pad:pad + 2 * T * T].reshape(2, T, T), full["matrix"][[3, 1]])


# ---- (b) the closed loop ----
def _same_numbers(a, b):
    """two dicts of numbers: the same keys and values, NaN equal to NaN"""
    return set(a) == set(b) and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


MUS, DELAYS, CMD, WARM, STEPS = (0.8, 0.1), (0, 3), 2.0, 300, 256
NEW_KEYS = {"recurrence", "matrix", "body"}


def _sweep(**kw):
    cfg = load_env_cfg("bp5_manual_eval.yaml", num_envs=4)
    return EV.robustness_sweep(TP.ACTOR, cfg, MUS, DELAYS, [CMD], warm_steps=WARM, steps=STEPS, persistent="auto", **kw), cfg


def test_robustness_sweep_recurrence_and_default():
    """each row's matrix == the twin's levels on the row's own body recorder but for pairs on a level boundary (at most 1e-5 of the entries; about
    5e-4 pairs are expected among 262 144, i.e. none); the row's measures come from counts and lag words that equal the integer stage of the
    twin on the DEVICE's matrix exactly; without `recurrence` the rows have today's keys and the same bits as a second call and as these rows"""
    rows, cfg = _sweep(recurrence=SPEC, recurrence_frames=STEPS, record_body=True)
    assert len(rows) == 4
    dt = float(cfg["control_dt"])
    left_out = 0
    for r in rows:
        assert NEW_KEYS <= set(r) and r["body"].shape == (STEPS, 13) and r["matrix"].shape == (STEPS, STEPS) and r["matrix"].dtype == np.uint8
        body = r["body"][:, None, :]
        want = EV.recurrence_levels_numpy(body, SPEC)[0]
        edge = EV.recurrence_edges(body, SPEC)[0]
        left_out += int(edge.sum())
        assert np.array_equal(r["matrix"][~edge], want[~edge]), (r["mu"], r["delay"])
        counts, lag = EV.recurrence_from_levels(r["matrix"], None, SPEC, lags=STEPS // 2 + 1)
        assert _same_numbers(r["recurrence"], EV.recurrence_row(counts, lag, STEPS, SPEC, dt)), (r["mu"], r["delay"])
        assert r["recurrence"]["kept"] == STEPS
    print("pairs left out for a level boundary: %d of %d" % (left_out, 4 * STEPS * STEPS))
    assert left_out <= 1e-5 * 4 * STEPS * STEPS
    print(EV.sweep_table(rows, recurrence=True))
    # the C call itself on the device's recorder: counts and all lag words == the integer stage on its own matrix
    rec = torch.from_numpy(np.ascontiguousarray(np.stack([r["body"] for r in rows], 1))).cuda()
    res = EV.recurrence_to_numpy(EV.recurrence_device(rec, SPEC, matrix_env=(0, 1, 2, 3)))
    counts, lag = EV.recurrence_from_levels(res["matrix"], None, SPEC)
    assert np.array_equal(res["counts"], counts) and np.array_equal(res["lag"], lag)
    assert all(np.array_equal(res["matrix"][i], r["matrix"]) for i, r in enumerate(rows))
    plain, _ = _sweep()
    again, _ = _sweep()
    old = set(rows[0]) - NEW_KEYS
    for p, a, r in zip(plain, again, rows):
        assert set(p) == old and _same_numbers(p, a) and _same_numbers(p, {k: r[k] for k in old})
    with pytest.raises(ValueError):
        _sweep(recurrence=SPEC, recurrence_frames=STEPS + 1)
    with pytest.raises(ValueError):
        _sweep(recurrence_frames=STEPS)


def test_perturbation_study_recurrence():
    """perturbation_study(recurrence=..., recurrence_frames=64) on frictions 0.8 / 0.1 x 6 explorations, 300 warm-up + 80 post-kick frames: every
    row's [E] arrays are the measures of the twin on the last 64 frames of the row's own body recorder (a robot with a pair on a level boundary
    left out; at most one of the 12 may be); the older keys are those of a study without it, bit for bit; refused together with frame_chunk"""
    noise = dict(z_noise=0.002, roll_noise=0.025, pitch_noise=0.025, z_dot_noise=0.1, roll_dot_noise=0.1, pitch_dot_noise=0.1)
    cfg = load_env_cfg("bp5_manual_eval.yaml", num_envs=12)
    study = lambda **kw: EV.perturbation_study(TP.ACTOR, cfg, (0.8, 0.1), (0,), CMD, 6, noise, warm_steps=300, frames=80, seed=3, record_body=True,
                                               persistent="auto", **kw)
    rows, plain = study(recurrence=SPEC, recurrence_frames=64), study()
    T, dt, left_out = 64, float(cfg["control_dt"]), 0
    for r, p in zip(rows, plain):
        assert set(r) == set(p) | {"recurrence"} and r["body"].tobytes() == p["body"].tobytes() and r["falls"].tobytes() == p["falls"].tobytes()
        assert all(r["stats"][k].tobytes() == p["stats"][k].tobytes() for k in p["stats"])
        body = r["body"][-T:]
        want = EV.recurrence_numpy(body, SPEC, lags=T // 2 + 1)
        clean = ~EV.recurrence_edges(body, SPEC).any((1, 2))
        left_out += int((~clean).sum())
        m = EV.recurrence_measures(want["counts"], T, SPEC)
        per = EV.recurrence_period(want["lag"], T, L.W, dt)
        m.update(period_s=per["period_s"], period_fraction=per["period_fraction"], kept=want["counts"][:, 0].astype(np.int64))
        assert set(r["recurrence"]) == set(m)
        for k in m:
            assert r["recurrence"][k].shape == (6,) and np.array_equal(r["recurrence"][k][clean], m[k][clean], equal_nan=True), k
    assert left_out <= 1
    print(EV.perturbation_table(rows, recurrence=True))
    with pytest.raises(ValueError):
        study(recurrence=SPEC, frame_chunk=16)
    with pytest.raises(ValueError):
        study(recurrence=SPEC, recurrence_frames=81)
