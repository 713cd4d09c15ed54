"""Host side of the trace recorders (irrl_lstm_eval_traced / irrl_mlp_eval_traced) and of the correlation moments of two recorder windows
(irrl_eval_correlation): the C-ABI surface and the refusals before any HIP call, the stated size of `work`, the accumulation rule
(csrc/eval_elements.hpp) compiled as a stand-alone host program (tests/eval_correlation_main.cpp, plain serial loops in the stated order) under
the address and undefined-behaviour sanitizers and compared with the numpy twin byte for byte, the twin against a plain triple loop, the
correlation out of the moments against numpy and pandas, the planted pair -- no GPU needed.

The moments are f64 sums added in one stated order (and integers, and minima / maxima): equal means equal bits."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import eval_correlation_lib as L
from conftest import ROOT
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV

FF, FE = L.FRAME_FIRST, L.FRAME_EVERY


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "irrl_env.h")).read(), flags=re.S)


def _flat(s):
    return re.sub(r"\s+", " ", s).strip()


def _args(text, name, ret="int"):
    return _flat(re.search(r"\b%s %s\s*\((.*?)\);" % (ret, name), text, flags=re.S).group(1))


# ---- the C-ABI ----
def test_abi_surface_of_the_trace_and_the_correlation():
    """header == SIGNATURES for the four new symbols; the traced calls' lists are the measured calls' with the trace struct in front of the
    stream; the structs' ctypes mirrors have the header's fields in order, types and sizes; the limits agree; the unit is in the build"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib, build
    text = _header()
    for pol in ("lstm", "mlp"):
        measured, traced = _args(text, "irrl_%s_eval_measured" % pol), _args(text, "irrl_%s_eval_traced" % pol)
        assert traced == measured.replace(", void *hip_stream", ", const irrl_eval_trace *trace, void *hip_stream")
        m, t = _lib.SIGNATURES["irrl_%s_eval_measured" % pol], _lib.SIGNATURES["irrl_%s_eval_traced" % pol]
        assert t[0] is C.c_int and t[1] == m[1][:-1] + [C.c_void_p, C.c_void_p]
    args = _args(text, "irrl_eval_correlation")
    assert args == ("const float *x, const float *y, const uint8_t *rec_done, int rows, int num_envs, int conditions, int robots, int frame_first, "
                    "int frame_every, int frames, const irrl_eval_corr_spec *spec, int64_t *count, double *sx, double *sy, double *sxy, float *range_x, "
                    "float *range_y, double *work, void *hip_stream")
    kinds = lambda a: [C.c_int if x.strip().startswith("int ") else C.c_void_p for x in a.split(",")]
    assert _lib.SIGNATURES["irrl_eval_correlation"] == (C.c_int, kinds(args))
    assert _args(text, "irrl_eval_correlation_work", "size_t") == "int num_envs, const irrl_eval_corr_spec *spec"
    assert _lib.SIGNATURES["irrl_eval_correlation_work"] == (C.c_size_t, [C.c_int, C.c_void_p])
    body = re.search(r"typedef struct irrl_eval_trace \{(.*?)\} irrl_eval_trace;", text, flags=re.S).group(1)
    assert [_flat(d) for d in body.split(";") if d.strip()] == ["float *rec_lstm", "float *rec_value"]
    assert [(f[0], f[1]) for f in _lib.EvalTrace._fields_] == [("rec_lstm", C.c_void_p), ("rec_value", C.c_void_p)] and C.sizeof(_lib.EvalTrace) == 16
    body = re.search(r"typedef struct irrl_eval_corr_spec \{(.*?)\} irrl_eval_corr_spec;", text, flags=re.S).group(1)
    assert [_flat(d) for d in body.split(";") if d.strip()] == ["int x_dim, x_first, x_count, y_dim, y_first, y_count"]
    names = ("x_dim", "x_first", "x_count", "y_dim", "y_first", "y_count")
    assert [(f[0], f[1]) for f in _lib.EvalCorrSpec._fields_] == [(k, C.c_int) for k in names] and C.sizeof(_lib.EvalCorrSpec) == 24
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    assert (define("IRRL_EVAL_CORR_MAX_FRAMES"), define("IRRL_EVAL_CORR_MAX_X"), define("IRRL_EVAL_CORR_MAX_Y")) == \
        (EV.CORR_MAX_FRAMES, EV.CORR_MAX_X, EV.CORR_MAX_Y) == (16384, 64, 1024)
    assert build.PLAIN_UNITS[-1] == "eval_correlation.hip"
    assert EV.CORR_SOURCES == {"contact": ("gait", 24, 4), "torque": ("gait", 0, 12), "joint_rate": ("gait", 12, 12), "body": ("body", 0, 13),
                               "obs": ("obs_cond", 0, 35), "action": ("act_applied", 0, 12), "lstm": ("lstm", 0, None), "value": ("value", 0, 1)}
    assert EV.correlation_source("lstm", 48) == ("lstm", 192, 0, 192) and EV.correlation_source("contact") == ("gait", 32, 24, 4)
    assert EV.correlation_source("value") == ("value", 1, 0, 1) and EV.correlation_source("obs") == ("obs_cond", 35, 0, 35)
    assert "lstm" not in EV.RECORDERS and "value" not in EV.RECORDERS and EV.TRACE_RECORDERS == ("lstm", "value")


def test_correlation_refusals_and_work_before_any_hip_call():
    """every refusal fires, with the entry point's name in front of the text, although every pointer is a host address no HIP call could take;
    irrl_eval_correlation_work gives the stated value without a GPU"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib, build
    build.build()
    lib = _lib.load()
    some = C.create_string_buffer(64)
    ptr = C.c_void_p(C.addressof(some))
    S = dict(x_dim=32, x_first=24, x_count=4, y_dim=192, y_first=0, y_count=192)
    good = dict(x=ptr, y=ptr, rec_done=ptr, rows=10, num_envs=6, conditions=2, robots=3, frame_first=0, frame_every=1, frames=10, spec=S, count=ptr,
                sx=ptr, sy=ptr, sxy=ptr, range_x=ptr, range_y=ptr, work=ptr)

    def refused(**over):
        a = dict(good, **over)
        st = None if a["spec"] is None else _lib.EvalCorrSpec(**a["spec"])
        rc = lib.irrl_eval_correlation(a["x"], a["y"], a["rec_done"], a["rows"], a["num_envs"], a["conditions"], a["robots"], a["frame_first"], a["frame_every"],
                                       a["frames"], None if st is None else C.cast(C.pointer(st), C.c_void_p), a["count"], a["sx"], a["sy"], a["sxy"],
                                       a["range_x"], a["range_y"], a["work"], None)
        text = _lib.last_error()
        assert rc != 0 and text.startswith("irrl_eval_correlation: "), (over, rc, text)
        return text

    for k in ("x", "y", "spec", "count", "sx", "sy", "sxy"):
        assert "NULL" in refused(**{k: None}), k
    assert "x window" in refused(spec=dict(S, x_first=29))
    assert "x window" in refused(spec=dict(S, x_first=-1))
    assert "y window" in refused(spec=dict(S, y_first=1))
    assert "y window" in refused(spec=dict(S, y_dim=191))
    assert "x_dim" in refused(spec=dict(S, x_dim=0))
    assert "x_count" in refused(spec=dict(S, x_count=0))
    assert "x_count" in refused(spec=dict(S, x_dim=100, x_first=0, x_count=65))
    assert "y_count" in refused(spec=dict(S, y_count=0))
    assert "y_count" in refused(spec=dict(S, y_dim=2000, y_count=1025))
    assert "conditions * robots" in refused(conditions=4)
    assert "conditions * robots" in refused(conditions=0)
    assert "conditions * robots" in refused(robots=0, conditions=6)
    assert "num_envs" in refused(num_envs=0)
    assert "16384" in refused(frames=0)
    assert "16384" in refused(frames=-1)
    assert "16384" in refused(frames=16385, rows=40000)
    assert "frame_every" in refused(frame_first=-1)
    assert "frame_every" in refused(frame_every=0)
    assert "past the recorder" in refused(frame_first=1)
    assert "past the recorder" in refused(frame_every=2)
    assert "past the recorder" in refused(frames=11)
    assert "work" in refused(work=None)

    def work(n, s):
        st = None if s is None else _lib.EvalCorrSpec(**s)
        return lib.irrl_eval_correlation_work(n, None if st is None else C.cast(C.pointer(st), C.c_void_p))
    assert work(6, S) == 6 * (4 * 192 + 3 * 4 + 3 * 192 + 1) == EV.correlation_work(6, S)
    assert work(4096, dict(S, x_dim=35, x_first=0, x_count=35, y_dim=35, y_count=35)) == 4096 * (35 * 35 + 6 * 35 + 1)
    assert work(0, S) == 0 and work(6, None) == 0 and work(6, dict(S, x_count=65)) == 0


def test_trace_refusals_before_any_hip_call():
    """a trace whose two pointers are NULL, and rec_lstm for an MlpPolicy, are refused with the entry point's name in the text -- with a NULL
    handle and NULL everywhere else, so no HIP call can have been made; a NULL trace falls through to the measured call's own checks"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib, build
    build.build()
    lib = _lib.load()
    some = C.create_string_buffer(64)
    addr = C.addressof(some)

    def call(name, trace):
        kinds = _lib.SIGNATURES[name][1]
        args = [0 if k is C.c_int or k is C.c_longlong else 0.0 if k is C.c_float else None for k in kinds]
        args[-2] = None if trace is None else C.cast(C.pointer(trace), C.c_void_p)
        rc = getattr(lib, name)(*args)
        return rc, _lib.last_error()

    for name in ("irrl_lstm_eval_traced", "irrl_mlp_eval_traced"):
        rc, text = call(name, _lib.EvalTrace(rec_lstm=None, rec_value=None))
        assert rc != 0 and text.startswith(name + ": ") and "both NULL" in text, text
        rc, text = call(name, None)
        assert rc != 0 and text == name + ": NULL handle", text
        rc, text = call(name, _lib.EvalTrace(rec_lstm=None, rec_value=addr))
        assert rc != 0 and text == name + ": NULL handle", text
    rc, text = call("irrl_mlp_eval_traced", _lib.EvalTrace(rec_lstm=addr, rec_value=addr))
    assert rc != 0 and text.startswith("irrl_mlp_eval_traced: ") and "no recurrent state" in text, text
    rc, text = call("irrl_lstm_eval_traced", _lib.EvalTrace(rec_lstm=addr, rec_value=None))
    assert rc != 0 and text == "irrl_lstm_eval_traced: NULL handle", text


def test_spec_and_twin_refusals():
    S = L.spec("contact_lstm")
    for bad, word in ((dict(x_count=0), "x_count"), (dict(x_dim=100, x_first=0, x_count=65), "x_count"), (dict(y_dim=2000, y_count=1025), "y_count"),
                      (dict(x_first=29), "x window"), (dict(y_first=1), "y window"), (dict(y_dim=0), "y_dim")):
        with pytest.raises(ValueError, match=word):
            EV.correlation_spec(**dict(S, **bad))
    x, y, done = L.case(5, "contact_lstm")
    with pytest.raises(ValueError, match="conditions"):
        EV.correlation_numpy(x, y, done, S, 2, FF, FE, 5)
    with pytest.raises(ValueError, match="frames"):
        EV.correlation_numpy(x, y, done, S, 5, FF, FE, 0)
    with pytest.raises(ValueError):
        EV.correlation_numpy(x, y, done, S, 5, FF, FE, 7)          # past the recorder's rows
    with pytest.raises(ValueError, match="float32"):
        EV.correlation_numpy(x.astype(np.float64), y, done, S, 5, FF, FE, 5)


# ---- the host program on the shared element functions ----
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host program"
    out = str(tmp_path_factory.mktemp("eval_correlation_main") / "eval_correlation_main")
    csrc = os.path.join(ROOT, "high_speed_quadrupedal_locomotion_by_irrl_amd", "csrc")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=on", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                           "-I" + csrc, os.path.join(ROOT, "tests", "eval_correlation_main.cpp"), "-o", out])
    return out


def run_program(program, tmp_path, x, y, done, s, conditions, T):
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    L.write_case(src, x, y, done, s, conditions, FF, FE, T)
    r = subprocess.run([program, src, dst], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    return L.read_result(dst, conditions, s)


@pytest.mark.parametrize("T,window,N,conditions", L.cases())
def test_program_equals_the_twin_byte_for_byte(program, tmp_path, T, window, N, conditions):
    """the sanitized program's serial loops over the header's text == the twin on all six outputs, with and without rec_done; T_e is what the
    case planted; the constant columns' ranges are exact"""
    x, y, done = L.case(T, window, N)
    s = L.spec(window)
    for with_done in (True, False):
        want = L.twin(T, window, N, conditions, with_done)
        got = run_program(program, tmp_path, x, y, done if with_done else None, s, conditions, T)
        L.same_bytes(got, want, (T, window, N, conditions, with_done))
        assert got["work_per_env"] * N == EV.correlation_work(N, s)
        te = L.expected_te(done, T) if with_done else np.full(N, T)
        assert np.array_equal(want["count"], te.reshape(conditions, N // conditions).sum(1))
        if s["x_count"] >= 3:
            seen = want["count"] > 0
            assert np.all(want["range_x"][seen, 1] == np.float32(0.0)) and np.all(want["range_x"][seen, 2] == np.float32(0.3))
            assert np.all(want["range_x"][~seen, :, 0] == np.inf) and np.all(want["range_x"][~seen, :, 1] == -np.inf)
            assert np.all(want["sx"][:, 1] == 0.0) and np.all(want["sxy"][:, 1] == 0.0) and not np.any(np.signbit(want["sxy"][:, 1]))


def test_spec_refusal_inside_the_sanitized_program(program, tmp_path):
    x, y, done = L.case(2, "one")
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    L.write_case(src, x, y, done, dict(L.spec("one"), x_count=2), 5, FF, FE, 2)
    r = subprocess.run([program, src, dst], stderr=subprocess.PIPE)
    assert r.returncode == 3 and b"x window" in r.stderr and not os.path.exists(dst)


# ---- the twin against plain loops ----
@pytest.mark.parametrize("T,window,N,conditions", [c for c in L.cases() if c[0] <= 65 and c[2] <= 6])
def test_twin_equals_a_plain_triple_loop(T, window, N, conditions):
    """robot by robot, frame by frame, pair by pair in Python floats: s = s + a * b from 0.0, then the condition's robots in order"""
    x, y, done = L.case(T, window, N)
    s = L.spec(window)
    want = L.twin(T, window, N, conditions)
    cx, cy, R = s["x_count"], s["y_count"], N // conditions
    te = L.expected_te(done, T)
    for g in range(conditions):
        sxy = [[0.0] * cy for _ in range(cx)]
        sx, sy = [[0.0, 0.0] for _ in range(cx)], [[0.0, 0.0] for _ in range(cy)]
        for e in range(g * R, (g + 1) * R):
            pxy = [[0.0] * cy for _ in range(cx)]
            px, py = [[0.0, 0.0] for _ in range(cx)], [[0.0, 0.0] for _ in range(cy)]
            for i in range(te[e]):
                xr = [float(v) for v in x[FF + FE * i, e, s["x_first"]:s["x_first"] + cx]]
                yr = [float(v) for v in y[FF + FE * i, e, s["y_first"]:s["y_first"] + cy]]
                for c, a in enumerate(xr):
                    px[c][0] = px[c][0] + a
                    px[c][1] = px[c][1] + a * a
                    row = pxy[c]
                    for j, b in enumerate(yr):
                        row[j] = row[j] + a * b
                for j, b in enumerate(yr):
                    py[j][0] = py[j][0] + b
                    py[j][1] = py[j][1] + b * b
            sxy = [[t + p for t, p in zip(tr, pr)] for tr, pr in zip(sxy, pxy)]
            sx = [[t[0] + p[0], t[1] + p[1]] for t, p in zip(sx, px)]
            sy = [[t[0] + p[0], t[1] + p[1]] for t, p in zip(sy, py)]
        assert np.asarray(sxy, np.float64).tobytes() == want["sxy"][g].tobytes(), g
        assert np.asarray(sx, np.float64).tobytes() == want["sx"][g].tobytes() and np.asarray(sy, np.float64).tobytes() == want["sy"][g].tobytes(), g


# ---- the correlation out of the moments ----
# The tolerance is derived, not measured: every sum carries at most n 2^-53 relative error, which the differences n sxy - sx sy amplify by at most
# 1 + mean^2 / sigma^2 <= 101 for the generated columns (|mean| <= 10 sigma); at n <= 7e4 that is about 3e-9, and the tolerance is thirty times it.
CORR_TOL = 1e-7


@pytest.mark.parametrize("T,window,N,conditions", [(1000, "contact_lstm", 5, 1), (1000, "contact_lstm", 5, 5), (257, "tiles", 6, 2), (1000, "obs_obs", 5, 1),
                                                   (65, "contact_lstm", 70, 1), (2, "tiles", 5, 5), (64, "one", 70, 1)])
def test_correlation_from_moments_against_numpy(T, window, N, conditions):
    x, y, done = L.case(T, window, N)
    s = L.spec(window)
    m = L.twin(T, window, N, conditions)
    res = EV.correlation_from_moments(m)
    cx = s["x_count"]
    checked = 0
    for g in range(conditions):
        xs, ys = L.pooled(x, y, done, s, conditions, g, T)
        assert len(xs) == m["count"][g] == res["count"][g]
        if len(xs) < 2:
            assert np.all(np.isnan(res["r"][g])) and np.all(np.isnan(res["cov"][g]))
            continue
        flat_x, flat_y = xs.min(0) == xs.max(0), ys.min(0) == ys.max(0)
        if cx >= 3:
            assert flat_x[1] and flat_x[2]                       # 0.0 and 0.3: the latter is not to be mistaken for a varying column
        with np.errstate(invalid="ignore", divide="ignore"):
            ref = np.corrcoef(np.concatenate([xs, ys], 1), rowvar=False)[:cx, cx:]
        live = ~flat_x[:, None] & ~flat_y[None, :]
        assert np.all(np.isnan(res["r"][g][~live])) and np.all(np.isfinite(res["r"][g][live]))
        err = np.abs(res["r"][g][live] - ref[live]).max() if live.any() else 0.0
        print("condition %d: n = %d, max |r - numpy| = %.3g" % (g, len(xs), err))
        assert err <= CORR_TOL
        cov = np.cov(np.concatenate([xs, ys], 1), rowvar=False)[:cx, cx:]
        scale = np.sqrt(np.outer(xs.var(0, ddof=1), ys.var(0, ddof=1)))
        assert np.all(np.abs(res["cov"][g] - cov)[live] <= CORR_TOL * scale[live])
        assert np.allclose(res["mean_x"][g], xs.mean(0), rtol=1e-12, atol=1e-12) and np.allclose(res["mean_y"][g], ys.mean(0), rtol=1e-12, atol=1e-12)
        checked += int(live.sum())
    assert checked > 0
    # without the ranges the constant columns are found by the variance: 0.0 is, 0.3 may or may not be -- which is why the ranges exist
    loose = EV.correlation_from_moments(dict(m, range_x=None, range_y=None))
    both = np.isfinite(res["r"]) & np.isfinite(loose["r"])
    assert np.array_equal(res["r"][both], loose["r"][both])
    if cx >= 3:
        assert np.all(np.isnan(loose["r"][:, 1]))


def test_correlation_against_pandas():
    import pandas as pd
    T, window, N, conditions = 257, "contact_lstm", 5, 1
    x, y, done = L.case(T, window, N)
    s = L.spec(window)
    res = EV.correlation_from_moments(L.twin(T, window, N, conditions))
    xs, ys = L.pooled(x, y, done, s, conditions, 0, T)
    ref = pd.DataFrame(np.concatenate([xs, ys], 1)).corr().to_numpy()[:4, 4:]
    assert np.array_equal(np.isnan(ref), np.isnan(res["r"][0])) and np.isnan(ref[1]).all() and np.isnan(ref[2]).all()
    ok = ~np.isnan(ref)
    assert ok.sum() == 2 * 192 and np.abs(ref[ok] - res["r"][0][ok]).max() <= CORR_TOL


def test_correlation_row_names_the_planted_pair():
    """y column 2 * 48 + 17 = layer 2's cell 17 is the contact flag of leg 2 plus noise: the row names leg HR and unit (2, "c", 17)"""
    rng = np.random.RandomState(5)
    T, N, hid = 400, 3, 48
    gait = rng.normal(size=(T, N, 32)).astype(np.float32)
    gait[:, :, 24:28] = rng.randint(0, 2, size=(T, N, 4))
    lstm = rng.normal(size=(T, N, 4 * hid)).astype(np.float32)
    lstm[:, :, 2 * hid + 17] = -gait[:, :, 26] + 0.2 * rng.normal(size=(T, N)).astype(np.float32)
    src = [EV.correlation_source(k, hid) for k in ("contact", "lstm")]
    s = EV.correlation_spec(src[0][1], src[0][2], src[0][3], src[1][1], src[1][2], src[1][3])
    for conditions in (N, 1):
        m = EV.correlation_numpy(gait, lstm, None, s, conditions)
        for g in range(conditions):
            row = EV.correlation_row(m, ("contact", "lstm"), g)
            assert row["corr_leg"] == EV.FOOTFALL_LEGS[2] == "HR" and row["corr_unit"] == (2, "c", 17), row
            assert 0.85 < row["corr_max"] <= 1.0 and row["corr_r"] == -row["corr_max"]
    assert EV.correlation_unit("lstm", 0, 192) == (1, "c", 0) and EV.correlation_unit("lstm", 48, 192) == (1, "h", 0)
    assert EV.correlation_unit("lstm", 191, 192) == (2, "h", 47) and EV.correlation_unit("obs", 7, 35) == ("obs", 7)
    flat = EV.correlation_numpy(np.zeros((4, 1, 32), np.float32), lstm[:4, :1], None, s)
    assert EV.correlation_row(flat, ("contact", "lstm")) == dict(corr_max=pytest.approx(float("nan"), nan_ok=True),
                                                                  corr_r=pytest.approx(float("nan"), nan_ok=True), corr_leg=None, corr_unit=None)
    m = EV.correlation_numpy(gait, gait, None, EV.correlation_spec(32, 0, 12, 32, 12, 12), 1)
    row = EV.correlation_row(m, ("torque", "joint_rate"))
    assert row["corr_leg"][0] == "torque" and row["corr_unit"][0] == "joint_rate"


def test_sweep_table_gains_the_three_columns():
    base = dict(mu=0.8, delay=0, cmd=2.0, falls=0, vx_body_mean=1.9, vx_body_std=0.1, z_mean=0.3, z_std=0.01, roll_std=0.01, pitch_mean=0.0,
                pitch_std=0.01, yaw_rate_mean=0.0)
    rows = [dict(base, corr_max=0.61, corr_r=-0.61, corr_leg="HR", corr_unit=(2, "c", 17)), dict(base, corr_max=float("nan"), corr_leg=None, corr_unit=None)]
    plain, table = EV.sweep_table(rows).split("\n"), EV.sweep_table(rows, correlation=True).split("\n")
    assert [t.startswith(p) for p, t in zip(plain, table)] == [True] * 3
    assert table[0].split()[-3:] == ["corr_max", "corr_leg", "corr_unit"] == list(EV.CORRELATION_TABLE_KEYS)
    assert table[1].split()[-3:] == ["+0.6100", "HR", "2:c:17"] and table[2].split()[-3:] == ["+nan", "-", "-"]
