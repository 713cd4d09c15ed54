"""Host side of the evaluation scenario (irrl_lstm_eval_scenario[_persistent]: command schedule, heading hold, statistics buckets): the C-ABI surface
and the refusals before any HIP call, the per-element arithmetic both device forms share (csrc/eval_elements.hpp) compiled as a stand-alone host
program (tests/eval_scenario_main.cpp) under the address and undefined-behaviour sanitizers and compared with the numpy twins, and the twins'
own keywords -- no GPU needed.

Case shape: N = 19, T = 60, D = 6, S = 5 command rows held 7 steps, B = 3 buckets of 16 steps, t0 = 4 (row 4 and bucket 2 are reached and held),
done with p = 0.05, yaw tracks spanning -3.3 .. 3.3 rad (several envs cross +-pi), heading gains zero on the envs e % 5 == 4.  The struct has ONE
windup W per scenario; it is small (0.125) here, so the envs with a sustained heading error reach the clamp and the others do not."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
from conftest import GOLDEN, ROOT, load_env_cfg
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV
from high_speed_quadrupedal_locomotion_by_irrl_amd.checkpoint import NumpyLstmActor
from high_speed_quadrupedal_locomotion_by_irrl_amd.helper import obs_normalisation

N, D, T = 19, 6, 60
S, CMD_EVERY, B, STAT_EVERY, T0 = 5, 7, 3, 16, 4
W = 0.125
DELAYS = np.arange(N) % D
CMDS = np.linspace(0.5, 5.0, N)
OFF = np.arange(N) % 5 == 4                   # envs without the heading hold
NS = len(EV.STAT_SLOTS)


# ---- the C-ABI ----
def test_scenario_abi_surface_and_refusals_before_any_hip_call():
    """header == SIGNATURES == exports for the two new entry points (the old argument lists with `const irrl_eval_scenario *` in front of the
    stream), the struct's ctypes mirror has the header's fields in order, and a NULL handle and every bad scenario are refused -- with the entry
    point's name in the text -- before a handle is ever dereferenced"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "irrl_env.h")).read(), flags=re.S)
    flat = lambda s: re.sub(r"\s+", " ", s).strip()
    for old, new in (("irrl_lstm_eval_rollout", "irrl_lstm_eval_scenario"), ("irrl_lstm_eval_rollout_persistent", "irrl_lstm_eval_scenario_persistent")):
        a = flat(re.search(r"\bint %s\s*\((.*?)\);" % old, text, flags=re.S).group(1))
        b = flat(re.search(r"\bint %s\s*\((.*?)\);" % new, text, flags=re.S).group(1))
        assert a.endswith(", void *hip_stream") and b == a[:-len("void *hip_stream")] + "const irrl_eval_scenario *scenario, void *hip_stream"
        assert _lib.SIGNATURES[new] == (_lib.SIGNATURES[old][0], _lib.SIGNATURES[old][1][:-1] + [C.c_void_p, C.c_void_p])
    body = re.search(r"typedef struct irrl_eval_scenario \{(.*?)\} irrl_eval_scenario;", text, flags=re.S).group(1)
    fields = [re.findall(r"\w+", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert fields == [f[0] for f in _lib.EvalScenario._fields_], fields
    build.build()
    lib = _lib.load()
    three = (C.c_float * 3)(0.0, 0.0, 0.0)
    some = C.create_string_buffer(64)                      # any non-NULL address: nothing reads it before the checks are through
    ptr = C.c_void_p(C.addressof(some))
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    table = (C.c_void_p * 12)(*[C.addressof(some)] * 12)
    good = dict(t0=0, cmd_rows=1, cmd_every=1, cmd_table=ptr.value, stat_buckets=1, stat_every=1, heading_ref=ptr.value, heading_kp=ptr.value,
                heading_ki=ptr.value, heading_int=ptr.value, heading_windup=1.0, heading_dt=0.002)
    bad = [(dict(cmd_rows=0), "cmd_rows"), (dict(cmd_every=0), "cmd_every"), (dict(stat_buckets=0), "stat_buckets"), (dict(stat_every=-1), "stat_every"),
           (dict(cmd_table=None), "cmd_table"), (dict(heading_kp=None), "all given or all NULL"), (dict(heading_ref=None, heading_ki=None), "all given or all NULL"),
           (dict(heading_int=None), "heading_int"), (dict(heading_windup=-0.5), "heading_windup"), (dict(heading_dt=0.0), "heading_dt")]
    for name in ("irrl_lstm_eval_scenario", "irrl_lstm_eval_scenario_persistent"):
        fn = getattr(lib, name)
        n_args = len(_lib.SIGNATURES[name][1])

        def call(handle, scenario):
            args = [None] * n_args
            args[0:6] = [handle, 1, 0, 48, 35, 12]
            args[6] = C.cast(table, C.c_void_p)
            args[7:12] = [ptr] * 5
            args[12] = 1
            args[13:23] = [ptr] * 10
            args[23:26] = [1.0, 1.0, 1.0]
            args[26:29] = [three, three, 1]
            args[-2] = None if scenario is None else C.cast(C.pointer(scenario), C.c_void_p)
            return fn(*args)

        assert call(None, None) != 0
        assert _lib.last_error() == name + ": NULL handle"
        for change, word in bad:
            assert call(fake, _lib.EvalScenario(**dict(good, **change))) != 0, change
            assert word in _lib.last_error() and _lib.last_error().startswith(name + ":"), (change, _lib.last_error())


# ---- the per-element functions on the host ----
def _build(tmp_path_factory, name):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host program"
    out = str(tmp_path_factory.mktemp(name) / name)
    csrc = os.path.join(ROOT, "high_speed_quadrupedal_locomotion_by_irrl_amd", "csrc")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-I" + csrc,
                           os.path.join(ROOT, "tests", name + ".cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory, "eval_scenario_main")


def _quaternion(yaw, roll, pitch):
    """ZYX Euler angles -> w x y z"""
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], -1)


def _case(seed):
    """random raw observations, done flags (p = 0.05), actions in [-1, 1], body frames whose yaw follows a track of its own per env (row 0 of
    `q`: the quaternion in front of step 0), a 5-row command table, heading references within 2.3 rad of the track"""
    rng = np.random.RandomState(seed)
    y0 = np.linspace(-3.3, 3.3, N)
    track = y0[None] + 0.3 * np.sin(2 * np.pi * np.arange(T + 1)[:, None] / T + np.arange(N)[None])            # [T + 1, N], unwrapped
    q = _quaternion(track, 0.05 * rng.normal(size=(T + 1, N)), 0.05 * rng.normal(size=(T + 1, N))).astype(np.float32)
    body = np.concatenate([rng.normal(size=(T, N, 2)), 0.28 + 0.01 * rng.normal(size=(T, N, 1)), q[1:], rng.normal(size=(T, N, 6))], 2).astype(np.float32)
    done = rng.uniform(size=(T, N)) < 0.05
    assert done.any()
    ref = (y0 + rng.uniform(-2.0, 2.0, size=N)).astype(np.float32)
    yaw = EV.yaw_from_quaternion(q)
    err = EV.wrap_angle(ref.astype(np.float64)[None] - yaw)
    # nearer pi the f32 and the f64 wrap may legitimately pick opposite branches: the inputs stay inside
    assert np.abs(err).max() < 3.0
    crossed = (np.abs(np.diff(yaw, axis=0)) > np.pi).any(0)
    assert crossed.sum() >= 3, "several envs cross +-pi"
    table = np.stack([(r + 1) / S * CMDS[None].T * np.array([1.0, 0.1, -0.05])[None] for r in range(S)], 0).astype(np.float32)     # [S, N, 3]
    return dict(ob_reset=rng.normal(size=(N, 35)).astype(np.float32), raw=rng.normal(size=(T, N, 35)).astype(np.float32), done=done,
                action=rng.uniform(-1, 1, size=(T, N, 12)).astype(np.float32), body=body, q=q, yaw=yaw, table=table, ref=ref,
                kp=np.where(OFF, 0.0, np.linspace(0.5, 1.5, N)).astype(np.float32), ki=np.where(OFF, 0.0, 0.1 + 0.05 * (np.arange(N) % 3)).astype(np.float32))


def _run(program, tmp_path, case, a_cmd, a_vel, a_act, mean, std, dt):
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    target = np.stack([CMDS, np.zeros(N), np.zeros(N)], 1).astype(np.float32)
    with open(src, "wb") as f:
        f.write(np.array([N, D, T, S, CMD_EVERY, B, STAT_EVERY, T0], np.int32).tobytes())
        f.write(np.array([a_cmd, a_vel, a_act] + list(mean) + list(std) + [W, dt], np.float32).tobytes())
        f.write(DELAYS.astype(np.int32).tobytes())
        for k in (target, case["table"], case["ref"], case["kp"], case["ki"], case["ob_reset"], case["q"][0], case["raw"], case["done"].astype(np.uint8),
                  case["action"], case["body"]):
            f.write(np.ascontiguousarray(k).tobytes())
    subprocess.check_call([program, src, dst])
    blob = open(dst, "rb").read()
    out, at = {}, 0
    for k, shape, dt_ in (("cond", (T, N, 35), np.float32), ("applied", (T, N, 12), np.float32), ("stats", (B, NS, N), np.float64), ("cmd", (N, 3), np.float32),
                          ("vel_his", (N, 35), np.float32), ("I_cond", (T, N), np.float32), ("I_end", (T, N), np.float32), ("row", (T,), np.int32),
                          ("bucket", (T,), np.int32)):
        n = int(np.prod(shape)) * np.dtype(dt_).itemsize
        out[k] = np.frombuffer(blob[at:at + n], dt_).reshape(shape)
        at += n
    assert at == len(blob)
    return out


def _setup():
    cfg = load_env_cfg("bp5_manual_eval.yaml")
    mean, std, _, _ = obs_normalisation(cfg)
    return cfg, mean, std, float(cfg["control_dt"])


def test_schedule_rows_and_buckets_are_exact_and_route_with_the_filters_off(program, tmp_path):
    """filters off: the row index and the bucket index of every step are min(max(t - t0, 0) // every, rows - 1), the last row holds; the command
    elements ARE the scaled table rows bit for bit (element 2 on the heading-off envs), elements 3-34 the delay line's"""
    cfg, mean, std, dt = _setup()
    case = _case(21)
    got = _run(program, tmp_path, case, 1.0, 1.0, 1.0, mean[0:3], std[0:3], dt)
    rows = np.array([min(max(t - T0, 0) // CMD_EVERY, S - 1) for t in range(T)])
    buckets = np.array([min(max(t - T0, 0) // STAT_EVERY, B - 1) for t in range(T)])
    assert np.array_equal(got["row"], rows) and np.array_equal(got["bucket"], buckets)
    assert rows[0] == rows[T0 + CMD_EVERY - 1] == 0 and rows[T0 + CMD_EVERY] == 1 and (rows[T0 + CMD_EVERY * (S - 1):] == S - 1).all() and T - T0 > CMD_EVERY * S
    assert np.array_equal(rows, [EV.schedule_row(t, T0, CMD_EVERY, S) for t in range(T)])
    scaled = (case["table"] - np.asarray(mean[0:3], np.float32)) / np.asarray(std[0:3], np.float32)
    assert np.array_equal(got["cond"][:, :, 0:2].view(np.uint32), scaled[rows][:, :, 0:2].view(np.uint32))
    assert np.array_equal(got["cond"][:, OFF, 2].view(np.uint32), scaled[rows][:, OFF, 2].view(np.uint32))
    assert not np.array_equal(got["cond"][:, ~OFF, 2], scaled[rows][:, ~OFF, 2])
    src = np.concatenate([case["ob_reset"][None], case["raw"]], 0)
    for t in range(T):
        want = src[np.maximum(t - DELAYS, 0), np.arange(N)]
        assert np.array_equal(got["cond"][t, :, 3:].view(np.uint32), want[:, 3:].view(np.uint32)), t


def test_scenario_elements_on_the_host_equal_the_numpy_twins(program, tmp_path):
    """filters at 1 / 50 / 30 Hz, under ASan + UBSan, against evaluate.condition with the scenario's keywords.  Elements 3-34 and the command
    elements within the bounds tests/test_eval_persistent_host.py derives for the same quantities (2e-5, 2e-4).  The heading element within 2e-5:
    atan2f is within a few ulp of pi (2.4e-7 each), the wrap and the gains keep that size, 60 integrator roundings stay below 1 ulp of W each
    (1.5e-8), and element 2 is out / std2 -- an f32 / f64 prototype of this case shape gave 1.2e-6 at |out| ~ 1.  I is zero behind a `done` and
    never leaves [-W, W]; the envs with a sustained error sit ON the clamp.  Each bucket's statistics equal body_statistics of that bucket's
    frames: means 1e-9 absolute, standard deviations 1e-6 relative; frames per bucket and falls exact."""
    cfg, mean, std, dt = _setup()
    a_cmd, a_vel, a_act = (float(np.float32(EV.lowpass_alpha(dt, f))) for f in (1.0, 50.0, 30.0))
    case = _case(22)
    got = _run(program, tmp_path, case, a_cmd, a_vel, a_act, mean[0:3], std[0:3], dt)
    heading = EV.heading_parameters(dict(ref=case["ref"], kp=case["kp"], ki=case["ki"], windup=W), N, float(cfg["Omega"]), dt)
    target = np.stack([CMDS, np.zeros(N), np.zeros(N)], 1)
    st = EV.condition_state(case["ob_reset"], D)
    rows, integ = [], []
    for t in range(T):
        rows.append(EV.condition(st, t, case["ob_reset"] if t == 0 else case["raw"][t - 1], DELAYS, target, a_cmd, a_vel, mean[0:3], std[0:3],
                                 cmd_schedule=case["table"], cmd_every=CMD_EVERY, heading=heading, t0=T0, yaw=case["yaw"][t]))
        integ.append(st["heading_int"].copy())
        st["cmd"][case["done"][t]] = 0.0
        st["heading_int"][case["done"][t]] = 0.0
    want, integ = np.stack(rows), np.stack(integ)
    cmd_el = np.ones((N, 3), bool)
    cmd_el[~OFF, 2] = False                                   # element 2 of a heading-on env is the heading element
    worst = (np.abs(want[:, :, 3:] - got["cond"][:, :, 3:]).max(), np.abs(want[:, :, 0:3] - got["cond"][:, :, 0:3])[:, cmd_el].max(),
             np.abs(want[:, ~OFF, 2] - got["cond"][:, ~OFF, 2]).max(), np.abs(integ - got["I_cond"]).max())
    print("max |host program - numpy|: elements 3-34 %.3g, command elements %.3g, heading element %.3g (|element| up to %.2f), integrator %.3g"
          % (worst[0:3] + (np.abs(want[:, ~OFF, 2]).max(), worst[3])))
    assert worst[0] <= 2e-5 and worst[1] <= 2e-4 and worst[2] <= 2e-5
    assert np.abs(st["cmd"] - got["cmd"]).max() <= 2e-4 and np.abs(st["vel_his"] - got["vel_his"]).max() <= 2e-5
    # the integrator: zero behind a done, off envs never move, inside the clamp, and ON it where the error is sustained
    assert np.all(got["I_end"][case["done"]] == 0.0) and np.all(got["I_cond"][:, OFF] == 0.0)
    assert np.abs(got["I_cond"]).max() <= np.float32(W)
    on_clamp = (np.abs(got["I_cond"]) == np.float32(W)).any(0)
    assert on_clamp.any() and (~on_clamp[~OFF]).any(), on_clamp
    assert np.array_equal(on_clamp, (np.abs(integ) == W).any(0))
    # statistics per bucket
    buckets = np.array([min(max(t - T0, 0) // STAT_EVERY, B - 1) for t in range(T)])
    worst_s = {}
    for b in range(B):
        stats = EV.statistics_from_sums(got["stats"][b])
        sel = buckets == b
        for e in range(N):
            for k, v in EV.body_statistics(case["body"][sel, e]).items():
                if k == "vx_body":
                    continue
                err = abs(stats[k][e] - v) if k.endswith("_mean") else abs(stats[k][e] - v) / abs(v)
                worst_s[k] = max(worst_s.get(k, 0.0), err)
        assert np.all(stats["frames"] == sel.sum()) and np.array_equal(stats["falls"], case["done"][sel].sum(0))
    assert [int((buckets == b).sum()) for b in range(B)] == [T0 + STAT_EVERY, STAT_EVERY, T - T0 - 2 * STAT_EVERY]
    print("worst |host program - body_statistics| per bucket (means absolute, stds relative):", {k: "%.2e" % v for k, v in worst_s.items()})
    for k, v in worst_s.items():
        assert v <= (1e-9 if k.endswith("_mean") else 1e-6), (k, v)


def test_a_neutral_scenario_is_todays_path_bit_for_bit(program, tmp_path_factory, tmp_path):
    """gains zero everywhere and every table row equal to cmd_target: what the scenario program writes equals what the program of the loop without
    a scenario (tests/eval_elements_main.cpp, untouched) writes for the same recording, bit for bit, the bucket sums added in bucket order"""
    import test_eval_persistent_host as TP
    plain = _build(tmp_path_factory, "eval_elements_main")
    cfg, mean, std, dt = _setup()
    a_cmd, a_vel, a_act = (float(np.float32(EV.lowpass_alpha(dt, f))) for f in (1.0, 50.0, 30.0))
    case = _case(23)
    target = np.stack([CMDS, np.zeros(N), np.zeros(N)], 1).astype(np.float32)
    case.update(table=np.repeat(target[None], S, 0), kp=np.zeros(N, np.float32), ki=np.zeros(N, np.float32))
    got = _run(program, tmp_path, case, a_cmd, a_vel, a_act, mean[0:3], std[0:3], dt)
    assert (TP.N, TP.D, TP.T) == (N, D, T) and np.array_equal(TP.CMDS, CMDS)
    old = TP._run(plain, tmp_path, case, a_cmd, a_vel, a_act, mean[0:3], std[0:3])
    for k in ("cond", "applied", "cmd", "vel_his"):
        assert np.array_equal(got[k].view(np.uint32), old[k].view(np.uint32)), k
    assert np.all(got["I_cond"] == 0.0)
    # one window against three: the counts and the falls are exact, the sums agree to the rounding of a different association
    assert np.array_equal(got["stats"][:, [0, NS - 1]].sum(0), old["stats"][[0, NS - 1]])
    assert np.allclose(got["stats"].sum(0), old["stats"], rtol=1e-13, atol=1e-13)


# ---- the twins' keywords ----
def test_staircase_schedule_is_the_scripts_line():
    """run_bp_v5.py:383-388: temp_vel_cmd = (t // (100 * 50) + 1) / 4 * flag_fix_cmd for t < 100 * 50 * 4, the full command afterwards"""
    cmds = np.array([5.0, 3.2, 0.7])
    table = EV.staircase_schedule(cmds, 4)
    assert table.shape == (4, 3, 3) and np.all(table[:, :, 1:] == 0.0)
    for t in (0, 1, 4999, 5000, 9999, 10000, 15000, 19999, 20000, 50000):
        line = ((t // (100 * 50) + 1) / 4 * cmds) if t < 100 * 50 * 4 else cmds
        assert np.array_equal(table[EV.schedule_row(t, 0, 5000, 4), :, 0], line), t
    assert np.array_equal(EV.staircase_schedule(np.array([[1.0, 0.5, -0.2]]), 2), np.array([[[0.5, 0.25, -0.1]], [[1.0, 0.5, -0.2]]]))
    assert abs(EV.yaw_from_quaternion([np.cos(0.35), 0.0, 0.0, np.sin(0.35)]) - 0.7) < 1e-15
    h = EV.heading_hold(3)
    assert np.all(h["kp"] == 1.0) and np.all(h["ki"] == 0.1) and np.all(h["ref"] == 0.0) and h["windup"] is None      # run_bp_v5.py:311-313


def test_reference_rollout_keywords_default_to_todays_results():
    """a one-row schedule equal to `cmd` and no heading give the records of today's call exactly (f64 oracle, 3 envs, 25 steps); a heading hold
    with zero gains too; with the hold on, heading_out is the PI output of the yaw in front of each step and element 2 its scaled value"""
    n, steps = 3, 25
    cfg = load_env_cfg("bp5_manual_eval.yaml", num_envs=n)
    actor = lambda: NumpyLstmActor.from_npz(os.path.join(GOLDEN, "actor_bp5_155.npz"))
    cmds = [1.0, 2.5, 4.0]
    args = (cfg, [0, 1, 2], cmds, steps)
    kw = dict(vel_hz=50.0, act_hz=30.0)
    old = EV.reference_rollout(O.OracleVecEnv(cfg), actor(), *args, **kw)
    row = EV.reference_rollout(O.OracleVecEnv(cfg), actor(), *args, cmd_schedule=np.asarray(cmds)[None], cmd_every=3, t0=7, **kw)
    zero = EV.reference_rollout(O.OracleVecEnv(cfg), actor(), *args, heading=EV.heading_hold(n, kp=0.0, ki=0.0), **kw)
    for k in old:
        assert np.array_equal(old[k], row[k]) and np.array_equal(old[k], zero[k]), k
    assert np.all(row["heading_out"] == 0.0) and set(row) == set(old)
    on = EV.reference_rollout(O.OracleVecEnv(cfg), actor(), *args, heading=EV.heading_hold(n, ref=0.3), **kw)
    mean, std, _, _ = obs_normalisation(cfg)
    assert np.allclose(on["obs_cond"][:, :, 2], (on["heading_out"] - mean[2]) / std[2], rtol=0, atol=1e-15)
    yaw_before = np.concatenate([np.zeros((1, n)), EV.yaw_from_quaternion(on["body"][:-1, :, 3:7])], 0)     # the reset pose has yaw 0
    integ = np.cumsum((0.3 - yaw_before) * float(cfg["control_dt"]), 0)
    assert on["falls"].sum() == 0 and np.abs(integ).max() < float(cfg["Omega"])
    assert np.allclose(on["heading_out"], 1.0 * (0.3 - yaw_before) + 0.1 * integ, rtol=0, atol=1e-12)
