"""Host side of the persistent policy evaluation (irrl_lstm_eval_rollout_persistent / irrl_lstm_eval_rollout_supports, csrc/env_eval_kernels.hpp):
the C-ABI surface, refusals before any HIP call, and the per-element arithmetic both device forms share (csrc/eval_elements.hpp) compiled as a
host program under the address and undefined-behaviour sanitizers and compared with the numpy twins -- no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_env_cfg
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV
from high_speed_quadrupedal_locomotion_by_irrl_amd.helper import obs_normalisation

N, D, T = 19, 6, 60
DELAYS = np.arange(N) % D
CMDS = np.linspace(0.5, 5.0, N)


def test_persistent_abi_surface_and_refusals_before_any_hip_call():
    """the header declares both new symbols with the argument list of irrl_lstm_eval_rollout, the ctypes table has them, and the new entry makes
    the refusals of the five-launch one -- with its own name in the text -- before a handle is ever dereferenced"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "irrl_env.h")).read(), flags=re.S)
    old = re.search(r"\bint irrl_lstm_eval_rollout\s*\((.*?)\);", text, flags=re.S).group(1)
    new = re.search(r"\bint irrl_lstm_eval_rollout_persistent\s*\((.*?)\);", text, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", old).strip() == re.sub(r"\s+", " ", new).strip()          # unchanged and in the same order
    assert re.search(r"\bint irrl_lstm_eval_rollout_supports\s*\(\s*irrl_env \*\w+,\s*int \w+\)", text)
    assert _lib.SIGNATURES["irrl_lstm_eval_rollout_persistent"] == _lib.SIGNATURES["irrl_lstm_eval_rollout"]
    assert len(_lib.SIGNATURES["irrl_lstm_eval_rollout_supports"][1]) == 2
    build.build()
    lib = _lib.load()
    n_args = len(_lib.SIGNATURES["irrl_lstm_eval_rollout_persistent"][1])
    three = (C.c_float * 3)(0.0, 0.0, 0.0)
    some = C.create_string_buffer(64)                      # any non-NULL address: nothing reads it before the checks are through
    ptr = C.c_void_p(C.addressof(some))

    def call(handle, depth=1, hid=48, ob=35, buffers=False, coeff=1.0):
        args = [None] * n_args
        args[0:6] = [handle, 1, 0, hid, ob, 12]
        args[12] = depth
        if buffers:                                        # weight table (12 entries read: NULL ones), heads, state, work, parameters
            table = (C.c_void_p * 12)(*[C.addressof(some)] * 12)
            args[6] = C.cast(table, C.c_void_p)
            args[7:12] = [ptr] * 5
            args[13:23] = [ptr] * 10
        args[23:26] = [coeff, 1.0, 1.0]
        args[26:29] = [three, three, 1]
        return lib.irrl_lstm_eval_rollout_persistent(*args)

    assert call(None) != 0
    assert "NULL handle" in _lib.last_error() and _lib.last_error().startswith("irrl_lstm_eval_rollout_persistent:")
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    for kw, word in ((dict(depth=0), "depth"), (dict(hid=40), "hid"), (dict(ob=34), "ob 35"), ({}, "NULL"), (dict(buffers=True, coeff=0.0), "(0, 1]")):
        assert call(fake, **kw) != 0
        assert word in _lib.last_error() and _lib.last_error().startswith("irrl_lstm_eval_rollout_persistent:"), (kw, _lib.last_error())
    assert lib.irrl_lstm_eval_rollout_supports(None, 48) == -1
    assert "irrl_lstm_eval_rollout_supports: NULL handle" in _lib.last_error()


def test_persistent_keyword_resolution():
    assert EV.resolve_persistent(False, None) is False and EV.resolve_persistent("off", None) is False
    assert EV.resolve_persistent(True, None) is True and EV.resolve_persistent("on", None) is True
    assert EV.resolve_persistent("auto", lambda: True) is True and EV.resolve_persistent("auto", lambda: False) is False
    with pytest.raises(ValueError):
        EV.resolve_persistent("maybe", None)
    assert EV.PERSISTENT_DEFAULT in (False, "auto")


# ---- the per-element functions on the host ----
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host program"
    out = str(tmp_path_factory.mktemp("eval_elements") / "eval_elements_main")
    csrc = os.path.join(ROOT, "high_speed_quadrupedal_locomotion_by_irrl_amd", "csrc")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-I" + csrc,
                           os.path.join(ROOT, "tests", "eval_elements_main.cpp"), "-o", out])
    return out


def _case(seed):
    """random raw observations, done flags (p = 0.05), actions in [-1, 1] and a random walk of body frames"""
    rng = np.random.RandomState(seed)
    q = rng.normal(size=(T, N, 4)) * 0.05 + np.array([1.0, 0, 0, 0])
    q /= np.linalg.norm(q, axis=2)[..., None]
    body = np.concatenate([rng.normal(size=(T, N, 2)), 0.28 + 0.01 * rng.normal(size=(T, N, 1)), q, rng.normal(size=(T, N, 6))], 2).astype(np.float32)
    done = rng.uniform(size=(T, N)) < 0.05
    assert done.any()
    return dict(ob_reset=rng.normal(size=(N, 35)).astype(np.float32), raw=rng.normal(size=(T, N, 35)).astype(np.float32), done=done,
                action=rng.uniform(-1, 1, size=(T, N, 12)).astype(np.float32), body=body)


def _run(program, tmp_path, case, a_cmd, a_vel, a_act, mean, std):
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    target = np.stack([CMDS, np.zeros(N), np.zeros(N)], 1).astype(np.float32)
    with open(src, "wb") as f:
        f.write(np.array([N, D, T], np.int32).tobytes())
        f.write(np.array([a_cmd, a_vel, a_act] + list(mean) + list(std), np.float32).tobytes())
        f.write(DELAYS.astype(np.int32).tobytes())
        for k in (target, case["ob_reset"], case["raw"], case["done"].astype(np.uint8), case["action"], case["body"]):
            f.write(np.ascontiguousarray(k).tobytes())
    subprocess.check_call([program, src, dst])
    blob = open(dst, "rb").read()
    out, at = {}, 0
    for k, shape, dt in (("cond", (T, N, 35), np.float32), ("applied", (T, N, 12), np.float32), ("stats", (len(EV.STAT_SLOTS), N), np.float64),
                         ("cmd", (N, 3), np.float32), ("vel_his", (N, 35), np.float32)):
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[k] = np.frombuffer(blob[at:at + n], dt).reshape(shape)
        at += n
    assert at == len(blob)
    return out


def _twin(case, a_cmd, a_vel, mean, std):
    target = np.stack([CMDS, np.zeros(N), np.zeros(N)], 1)
    st = EV.condition_state(case["ob_reset"], D)
    rows = []
    for t in range(T):
        rows.append(EV.condition(st, t, case["ob_reset"] if t == 0 else case["raw"][t - 1], DELAYS, target, a_cmd, a_vel, mean, std))
        st["cmd"][case["done"][t]] = 0.0
    return np.stack(rows), st


def test_element_functions_on_the_host_equal_the_numpy_twins(program, tmp_path):
    """19 envs x 60 steps x D = 6, filters at 1 / 50 / 30 Hz, under ASan + UBSan.  Bounds as tests/test_gpu_eval_rollout.py has them for the same
    quantities: f32 rounding of a convex low-pass is at most 2 ulp per step, summing to 2 ulp / alpha -- 2e-5 on elements 3-34 (alpha_vel 0.386,
    |o| <~ 10), 2e-4 on the command elements (alpha_cmd 0.0124, |cmd| <= 5), 1e-5 on the action (alpha_act 0.274, |a| <= 1); statistics: means
    1e-9 absolute, standard deviations 1e-6 relative (f64 accumulation of f32 samples of O(1) on both sides)."""
    cfg = load_env_cfg("bp5_manual_eval.yaml")
    mean, std, _, _ = obs_normalisation(cfg)
    dt = float(cfg["control_dt"])
    a_cmd, a_vel, a_act = (float(np.float32(EV.lowpass_alpha(dt, f))) for f in (1.0, 50.0, 30.0))
    case = _case(11)
    got = _run(program, tmp_path, case, a_cmd, a_vel, a_act, mean[0:3], std[0:3])
    want, st = _twin(case, a_cmd, a_vel, mean[0:3], std[0:3])
    worst = (np.abs(want[:, :, 3:] - got["cond"][:, :, 3:]).max(), np.abs(want[:, :, 0:3] - got["cond"][:, :, 0:3]).max())
    print("max |host program - numpy| conditioned observation: elements 3-34 %.3g, command elements %.3g" % worst)
    assert worst[0] <= 2e-5 and worst[1] <= 2e-4
    assert np.abs(st["cmd"] - got["cmd"]).max() <= 2e-4 and np.abs(st["vel_his"] - got["vel_his"]).max() <= 2e-5
    assert np.all(got["cmd"][case["done"][-1]] == 0.0)                 # cmd = 0 on done
    y, worst_a = np.zeros((N, 12)), 0.0
    for t in range(T):
        y = (1 - a_act) * y + a_act * case["action"][t].astype(np.float64)
        worst_a = max(worst_a, np.abs(y - got["applied"][t]).max())
    print("max |host program - float64| applied action: %.3g" % worst_a)
    assert worst_a <= 1e-5
    stats = EV.statistics_from_sums(got["stats"])
    worst_s = {}
    for e in range(N):
        for k, v in EV.body_statistics(case["body"][:, e]).items():
            if k == "vx_body":
                continue
            err = abs(stats[k][e] - v) if k.endswith("_mean") else abs(stats[k][e] - v) / abs(v)
            worst_s[k] = max(worst_s.get(k, 0.0), err)
    print("worst |host program - body_statistics| (means absolute, stds relative):", {k: "%.2e" % v for k, v in worst_s.items()})
    for k, v in worst_s.items():
        assert v <= (1e-9 if k.endswith("_mean") else 1e-6), (k, v)
    assert np.array_equal(stats["falls"], case["done"].sum(0)) and np.all(stats["frames"] == T)


def test_element_functions_with_the_filters_off_route_exactly(program, tmp_path):
    """a_vel = a_act = 1 (off): elements 3-34 of the conditioned row ARE the raw observation of max(t - delay, 0) steps earlier (index -1: the
    reset observation), the applied action IS the action, bit for bit; a_cmd = 1: the command elements are the scaled target"""
    cfg = load_env_cfg("bp5_manual_eval.yaml")
    mean, std, _, _ = obs_normalisation(cfg)
    case = _case(12)
    got = _run(program, tmp_path, case, 1.0, 1.0, 1.0, mean[0:3], std[0:3])
    src = np.concatenate([case["ob_reset"][None], case["raw"]], 0)          # src[k + 1] = raw[k]
    for t in range(T):
        want = src[np.maximum(t - DELAYS, 0), np.arange(N)]
        assert np.array_equal(got["cond"][t, :, 3:].view(np.uint32), want[:, 3:].view(np.uint32)), t
    assert np.array_equal(got["applied"].view(np.uint32), case["action"].view(np.uint32))
    target = np.stack([CMDS, np.zeros(N), np.zeros(N)], 1).astype(np.float32)
    scaled = (target - np.asarray(mean[0:3], np.float32)) / np.asarray(std[0:3], np.float32)
    assert np.array_equal(got["cond"][:, :, 0:3], np.repeat(scaled[None], T, 0))
