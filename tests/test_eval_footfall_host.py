"""Host side of the gait recorder's analyses (irrl_eval_footfall: debounced footfalls, stride statistics, support patterns and leg phases per
robot; irrl_eval_motor_plane: the joints against the motor's torque-speed envelope and the stride-folded loop per condition): the C-ABI surface
and the refusals before any HIP call, the filter rule against the reference's literal formula and against its closed form, the per-sample rules
(csrc/eval_elements.hpp) compiled as a stand-alone host program (tests/eval_footfall_main.cpp, plain serial loops) under the address and
undefined-behaviour sanitizers and compared with the numpy twins word for word, hand-made gait diagrams with known answers, the window rules,
the motor plane against a plain Python loop and on RaiSim's own torques and rates -- no GPU needed.

Everything here is integers, or f64 sums added in one stated order: equal means equal bits."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import eval_footfall_lib as L
from conftest import ROOT
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV

SPEC = L.SPEC
NONE = EV.FOOTFALL_NONE
IDX = {k: i for i, k in enumerate(EV.FOOTFALL_COUNTS)}


# ---- the C-ABI ----
def test_footfall_abi_surface_and_refusals_before_any_hip_call():
    """header == SIGNATURES for both entry points, the structs' ctypes mirrors have the header's fields in order, types and sizes, the limits
    agree with the header's, and every refusal fires -- with the entry point's name in front of the text -- although every pointer is a host
    address no HIP call could take: nothing touches the device before the checks are through"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "irrl_env.h")).read(), flags=re.S)
    flat = lambda s: re.sub(r"\s+", " ", s).strip()
    args = flat(re.search(r"\bint irrl_eval_footfall\s*\((.*?)\);", text, flags=re.S).group(1))
    assert args == ("const float *rec_gait, const uint8_t *rec_done, int rows, int num_envs, int frame_first, int frame_every, int frames, "
                    "const irrl_eval_footfall_spec *spec, uint32_t *counts, uint32_t *support, uint32_t *phase, uint8_t *pattern, void *hip_stream")
    kinds = lambda a: [C.c_int if x.strip().startswith("int ") else C.c_void_p for x in a.split(",")]
    assert _lib.SIGNATURES["irrl_eval_footfall"] == (C.c_int, kinds(args))
    margs = flat(re.search(r"\bint irrl_eval_motor_plane\s*\((.*?)\);", text, flags=re.S).group(1))
    assert margs == ("const float *rec_gait, const uint8_t *rec_done, int rows, int num_envs, int conditions, int robots, int frame_first, int frame_every, "
                     "int frames, const irrl_eval_motor_spec *spec, uint32_t *counts, uint32_t *hist, double *fold, void *hip_stream")
    assert _lib.SIGNATURES["irrl_eval_motor_plane"] == (C.c_int, kinds(margs))
    body = re.search(r"typedef struct irrl_eval_footfall_spec \{(.*?)\} irrl_eval_footfall_spec;", text, flags=re.S).group(1)
    assert [flat(d) for d in body.split(";") if d.strip()] == ["int reach, hold, phase_bins"]
    assert [(f[0], f[1]) for f in _lib.EvalFootfallSpec._fields_] == [(k, C.c_int) for k in ("reach", "hold", "phase_bins")]
    assert C.sizeof(_lib.EvalFootfallSpec) == 12
    body = re.search(r"typedef struct irrl_eval_motor_spec \{(.*?)\} irrl_eval_motor_spec;", text, flags=re.S).group(1)
    assert [flat(d) for d in body.split(";") if d.strip()] == ["double tau_max, w_crit, w_max, knee_ratio, sat, t_lo, t_hi, w_lo, w_hi", "int t_bins, w_bins, period"]
    doubles, ints = ("tau_max", "w_crit", "w_max", "knee_ratio", "sat", "t_lo", "t_hi", "w_lo", "w_hi"), ("t_bins", "w_bins", "period")
    assert [(f[0], f[1]) for f in _lib.EvalMotorSpec._fields_] == [(k, C.c_double) for k in doubles] + [(k, C.c_int) for k in ints]
    assert C.sizeof(_lib.EvalMotorSpec) == 9 * 8 + 3 * 4 + 4 and _lib.EvalMotorSpec.t_bins.offset == 72
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    assert define("IRRL_EVAL_FOOTFALL_MAX_FRAMES") == EV.FOOTFALL_MAX_FRAMES == 16384
    assert (define("IRRL_EVAL_FOOTFALL_MAX_REACH"), define("IRRL_EVAL_FOOTFALL_MAX_HOLD"), define("IRRL_EVAL_FOOTFALL_MAX_BINS")) == \
        (EV.FOOTFALL_MAX_REACH, EV.FOOTFALL_MAX_HOLD, EV.FOOTFALL_MAX_BINS) == (8, 64, 64)
    assert define("IRRL_EVAL_FOOTFALL_COUNTS") == len(EV.FOOTFALL_COUNTS) == 14
    assert (define("IRRL_EVAL_MOTOR_MAX_FRAMES"), define("IRRL_EVAL_MOTOR_MAX_BINS"), define("IRRL_EVAL_MOTOR_MAX_PERIOD")) == \
        (EV.MOTOR_MAX_FRAMES, EV.MOTOR_MAX_BINS, EV.MOTOR_MAX_PERIOD) == (16384, 64, 1024)
    assert define("IRRL_EVAL_MOTOR_COUNTS") == len(EV.MOTOR_COUNTS) == 6
    names = re.search(r"enum \{\s*IRRL_EVAL_FOOTFALL_FRAMES = 0,(.*?)\};", text, flags=re.S).group(1)
    assert ["frames"] + [n.strip()[len("IRRL_EVAL_FOOTFALL_"):].lower() for n in names.split(",")] == list(EV.FOOTFALL_COUNTS)
    assert EV.FOOTFALL_SPEC_REFERENCE == dict(reach=2, hold=10, phase_bins=16)
    build.build()
    lib = _lib.load()
    some = C.create_string_buffer(64)
    ptr = C.c_void_p(C.addressof(some))

    good = dict(rows=10, num_envs=6, frame_first=0, frame_every=1, frames=10, spec=SPEC, rec_gait=ptr, rec_done=ptr, counts=ptr)

    def refused(**over):
        a = dict(good, **over)
        st = None if a["spec"] is None else _lib.EvalFootfallSpec(**a["spec"])
        rc = lib.irrl_eval_footfall(a["rec_gait"], a["rec_done"], a["rows"], a["num_envs"], a["frame_first"], a["frame_every"], a["frames"],
                                    None if st is None else C.cast(C.pointer(st), C.c_void_p), a["counts"], ptr, ptr, ptr, None)
        text = _lib.last_error()
        assert rc != 0 and text.startswith("irrl_eval_footfall: "), (over, rc, text)
        return text

    assert "NULL" in refused(rec_gait=None)
    assert "NULL" in refused(spec=None)
    assert "NULL" in refused(counts=None)
    assert "num_envs" in refused(num_envs=0)
    assert "16384" in refused(frames=-1)
    assert "16384" in refused(frames=16385, rows=40000)
    assert "frame_every" in refused(frame_first=-1)
    assert "frame_every" in refused(frame_every=0)
    assert "past the recorder" in refused(frame_first=1)
    assert "past the recorder" in refused(frame_every=2)
    assert "past the recorder" in refused(frames=11)
    assert "reach" in refused(spec=dict(SPEC, reach=-1))
    assert "reach" in refused(spec=dict(SPEC, reach=9))
    assert "hold" in refused(spec=dict(SPEC, hold=-1))
    assert "hold" in refused(spec=dict(SPEC, hold=65))
    assert "phase_bins" in refused(spec=dict(SPEC, phase_bins=-1))
    assert "phase_bins" in refused(spec=dict(SPEC, phase_bins=65))
    st = _lib.EvalFootfallSpec(**SPEC)
    assert lib.irrl_eval_footfall(ptr, None, 10, 6, 0, 1, 0, C.cast(C.pointer(st), C.c_void_p), ptr, None, None, None, None) == 0

    mgood = dict(good, conditions=2, robots=3, spec=L.MOTOR_SPEC)

    def mrefused(**over):
        a = dict(mgood, **over)
        st = None if a["spec"] is None else _lib.EvalMotorSpec(**a["spec"])
        rc = lib.irrl_eval_motor_plane(a["rec_gait"], a["rec_done"], a["rows"], a["num_envs"], a["conditions"], a["robots"], a["frame_first"], a["frame_every"],
                                       a["frames"], None if st is None else C.cast(C.pointer(st), C.c_void_p), a["counts"], ptr, ptr, None)
        text = _lib.last_error()
        assert rc != 0 and text.startswith("irrl_eval_motor_plane: "), (over, rc, text)
        return text

    M = L.MOTOR_SPEC
    inf, nan = float("inf"), float("nan")
    assert "NULL" in mrefused(rec_gait=None)
    assert "NULL" in mrefused(spec=None)
    assert "NULL" in mrefused(counts=None)
    assert "num_envs" in mrefused(num_envs=0)
    assert "16384" in mrefused(frames=-1)
    assert "16384" in mrefused(frames=16385, rows=40000)
    assert "frame_every" in mrefused(frame_first=-1)
    assert "frame_every" in mrefused(frame_every=0)
    assert "past the recorder" in mrefused(frame_first=1)
    assert "past the recorder" in mrefused(frame_every=2)
    assert "past the recorder" in mrefused(frames=11)
    assert "conditions * robots" in mrefused(conditions=4)
    assert "conditions * robots" in mrefused(robots=0, conditions=6)
    assert "conditions * robots" in mrefused(conditions=0)
    for bad in (0.0, -1.0, inf, nan):
        assert "tau_max" in mrefused(spec=dict(M, tau_max=bad))
    for bad in (0.0, -1.55, inf, nan):
        assert "knee_ratio" in mrefused(spec=dict(M, knee_ratio=bad))
    for bad in (-1e-9, inf, nan):
        assert "sat" in mrefused(spec=dict(M, sat=bad))
    assert "w_crit < w_max" in mrefused(spec=dict(M, w_max=14.2))
    assert "w_crit < w_max" in mrefused(spec=dict(M, w_max=10.0))
    assert "w_crit < w_max" in mrefused(spec=dict(M, w_crit=nan))
    assert "t_bins" in mrefused(spec=dict(M, t_bins=65))
    assert "t_bins" in mrefused(spec=dict(M, w_bins=-1))
    assert "period" in mrefused(spec=dict(M, period=1025))
    assert "period" in mrefused(spec=dict(M, period=-1))
    assert "t_lo < t_hi" in mrefused(spec=dict(M, t_hi=-20.0))
    assert "t_lo < t_hi" in mrefused(spec=dict(M, t_lo=nan))
    assert "w_lo < w_hi" in mrefused(spec=dict(M, w_hi=-45.0))
    assert "w_lo < w_hi" in mrefused(spec=dict(M, w_hi=inf))
    st = _lib.EvalMotorSpec(**dict(M, t_hi=-20.0, t_bins=0))            # a bad range with the bins off is no one's business
    assert lib.irrl_eval_motor_plane(ptr, None, 10, 6, 2, 3, 0, 1, 0, C.cast(C.pointer(st), C.c_void_p), ptr, None, None, None) == 0
    # the twins refuse the same specs and calls
    for bad in (dict(SPEC, reach=9), dict(SPEC, hold=65), dict(SPEC, phase_bins=65), dict(SPEC, reach=-1)):
        with pytest.raises(ValueError):
            EV.footfall_spec(bad)
    for bad in (dict(M, tau_max=0.0), dict(M, w_max=14.2), dict(M, knee_ratio=nan), dict(M, sat=-1.0), dict(M, t_bins=65), dict(M, period=1025), dict(M, t_hi=-20.0)):
        with pytest.raises(ValueError):
            EV.motor_spec_check(bad)
    zeros = np.zeros((10, 6, 32), np.float32)
    for kw in (dict(frames=11), dict(frame_first=1, frames=10), dict(frame_every=0)):
        with pytest.raises(ValueError):
            EV.footfall_numpy(zeros, None, SPEC, **kw)
        with pytest.raises(ValueError):
            EV.motor_plane_numpy(zeros, None, M, 2, **kw)
    with pytest.raises(ValueError):
        EV.motor_plane_numpy(zeros, None, M, 4)
    with pytest.raises(ValueError):
        EV.footfall_numpy(np.zeros((16385, 1, 32), np.float32), None, SPEC)


def test_one_list_of_plain_driver_units():
    """build.build() and tools/build_variants.py take the plain-driver units from ONE list, which names the C-ABI unit first and every other
    unit whose launcher it references"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import build
    assert build.PLAIN_UNITS[0] == "irrl_env_abi.hip" and len(set(build.PLAIN_UNITS)) == len(build.PLAIN_UNITS)
    assert {"eval_ensemble.hip", "eval_recurrence.hip", "eval_footfall.hip"} <= set(build.PLAIN_UNITS)
    assert all(os.path.exists(os.path.join(build.CSRC, u)) for u in build.PLAIN_UNITS)
    abi = open(os.path.join(build.CSRC, "irrl_env_abi.hip")).read()
    for launcher in re.findall(r"\b(irrl_eval_\w+_launch)\(", abi):
        assert any(re.search(r"^hipError_t %s\(" % launcher, open(os.path.join(build.CSRC, u)).read(), flags=re.M) for u in build.PLAIN_UNITS[1:]), launcher
    tool = open(os.path.join(ROOT, "tools", "build_variants.py")).read()
    assert "B.PLAIN_UNITS" in tool and not re.search(r'"eval_\w+\.hip"', tool)


# ---- the filter ----
def _reference_filter(c):
    """Data_Visualization_Code/Figure2.py:97-116 for one leg, literally"""
    kernel_size = 5
    kernel = np.ones(kernel_size) / kernel_size
    flag = np.convolve(np.asarray(c, np.float64), kernel, mode="same").astype(bool)
    for j in range(len(flag) - 11):
        if flag[j] == 1 and flag[j + 1] == 0:
            flag[j + 1] = flag[j + 1:j + 11].any()
    return flag


def _random_flags(rng, T):
    kind = rng.randint(0, 3)
    if kind == 0:
        return rng.uniform(size=T) < rng.uniform(0.02, 0.98)
    return L._runs(rng, T, int(rng.randint(1, 25)))


def test_filter_is_the_reference_formula():
    """the twin's sequential rule at (2, 10) == np.convolve(c, ones(5) / 5, 'same').astype(bool) and the reference's loop, on 3000 generated rows
    with T = 5 .. 119"""
    rng = np.random.RandomState(5)
    for _ in range(3000):
        c = _random_flags(rng, int(rng.randint(5, 120)))
        assert np.array_equal(EV.footfall_filter_numpy(c, 2, 10), _reference_filter(c)), c.astype(int).tolist()


def test_filter_sequential_equals_closed_form():
    """the sequential rule == the dilation and footfall_fill_end gap by gap, reach 0 .. 4, hold 0 .. 19, T 1 .. 90"""
    rng = np.random.RandomState(6)
    seen = set()
    for _ in range(4000):
        T, reach, hold = int(rng.randint(1, 91)), int(rng.randint(0, 5)), int(rng.randint(0, 20))
        seen.add((reach, hold))
        c = _random_flags(rng, T)
        assert np.array_equal(EV.footfall_filter_numpy(c, reach, hold), EV.footfall_filter_closed_numpy(c, reach, hold)), (reach, hold, c.astype(int).tolist())
    assert len(seen) == 100


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host program"
    out = str(tmp_path_factory.mktemp("eval_footfall_main") / "eval_footfall_main")
    csrc = os.path.join(ROOT, "high_speed_quadrupedal_locomotion_by_irrl_amd", "csrc")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=on", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                           "-I" + csrc, os.path.join(ROOT, "tests", "eval_footfall_main.cpp"), "-o", out])
    return out


def run_footfall(program, tmp_path, rec, done, spec, frame_first, frame_every, T):
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    L.write_footfall_case(src, rec, done, spec, frame_first, frame_every, T)
    r = subprocess.run([program, src, dst], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    return L.read_footfall_result(dst, rec.shape[1], T, spec["phase_bins"])


def run_motor(program, tmp_path, rec, done, spec, conditions, frame_first, frame_every, T):
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    L.write_motor_case(src, rec, done, spec, conditions, frame_first, frame_every, T)
    r = subprocess.run([program, src, dst], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    return L.read_motor_result(dst, conditions, spec)


def _same_words(got, want, keys, what):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k)


@pytest.mark.parametrize("T", L.TS)
def test_program_equals_the_footfall_twin_word_for_word(program, tmp_path, T):
    """the sanitized program's serial loops over the header's text == the twin on every counter, support, phase and pattern word, with and
    without rec_done and at other (reach, hold); inside the program the sequential rule == the closed form on every flag"""
    rec, done = L.footfall_case(T)
    for dn, spec in ((done, SPEC), (None, SPEC), (done, dict(reach=0, hold=3, phase_bins=5)), (done, dict(reach=8, hold=64, phase_bins=64)),
                     (done, dict(reach=1, hold=0, phase_bins=1))):
        want = EV.footfall_numpy(rec, dn, spec, L.FRAME_FIRST, L.FRAME_EVERY, T)
        got = run_footfall(program, tmp_path, rec, dn, spec, L.FRAME_FIRST, L.FRAME_EVERY, T)
        _same_words(got, want, ("counts", "support", "phase", "pattern"), (T, spec))
        assert np.array_equal(got["f"], got["f_closed"])
        assert np.array_equal(got["pattern"].T, (got["f"] << np.arange(4, dtype=np.uint8)[None, :, None]).sum(1))


def test_spec_refusals_inside_the_sanitized_program(program, tmp_path):
    rec, done = L.footfall_case(5)
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    L.write_footfall_case(src, rec, done, dict(SPEC, hold=65), L.FRAME_FIRST, L.FRAME_EVERY, 5)
    r = subprocess.run([program, src, dst], stderr=subprocess.PIPE)
    assert r.returncode == 3 and b"hold" in r.stderr and not os.path.exists(dst)
    mrec, mdone = L.motor_case(13)
    L.write_motor_case(src, mrec, mdone, dict(L.MOTOR_SPEC, w_max=14.0), 2, L.FRAME_FIRST, L.FRAME_EVERY, 13)
    r = subprocess.run([program, src, dst], stderr=subprocess.PIPE)
    assert r.returncode == 3 and b"w_crit < w_max" in r.stderr and not os.path.exists(dst)


# ---- hand-made diagrams with known answers ----
GAITS = {"trot": ((0.0, 0.5, 0.5, 0.0), (8, 8, 0), {0b1001, 0b0110}), "pace": ((0.0, 0.5, 0.0, 0.5), (8, 0, 8), {0b0101, 0b1010}),
         "bound": ((0.0, 0.0, 0.5, 0.5), (0, 8, 8), {0b0011, 0b1100}), "pronk": ((0.0, 0.0, 0.0, 0.0), (0, 0, 0), {0b1111})}


@pytest.mark.parametrize("name", sorted(GAITS))
def test_hand_made_diagram(program, tmp_path, name):
    """a 100-frame gait at duty 0.4 over 1000 frames (leg 0 touches down at frames 10, 110, ..), 2 dropouts of 1 - 3 frames in every stance:
    TOUCHDOWNS is the number of strides while RAW_TOUCHDOWNS is larger, the mean stance within the dilation's 2 * reach of 40 frames, the
    stride period exactly 100 frames, the phase bins and the support patterns those of the gait, and footfall_row names it"""
    lags, bins, pairs = GAITS[name]
    rng = np.random.RandomState(3)
    flags = L.gait_flags(1000, 100, 0.4, lags, rng, dropouts=2, start=-10)
    rec, done = L.diagram_recorder(flags)
    res = EV.footfall_numpy(rec, done, SPEC)
    _same_words(run_footfall(program, tmp_path, rec, done, SPEC, 0, 1, 1000), res, ("counts", "support", "phase", "pattern"), name)
    c = res["counts"][0].astype(np.int64)
    assert np.all(c[:, IDX["frames"]] == 1000)
    assert np.all(c[:, IDX["touchdowns"]] == 10) and np.all(c[:, IDX["raw_touchdowns"]] > 20)
    assert np.all(c[:, IDX["last_td"]] - c[:, IDX["first_td"]] == 900)
    mean_stance = c[:, IDX["stance_sum"]] / c[:, IDX["stance_phases"]]
    assert np.all(mean_stance >= 40) and np.all(mean_stance <= 40 + 2 * SPEC["reach"])
    assert np.all(c[:, IDX["stance_max"]] == 44) and np.all(c[:, IDX["swing_max"]] == 56) and np.all(c[:, IDX["swing_phases"]] == 9)
    assert tuple(int(np.argmax(res["phase"][0, l])) for l in range(3)) == bins
    assert all(res["phase"][0, l].sum() == res["phase"][0, l].max() for l in range(3))       # every touchdown in the one bin
    assert set(np.flatnonzero(res["support"][0]).tolist()) == pairs | {0} and res["support"][0].sum() == 1000
    row = EV.footfall_row(res["counts"][0], res["support"][0], res["phase"][0], 0.01)
    assert row["gait"] == name
    assert all(abs(row["stride_hz%d" % l] - 1.0) < 1e-12 and abs(row["stride_s%d" % l] - 1.0) < 1e-12 for l in range(4))
    assert all(row["raw_hz%d" % l] > 2.0 for l in range(4)) and abs(row["duty"] - 0.44) < 0.005
    assert abs(row["stance_s0"] - 0.44) < 1e-12 and abs(row["swing_s0"] - 0.56) < 1e-12


def test_gait_names_need_all_three_lags():
    """a walk (legs a quarter stride apart) is "other"; no touchdowns at all: NaN lags, "other" """
    flags = L.gait_flags(1000, 100, 0.7, (0.0, 0.5, 0.25, 0.75), start=-10)
    rec, done = L.diagram_recorder(flags)
    res = EV.footfall_numpy(rec, done, SPEC)
    row = EV.footfall_row(res["counts"][0], res["support"][0], res["phase"][0], 0.01)
    assert row["gait"] == "other" and abs(row["lag1"] - 0.5) < 1e-9 and abs(row["lag2"] - 0.25) < 1e-9 and abs(row["lag3"] - 0.75) < 1e-9
    res = EV.footfall_numpy(*L.diagram_recorder(np.ones((50, 4), bool)), SPEC)
    row = EV.footfall_row(res["counts"][0], res["support"][0], res["phase"][0], 0.01)
    assert row["gait"] == "other" and row["lag1"] != row["lag1"] and row["stride_hz0"] != row["stride_hz0"] and row["duty"] == 1.0


# ---- the window rules ----
def test_window_rules(program, tmp_path):
    """`done` at frame 0 (all counters 0, the sentinels), `done` at T - 1, all-zero and all-one flags, gaps of hold - 1 and hold frames, a gap
    inside and across the last `hold` frames -- the twin and the program against answers written out by hand"""
    T, hold = 60, 10
    spec = dict(reach=0, hold=hold, phase_bins=4)
    flags = np.zeros((T, 6, 4), bool)
    flags[:, 0] = True                                          # robot 0: `done` at frame 0
    flags[:, 1] = True                                          # robot 1: all one, `done` at T - 1
    flags[:, 3] = True                                          # robot 2: all zero; robot 3: all one
    for l, gap in enumerate((hold - 1, hold, 1, hold - 2)):     # robot 4: ones, a gap behind frame 4, ones again
        flags[:5, 4, l] = True
        flags[5 + gap:, 4, l] = True
    flags[:, 5] = True                                          # robot 5: gaps at the window's end
    flags[52:56, 5, 0] = False                                  # inside the last `hold` frames: not filled
    flags[46:53, 5, 1] = False                                  # across: frames 46 .. 49 filled (k <= T - hold - 1), 50 .. 52 not
    flags[40:49, 5, 2] = False                                  # in front: filled
    flags[55:, 5, 3] = False                                    # a trailing gap: never filled
    rec, done = L.diagram_recorder(flags)
    done[0, 0] = 1
    done[T - 1, 1] = 1
    res = EV.footfall_numpy(rec, done, spec)
    _same_words(run_footfall(program, tmp_path, rec, done, spec, 0, 1, T), res, ("counts", "support", "phase", "pattern"), "window rules")
    c = res["counts"].astype(np.int64)
    sent = [0, 0, 0, 0, 0, 0, NONE, NONE, 0, 0, 0, 0, 0, 0]
    assert c[0].tolist() == [sent] * 4 and not res["support"][0].any() and not res["pattern"][:, 0].any() and not res["phase"][0].any()
    assert c[1].tolist() == [[T - 1, T - 1, 0, T - 1, 0, 0, NONE, NONE, 0, 0, 0, 0, 0, 0]] * 4 and res["support"][1, 15] == T - 1 and res["pattern"][T - 1, 1] == 0
    assert c[2].tolist() == [[T] + sent[1:]] * 4 and res["support"][2, 0] == T
    assert c[3].tolist() == [[T, T, 0, T, 0, 0, NONE, NONE, 0, 0, 0, 0, 0, 0]] * 4 and res["support"][3, 15] == T
    #            frames raw_st     raw_td st      td lo first     last     stance ..  swing
    assert c[4, 0].tolist() == [T, T - 9, 1, T, 0, 0, NONE, NONE, 0, 0, 0, 0, 0, 0]                        # hold - 1: filled
    assert c[4, 1].tolist() == [T, T - 10, 1, T - 10, 1, 1, 15, 15, 0, 0, 0, 1, 10, 10]                    # hold: stays
    assert c[4, 2].tolist() == [T, T - 1, 1, T, 0, 0, NONE, NONE, 0, 0, 0, 0, 0, 0]
    assert c[4, 3].tolist() == [T, T - 8, 1, T, 0, 0, NONE, NONE, 0, 0, 0, 0, 0, 0]
    assert c[5, 0].tolist() == [T, T - 4, 1, T - 4, 1, 1, 56, 56, 0, 0, 0, 1, 4, 4]
    assert c[5, 1].tolist() == [T, T - 7, 1, T - 3, 1, 1, 53, 53, 0, 0, 0, 1, 3, 3]
    assert c[5, 2].tolist() == [T, T - 9, 1, T, 0, 0, NONE, NONE, 0, 0, 0, 0, 0, 0]
    assert c[5, 3].tolist() == [T, T - 5, 0, T - 5, 0, 1, NONE, NONE, 0, 0, 0, 0, 0, 0]
    assert res["pattern"][46:53, 5].tolist() == [0b1111] * 4 + [0b1101] * 2 + [0b1100]      # (leg 0's own gap begins at frame 52)


# ---- the motor plane ----
def _motor_loop(rec, done, s, conditions, frame_first, frame_every, T):
    """irrl_eval_motor_plane as a plain Python loop over scalars"""
    import math
    N = rec.shape[1]
    R = N // conditions
    tb, wb, period = s["t_bins"], s["w_bins"], s["period"]
    counts = np.zeros((conditions, 12, 6), np.uint32)
    hist = np.zeros((conditions, 12, tb, wb), np.uint32)
    fold = np.zeros((conditions, 12, period, 3))

    def up(w):
        return s["tau_max"] - (w - s["w_crit"]) * (s["tau_max"] / (s["w_max"] - s["w_crit"])) if w > s["w_crit"] else s["tau_max"]

    def bin_of(x, lo, hi, bins):
        if not (x >= lo and x <= hi):
            return -1
        if x == hi:
            return bins - 1
        return min(int(math.floor((x - lo) * (bins / (hi - lo)))), bins - 1)

    for e in range(N):
        c = e // R
        for i in range(T):
            row = frame_first + i * frame_every
            if done is not None and done[row, e] != 0:
                break
            for j in range(12):
                ratio = s["knee_ratio"] if j % 3 == 2 else 1.0
                m, w = float(rec[row, e, j]) / ratio, float(rec[row, e, 12 + j]) * ratio
                if not (math.isfinite(m) and math.isfinite(w)):
                    continue
                u, lo = up(w), -up(-w)
                counts[c, j] += np.array([1, m >= u - s["sat"], m <= lo + s["sat"], m > u + s["sat"] or m < lo - s["sat"], m * w > 0, m * w < 0], np.uint32)
                if tb > 0 and wb > 0:
                    bt, bw = bin_of(m, s["t_lo"], s["t_hi"], tb), bin_of(w, s["w_lo"], s["w_hi"], wb)
                    if bt >= 0 and bw >= 0:
                        hist[c, j, bt, bw] += 1
                if period > 0:
                    fold[c, j, i % period] += (1.0, m, w)
    return dict(counts=counts, hist=hist, fold=fold)


@pytest.mark.parametrize("period,bins", [(7, 40), (1, 1), (100, 64)])
def test_motor_twin_program_and_plain_loop(program, tmp_path, period, bins):
    """conditions x robots = 2 x 3 with different T_e, samples exactly on up(w) and low(w), at w_crit, at +-w_max and beyond, NaN and inf words:
    the twin == a plain Python loop == the sanitized program, counts and hist as integers and fold as f64 bits; on-envelope samples count as
    saturated and not as outside even with sat = 0"""
    spec = dict(L.MOTOR_SPEC, period=period, t_bins=bins, w_bins=bins if bins != 40 else 45)
    rec, done = L.motor_case(61)
    for dn, sp in ((done, spec), (None, spec), (done, dict(spec, sat=0.0))):
        want = EV.motor_plane_numpy(rec, dn, sp, 2, L.FRAME_FIRST, L.FRAME_EVERY, 61)
        _same_words(_motor_loop(rec, dn, EV.motor_spec_check(sp), 2, L.FRAME_FIRST, L.FRAME_EVERY, 61), want, ("counts", "hist", "fold"), ("loop", sp))
        _same_words(run_motor(program, tmp_path, rec, dn, sp, 2, L.FRAME_FIRST, L.FRAME_EVERY, 61), want, ("counts", "hist", "fold"), ("program", sp))
    assert want["counts"][0, :, 0].max() > want["counts"][0, :, 0].min()          # the NaN / inf words dropped samples of some joints only
    # robot (0, 0) alone, its first 11 frames: on the envelope to the rounding of the f32 torque word (1e-6 N m), alternately above and below
    alone = EV.motor_plane_numpy(rec[:, :1], None, dict(spec, sat=1e-5), 1, L.FRAME_FIRST, L.FRAME_EVERY, 11)["counts"][0]
    assert np.all(alone[:, 0] == 11) and np.all(alone[:, 3] == 0) and np.all(alone[:, 1] >= 6) and np.all(alone[:, 2] >= 5)
    # its first 3 frames (w = 0, +-w_crit) on the abad and hip joints: m is tau_max EXACTLY -- saturated and not outside with sat = 0
    exact = EV.motor_plane_numpy(rec[:, :1], None, dict(spec, sat=0.0), 1, L.FRAME_FIRST, L.FRAME_EVERY, 3)["counts"][0]
    plain = np.arange(12) % 3 != 2
    assert np.all(exact[plain, 3] == 0) and np.all(exact[plain, 1] + exact[plain, 2] == 3)
    assert want["counts"][:, :, 3].min() > 0                                       # the random samples do leave the envelope
    # one robot per condition is the default
    each = EV.motor_plane_numpy(rec, done, spec, None, L.FRAME_FIRST, L.FRAME_EVERY, 61)
    pooled = EV.motor_plane_numpy(rec, done, spec, 2, L.FRAME_FIRST, L.FRAME_EVERY, 61)
    assert each["counts"].shape == (6, 12, 6) and not each["counts"][1].any()                 # (robot 1 is `done` at frame 0)
    assert np.array_equal(each["counts"].reshape(2, 3, 12, 6).sum(1), pooled["counts"])


def test_motor_plane_on_raisims_torques_and_rates(program, tmp_path):
    """slot 7 of every control frame of RaiSim's bp5_155 run at 5 m/s against the config's envelope (18 N m, 14.2 rad/s, 40 rad/s, knee ratio
    1.55) with sat = 1e-3: no joint is ever outside, the four hip joints (1, 4, 7, 10) and no others sit on the envelope, in the recorded
    number of frames, and the folded loop of joint 7 at the reference's period of 100 frames has 10 samples in every phase"""
    rec, d = L.raisim_motor_recorder()
    spec = EV.motor_spec(None, tau_max=18.0, w_crit=14.2, w_max=40.0, sat=float(d["sat"]))
    assert (spec["period"], spec["t_bins"], spec["w_bins"], spec["knee_ratio"]) == (100, 40, 45, 1.55)
    res = EV.motor_plane_numpy(rec, None, spec)
    _same_words(run_motor(program, tmp_path, rec, None, spec, 1, 0, 1, 1000), res, ("counts", "hist", "fold"), "fixture")
    c = res["counts"][0].astype(np.int64)
    assert np.all(c[:, 0] == 1000) and np.all(c[:, 3] == 0)
    sat = c[:, 1] + c[:, 2]
    assert np.flatnonzero(sat).tolist() == [1, 4, 7, 10]
    assert np.array_equal(res["counts"][0], d["counts"]) and np.all(d["counts_all_substeps"][:, 3] == 0)
    assert np.all(res["fold"][0, 7, :, 0] == 10.0) and res["fold"].shape == (1, 12, 100, 3)
    assert res["hist"].sum() <= 12000 and res["hist"][0, 7].sum() > 900
    row = EV.motor_plane_row(res["counts"][0])
    assert np.all(row["outside"] == 0.0) and np.array_equal(row["saturated"] > 0, np.isin(np.arange(12), [1, 4, 7, 10]))
    assert np.allclose(row["motoring"] + row["braking"], 1.0, atol=0.01)
    cfg_spec = EV.motor_spec(dict(MotorMaxTorque=18.0, MotorCriticalSpeed=14.2, MotorMaxSpeed=40.0))
    assert cfg_spec == dict(spec, sat=0.01)
