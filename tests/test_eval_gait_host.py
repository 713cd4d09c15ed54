"""Host side of the gait measurements (irrl_lstm_eval_measured[_persistent]: joint power, torque and ground-force sums and the footfall pattern at
control-step rate): the C-ABI surface and the refusals before any HIP call, the epilogue's arithmetic (csrc/eval_elements.hpp
irrl_eval_gait_epilogue) compiled as a stand-alone host program (tests/eval_gait_main.cpp) under the address and undefined-behaviour sanitizers and
compared with the numpy twin (evaluate.gait_rows_numpy), the touchdown rule, the buckets, gait_from_sums on hand-made sums, and the gait=False
paths of the tables and of reference_rollout -- no GPU needed.

Case shape: T = 37 steps of N = 11 envs from a generator (no fixture): torques up to +-30 N m and rates up to +-25 rad/s of both signs, contact
flags with probability 0.55 per leg, env 3 with all legs off throughout, the flag value 2 here and there (any non-zero word is a contact), impulses
up to 0.3 N s (zero where the leg is off, as the pool leaves them), a `done` with probability 0.12 and a whole step of them.
Which rows are compared bit for bit: every row whose f64 arithmetic is exact or a plain sequence of adds -- n, p, ppos, pneg, stance, touchdown,
flight, grfz and the three peaks (products of two widened f32 words are exact, f64 sqrt is correctly rounded).  p2, tau2 and tau2_knee: 1e-12
relative."""
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

G = {k: i for i, k in enumerate(EV.GAIT_SLOTS)}
SQUARED = ("p2", "tau2", "tau2_knee")
EXACT = tuple(k for k in EV.GAIT_SLOTS if k not in SQUARED)
INV_DT = np.float32(1.0) / np.float32(0.01)


def compare_rows(got, want, what, skip=()):
    """the file's rule: EXACT rows bit for bit, SQUARED rows to 1e-12 relative"""
    for k in EXACT:
        if k not in skip:
            assert np.array_equal(got[..., G[k], :].view(np.uint64), want[..., G[k], :].view(np.uint64)), (what, k)
    for k in SQUARED:
        a, b = got[..., G[k], :], want[..., G[k], :]
        assert np.all(np.abs(a - b) <= 1e-12 * np.abs(b)), (what, k, np.abs(a - b).max())


# ---- the C-ABI ----
def test_gait_abi_surface_and_refusals_before_any_hip_call():
    """header == SIGNATURES for the new entry points (the kick call's argument lists with `const irrl_eval_gait *` behind the kicks), the struct's
    ctypes mirror has the header's fields in order and types, the row names and counts agree with the header's enum, IRRL_EVAL_STAT_COUNT is what it
    was, and a NULL handle, a struct with `gait` and no prev_contact and an all-NULL struct are refused -- with the entry point's name in the text --
    before a handle is ever dereferenced (that the recorder alone is accepted needs a pool: tests/test_gpu_eval_gait.py)"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "irrl_env.h")).read(), flags=re.S)
    flat = lambda s: re.sub(r"\s+", " ", s).strip()
    for old, new in (("irrl_lstm_eval_perturbed", "irrl_lstm_eval_measured"), ("irrl_lstm_eval_perturbed_persistent", "irrl_lstm_eval_measured_persistent")):
        a = flat(re.search(r"\bint %s\s*\((.*?)\);" % old, text, flags=re.S).group(1))
        b = flat(re.search(r"\bint %s\s*\((.*?)\);" % new, text, flags=re.S).group(1))
        assert a.endswith(", void *hip_stream") and b == a[:-len("void *hip_stream")] + "const irrl_eval_gait *gait, void *hip_stream"
        assert _lib.SIGNATURES[new] == (_lib.SIGNATURES[old][0], _lib.SIGNATURES[old][1][:-1] + [C.c_void_p, C.c_void_p])
    body = re.search(r"typedef struct irrl_eval_gait \{(.*?)\} irrl_eval_gait;", text, flags=re.S).group(1)
    assert [flat(d) for d in body.split(";") if d.strip()] == ["double *gait", "uint8_t *prev_contact", "float *rec_gait"]
    assert [(f[0], f[1]) for f in _lib.EvalGait._fields_] == [("gait", C.c_void_p), ("prev_contact", C.c_void_p), ("rec_gait", C.c_void_p)]
    names = re.findall(r"IRRL_EVAL_GAIT_([A-Z0-9_]+)\s*(?:=\s*0)?\s*,", re.search(r"enum \{\s*IRRL_EVAL_GAIT_N = 0.*?\};", text, flags=re.S).group(0))
    assert [n.lower() for n in names] == list(EV.GAIT_SLOTS) and len(EV.GAIT_SLOTS) == 20
    assert int(re.search(r"#define IRRL_EVAL_GAIT_REC_DIM (\d+)", text).group(1)) == EV.GAIT_REC_DIM == 32
    stat = re.search(r"enum \{\s*IRRL_EVAL_STAT_N = 0.*?IRRL_EVAL_STAT_COUNT", text, flags=re.S).group(0)
    assert len(re.findall(r"IRRL_EVAL_STAT_[A-Z0-9]+\s*(?:=\s*0)?\s*,", stat)) == len(EV.STAT_SLOTS) == 18
    build.build()
    lib = _lib.load()
    three = (C.c_float * 3)(0.0, 0.0, 0.0)
    some = C.create_string_buffer(64)                      # any non-NULL address: nothing reads it before the checks are through
    ptr = C.c_void_p(C.addressof(some))
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    table = (C.c_void_p * 12)(*[C.addressof(some)] * 12)
    for name in ("irrl_lstm_eval_measured", "irrl_lstm_eval_measured_persistent"):
        fn = getattr(lib, name)
        n_args = len(_lib.SIGNATURES[name][1])

        def call(handle, gait, depth=1):
            args = [None] * n_args
            args[0:6] = [handle, 1, 0, 48, 35, 12]
            args[6] = C.cast(table, C.c_void_p)
            args[7:12] = [ptr] * 5
            args[12] = depth
            args[13:23] = [ptr] * 10
            args[23:26] = [1.0, 1.0, 1.0]
            args[26:29] = [three, three, 1]
            args[-2] = None if gait is None else C.cast(C.pointer(gait), C.c_void_p)
            return fn(*args)

        assert call(None, None) != 0 and _lib.last_error() == name + ": NULL handle"
        assert call(None, _lib.EvalGait(gait=ptr.value, prev_contact=ptr.value)) != 0 and _lib.last_error() == name + ": NULL handle"
        assert call(fake, _lib.EvalGait(gait=ptr.value, rec_gait=ptr.value)) != 0
        assert _lib.last_error().startswith(name + ": gait:") and "prev_contact" in _lib.last_error()
        assert call(fake, _lib.EvalGait()) != 0
        assert _lib.last_error().startswith(name + ": gait:") and "all NULL" in _lib.last_error()
        # the older refusals come first and keep their texts under the new name
        assert call(fake, _lib.EvalGait(rec_gait=ptr.value), depth=0) != 0 and _lib.last_error().startswith(name + ": the delay line")


# ---- the epilogue on the host ----
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host program"
    out = str(tmp_path_factory.mktemp("eval_gait_main") / "eval_gait_main")
    csrc = os.path.join(ROOT, "high_speed_quadrupedal_locomotion_by_irrl_amd", "csrc")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=on", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                           "-I" + csrc, os.path.join(ROOT, "tests", "eval_gait_main.cpp"), "-o", out])
    return out


def gait_case(seed, T=37, N=11):
    rng = np.random.RandomState(seed)
    tq = rng.uniform(-30, 30, size=(T, N, 12)).astype(np.float32)
    qd = rng.uniform(-25, 25, size=(T, N, 12)).astype(np.float32)
    contact = (rng.uniform(size=(T, N, 4)) < 0.55).astype(np.int32)
    contact[rng.uniform(size=(T, N, 4)) < 0.05] *= 2
    if N > 3:
        contact[:, 3] = 0
    lamw = (rng.uniform(-0.3, 0.3, size=(T, N, 4, 3)) * (contact != 0)[..., None]).astype(np.float32)
    done = (rng.uniform(size=(T, N)) < 0.12).astype(np.uint8)
    if T > 20:
        done[20] = 1
    return tq, qd, contact, lamw, done


def run_program(program, tmp_path, case, buckets=1, every=1, t=0, t0=0, prev=None):
    tq, qd, contact, lamw, done = case
    T, N = done.shape
    prev = np.zeros((N, 4), np.uint8) if prev is None else prev
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(src, "wb") as f:
        f.write(np.array([T, N, buckets, every], np.int32).tobytes())
        f.write(np.array([t, t0], np.int64).tobytes())
        f.write(np.array([INV_DT], np.float32).tobytes())
        for a, dt in ((tq, np.float32), (qd, np.float32), (contact, np.int32), (lamw, np.float32), (done, np.uint8), (prev, np.uint8)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    subprocess.check_call([program, src, dst])
    blob = open(dst, "rb").read()
    B = max(buckets, 1)
    ng = B * 20 * N * 8
    gait = np.frombuffer(blob[:ng], np.float64).reshape(B, 20, N)
    prev_out = np.frombuffer(blob[ng:ng + N * 4], np.uint8).reshape(N, 4)
    rec = np.frombuffer(blob[ng + N * 4:], np.float32).reshape(T, N, 32)
    return gait, prev_out, rec


def test_gait_epilogue_on_the_host_equals_the_numpy_twin(program, tmp_path):
    """under ASan + UBSan against evaluate.gait_rows_numpy on the recorder's rows: the file's bit-for-bit / 1e-12 rule; the recorder's row is the
    words it was given; the invariants stance <= n, touchdown <= stance, ppos + pneg == p (1e-12 of ppos - pneg); a `done` step adds nothing"""
    case = gait_case(7)
    tq, qd, contact, lamw, done = case
    assert done.any() and (~done.astype(bool)).any() and (tq * qd > 0).any() and (tq * qd < 0).any() and not contact[:, 3].any() and (contact == 2).any()
    gait, prev, rec = run_program(program, tmp_path, case)
    assert np.array_equal(rec[:, :, 0:12], tq) and np.array_equal(rec[:, :, 12:24], qd) and np.array_equal(rec[:, :, 24:28], (contact != 0).astype(np.float32))
    assert np.array_equal(rec[:, :, 28:32], lamw[..., 2] * INV_DT)
    want, want_prev = EV.gait_rows_numpy(rec, done, lamw=lamw, inv_control_dt=INV_DT)
    compare_rows(gait, want, "host program against the twin")
    assert np.array_equal(prev, want_prev) and np.array_equal(prev, (contact[-1] != 0).astype(np.uint8))
    no_lamw, _ = EV.gait_rows_numpy(rec, done)
    assert np.isnan(no_lamw[:, G["peak_grf"]]).all()
    compare_rows(gait, no_lamw, "the twin without lamw", skip=("peak_grf",))
    g = gait[0]
    assert np.array_equal(g[G["n"]], (done == 0).sum(0)) and g[G["n"]].min() >= 1
    for l in range(4):
        assert np.all(g[G["stance0"] + l] <= g[G["n"]]) and np.all(g[G["touchdown0"] + l] <= g[G["stance0"] + l])
    assert np.all(np.abs(g[G["ppos"]] + g[G["pneg"]] - g[G["p"]]) <= 1e-12 * (g[G["ppos"]] - g[G["pneg"]]))
    assert np.all(g[G["ppos"]] > 0) and np.all(g[G["pneg"]] < 0)
    assert np.array_equal(g[G["flight"]][3], g[G["n"]][3]) and g[G["grfz"]][3] == 0 and g[G["peak_grf"]][3] == 0 and g[G["stance0"]][3] == 0
    live = done == 0
    assert np.array_equal(g[G["peak_tau"]], np.where(live[..., None], np.abs(tq), 0).max((0, 2)).astype(np.float64))
    assert np.array_equal(g[G["peak_qd"]], np.where(live[..., None], np.abs(qd), 0).max((0, 2)).astype(np.float64))
    # a window of `done` steps alone adds nothing and still moves prev_contact
    only = (tq[:3], qd[:3], contact[:3], lamw[:3], np.ones_like(done[:3]))
    gait0, prev0, _ = run_program(program, tmp_path, only)
    assert not gait0.any() and np.array_equal(prev0, (contact[2] != 0).astype(np.uint8))


def test_touchdown_rule_with_a_done_in_the_middle(program, tmp_path):
    """leg 0's contact sequence 0 1 1 0 1: without a `done` two touchdowns (steps 1 and 4) and three stance frames; with step 2 ending in `done` the
    same two touchdowns -- step 2 adds nothing but leaves its post-reset flags in prev_contact, so step 4 still follows a 0 -- and two stance frames;
    with the `done` at step 3, whose post-reset flag is 0, likewise; with the `done` at step 1 the touchdown of step 1 is not counted and step 2,
    which follows the post-reset 1, is none.  Leg 1 stays down: one touchdown from the fresh evaluation's zero, none from a prev_contact of 1."""
    seq = np.array([0, 1, 1, 0, 1])
    contact = np.zeros((5, 1, 4), np.int32)
    contact[:, 0, 0] = seq
    contact[:, 0, 1] = 1
    z = np.zeros((5, 1, 12), np.float32)
    for done_at, touchdowns, stance, frames in ((None, 2, 3, 5), (2, 2, 2, 4), (3, 2, 3, 4), (1, 1, 2, 4)):
        done = np.zeros((5, 1), np.uint8)
        if done_at is not None:
            done[done_at] = 1
        gait, prev, rec = run_program(program, tmp_path, (z, z, contact, z.reshape(5, 1, 4, 3), done))
        g = gait[0, :, 0]
        assert (g[G["touchdown0"]], g[G["stance0"]], g[G["n"]]) == (touchdowns, stance, frames), done_at
        assert g[G["touchdown1"]] == (0 if done_at == 0 else 1) and g[G["stance1"]] == frames
        assert np.array_equal(prev[0], [1, 1, 0, 0])
        want, _ = EV.gait_rows_numpy(rec, done)
        compare_rows(gait, want, "touchdown case", skip=("peak_grf",))
    done = np.zeros((5, 1), np.uint8)
    gait, _, _ = run_program(program, tmp_path, (z, z, contact, z.reshape(5, 1, 4, 3), done), prev=np.array([[1, 1, 0, 0]], np.uint8))
    assert gait[0, G["touchdown0"], 0] == 2 and gait[0, G["touchdown1"], 0] == 0
    # prev_contact after a `done` is that step's (post-reset) flags
    done[4] = 1
    _, prev, _ = run_program(program, tmp_path, (z, z, contact[:, :, [2, 0, 1, 3]], z.reshape(5, 1, 4, 3), done))
    assert np.array_equal(prev[0], [0, 1, 1, 0])


def test_buckets_of_a_window_across_two_boundaries_add_up(program, tmp_path):
    """T = 37 steps from t = 5 with t0 = 9, stat_every = 11, three buckets (boundaries at t = 20 and t = 31 inside the window, the steps in front of
    t0 in bucket 0, the last bucket holding on): the sum rows of the buckets add up to the one-bucket sums to 1e-12 relative (counts exactly), the peak
    rows combine with max exactly (evaluate.gait_merge), the frames land in the buckets of the rule, and the twin agrees per bucket"""
    case = gait_case(11)
    done = case[4]
    one, prev1, rec = run_program(program, tmp_path, case)
    three, prev3, _ = run_program(program, tmp_path, case, buckets=3, every=11, t=5, t0=9)
    assert np.array_equal(prev1, prev3)
    merged = EV.gait_merge(three)
    for k in EV.GAIT_SLOTS:
        a, b = merged[G[k]], one[0, G[k]]
        if k in ("n", "flight") or k.startswith(("stance", "touchdown", "peak")):
            assert np.array_equal(a, b), k
        else:     # relative to the size of what was added: p and grfz are sums of both signs
            scale = one[0, G["ppos"]] - one[0, G["pneg"]] if k == "p" else 120.0 * one[0, G["n"]] if k == "grfz" else np.abs(b)
            assert np.all(np.abs(a - b) <= 1e-12 * scale), k
    bucket = np.array([EV.schedule_row(5 + k, 9, 11, 3) for k in range(37)])
    assert np.array_equal(np.unique(bucket), [0, 1, 2]) and (bucket == 0).sum() == 15 and (bucket == 1).sum() == 11
    for b in range(3):
        assert np.array_equal(three[b, G["n"]], (done[bucket == b] == 0).sum(0))
    want, _ = EV.gait_rows_numpy(rec, done, stat_buckets=3, stat_every=11, t=5, t0=9, lamw=case[3], inv_control_dt=INV_DT)
    compare_rows(three, want, "three buckets")
    # two calls, the second continuing from the first's sums and prev_contact, are the one call
    a, pa = EV.gait_rows_numpy(rec[:16], done[:16], 3, 11, 5, 9, lamw=case[3][:16], inv_control_dt=INV_DT)
    b, pb = EV.gait_rows_numpy(rec[16:], done[16:], 3, 11, 5 + 16, 9, prev_contact=pa, sums=a, lamw=case[3][16:], inv_control_dt=INV_DT)
    assert np.array_equal(b, want) and np.array_equal(pb, prev3)


# ---- host arithmetic ----
def test_gait_from_sums_on_hand_made_sums():
    """two envs with sums written by hand: mean and std of power, work rates, CoT = mean P / (m g mean v_x) with the reference figure's m = 10,
    g = 9.8 and with per-env masses, NaN below the floor of |mean v_x| and where no frame was added, duty factors, stride frequency = touchdowns
    over frames * control_dt, flight fraction, GRFZ over the weight, peaks passed through"""
    s = np.zeros((20, 3))
    b = np.zeros((18, 3))
    s[G["n"]] = [200, 200, 0]
    s[G["p"]] = [200 * 50.0, 200 * 30.0, 0]
    s[G["p2"]] = [200 * (50.0 ** 2 + 4.0 ** 2), 200 * 30.0 ** 2, 0]
    s[G["ppos"]], s[G["pneg"]] = [200 * 70.0, 200 * 30.0, 0], [-200 * 20.0, 0, 0]
    s[G["stance0"]], s[G["stance3"]] = [100, 200, 0], [50, 0, 0]
    s[G["touchdown0"]], s[G["touchdown3"]] = [10, 0, 0], [5, 0, 0]
    s[G["flight"]] = [20, 0, 0]
    s[G["grfz"]] = [200 * 98.0, 200 * 49.0, 0]
    s[G["peak_tau"]], s[G["peak_qd"]], s[G["peak_grf"]] = [33, 20, 0], [21, 9, 0], [400, 100, 0]
    s[G["tau2"]], s[G["tau2_knee"]] = [200 * 8.0, 0, 0], [200 * 2.0, 0, 0]
    b[0] = [200, 200, 0]
    b[1] = [200 * 2.0, 200 * 0.01, 0]
    r = EV.gait_from_sums(s, b, 10.0, 0.01, g=9.8)
    assert np.allclose(r["power_mean"][:2], [50, 30], rtol=0, atol=1e-12) and np.allclose(r["power_std"][:2], [4, 0], rtol=0, atol=1e-9)
    assert np.allclose(r["power_pos"][:2], [70, 30]) and np.allclose(r["power_neg"][:2], [-20, 0])
    assert abs(r["cot"][0] - 50.0 / (10.0 * 9.8 * 2.0)) < 1e-15 and np.isnan(r["cot"][1]) and np.isnan(r["cot"][2])
    assert EV.COT_VX_FLOOR == 0.05
    assert np.isfinite(EV.gait_from_sums(s, b, 10.0, 0.01, g=9.8, vx_floor=0.005)["cot"][1])
    assert np.allclose(r["duty0"][:2], [0.5, 1.0]) and np.allclose(r["duty3"][:2], [0.25, 0]) and np.allclose(r["duty1"], 0)
    assert np.allclose(r["stride_hz0"][:2], [5.0, 0.0]) and np.allclose(r["stride_hz3"][:2], [2.5, 0.0])
    assert np.allclose(r["flight"][:2], [0.1, 0]) and np.allclose(r["grfz_bw"][:2], [1.0, 0.5])
    assert np.array_equal(r["peak_tau"], s[G["peak_tau"]]) and np.array_equal(r["peak_grf"], s[G["peak_grf"]]) and np.array_equal(r["gait_frames"], [200, 200, 0])
    assert np.allclose(r["tau2_mean"][:2], [8, 0]) and np.allclose(r["tau2_knee_mean"][:2], [2, 0])
    per_env = EV.gait_from_sums(s, b, np.array([10.0, 12.0, 11.0]), 0.01)
    assert abs(per_env["cot"][0] - 50.0 / (10.0 * 9.81 * 2.0)) < 1e-15 and abs(per_env["grfz_bw"][1] - 49.0 / (12.0 * 9.81)) < 1e-15
    backwards = b.copy()
    backwards[1] = -b[1]
    assert EV.gait_from_sums(s, backwards, 10.0, 0.01, g=9.8)["cot"][0] == -r["cot"][0]
    merged = EV.gait_merge(np.stack([s, 2 * s]))
    assert np.array_equal(merged[G["p"]], 3 * s[G["p"]]) and np.array_equal(merged[G["peak_tau"]], 2 * s[G["peak_tau"]])


def test_tables_without_gait_are_what_they_were_and_gain_columns_with_it():
    """sweep_table / perturbation_table of fixed rows: the strings of the default call are today's, byte for byte (written out here), rows that carry
    gait keys print the same without the keyword, and with it every line gains the gait columns behind the old text"""
    row = dict(mu=0.4, delay=2, cmd=3.0, falls=1, frames=2000, vx_body_mean=2.9, vx_body_std=0.1, z_mean=0.28, z_std=0.01, roll_std=0.02, pitch_mean=-0.01,
               pitch_std=0.03, yaw_rate_mean=0.002)
    old = ("mu     delay cmd   falls vx_body_mean vx_body_std  z_mean       z_std        roll_std     pitch_mean   pitch_std    yaw_rate_mean\n"
           "0.4    2     3     1          +2.9000      +0.1000      +0.2800      +0.0100      +0.0200      -0.0100      +0.0300      +0.0020")
    assert EV.sweep_table([row]) == old
    grow = dict(row, cot=0.51, power_mean=150.0, duty0=0.4, duty1=0.41, duty2=0.42, duty3=0.43, stride_hz0=5.0, stride_hz1=5.0, stride_hz2=4.0, stride_hz3=6.0,
                flight=0.1)
    assert EV.sweep_table([grow]) == old
    new = EV.sweep_table([grow], gait=True).split("\n")
    assert [a.startswith(b) for a, b in zip(new, old.split("\n"))] == [True, True]
    assert new[0].split()[-8:] == ["cot", "power_mean", "duty0", "duty1", "duty2", "duty3", "stride_hz", "flight"]
    assert new[1].split()[-8:] == ["+0.5100", "+150.0000", "+0.4000", "+0.4100", "+0.4200", "+0.4300", "+5.0000", "+0.1000"]
    stair = dict(row, level=2, cmd_level=1.5)
    assert EV.sweep_table([stair]).split("\n")[1].startswith("0.4    2     3     2     1.5       1     ")
    st = {k: np.array([[1.0, 2.0], [3.0, 5.0]]) for k in ("vx_body_mean", "z_mean", "pitch_mean")}
    prow = dict(mu=0.8, delay=0, cmd=5.0, explorations=2, surviving=0.5, falls=np.array([0, 1]), stats=st)
    pold = ("mu     delay cmd   E     surviving vx_before    vx_last      z_before     z_last       pitch_before pitch_last  \n"
            "0.8    0     5     2     0.5000         +1.0000      +3.0000      +1.0000      +3.0000      +1.0000      +3.0000")
    assert EV.perturbation_table([prow]) == pold
    gt = {k: np.array([[0.5, 9.0], [0.7, 9.0]]) for k in ("cot", "duty0", "duty1", "duty2", "duty3")}
    assert EV.perturbation_table([dict(prow, gait=gt)]) == pold
    pnew = EV.perturbation_table([dict(prow, gait=gt)], gait=True).split("\n")
    assert pnew[0].startswith(pold.split("\n")[0]) and pnew[1].startswith(pold.split("\n")[1])
    assert pnew[0].split()[-4:] == ["cot_before", "cot_last", "duty_before", "duty_last"] and pnew[1].split()[-4:] == ["+0.5000", "+0.7000", "+0.5000", "+0.7000"]


def test_reference_rollout_gait_keyword_defaults_to_todays_results():
    """gait=False (the default) gives the records of today's call exactly and no new key (f64 oracle, 3 envs, 60 steps from the reset drop: the feet land inside); gait=True adds `gait`
    [steps, n, 32] = the pool's torque | joint rates | contact flags | lam_w_z / control_dt behind every step and changes nothing else; the twin's
    sums of that record have the frame count of the steps that did not end in `done`"""
    n, steps = 3, 60
    cfg = load_env_cfg("bp5_manual_eval.yaml", num_envs=n)
    actor = lambda: NumpyLstmActor.from_npz(os.path.join(GOLDEN, "actor_bp5_155.npz"))
    args = (cfg, [0, 1, 2], [1.0, 2.5, 4.0], steps)
    kw = dict(vel_hz=50.0, act_hz=30.0)
    old = EV.reference_rollout(O.OracleVecEnv(cfg), actor(), *args, **kw)
    off = EV.reference_rollout(O.OracleVecEnv(cfg), actor(), *args, gait=False, **kw)
    assert set(old) == set(off) and "gait" not in old
    env = O.OracleVecEnv(cfg)
    on = EV.reference_rollout(env, actor(), *args, gait=True, **kw)
    for k in old:
        assert np.array_equal(old[k], off[k]) and np.array_equal(old[k], on[k]), k
    assert set(on) == set(old) | {"gait"} and on["gait"].shape == (steps, n, 32)
    assert np.array_equal(on["gait"][:, :, 0:12], on["torque"])
    s = env.get_state()
    assert np.array_equal(on["gait"][-1, :, 12:24], s[:, 25:37]) and np.array_equal(on["gait"][-1, :, 24:28], (s[:, 147:151] != 0).astype(float))
    assert np.allclose(on["gait"][-1, :, 0:12], env.joint_effort(), rtol=1e-6, atol=1e-6)
    assert np.allclose(on["gait"][-1, :, 12:24], env.origin_state()[:, 25:37], rtol=1e-6, atol=1e-7)
    assert np.array_equal(on["gait"][-1, :, 24:28], env.origin_state()[:, 37:41])
    assert np.array_equal(on["gait"][-1, :, 28:32], s[:, 137:147:3] / float(cfg["control_dt"]))
    assert set(np.unique(on["gait"][:, :, 24:28])) <= {0.0, 1.0} and on["gait"][:, :, 24:28].any()
    sums, prev = EV.gait_rows_numpy(on["gait"], on["done"])
    assert np.array_equal(sums[0, G["n"]], (~on["done"]).sum(0)) and np.array_equal(prev, on["gait"][-1, :, 24:28].astype(np.uint8))
    assert np.all(sums[0, G["grfz"]] > 0) and np.all(sums[0, G["stance0"]] <= sums[0, G["n"]])
