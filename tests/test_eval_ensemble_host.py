"""Host side of the ensemble analysis (irrl_eval_ensemble: state-space entropy, cell counts, histograms and moments per (condition, frame) of a
body recorder): the C-ABI surface and the refusals before any HIP call, the per-sample arithmetic (csrc/eval_elements.hpp
irrl_eval_ensemble_features / _key / _bin) compiled as a stand-alone host program (tests/eval_ensemble_main.cpp) under the address and
undefined-behaviour sanitizers and compared with the numpy twin (evaluate.ensemble_numpy), the twin against the reference's own formula written
out here, mask / non-finite rows / permutations / frame strides, the entropy-rate fit and the return map -- no GPU needed.

Cases: tests/eval_ensemble_lib.py, [F = 7, 3 * E, 13] with E = 1, 37, 1000.  The rule: the generated cases hold no sample on a cell edge (asserted;
evaluate.ensemble_edges), and then keys, kept, occupied, largest and hist are equal as integers, the entropy agrees within 1e-12 * max(1, ln M)
and the moments within 1e-12 relative."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import eval_ensemble_lib as L
from conftest import ROOT
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV

SPEC = L.SPEC
ES = (1, 37, 1000)


@pytest.fixture(scope="module")
def cases():
    """E -> (body, the twin's result): computed once, read by every test, changed by none"""
    out = {}
    for E in ES:
        body = L.ensemble_case(L.SEED, L.F_HOST, L.C, E)
        body.setflags(write=False)
        out[E] = (body, EV.ensemble_numpy(body, L.C, SPEC))
    return out


# ---- the C-ABI ----
def _spec_struct(spec):
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib
    st = _lib.EvalEnsembleSpec(hist_bins=int(spec.get("hist_bins", 0)))
    for k in ("lb", "ub", "prec", "hist_lo", "hist_hi"):
        setattr(st, k, (C.c_double * 6)(*spec[k]))
    return st


def test_ensemble_abi_surface_and_refusals_before_any_hip_call():
    """header == SIGNATURES for irrl_eval_ensemble, the struct's ctypes mirror has the header's fields in order, types and sizes, the limits agree
    with the header's, and every refusal fires -- with the entry point's name in the text -- although every pointer is a host address no HIP call
    could take: nothing touches the device before the checks are through.  The radix overflow is exercised with prec = 1e-6."""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "irrl_env.h")).read(), flags=re.S)
    flat = lambda s: re.sub(r"\s+", " ", s).strip()
    args = flat(re.search(r"\bint irrl_eval_ensemble\s*\((.*?)\);", text, flags=re.S).group(1))
    assert args == ("const float *rec_body, int rows, int num_envs, int conditions, int explorations, int frame_first, int frame_every, int frames, "
                    "const uint8_t *mask, const irrl_eval_ensemble_spec *spec, double *entropy, uint32_t *counts, uint32_t *hist, double *moments, "
                    "void *hip_stream")
    kinds = [C.c_int if a.strip().startswith("int ") else C.c_void_p for a in args.split(",")]
    assert _lib.SIGNATURES["irrl_eval_ensemble"] == (C.c_int, kinds)
    body = re.search(r"typedef struct irrl_eval_ensemble_spec \{(.*?)\} irrl_eval_ensemble_spec;", text, flags=re.S).group(1)
    assert [flat(d) for d in body.split(";") if d.strip()] == ["double lb[6], ub[6], prec[6]", "double hist_lo[6], hist_hi[6]", "int hist_bins"]
    assert [(f[0], f[1]) for f in _lib.EvalEnsembleSpec._fields_] == [(k, C.c_double * 6) for k in ("lb", "ub", "prec", "hist_lo", "hist_hi")] + [("hist_bins", C.c_int)]
    assert C.sizeof(_lib.EvalEnsembleSpec) == 30 * 8 + 8 and _lib.EvalEnsembleSpec.hist_bins.offset == 240
    assert int(re.search(r"#define IRRL_EVAL_ENSEMBLE_MAX (\d+)", text).group(1)) == EV.ENSEMBLE_MAX == 16384
    assert int(re.search(r"#define IRRL_EVAL_ENSEMBLE_MAX_BINS (\d+)", text).group(1)) == EV.ENSEMBLE_MAX_BINS == 256
    assert int(re.search(r"#define IRRL_EVAL_ENSEMBLE_DIM (\d+)", text).group(1)) == len(EV.ENSEMBLE_FEATURES) == 6
    build.build()
    lib = _lib.load()
    some = C.create_string_buffer(64)
    ptr = C.c_void_p(C.addressof(some))
    good = dict(rows=10, num_envs=12, conditions=3, explorations=4, frame_first=0, frame_every=1, frames=10, spec=SPEC, rec_body=ptr, entropy=ptr)

    def refused(**over):
        a = dict(good, **over)
        st = None if a["spec"] is None else _spec_struct(a["spec"])
        rc = lib.irrl_eval_ensemble(a["rec_body"], a["rows"], a["num_envs"], a["conditions"], a["explorations"], a["frame_first"], a["frame_every"], a["frames"],
                                    ptr, None if st is None else C.cast(C.pointer(st), C.c_void_p), a["entropy"], ptr, ptr, ptr, None)
        text = _lib.last_error()
        assert rc != 0 and text.startswith("irrl_eval_ensemble: "), (over, rc, text)
        return text

    assert "num_envs" in refused(conditions=5)
    assert "num_envs" in refused(num_envs=13)
    assert "16384" in refused(explorations=0, num_envs=12)
    assert "16384" in refused(explorations=16385, conditions=1, num_envs=16385)
    assert "frame_every" in refused(frame_every=0)
    assert "frame_every" in refused(frame_first=-1)
    assert "past the recorder" in refused(frame_first=1)
    assert "past the recorder" in refused(frame_every=2)
    assert "past the recorder" in refused(frames=11)
    assert "prec" in refused(spec=dict(SPEC, prec=(0.005, 0.02, 0.0, 0.005, 0.025, 0.025)))
    assert "prec" in refused(spec=dict(SPEC, prec=(0.005, 0.02, -0.02, 0.005, 0.025, 0.025)))
    assert "lb_i <= ub_i" in refused(spec=dict(SPEC, lb=(0.6, -3.14, -1.57, -10, -10, -10)))
    assert "2^63" in refused(spec=dict(SPEC, prec=(1e-6,) * 6))
    assert "2^62" in refused(spec=dict(SPEC, ub=(1e300, 3.14, 1.57, 10, 10, 10)))
    assert "hist_bins" in refused(spec=dict(SPEC, hist_bins=257))
    assert "hist_bins" in refused(spec=dict(SPEC, hist_bins=-1))
    assert "hist_lo" in refused(spec=dict(SPEC, hist_hi=(0.4, 1.0, -1.0, 5.0, 5.0, 5.0)))
    assert "NULL" in refused(rec_body=None)
    assert "NULL" in refused(spec=None)
    assert "NULL" in refused(entropy=None)
    # the twin refuses the same specs and shapes
    for bad in (dict(SPEC, prec=(1e-6,) * 6), dict(SPEC, prec=(0.0,) * 6), dict(SPEC, lb=(0.6, -3.14, -1.57, -10, -10, -10)), dict(SPEC, hist_bins=257),
                dict(SPEC, hist_hi=SPEC["hist_lo"])):
        with pytest.raises(ValueError):
            EV.ensemble_spec(bad)
    with pytest.raises(ValueError):
        EV.ensemble_numpy(np.zeros((2, 7, 13), np.float32), 3, SPEC)
    with pytest.raises(ValueError):
        EV.ensemble_numpy(np.zeros((2, 6, 13), np.float32), 3, SPEC, frame_first=1, frames=2)
    # hist_lo >= hist_hi is no refusal without bins
    assert EV.ensemble_spec(dict(SPEC, hist_bins=0, hist_hi=SPEC["hist_lo"]))["hist_bins"] == 0


# ---- the element functions on the host ----
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host program"
    out = str(tmp_path_factory.mktemp("eval_ensemble_main") / "eval_ensemble_main")
    csrc = os.path.join(ROOT, "high_speed_quadrupedal_locomotion_by_irrl_amd", "csrc")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=on", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                           "-I" + csrc, os.path.join(ROOT, "tests", "eval_ensemble_main.cpp"), "-o", out])
    return out


def run_program(program, tmp_path, body, conditions, spec, mask=None, check=True):
    rows, n = body.shape[0], body.shape[1]
    s = {k: np.asarray(spec[k], np.float64) for k in ("lb", "ub", "prec", "hist_lo", "hist_hi")}
    bins = int(spec["hist_bins"])
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(src, "wb") as f:
        f.write(np.array([rows, n, conditions], np.int32).tobytes())
        for k in ("lb", "ub", "prec", "hist_lo", "hist_hi"):
            f.write(s[k].tobytes())
        f.write(np.array([bins], np.int32).tobytes())
        f.write((np.ones(n, np.uint8) if mask is None else np.asarray(mask, np.uint8)).tobytes())
        f.write(np.ascontiguousarray(body, np.float32).tobytes())
    r = subprocess.run([program, src, dst], stderr=subprocess.PIPE)
    if not check:
        return r
    assert r.returncode == 0, r.stderr.decode()
    blob = open(dst, "rb").read()
    rn, o = rows * n, 0
    take = lambda cnt, dt: np.frombuffer(blob, dt, cnt, o)
    x = take(rn * 6, np.float64).reshape(rows, n, 6); o += rn * 48
    key = take(rn, np.uint64).reshape(rows, n); o += rn * 8
    kept = take(rn, np.uint8).reshape(rows, n) != 0; o += rn
    bin_ = take(rn * 6, np.int32).reshape(rows, n, 6); o += rn * 24
    entropy = take(conditions * rows, np.float64).reshape(conditions, rows); o += conditions * rows * 8
    counts = take(conditions * rows * 3, np.uint32).reshape(conditions, rows, 3); o += conditions * rows * 12
    assert o == len(blob)
    hist = None
    if bins > 0:
        E = n // conditions
        hist = np.zeros((conditions, rows, 6, bins), np.uint32)
        for c in range(conditions):
            for i in range(6):
                b = bin_[:, c * E:(c + 1) * E, i]
                for r_ in range(rows):
                    hist[c, r_, i] = np.bincount(b[r_][b[r_] >= 0], minlength=bins)
    return dict(x=x, key=key, sample_kept=kept, bin=bin_, entropy=entropy, kept=counts[..., 0], occupied=counts[..., 1], largest=counts[..., 2], hist=hist, moments=None)


@pytest.mark.parametrize("E", ES)
def test_host_program_equals_the_twin(program, tmp_path, cases, E):
    """the element functions compiled for the host (ASan + UBSan) against the numpy twin on the generated bodies: no sample on a cell edge, then the
    keys of all F * 3 * E samples, the bins, kept, occupied and largest equal as integers, the features within 4 ulp of their magnitude (libm's atan2 and
    asin against numpy's), the entropy within 1e-12 * max(1, ln M); the special frames are what the generator promises"""
    body, want = cases[E]
    L.assert_no_edges(body)
    got = run_program(program, tmp_path, body, L.C, SPEC)
    x = EV.ensemble_features(body)
    key, kept = EV.ensemble_keys(x, SPEC)
    assert kept.all() and got["sample_kept"].all()
    assert np.all(np.abs(got["x"] - x) <= 4 * np.spacing(np.abs(x)))
    assert np.array_equal(got["key"], key)
    s = EV.ensemble_spec(SPEC)
    for i in range(6):
        assert np.array_equal(got["bin"][..., i], EV.ensemble_bins(x[..., i], s["hist_lo"][i], s["hist_hi"][i], s["hist_bins"]))
    L.assert_same_result(got, want, "E = %d" % E)
    # the special frames
    assert np.all(want["kept"] == E)
    assert np.all(want["occupied"][:, 1] == 1) and np.all(want["largest"][:, 1] == E) and np.all(want["entropy"][:, 1] == 0.0)
    for f in (0, 2):
        assert np.all(want["occupied"][:, f] == E) and np.all(np.abs(want["entropy"][:, f] - np.log(E)) <= 1e-12)
    if E >= 37:
        assert np.all(want["largest"][:, 3:] > 1) and np.all(want["occupied"][:, 3:] < E)
        x0 = x[0].reshape(L.C, E, 6)                      # frame 0: every feature beyond both bounds in every condition
        assert np.all((x0 < s["lb"]).any(1)) and np.all((x0 > s["ub"]).any(1))
        assert (body[..., 3] < 0).any() and (body[..., 3] > 0).any()


def test_twin_equals_the_reference_formula(cases):
    """evaluate.ensemble_numpy against the formula of the reference's figure scripts written out: np.clip -> / prec -> astype(int64) ->
    np.unique(axis=0, return_counts=True) -> -sum f ln f (Figure4.py:160-166), entropy within 1e-12; and hist == np.histogram(range=, bins=) over
    the samples further than 1e-9 bin widths from every bin edge (all of them: asserted)"""
    body, want = cases[1000]
    E, bins = 1000, SPEC["hist_bins"]
    lb, ub, prec = (np.array(SPEC[k]) for k in ("lb", "ub", "prec"))
    x = EV.ensemble_features(body)
    assert not L.histogram_edges(x, SPEC).any()
    for f in range(body.shape[0]):
        for c in range(L.C):
            data = x[f, c * E:(c + 1) * E]
            _, freq = np.unique((np.clip(data, lb, ub) / prec).astype(np.int64), axis=0, return_counts=True)
            freq = freq / data.shape[0]
            assert abs(-np.sum(freq * np.log(freq)) - want["entropy"][c, f]) <= 1e-12
            assert len(freq) == want["occupied"][c, f]
            for i in range(6):
                h, _ = np.histogram(data[:, i], range=(SPEC["hist_lo"][i], SPEC["hist_hi"][i]), bins=bins)
                assert np.array_equal(h, want["hist"][c, f, i])
            assert np.allclose(want["moments"][c, f, :, 0], data.sum(0), rtol=1e-13, atol=0) and np.allclose(want["moments"][c, f, :, 1], (data * data).sum(0), rtol=1e-13)


def test_truncation_keeps_the_double_width_cell_around_zero():
    """the reference's astype(int) truncates toward zero: +-0.019 rad of roll share the cell 0 (precision 0.02), -0.021 and 0.021 do not; the key's
    digits are the cells counted from trunc(lb / prec), feature 0 the most significant"""
    x = np.zeros((4, 6))
    x[:, 0] = 0.3025
    x[:, 1] = (-0.021, -0.019, 0.019, 0.021)
    key, kept = EV.ensemble_keys(x, SPEC)
    assert kept.all() and key[1] == key[2] and len({int(k) for k in key}) == 3
    lo, radix = EV.ensemble_radix(EV.ensemble_spec(SPEC))
    assert list(lo) == [0, -157, -78, -2000, -400, -400] and list(radix) == [101, 315, 157, 4001, 801, 801]
    digits = []
    k = int(key[3])
    for r in radix[::-1]:
        digits.append(k % int(r))
        k //= int(r)
    assert digits[::-1] == [60, 158, 78, 2000, 400, 400]     # z 0.3025 -> cell 60; roll 0.021 -> cell 1 - (-157)


def test_mask_nonfinite_permutation_and_strides(program, tmp_path, cases):
    """a mask and non-finite rows take samples out of M (twin and host program alike); permuting a condition's explorations changes no counter, no
    histogram and -- the keys are sorted -- not a bit of the twin's entropy; frame_first / frame_every / frames pick the rows they name"""
    body, want = cases[37]
    E, n = 37, 3 * 37
    rng = np.random.RandomState(3)
    mask = (rng.uniform(size=n) < 0.7).astype(np.uint8)
    mask[E:2 * E] = 0                                      # a whole condition masked out: M = 0, H = 0, zero counts
    bad = body.copy()
    bad[0, 2, 2] = np.nan
    bad[0, 3, 9] = np.inf
    bad[3, 5, 3:7] = np.nan
    bad[4, 2 * E + 1, 12] = -np.inf
    got = EV.ensemble_numpy(bad, L.C, SPEC, mask=mask)
    prog = run_program(program, tmp_path, bad, L.C, SPEC, mask=mask)
    L.assert_same_result(prog, got, "mask + non-finite")
    assert np.all(got["kept"][1] == 0) and np.all(got["entropy"][1] == 0) and np.all(got["occupied"][1] == 0) and np.all(got["largest"][1] == 0)
    assert np.all(got["hist"][1] == 0) and np.all(got["moments"][1] == 0)
    m0 = int(mask[:E].sum())
    assert got["kept"][0, 0] == m0 - int(mask[2]) - int(mask[3]) and got["kept"][0, 3] == m0 - int(mask[5]) and got["kept"][0, 1] == m0
    assert got["kept"][2, 4] == int(mask[2 * E:].sum()) - int(mask[2 * E + 1])
    assert np.all(np.isfinite(got["moments"])) and np.all(got["hist"].sum(-1) <= got["kept"][..., None])
    # permutation
    perm = np.concatenate([c * E + rng.permutation(E) for c in range(L.C)])
    again = EV.ensemble_numpy(body[:, perm], L.C, SPEC)
    for k in ("kept", "occupied", "largest", "hist"):
        assert np.array_equal(again[k], want[k])
    assert np.array_equal(again["entropy"].view(np.uint64), want["entropy"].view(np.uint64))
    assert np.all(np.abs(again["moments"] - want["moments"]) <= 1e-12 * np.abs(want["moments"]))
    # strides
    part = EV.ensemble_numpy(body, L.C, SPEC, frame_first=1, frame_every=2)
    assert part["entropy"].shape == (L.C, 3)
    for k in ("entropy", "kept", "occupied", "largest", "hist", "moments"):
        assert np.array_equal(part[k], want[k][:, 1::2])
    one = EV.ensemble_numpy(body, L.C, SPEC, frame_first=2, frame_every=3, frames=1)
    assert one["entropy"].shape == (L.C, 1) and np.array_equal(one["entropy"][:, 0], want["entropy"][:, 2])
    row = EV.ensemble_row(want, 2, 0.01)
    assert np.array_equal(row["t"], np.arange(L.F_HOST) * 0.01) and np.array_equal(row["entropy"], want["entropy"][2]) and row["hist"].shape == (L.F_HOST, 6, 101)
    x = EV.ensemble_features(body)[:, 2 * E:]
    assert np.allclose(row["mean"], x.mean(1), rtol=1e-12, atol=1e-12) and np.allclose(row["std"], x.std(1), rtol=1e-9, atol=1e-6)   # (sum x^2 / M - mean^2 of identical robots: the root of a rounding error)


def test_host_program_refuses_what_the_library_refuses(program, tmp_path, cases):
    """irrl_eval_ensemble_spec_error under the sanitizers: the radix overflow of prec = 1e-6 and a bound beyond 2^62 cells are refused (exit status 3)
    before any key is computed -- no signed overflow, no out-of-range cast for UBSan to find"""
    body = cases[1][0]
    for bad, word in ((dict(SPEC, prec=(1e-6,) * 6), b"2^63"), (dict(SPEC, lb=(-1e300, -3.14, -1.57, -10, -10, -10)), b"2^62"),
                      (dict(SPEC, prec=(0.0,) * 6), b"prec")):
        r = run_program(program, tmp_path, body, L.C, bad, check=False)
        assert r.returncode == 3 and word in r.stderr, (r.returncode, r.stderr)


# ---- the entropy-rate fit and the return map ----
def test_entropy_rate_recovers_a_synthetic_curve():
    """entropy_rate on piecewise_func3 (Figure4.py:169-173) with its corners on frame times: a and c exactly, b and d to rounding; with N(0, 0.02)
    noise: the fit's residual is no worse than the true curve's, and the parameters lie within the noise's reach of the truth"""
    t = np.arange(300) * 0.01
    a, b, c, d = 0.4, 9.21, 1.9, -4.5
    H = EV.entropy_curve(t, a, b, c, d)
    assert np.array_equal(H, np.where(t <= a, b, np.where(t <= c, d * (t - a) + b, d * (c - a) + b)))
    fit = EV.entropy_rate(t, H)
    assert fit["a"] == t[40] and fit["c"] == t[190] and abs(fit["b"] - b) <= 1e-12 and abs(fit["d"] - d) <= 1e-12 and fit["residual"] <= 1e-13
    assert fit["kappa"] == fit["d"] and fit["t_floor"] == fit["c"]
    noisy = H + np.random.RandomState(1).normal(0.0, 0.02, len(t))
    fit = EV.entropy_rate(t, noisy)
    truth = float(np.sqrt(np.mean((H - noisy) ** 2)))
    assert fit["residual"] <= truth
    assert abs(fit["a"] - a) <= 0.03 and abs(fit["c"] - c) <= 0.03 and abs(fit["b"] - b) <= 0.01 and abs(fit["d"] - d) <= 0.05
    coarse = EV.entropy_rate(t, H, stride=10)
    assert coarse["a"] == t[40] and coarse["c"] == t[190] and coarse["residual"] <= 1e-13
    with pytest.raises(ValueError):
        EV.entropy_rate(t[:2], H[:2])


def test_poincare_section_against_slicing(cases):
    body = cases[37][0]
    one = np.ascontiguousarray(np.tile(body[:, 5], (30, 1)))          # [210, 13]: one robot's frames
    x = EV.ensemble_features(one)
    for every, offset in ((100, 50), (7, 0), (7, 3), (1, 0), (300, 0), (5, 209)):
        sec = EV.poincare_section(one, every, offset)
        assert np.array_equal(sec, x[np.arange(offset, len(one), every)])
    assert EV.poincare_section(one, 100, 50).shape == (2, 6) and EV.poincare_section(one, 5, 210).shape == (0, 6)
    with pytest.raises(ValueError):
        EV.poincare_section(one, 0, 0)


# ---- the study's signature ----
def test_perturbation_study_signature_and_table_without_the_ensemble():
    """the new keywords default to off; the table without `ensemble` is the old text, with it four more columns"""
    import inspect
    p = inspect.signature(EV.perturbation_study).parameters
    assert p["ensemble"].default is None and p["frame_chunk"].default is None and p["ensemble_survivors"].default is False
    assert list(p)[-3:] == ["ensemble", "frame_chunk", "ensemble_survivors"] and p["record_body"].default is False
    t = np.arange(50) * 0.01
    ens = dict(t=t, entropy=EV.entropy_curve(t, 0.1, 3.0, 0.3, -10.0))
    st = {k: np.zeros((2, 4)) for k in ("vx_body_mean", "z_mean", "pitch_mean")}
    rows = [dict(mu=0.8, delay=1, cmd=5.0, explorations=4, surviving=1.0, falls=np.zeros(4, int), stats=st, ensemble=ens)]
    old, new = EV.perturbation_table(rows), EV.perturbation_table(rows, ensemble=True)
    assert old == EV.perturbation_table([{k: v for k, v in rows[0].items() if k != "ensemble"}])
    assert [l[:len(o)] for l, o in zip(new.split("\n"), old.split("\n"))] == old.split("\n")
    assert new.split("\n")[0].split()[-4:] == ["H0", "H_last", "kappa", "t_floor"]
    assert [float(v) for v in new.split("\n")[1].split()[-4:]] == [3.0, 1.0, -10.0, 0.3]
    for bad in (dict(ensemble_survivors=True), dict(ensemble=L.SPEC, frame_chunk=0), dict(ensemble=L.SPEC, frame_chunk=8, ensemble_survivors=True),
                dict(ensemble=dict(L.SPEC, prec=(1e-6,) * 6))):
        with pytest.raises(ValueError):                       # refused before a pool is built
            EV.perturbation_study(None, {}, (0.8,), (0,), 1.0, 4, {}, **bad)
