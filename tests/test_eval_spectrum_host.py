"""Host side of the spectrogram and Welch spectrum of recorder columns (irrl_eval_spectrum): the C-ABI surface, every refusal before any HIP
call, the stated size of `work`, the accepted frames < nperseg case, the tables against scipy's windows, the rules of csrc/eval_elements.hpp
compiled as a stand-alone host program (tests/eval_spectrum_main.cpp, plain serial loops in the stated order) under the address and undefined-
behaviour sanitizers against the numpy twin, the twin against scipy.signal.spectrogram and scipy.signal.welch on every generated case, the
planted sines, spectrum_row and the sweep table -- no GPU needed.

The bound of every floating-point comparison is tests/eval_spectrum_lib.py's: derived, not measured."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import eval_spectrum_lib as L
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
def test_abi_surface_of_the_spectrum():
    """header == SIGNATURES for the three new symbols; the struct's ctypes mirror has the header's fields in order, types and sizes; the limits
    agree; the unit is in the build in front of the correlation's"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib, build
    text = _header()
    args = _args(text, "irrl_eval_spectrum")
    assert args == ("const float *x, const uint8_t *rec_done, int rows, int num_envs, int conditions, int robots, int frame_first, int frame_every, "
                    "int frames, const irrl_eval_spectrum_spec *spec, const double *window, const double *tw, int64_t *segments, double *psd_sum, "
                    "double *sxx, double *work, void *hip_stream")
    kinds = lambda a: [C.c_int if x.strip().startswith("int ") else C.c_void_p for x in a.split(",")]
    assert _lib.SIGNATURES["irrl_eval_spectrum"] == (C.c_int, kinds(args))
    assert _args(text, "irrl_eval_spectrum_work", "size_t") == "int num_envs, const irrl_eval_spectrum_spec *spec"
    assert _lib.SIGNATURES["irrl_eval_spectrum_work"] == (C.c_size_t, [C.c_int, C.c_void_p])
    assert _args(text, "irrl_eval_spectrum_tables") == "int nperseg, int window_kind, double alpha, double *window, double *tw"
    assert _lib.SIGNATURES["irrl_eval_spectrum_tables"] == (C.c_int, [C.c_int, C.c_int, C.c_double, _lib.dp, _lib.dp])
    body = re.search(r"typedef struct irrl_eval_spectrum_spec \{(.*?)\} irrl_eval_spectrum_spec;", text, flags=re.S).group(1)
    assert [_flat(d) for d in body.split(";") if d.strip()] == ["int x_dim, x_first, x_count, nperseg, hop, detrend, matrix_count", "int matrix_env[8]",
                                                                "double fs", "double scale[64]"]
    ints = ("x_dim", "x_first", "x_count", "nperseg", "hop", "detrend", "matrix_count")
    assert [(f[0], f[1]) for f in _lib.EvalSpectrumSpec._fields_] == [(k, C.c_int) for k in ints] + [("matrix_env", C.c_int * 8), ("fs", C.c_double),
                                                                                                      ("scale", C.c_double * 64)]
    assert C.sizeof(_lib.EvalSpectrumSpec) == 64 + 8 + 512 and _lib.EvalSpectrumSpec.fs.offset == 64
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    assert (define("IRRL_EVAL_SPECTRUM_MAX_FRAMES"), define("IRRL_EVAL_SPECTRUM_MAX_X"), define("IRRL_EVAL_SPECTRUM_MAX_NPERSEG"),
            define("IRRL_EVAL_SPECTRUM_MAX_MATRICES")) == (EV.SPECTRUM_MAX_FRAMES, EV.SPECTRUM_MAX_X, EV.SPECTRUM_MAX_NPERSEG, EV.SPECTRUM_MAX_MATRICES) \
        == (16384, 64, 1024, 8)
    assert build.PLAIN_UNITS[0] == "irrl_env_abi.hip" and build.PLAIN_UNITS[-2:] == ["eval_spectrum.hip", "eval_correlation.hip"]
    assert EV.SPECTRUM_SOURCES == {"joint": ("obs_cond", 5, 12), "joint_rate": ("obs_cond", 17, 12), "action": ("act_applied", 0, 12)}
    assert EV.SPECTRUM_WINDOWS == {"boxcar": 0, "hann": 1, "tukey": 2}
    assert EV.SPECTRUM_REFERENCE == dict(nperseg=256, hop=224, window="tukey", alpha=0.25, detrend=1, band_hz=50.0)


S_GOOD = dict(x_dim=35, x_first=5, x_count=12, nperseg=16, hop=8, detrend=1, matrix_count=2, matrix_env=(0, 5), fs=100.0, scale=(1.0,) * 12)


def _struct(s):
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib
    st = _lib.EvalSpectrumSpec(**{k: v for k, v in s.items() if k not in ("matrix_env", "scale")})
    for i, e in enumerate(s["matrix_env"]):
        st.matrix_env[i] = e
    for i, v in enumerate(s["scale"]):
        st.scale[i] = v
    return st


def test_spectrum_refusals_and_work_before_any_hip_call():
    """every refusal fires, with the entry point's name in front of the text, although every pointer is a host address no HIP call could take;
    irrl_eval_spectrum_work gives the stated value without a GPU"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib, build
    build.build()
    lib = _lib.load()
    some = C.create_string_buffer(64)
    ptr = C.c_void_p(C.addressof(some))
    good = dict(x=ptr, rec_done=ptr, rows=40, num_envs=6, conditions=2, robots=3, frame_first=0, frame_every=1, frames=40, spec=S_GOOD, window=ptr, tw=ptr,
                segments=ptr, psd_sum=ptr, sxx=ptr, work=ptr)

    def refused(**over):
        a = dict(good, **over)
        st = None if a["spec"] is None else _struct(a["spec"])
        rc = lib.irrl_eval_spectrum(a["x"], a["rec_done"], a["rows"], a["num_envs"], a["conditions"], a["robots"], a["frame_first"], a["frame_every"],
                                    a["frames"], None if st is None else C.cast(C.pointer(st), C.c_void_p), a["window"], a["tw"], a["segments"],
                                    a["psd_sum"], a["sxx"], a["work"], None)
        text = _lib.last_error()
        assert rc != 0 and text.startswith("irrl_eval_spectrum: "), (over, rc, text)
        return text

    S = S_GOOD
    for k in ("x", "spec", "window", "tw", "segments", "psd_sum"):
        assert "NULL" in refused(**{k: None}), k
    assert "x window" in refused(spec=dict(S, x_first=24))
    assert "x window" in refused(spec=dict(S, x_first=-1))
    assert "x_dim" in refused(spec=dict(S, x_dim=0))
    assert "x_count" in refused(spec=dict(S, x_count=0))
    assert "x_count" in refused(spec=dict(S, x_dim=100, x_first=0, x_count=65, scale=(1.0,) * 64))
    assert "nperseg" in refused(spec=dict(S, nperseg=7, hop=4))
    assert "nperseg" in refused(spec=dict(S, nperseg=1025))
    assert "hop" in refused(spec=dict(S, hop=0))
    assert "hop" in refused(spec=dict(S, hop=17))
    assert "detrend" in refused(spec=dict(S, detrend=2))
    assert "detrend" in refused(spec=dict(S, detrend=-1))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert "fs" in refused(spec=dict(S, fs=bad)), bad
        assert "scale" in refused(spec=dict(S, scale=(1.0,) * 11 + (bad,))), bad
    refused_not = dict(S, scale=(1.0,) * 12 + (float("nan"),))          # an entry behind the analysed columns is not read: the next check speaks
    assert "conditions * robots" in refused(spec=refused_not, conditions=4)
    assert "matrix_count" in refused(spec=dict(S, matrix_count=9))
    assert "matrix_count" in refused(spec=dict(S, matrix_count=-1))
    assert "NULL sxx" in refused(sxx=None)
    assert "matrix_env" in refused(spec=dict(S, matrix_env=(0, 6)))
    assert "matrix_env" in refused(spec=dict(S, matrix_env=(-1, 0)))
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
    assert "past the recorder" in refused(frames=41)
    assert "work" in refused(work=None)

    def work(n, s):
        st = None if s is None else _struct(s)
        return lib.irrl_eval_spectrum_work(n, None if st is None else C.cast(C.pointer(st), C.c_void_p))
    assert work(6, S) == 6 * (12 * 9 + 1) == EV.spectrum_work(6, EV.spectrum_spec(35, 5, 12, 16, 8, 100.0))
    assert work(4096, dict(S, nperseg=256, hop=224)) == 4096 * (12 * 129 + 1)
    assert work(6, dict(S, nperseg=9, hop=1)) == 6 * (12 * 5 + 1)
    assert work(0, S) == 0 and work(6, None) == 0 and work(6, dict(S, nperseg=7)) == 0

    # the tables' own refusals
    buf = (C.c_double * 64)()
    for bad, word in (((7, 0, 0.0, buf, buf), "nperseg"), ((1025, 0, 0.0, buf, buf), "nperseg"), ((16, 3, 0.0, buf, buf), "window_kind"),
                      ((16, -1, 0.0, buf, buf), "window_kind"), ((16, 2, float("nan"), buf, buf), "alpha"), ((16, 0, 0.0, None, buf), "NULL"),
                      ((16, 0, 0.0, buf, None), "NULL")):
        assert lib.irrl_eval_spectrum_tables(*bad) != 0
        assert _lib.last_error().startswith("irrl_eval_spectrum_tables: ") and word in _lib.last_error(), bad


def test_fewer_frames_than_a_segment_is_accepted_and_writes_zeros():
    """frames < nperseg: the call launches nothing, sets segments and psd_sum to zero and no error -- exercised with host memory, which the call
    writes itself (tables and x are never read: they are addresses of 64 bytes)"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib, build
    build.build()
    lib = _lib.load()
    some = C.create_string_buffer(64)
    ptr = C.c_void_p(C.addressof(some))
    for conditions, robots in ((6, 1), (2, 3)):
        segments = np.full(conditions + 1, -7, np.int64)
        psd = np.full(conditions * 12 * 9 + 1, np.nan)
        st = _struct(dict(S_GOOD, matrix_count=0, matrix_env=()))
        rc = lib.irrl_eval_spectrum(ptr, ptr, 40, 6, conditions, robots, 3, 2, 15, C.cast(C.pointer(st), C.c_void_p), ptr, ptr,
                                    C.c_void_p(segments.ctypes.data), C.c_void_p(psd.ctypes.data), None, ptr, None)
        assert rc == 0, _lib.last_error()
        assert np.all(segments[:-1] == 0) and segments[-1] == -7                       # and not a word more
        assert np.all(psd[:-1] == 0.0) and not np.any(np.signbit(psd[:-1])) and np.isnan(psd[-1])
    x, done = L.case(16, 15)
    win, tw = L.tables(16, "hann")
    res = EV.spectrum_numpy(x, done, L.spec(16, 5, 1), win, tw, 2, FF, FE, 15)
    assert np.all(res["segments"] == 0) and np.all(res["psd_sum"] == 0.0) and res["sxx"].shape == (4, 5, 0, 9)


def test_spec_and_twin_refusals():
    good = dict(x_dim=7, x_first=2, x_count=5, nperseg=16, hop=5, fs=100.0)
    for bad, word in ((dict(x_count=0), "x_count"), (dict(x_dim=100, x_first=0, x_count=65), "x_count"), (dict(x_first=3), "x window"), (dict(x_dim=0), "x_dim"),
                      (dict(nperseg=7), "nperseg"), (dict(nperseg=1025), "nperseg"), (dict(hop=0), "hop"), (dict(hop=17), "hop"), (dict(detrend=2), "detrend"),
                      (dict(fs=0.0), "fs"), (dict(fs=float("nan")), "fs"), (dict(scale=(1.0,) * 4), "scale"), (dict(scale=(1.0, 1.0, 0.0, 1.0, 1.0)), "scale"),
                      (dict(matrix_env=tuple(range(9))), "matrix_env")):
        with pytest.raises(ValueError, match=word):
            EV.spectrum_spec(**dict(good, **bad))
    s = EV.spectrum_spec(**good)
    assert EV.spectrum_spec(**s) == s and s["scale"] == (1.0,) * 5 and s["detrend"] == 1 and s["matrix_env"] == ()
    x, done = L.case(16, 61)
    win, tw = L.tables(16, "hann")
    with pytest.raises(ValueError, match="conditions"):
        EV.spectrum_numpy(x, done, s, win, tw, 4, FF, FE, 61)
    with pytest.raises(ValueError, match="frames"):
        EV.spectrum_numpy(x, done, s, win, tw, 6, FF, FE, 0)
    with pytest.raises(ValueError):
        EV.spectrum_numpy(x, done, s, win, tw, 6, FF, FE, 63)          # past the recorder's rows
    with pytest.raises(ValueError, match="float32"):
        EV.spectrum_numpy(x.astype(np.float64), done, s, win, tw, 6, FF, FE, 61)
    with pytest.raises(ValueError, match="spectrum_tables"):
        EV.spectrum_numpy(x, done, s, win[:-1], tw, 6, FF, FE, 61)
    with pytest.raises(ValueError, match="matrix_env"):
        EV.spectrum_numpy(x, done, dict(s, matrix_env=(6,)), win, tw, 6, FF, FE, 61)
    with pytest.raises(KeyError):
        EV.spectrum_tables(16, "kaiser")
    with pytest.raises(ValueError, match="nperseg"):
        EV.spectrum_tables(7)


# ---- the tables ----
@pytest.mark.parametrize("nperseg", (8, 9, 12, 16, 256, 1000, 1024))
def test_tables_against_scipy(nperseg):
    """boxcar, periodic Hann and periodic Tukey as scipy.signal.get_window gives them (fftbins=True, what spectrogram and welch use); the twiddles
    against numpy's cos, sin.  The formulas are scipy's, the order of their operations need not be: either side rounds the cosine's argument, at
    most 2 pi in size, in up to four operations of 2^-53 relative error each, and the cosine's slope is at most 1, so the two sides differ by at
    most 8 * 2 pi * 2^-53 = 5.6e-15 (the cosine's own rounding and the final 0.5 (1 + .) are below a tenth of that)."""
    sig = pytest.importorskip("scipy.signal")
    tol = 8 * 2 * np.pi * 2.0 ** -53
    for name, alpha, ref in (("boxcar", 0.0, "boxcar"), ("hann", 0.0, "hann"), ("tukey", 0.25, ("tukey", 0.25)), ("tukey", 0.6, ("tukey", 0.6)),
                             ("tukey", 0.0, "boxcar"), ("tukey", 1.0, "hann"), ("tukey", 1.5, "hann"), ("tukey", -1.0, "boxcar")):
        win, tw = EV.spectrum_tables(nperseg, name, alpha)
        want = sig.get_window(ref, nperseg)
        assert win.shape == (nperseg,) and np.abs(win - want).max() <= tol, (name, alpha, np.abs(win - want).max())
    j = np.arange(nperseg)
    assert tw.shape == (nperseg, 2) and np.abs(tw[:, 0] - np.cos(2 * np.pi * j / nperseg)).max() <= tol
    assert np.abs(tw[:, 1] - np.sin(2 * np.pi * j / nperseg)).max() <= tol
    assert tw[0, 0] == 1.0 and tw[0, 1] == 0.0
    assert np.all(EV.spectrum_tables(nperseg, "boxcar")[0] == 1.0)


# ---- the host program on the shared element functions ----
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host program"
    out = str(tmp_path_factory.mktemp("eval_spectrum_main") / "eval_spectrum_main")
    csrc = os.path.join(ROOT, "high_speed_quadrupedal_locomotion_by_irrl_amd", "csrc")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=on", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                           "-I" + csrc, os.path.join(ROOT, "tests", "eval_spectrum_main.cpp"), "-o", out])
    return out


def run_program(program, tmp_path, x, done, s, window, tw, conditions, T):
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    L.write_case(src, x, done, s, window, tw, conditions, FF, FE, T)
    r = subprocess.run([program, src, dst], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    return L.read_result(dst, conditions, s, T)


@pytest.mark.parametrize("nperseg,hop,T,conditions,detrend,window", L.cases())
def test_program_against_the_twin(program, tmp_path, nperseg, hop, T, conditions, detrend, window):
    """the sanitized program's serial loops over the header's text against the twin on all three outputs, with and without rec_done: segments
    equal, a NaN in the same places, the rest within the bound -- and, since neither the host compiler (no fused multiply-add on plain x86-64)
    nor numpy fuses, bit for bit; S_e is what the case planted; the constant column's spectrum is zero up to the bound"""
    x, done = L.case(nperseg, T)
    s = L.spec(nperseg, hop, detrend)
    win, tw = L.tables(nperseg, window)
    for with_done in (True, False):
        what = (nperseg, hop, T, conditions, detrend, window, with_done)
        want = L.twin(nperseg, hop, T, conditions, detrend, window, with_done)
        got = run_program(program, tmp_path, x, done if with_done else None, s, win, tw, conditions, T)
        bound = L.bounds(want, nperseg, window, conditions)
        L.within(got, want, bound, what)
        L.same_bytes(got, want, what)
        assert got["work_per_env"] * L.N == EV.spectrum_work(L.N, s)
        S = L.expected_segments(done if with_done else None, T, nperseg, hop)
        assert np.array_equal(want["segments"], S.reshape(conditions, L.N // conditions).sum(1))
        if with_done and T == 61:
            assert S[1] == 0 and S[4] == 0 and S[2] == (nperseg + 2 - nperseg) // hop + 1 and S[0] == (61 - nperseg) // hop + 1
        if detrend:
            assert np.all(want["psd_sum"][:, 2] <= bound["psd_sum"][:, 2])           # the constant column
        for m, e in enumerate(L.MATRIX_ENV):                                       # the segments a robot did not live to see are zeros
            assert np.all(want["sxx"][m, :, S[e]:] == 0.0)
        assert want["sxx"][0].tobytes() == want["sxx"][2].tobytes()                  # the robot listed twice
        # the NaN of robot 0, column 4: the segments that hold its frame, the sum of its condition and column, and nothing else
        frame = min(T - 1, 20)
        hit = [seg for seg in range(S[0]) if seg * hop <= frame < seg * hop + nperseg]
        in_sum, in_sxx = np.zeros(want["psd_sum"].shape, bool), np.zeros(want["sxx"].shape, bool)
        in_sum[0, 4] = bool(hit)
        in_sxx[1, 4, hit] = True
        assert np.array_equal(np.isnan(want["psd_sum"]), in_sum) and np.array_equal(np.isnan(want["sxx"]), in_sxx)
        assert bool(hit) == (T >= nperseg)


def test_tables_and_refusals_inside_the_sanitized_program(program, tmp_path):
    dst = str(tmp_path / "tables.bin")
    for nperseg, kind, alpha, name in ((16, 2, 0.25, "tukey"), (9, 1, 0.0, "hann"), (1024, 2, 0.25, "tukey"), (12, 0, 0.0, "boxcar")):
        r = subprocess.run([program, "tables", str(nperseg), str(kind), repr(alpha), dst], stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()
        got = np.fromfile(dst, np.float64)
        win, tw = EV.spectrum_tables(nperseg, name, alpha)
        assert got.shape == (3 * nperseg,)
        assert np.abs(got[:nperseg] - win).max() <= 2.0 ** -52 and np.abs(got[nperseg:] - tw.reshape(-1)).max() <= 2.0 ** -52
    r = subprocess.run([program, "tables", "7", "0", "0.0", dst], stderr=subprocess.PIPE)
    assert r.returncode == 3 and b"nperseg" in r.stderr
    x, done = L.case(16, 16)
    win, tw = L.tables(16, "hann")
    src, out = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    L.write_case(src, x, done, dict(L.spec(16, 5, 1), hop=17), win, tw, 6, FF, FE, 16)
    r = subprocess.run([program, src, out], stderr=subprocess.PIPE)
    assert r.returncode == 3 and b"hop" in r.stderr and not os.path.exists(out)


# ---- the twin against scipy ----
@pytest.mark.parametrize("nperseg,hop,T,conditions,detrend,window", L.cases())
def test_twin_against_scipy_spectrogram_and_welch(nperseg, hop, T, conditions, detrend, window):
    """robot by robot and column by column: scipy.signal.spectrogram(mode='psd', scaling='density', return_onesided=True, nfft=nperseg, noverlap =
    nperseg - hop) of the frames i < T_e with THE SAME window array == the twin's segments (sxx, and summed psd_sum) within the bound, NaN in the
    same places; scipy.signal.welch == psd_sum / segments for the per-robot grouping"""
    sig = pytest.importorskip("scipy.signal")
    x, done = L.case(nperseg, T)
    win, _ = L.tables(nperseg, window)
    want = L.twin(nperseg, hop, T, conditions, detrend, window)
    bound = L.bounds(want, nperseg, window, conditions)
    S = L.expected_segments(done, T, nperseg, hop)
    sel = FF + FE * np.arange(T)
    dn = done[sel] != 0
    te = np.where(dn.any(0), dn.argmax(0), T)
    K = nperseg // 2 + 1
    kw = dict(fs=L.FS, window=win, nperseg=nperseg, noverlap=nperseg - hop, nfft=nperseg, detrend="constant" if detrend else False, return_onesided=True,
              scaling="density")
    total = np.zeros((L.N, L.X_COUNT, K))
    worst = 0.0
    for e in range(L.N):
        if S[e] == 0:
            continue
        for c in range(L.X_COUNT):
            v = x[sel[:te[e]], e, L.X_FIRST + c].astype(np.float64) * L.SCALE[c]
            with np.errstate(invalid="ignore"):
                f, t, sxx = sig.spectrogram(v, mode="psd", **kw)
                fw, pw = sig.welch(v, average="mean", **kw)
            assert sxx.shape == (K, S[e]) and np.allclose(f, EV.spectrum_frequencies(nperseg, L.FS), rtol=1e-15, atol=0)
            total[e, c] = sxx.sum(1)
            for m, em in enumerate(L.MATRIX_ENV):
                if em == e:
                    got, b = want["sxx"][m, c, :S[e]], bound["sxx"][m, c, :S[e]]
                    nan = np.isnan(got)
                    assert np.array_equal(nan, np.isnan(sxx.T))
                    err = np.abs(got - sxx.T)[~nan]
                    assert np.all(err <= b[~nan]), (e, c, err.max())
                    worst = max(worst, float((err[err > 0] / b[~nan][err > 0]).max()) if (err > 0).any() else 0.0)
            if conditions == L.N:
                got, b = want["psd_sum"][e, c] / S[e], bound["psd_sum"][e, c] / S[e]
                nan = np.isnan(got)
                assert np.array_equal(nan, np.isnan(pw)) and np.all(np.abs(got - pw)[~nan] <= b[~nan]), (e, c)
    pooled = total.reshape(conditions, L.N // conditions, L.X_COUNT, K).sum(1)
    nan = np.isnan(want["psd_sum"])
    assert np.array_equal(nan, np.isnan(pooled))
    assert np.all(np.abs(want["psd_sum"] - pooled)[~nan] <= bound["psd_sum"][~nan])
    print("largest |twin - scipy| / bound over the spectrograms: %.3g" % worst)


def test_planted_sines_peak_and_parseval():
    """boxcar, detrend, nperseg 16, hop 16: the sine at the exact bin 3 has all its power there (every other bin is zero up to the bound), the one
    between the bins 2 and 3 leaks into its neighbours with its peak at one of the two; for both, sum_k P_k fs / nperseg is the detrended segment's
    mean square (Parseval: the density integrates to the variance)"""
    P, hop, T = 16, 16, 61
    want = L.twin(P, hop, T, 6, 1, "boxcar", with_done=False)
    bound = L.bounds(want, P, "boxcar", 6)
    x, _ = L.case(P, T)
    df = L.FS / P
    for e in range(L.N):
        sxx = EV.spectrum_numpy(x, None, L.spec(P, hop, 1, matrix_env=(e,)), *L.tables(P, "boxcar"), frame_first=FF, frame_every=FE, frames=T)["sxx"][0]
        b = L.bounds(want, P, "boxcar", 6, matrix_env=(e,))["sxx"][0]
        for seg in range(sxx.shape[1]):
            exact, between = sxx[0, seg], sxx[1, seg]
            assert exact.argmax() == 3 and between.argmax() in (2, 3)
            others = np.delete(np.arange(P // 2 + 1), 3)
            assert np.all(exact[others] <= b[0, seg, others])
            assert abs(exact[3] * df - (1.3 * L.SCALE[0]) ** 2 / 2) <= 1e-6 * exact[3] * df      # amplitude^2 / 2, to the f32 rounding of the samples
            assert between[1] > b[1, seg, 1] and between[4] > b[1, seg, 4]                      # leakage is real
            for c in range(L.X_COUNT - 1):                                                     # (column 4 of robot 0 holds the NaN)
                a = want["a"][e, seg, c]
                assert abs(sxx[c, seg].sum() * df - np.mean(a * a)) <= b[c, seg].sum() * df + 4 * P * L.U * np.mean(a * a), (e, seg, c)


def test_spectrum_row():
    """a spectrum with its peak planted at bin 5 of 9 (nperseg 16, fs 100: 31.25 Hz) and a known share above 30 Hz; bin 0 is ignored however
    large; no segment or no power gives NaN; the odd nperseg has to be named"""
    K = 9
    p = np.zeros((12, K))
    p[:, 0] = 1e9
    p[:, 2] = 1.0
    p[3, 5] = 40.0
    p[:, 7] = 0.5
    row = EV.spectrum_row(dict(joint=p * 4, action=np.zeros((12, K))), dict(joint=4, action=4), 100.0, ("joint", "action"), 30.0)
    assert row["vib_peak_hz_joint"] == 5 * 100.0 / 16 and row["vib_frac_joint"] == pytest.approx((40.0 + 6.0) / (12.0 + 40.0 + 6.0), rel=1e-15)
    assert np.isnan(row["vib_peak_hz_action"]) and np.isnan(row["vib_frac_action"])
    assert EV.spectrum_row(dict(joint=p), 1, 100.0, ("joint",), 50.0)["vib_frac_joint"] == 0.0           # (bin 8 = 50 Hz is not ABOVE 50 Hz)
    none = EV.spectrum_row(dict(joint=p), 0, 100.0, ("joint",), 30.0)
    assert np.isnan(none["vib_peak_hz_joint"]) and np.isnan(none["vib_frac_joint"])
    nan = EV.spectrum_row(dict(joint=np.where(p == 40.0, np.nan, p)), 1, 100.0, ("joint",), 30.0)
    assert np.isnan(nan["vib_peak_hz_joint"]) and np.isnan(nan["vib_frac_joint"])
    odd = EV.spectrum_row(dict(joint=p), 1, 100.0, ("joint",), 30.0, nperseg=17)
    assert odd["vib_peak_hz_joint"] == pytest.approx(5 * 100.0 / 17)
    with pytest.raises(ValueError, match="bins"):
        EV.spectrum_row(dict(joint=p), 1, 100.0, ("joint",), 30.0, nperseg=12)
    assert np.array_equal(EV.spectrum_frequencies(16, 100.0), np.arange(9) * 6.25)
    # the twin's sums of a planted case through the row: the exact-bin sine of nperseg 16 at fs 100 peaks at 18.75 Hz
    want = L.twin(16, 5, 61, 6, 1, "hann", with_done=False)
    row = EV.spectrum_row(dict(sine=want["psd_sum"][3, 0:1]), int(want["segments"][3]), L.FS, ("sine",), 30.0)
    assert row["vib_peak_hz_sine"] == 18.75 and 0.0 <= row["vib_frac_sine"] < 1e-6


def test_sweep_table_gains_the_two_columns_per_source():
    base = dict(mu=0.8, delay=0, cmd=2.0, falls=0, vx_body_mean=1.9, vx_body_std=0.1, z_mean=0.3, z_std=0.01, roll_std=0.01, pitch_mean=0.0,
                pitch_std=0.01, yaw_rate_mean=0.0)
    vib = {"vib_peak_hz_joint": 3.125, "vib_frac_joint": 0.001, "vib_peak_hz_joint_rate": 46.875, "vib_frac_joint_rate": 0.25,
           "vib_peak_hz_action": float("nan"), "vib_frac_action": float("nan")}
    rows = [dict(base, **vib)]
    plain, table = EV.sweep_table(rows).split("\n"), EV.sweep_table(rows, spectrum=True).split("\n")
    assert [t.startswith(p) for p, t in zip(plain, table)] == [True] * 2
    assert table[0].split()[-6:] == ["vib_peak_hz_joint", "vib_frac_joint", "vib_peak_hz_joint_rate", "vib_frac_joint_rate", "vib_peak_hz_action",
                                     "vib_frac_action"] == list(EV.spectrum_table_keys())
    assert table[1].split()[-6:] == ["+3.1250", "+0.0010", "+46.8750", "+0.2500", "+nan", "+nan"]
    assert EV.sweep_table(rows, spectrum=("action",)).split("\n")[0].split()[-2:] == ["vib_peak_hz_action", "vib_frac_action"]
