"""The ensemble analysis of a body recorder (evaluate.ensemble_device -> irrl_eval_ensemble: one workgroup per (condition, frame) sorts the
condition's cell keys in LDS) on the MI355X against the float64 twin (evaluate.ensemble_numpy), and the perturbation study that carries it.

(a) the generated recorders of tests/eval_ensemble_lib.py, uploaded: [F, 3 * E, 13] with E = 1, 37, 256, 257 (one past a power of two: the padding),
    1000 and 10 000 (the 128 KB sort; F = 2 there, 7 elsewhere).  No sample lies on a cell edge (asserted), so kept, occupied, largest and hist are
    equal as integers, the entropy agrees within 1e-12 * max(1, ln M), the moments within 1e-12 relative.
(b) the closed loop: perturbation_study on frictions 0.8 / 0.1 x delays 0 / 1 x 24 explorations (the two named conditions and the two mixed ones
    of the grid the study builds: 96 robots), 300 warm-up steps, a tenth of the Param amplitudes (tests/test_gpu_eval_kick.py's choice), 40 frames.
    These trajectories come from the GPU: a (condition, frame) entry in which the twin finds a sample on a cell edge is left out of the comparison,
    and the test fails if more than 1 % of the entries are."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_ensemble_lib as L
import test_gpu_eval_persistent as TP
from conftest import load_env_cfg
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV

SPEC = L.SPEC
NOISE = dict(z_noise=0.02, roll_noise=0.25, pitch_noise=0.25, z_dot_noise=1.0, roll_dot_noise=1.0, pitch_dot_noise=1.0)      # Exp_Raw_Data/Param-*.txt
BITS = ("entropy", "kept", "occupied", "largest", "hist")      # what the sort makes order-independent


def _device(body, **kw):
    res = EV.ensemble_to_numpy(EV.ensemble_device(torch.from_numpy(np.ascontiguousarray(body)).cuda(), L.C, kw.pop("spec", SPEC), **kw))
    return res


def _same_bits(a, b, keys):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


# ---- (a) generated recorders ----
@pytest.mark.parametrize("E", [1, 37, 256, 257, 1000, 10000])
def test_device_equals_the_twin_and_is_order_independent(E):
    """ensemble_device against ensemble_numpy under the file's rule; a second run is the first bit for bit (moments included); with every
    condition's explorations permuted, entropy, counters and histograms are the same bits and the moments agree within 1e-12 relative"""
    F = 2 if E == 10000 else L.F_HOST
    body = L.ensemble_case(L.SEED, F, L.C, E)
    L.assert_no_edges(body)
    want = EV.ensemble_numpy(body, L.C, SPEC)
    got = _device(body)
    print("E = %d: max |H - twin| = %.3g, H(frame 0) = %s (ln E = %.6f)" % (E, np.abs(got["entropy"] - want["entropy"]).max(), got["entropy"][:, 0], np.log(E)))
    L.assert_same_result(got, want, "E = %d" % E)
    assert np.all(got["kept"] == E) and np.all(got["largest"][:, 1] == E) and np.all(got["entropy"][:, 1] == 0.0)
    _same_bits(_device(body), got, BITS + ("moments",))
    rng = np.random.RandomState(E)
    perm = np.concatenate([c * E + rng.permutation(E) for c in range(L.C)])
    again = _device(body[:, perm])
    _same_bits(again, got, BITS)
    assert np.all(np.abs(again["moments"] - got["moments"]) <= 1e-12 * np.abs(got["moments"]))


@pytest.mark.parametrize("E", [37, 257])
def test_mask_nonfinite_strides_and_optional_outputs(E):
    """a mask (one condition masked out entirely: M = 0, H = 0, zero counts) and non-finite rows take samples out of M; frame_first / frame_every /
    frames pick their rows; hist=False (NULL), moments=False (NULL) and hist_bins = 0 leave the other outputs what they were"""
    body = L.ensemble_case(L.SEED, L.F_HOST, L.C, E)
    n = L.C * E
    rng = np.random.RandomState(3)
    mask = (rng.uniform(size=n) < 0.7).astype(np.uint8)
    mask[E:2 * E] = 0
    bad = body.copy()
    bad[0, 2, 2] = np.nan
    bad[0, 3, 9] = np.inf
    bad[3, 5, 3:7] = np.nan
    bad[4, 2 * E + 1, 12] = -np.inf
    want = EV.ensemble_numpy(bad, L.C, SPEC, mask=mask)
    got = _device(bad, mask=torch.from_numpy(mask).cuda())
    L.assert_same_result(got, want, "mask + non-finite")
    assert np.all(got["kept"][1] == 0) and np.all(got["entropy"][1] == 0) and np.all(got["occupied"][1] == 0) and np.all(got["hist"][1] == 0)
    assert got["kept"][0, 0] == int(mask[:E].sum()) - int(mask[2]) - int(mask[3]) and np.all(np.isfinite(got["moments"]))
    full = _device(body)
    part = _device(body, frame_first=1, frame_every=2)
    assert part["entropy"].shape == (L.C, 3)
    _same_bits(part, {k: np.ascontiguousarray(v[:, 1::2]) for k, v in full.items()}, BITS + ("moments",))
    one = _device(body, frame_first=2, frame_every=3, frames=1)
    _same_bits(one, {k: np.ascontiguousarray(v[:, 2:3]) for k, v in full.items()}, BITS + ("moments",))
    rest = ("entropy", "kept", "occupied", "largest")
    a = _device(body, hist=False)
    assert a["hist"] is None
    _same_bits(a, full, rest + ("moments",))
    b = _device(body, moments=False)
    assert b["moments"] is None
    _same_bits(b, full, BITS)
    c = _device(body, spec=dict(SPEC, hist_bins=0))
    assert c["hist"] is None
    _same_bits(c, full, rest + ("moments",))
    with pytest.raises(ValueError):
        _device(body, frame_first=1, frames=L.F_HOST)


def test_on_a_callers_stream():
    """the launch goes to torch's current stream: a call under torch.cuda.stream(s) behind a fill on s sees the filled recorder, and gives the
    default stream's result"""
    E = 257
    body = L.ensemble_case(L.SEED, L.F_HOST, L.C, E)
    want = _device(body)
    s = torch.cuda.Stream()
    host = torch.from_numpy(body).pin_memory()
    with torch.cuda.stream(s):
        dev = torch.empty(body.shape, device="cuda", dtype=torch.float32)
        dev.copy_(host, non_blocking=True)
        res = EV.ensemble_device(dev, L.C, SPEC)
    s.synchronize()
    _same_bits(EV.ensemble_to_numpy(res), want, BITS + ("moments",))


# ---- (b) the closed loop ----
MUS, DELAYS, CMD, E_LOOP, WARM, FRAMES, SEED, SCALE = (0.8, 0.1), (0, 1), 5.0, 24, 300, 40, 7, 0.1
OLD_KEYS = {"mu", "delay", "cmd", "explorations", "surviving", "falls", "stats", "kicks", "body"}


def _study(**kw):
    n = len(MUS) * len(DELAYS) * E_LOOP
    cfg = load_env_cfg("bp5_manual_eval.yaml", num_envs=n)
    noise = {k: SCALE * v for k, v in NOISE.items()}
    return EV.perturbation_study(TP.ACTOR, cfg, MUS, DELAYS, CMD, E_LOOP, noise, warm_steps=WARM, frames=FRAMES, seed=SEED, record_body=True,
                                 persistent="auto", **kw), cfg


def _flat(v, path=""):
    if isinstance(v, dict):
        for k in sorted(v):
            yield from _flat(v[k], path + "/" + str(k))
    else:
        yield path, v


def _rows_same_bits(a, b, what):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        fa, fb = dict(_flat(ra)), dict(_flat(rb))
        assert sorted(fa) == sorted(fb), what
        for k in fa:
            x, y = fa[k], fb[k]
            if isinstance(x, np.ndarray):
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)
            else:
                assert x == y or (x is None and y is None), (what, k)


def _compare_with_twin(rows, cfg, mask=None):
    body = np.concatenate([r["body"] for r in rows], 1)
    want = EV.ensemble_numpy(body, len(rows), SPEC, mask=mask)
    x = EV.ensemble_features(body)
    edge = EV.ensemble_edges(x, SPEC) | L.histogram_edges(np.where(np.isfinite(x), x, 0.0), SPEC).any(-1)
    skip = edge.reshape(FRAMES, len(rows), E_LOOP).any(2).T                      # [C, F]
    print("entries left out for a sample on an edge: %d of %d" % (skip.sum(), skip.size))
    assert skip.mean() <= 0.01
    dt = float(cfg["control_dt"])
    for c, r in enumerate(rows):
        e, w = r["ensemble"], EV.ensemble_row(want, c, dt)
        assert set(e) == {"t", "entropy", "kept", "occupied", "largest", "hist", "mean", "std"}
        assert np.array_equal(e["t"], np.arange(FRAMES) * dt)
        keep = ~skip[c]
        for k in ("kept", "occupied", "largest", "hist"):
            assert np.array_equal(np.asarray(e[k], np.int64)[keep], np.asarray(w[k], np.int64)[keep]), (c, k)
        m = np.maximum(np.asarray(w["kept"], np.float64), 1.0)
        assert np.all(np.abs(e["entropy"] - w["entropy"])[keep] <= (1e-12 * np.maximum(1.0, np.log(m)))[keep]), c
        # the moments within 1e-12 relative, seen through mean = S1 / M and std^2 = S2 / M - mean^2
        assert np.all(np.abs(e["mean"] - w["mean"])[keep] <= 1e-12 * np.abs(w["mean"])[keep]), c
        s2 = want["moments"][c][:, :, 1] / m[:, None]
        assert np.all(np.abs(e["std"] ** 2 - w["std"] ** 2)[keep] <= 4e-12 * s2[keep]), c
    return want


def test_perturbation_study_ensemble_chunks_and_default():
    """the row's `ensemble` equals the twin on the row's own body recorder; frame_chunk = 16 (chunks of 16, 16 and 8 steps) equals the unchunked
    run bit for bit, every older key of the row included; without `ensemble` the rows have today's keys and the same bits"""
    rows, cfg = _study(ensemble=SPEC)
    assert len(rows) == 4 and all(set(r) == OLD_KEYS | {"ensemble"} for r in rows)
    want = _compare_with_twin(rows, cfg)
    h = np.stack([r["ensemble"]["entropy"] for r in rows])
    print("H per condition, frames 0 / 10 / 39: %s (ln 24 = %.4f); occupied at frame 39: %s" % (h[:, [0, 10, 39]].round(4).tolist(), np.log(E_LOOP), want["occupied"][:, 39].tolist()))
    assert np.all(want["kept"] == E_LOOP) and all(r["surviving"] == 1.0 for r in rows)
    chunked, _ = _study(ensemble=SPEC, frame_chunk=16)
    _rows_same_bits(chunked, rows, "frame_chunk = 16")
    plain, _ = _study()
    assert all(set(r) == OLD_KEYS for r in plain)
    _rows_same_bits(plain, [{k: v for k, v in r.items() if k != "ensemble"} for r in rows], "ensemble = None")


def test_perturbation_study_survivors_mask():
    """ensemble_survivors: exploration 5 of condition 0 is kicked over (a roll of 1.5 rad: its episode ends on the step the kick hits), the mask
    takes it out of `kept` in every frame, and the analysis equals the twin's with that mask; together with frame_chunk it is refused"""
    n = len(MUS) * len(DELAYS) * E_LOOP
    noise = {k: SCALE * v for k, v in NOISE.items()}
    kicks = EV.exploration_kicks(n, noise, np.random.default_rng(SEED))
    kicks[5] = EV.kick_rows(roll=[1.5])[0]
    rows, cfg = _study(ensemble=SPEC, ensemble_survivors=True, kicks=kicks)
    falls = np.concatenate([r["falls"] for r in rows])
    assert falls[5] >= 1 and falls.sum() == falls[5] and abs(rows[0]["surviving"] - (1.0 - 1.0 / E_LOOP)) < 1e-12
    up = falls == 0
    _compare_with_twin(rows, cfg, mask=up.astype(np.uint8))
    for c, r in enumerate(rows):
        assert np.all(r["ensemble"]["kept"] == up[c * E_LOOP:(c + 1) * E_LOOP].sum())
    assert np.all(rows[0]["ensemble"]["kept"] == E_LOOP - 1)
    with pytest.raises(ValueError):
        _study(ensemble=SPEC, ensemble_survivors=True, frame_chunk=16)
