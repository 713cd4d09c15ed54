"""CPU side of tests/test_gpu_lstm_forms.py: the inputs and the float64 reference that module relies on, checked without a GPU.

  * every case of the shared lists (lstm_forms_lib): the eager definition in f32 stays under ONE QUARTER of the bound the kernels are held to,
    per tensor -- the inputs are conditioned well enough for the bound to mean something;
  * the float64 eager forward equals an independent numpy recurrence;
  * the saturated-gate inputs are saturated; the float64 model of the bf16x3 operand split behaves like a ~2^-16 arithmetic;
  * the entry points refuse the observation widths the policy-step kernels are not written for, before any launch.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import lstm_forms_lib as L
from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import SBLstm


@pytest.mark.parametrize("case", L.ALL_SEQ_CASES, ids=L.case_id)
def test_eager_f32_stays_under_a_quarter_of_the_kernel_bound(case):
    layer, x, state, masks, wgt = L.make_seq_inputs(case)
    ref = L.reference_sequence(layer, x, state, masks, wgt, case.need_dx)
    out = L.eager_sequence(layer, x, state, masks, wgt, case.need_dx)
    assert SBLstm.use_fused
    assert ("dx" in ref) == case.need_dx and all(torch.isfinite(v).all() for k, v in ref.items() if k != "_fn")
    errs = L.rel_errors(out, ref)
    print("\n[lstm eager f32 on the CPU, %s] max |f32 - float64| / max |float64|: %s" % (L.case_id(case), L.fmt(errs)))
    for name, e in errs.items():
        assert e <= 0.25 * L.BOUNDS[case.prec], (L.case_id(case), name, e)
    if case.mask == "ones":
        assert not ref["dwh"].any() and not out["dwh"].any()
    else:
        assert all(float(ref[k].abs().max()) > 0 for k in errs)


@pytest.mark.parametrize("pc", L.POLICY_CASES, ids=L.case_id)
def test_eager_f32_policy_stays_under_a_quarter_of_the_kernel_bound(pc):
    args = L.make_policy_inputs(pc)
    nlp64, val64, g64 = L.reference_policy(*args)
    nlp, val, g = L.eager_policy(*args)
    errs = {k: L.rel_err(g[k], g64[k]) for k in L.POLICY_PARAM_NAMES}
    errs.update(nlp=L.rel_err(nlp, nlp64), val=L.rel_err(val, val64))
    print("\n[lstm policy %s eager f32 on the CPU] %s" % (L.case_id(pc), L.fmt(errs)))
    for name, e in errs.items():
        assert e <= 0.25 * 2e-5, (name, e)
    assert all(float(v.abs().max()) > 0 for v in g64.values())


@pytest.mark.parametrize("fc", L.F_LSTM_CASES, ids=L.case_id)
def test_eager_f32_lstm_step_stays_under_a_quarter_of_the_kernel_bound(fc):
    pol, obs, st, dones, noise = L.make_lstm_step_inputs(fc)
    ref = dict(zip(("action", "value", "state", "neglogp"), L.lstm_step_reference(pol, obs, st, dones, noise)))
    out = dict(zip(("action", "value", "state", "neglogp"), L.lstm_step_reference(pol, obs, st, dones, noise, dtype=torch.float32)))
    for name, e in L.step_errors(out, ref).items():
        assert e <= 0.25 * L.STEP_TOL[name], (fc, name, e)
    assert 0 < int(dones.sum()) < fc[2]          # the draw has both kinds of rows


@pytest.mark.parametrize("fc", L.F_MLP_CASES, ids=L.case_id)
def test_eager_f32_mlp_step_stays_under_a_quarter_of_the_kernel_bound(fc):
    pol, obs, dones, noise = L.make_mlp_step_inputs(fc)
    ref = dict(zip(("action", "value", "neglogp"), L.mlp_step_reference(pol, obs, noise)))
    out = dict(zip(("action", "value", "neglogp"), L.mlp_step_reference(pol, obs, noise, dtype=torch.float32)))
    for name, e in L.step_errors(out, ref).items():
        assert e <= 0.25 * L.STEP_TOL[name], (fc, name, e)


@pytest.mark.parametrize("gc", L.G_LSTM_CASES, ids=L.case_id)
def test_lstm_step_reference_at_other_action_widths(gc):
    """group G: the float64 step reference returns tensors of the asked width, the eager f32 step stays under a quarter of the kernel bound, and
    the width-12 draw is the F cases' draw (the action width enters the seed only when it is not 12)"""
    hid, A, N = gc
    pol, obs, st, dones, noise = L.make_lstm_step_inputs((hid, L.G_OB, N), act=A)
    assert pol.act_dim == A and noise.shape == (N, A) and obs.shape == (N, L.G_OB) and pol.logstd.shape == (1, A)
    ref = dict(zip(("action", "value", "state", "neglogp"), L.lstm_step_reference(pol, obs, st, dones, noise)))
    assert ref["action"].shape == (N, A) and ref["value"].shape == (N,) and ref["state"].shape == (N, 8 * hid) and ref["neglogp"].shape == (N,)
    assert all(v.dtype == torch.float64 and torch.isfinite(v).all() for v in ref.values())
    out = dict(zip(("action", "value", "state", "neglogp"), L.lstm_step_reference(pol, obs, st, dones, noise, dtype=torch.float32)))
    for name, e in L.step_errors(out, ref).items():
        assert e <= 0.25 * L.STEP_TOL[name], (gc, name, e)
    assert 0 < int(dones.sum()) < N
    assert (16 * A + 16 <= 8 * hid) and A <= 16


@pytest.mark.parametrize("gc", L.G_MLP_CASES, ids=L.case_id)
def test_mlp_step_reference_at_other_action_widths(gc):
    A, N = gc
    pol, obs, dones, noise = L.make_mlp_step_inputs((L.G_OB, N), act=A)
    assert pol.act_dim == A and noise.shape == (N, A) and pol.logstd.shape == (1, A)
    ref = dict(zip(("action", "value", "neglogp"), L.mlp_step_reference(pol, obs, noise)))
    assert ref["action"].shape == (N, A) and ref["value"].shape == (N,) and ref["neglogp"].shape == (N,)
    out = dict(zip(("action", "value", "neglogp"), L.mlp_step_reference(pol, obs, noise, dtype=torch.float32)))
    for name, e in L.step_errors(out, ref).items():
        assert e <= 0.25 * L.STEP_TOL[name], (gc, name, e)
    assert 4 * A + 4 <= 64


def test_action_width_twelve_keeps_the_draws_of_the_observation_width_cases():
    a = L.make_lstm_step_inputs(L.F_LSTM_CASES[0])
    b = L.make_lstm_step_inputs(L.F_LSTM_CASES[0], act=12)
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])) and all(torch.equal(x, y) for x, y in zip(a[0].parameters(), b[0].parameters()))
    c = L.make_lstm_step_inputs(L.F_LSTM_CASES[0], act=5)
    assert not torch.equal(a[1], c[1])
    a, b = L.make_mlp_step_inputs(L.F_MLP_CASES[0]), L.make_mlp_step_inputs(L.F_MLP_CASES[0], act=12)
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    assert L.G_LSTM_REFUSED == (32, 16) and 16 * 16 + 16 > 8 * 32 and 16 * 15 + 16 == 8 * 32 and 4 * 15 + 4 == 64 and L.G_MLP_REFUSED == 16


@pytest.mark.parametrize("act", [1, 5, 15, 16])
def test_sampler_reference_at_other_action_widths_is_the_oracle_generator(act):
    """rollout_replay_lib.sampler_reference(..., act_dim): slot a comes from Philox block a >> 2 (purpose word 0x50 + block, up to 0x53 for slots
    12 .. 15) of the oracle's independent C statement of the generator, through Box-Muller on (u0, u1) and (u2, u3)"""
    import oracle as O
    import rollout_replay_lib as R
    seed, step = L.G_RNG_SEED, L.G_RNG_STEP + 3
    envs = np.array([0, 6, 39]) + L.G_RNG_ENV0
    z = R.sampler_reference(seed, envs, step, act)
    assert z.shape == (3, act)
    for i, env in enumerate(envs):
        want = []
        for q in range((act + 3) // 4):
            u = O.rng_u01(seed, int(env), step >> 32, step & 0xFFFFFFFF, 0x50 + q)
            for a, b in ((u[0], u[1]), (u[2], u[3])):
                r = np.sqrt(-2.0 * np.log(1.0 - a))
                want += [r * np.cos(2 * np.pi * b), r * np.sin(2 * np.pi * b)]
        assert (act + 3) // 4 - 1 == (act - 1) >> 2 <= 3
        assert np.abs(z[i] - np.array(want[:act])).max() < 1e-12, (env, act)
    # a narrower policy draws the front of a wider one's noise
    assert np.array_equal(z, R.sampler_reference(seed, envs, step, 16)[:, :act])


@pytest.mark.parametrize("case", [L.A_CASES[1], L.D_CASES[1]], ids=L.case_id)
def test_float64_eager_forward_equals_an_independent_numpy_recurrence(case):
    """pins the reference itself: (9, 40, 35, 48) with random episode starts, and (9, 16, 35, 48) with a start at t = 0 only"""
    layer, x, state, masks, wgt = L.make_seq_inputs(case)
    ref = L.reference_sequence(layer, x, state, masks, wgt, case.need_dx)
    hs, s = L.numpy_sequence(layer.wx.detach().double().numpy(), layer.wh.detach().double().numpy(), layer.b.detach().double().numpy(),
                             x.double().numpy(), state.double().numpy(), masks.double().numpy())
    assert np.abs(ref["h_seq"].numpy() - hs).max() < 1e-13 and np.abs(ref["state"].numpy() - s).max() < 1e-13
    assert masks.any() and np.abs(hs).max() > 0.1


def test_seeds_differ_between_cases_and_agree_between_arithmetics():
    seeds = {}
    for c in L.ALL_SEQ_CASES + L.E_WIDE_CASES:
        seeds.setdefault(L.seed_of(c), set()).add(c._replace(prec="f32", saturated=bool(c.saturated)))
    assert all(len(v) == 1 for v in seeds.values())
    assert len({L.case_id(c) for c in L.ALL_SEQ_CASES}) == len(set(L.ALL_SEQ_CASES))


def _shares(case):
    layer, x, state, masks, _ = L.make_seq_inputs(case)
    z = L.preactivations(layer, x, state, masks).abs()
    return float((z > 20).double().mean()), float((z < 2).double().mean()), float(z.max())


def test_saturated_inputs_are_saturated():
    """Group E.  With wx, wh x 8 and b = +-6 only a sliver of the pre-activations passes |20| (measured: 0.04 %, largest 23) -- that case is
    kept because it is the well-conditioned one (the quarter-bound test above).  The x 24 inputs are the ones of which at least 10 % lie
    beyond |20| while some stay inside |z| < 2 (measured 12 % / 12 %)."""
    big, small, top = _shares(L.E_CASES[0])
    print("\n[lstm saturated x 8] |z| > 20: %.4f, |z| < 2: %.4f, max |z| %.1f" % (big, small, top))
    assert big > 0 and small > 0.05 and top > 20
    big, small, top = _shares(L.E_WIDE_CASES[0])
    print("[lstm saturated x 24] |z| > 20: %.4f, |z| < 2: %.4f, max |z| %.1f" % (big, small, top))
    assert big >= 0.10 and small > 0.05


@pytest.mark.parametrize("case", [L.E_CASES[2], L.E_WIDE_CASES[2], L.A_CASES[0]._replace(prec="bf16x3", need_dx=True)], ids=L.case_id)
def test_bf16x3_model_is_a_two_plane_arithmetic(case):
    """The float64 model of the three-product split (hi hi + hi lo + lo hi; the dropped lo lo term is ~2^-16 of a product) against plain
    float64: above the f32 level, below a single-plane bf16 arithmetic, on every tensor."""
    args = L.make_seq_inputs(case)
    ref = L.reference_sequence(*args, True)
    errs = L.rel_errors(L.bf16x3_model_sequence(*args, True), ref)
    print("\n[lstm bf16x3 float64 model, %s] %s" % (L.case_id(case), L.fmt(errs)))
    lim = 2.0 ** -8 if case.saturated else 2.0 ** -12
    assert all(1e-8 < e < lim for e in errs.values()), errs
    hi, lo = L._bf16_planes(args[1].double())
    assert float((args[1].double() - hi - lo).abs().max()) <= 2.0 ** -16 * float(args[1].abs().max())


def test_policy_step_entry_points_refuse_unsupported_widths_before_any_launch():
    """irrl_mlp_policy_step keeps four observation rows of at most 64 words in a wave's LDS scratch: 65 is refused (rc 1) by the entry point, and
    `mlp_policy_step_supported` says so beforehand; non-positive widths are refused by both entry points.  Refusals happen before any HIP call,
    so this runs without a GPU (all pointers NULL)."""
    from types import SimpleNamespace
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib, lstm_fused
    from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import CustomLSTMPolicy, MlpPolicy
    lib = _lib.load()
    none = [None]
    table = (C.c_void_p * 12)()          # the HOST array of weight pointers (all NULL: nothing is launched)

    def mlp_rc(ob, hid=64, act=12, n=5):
        return lib.irrl_mlp_policy_step(hid, ob, act, n, None, None, table, *(none * 6), 0, 0, 0, None, 0, *(none * 4), -1, *(none * 8))

    def lstm_rc(ob, hid=48, act=12, n=5):
        return lib.irrl_lstm_policy_step(hid, ob, act, n, None, None, None, None, table, *(none * 6), 0, 0, 0, None, 0, *(none * 4), -1, *(none * 8))

    assert mlp_rc(L.MLP_STEP_MAX_OB + 1) == 1 and mlp_rc(0) == 1 and mlp_rc(-3) == 1 and mlp_rc(1 << 20) == 1
    assert mlp_rc(35, hid=48) == 1 and mlp_rc(35, act=16) == 1 and mlp_rc(35, n=0) == 1
    assert lstm_rc(0) == 1 and lstm_rc(-1) == 1 and lstm_rc(35, hid=40) == 1 and lstm_rc(35, hid=16) == 1 and lstm_rc(35, act=17) == 1 and lstm_rc(35, n=0) == 1

    # the thread budgets: 16 act + 16 <= 8 hid (LSTM), act <= 15 (MLP: 4 act + 4 <= 64)
    assert lstm_rc(35, hid=L.G_LSTM_REFUSED[0], act=L.G_LSTM_REFUSED[1]) == 1 and mlp_rc(35, act=L.G_MLP_REFUSED) == 1

    def fake_obs(ob):
        return SimpleNamespace(is_cuda=True, dtype=torch.float32, shape=(5, ob))

    mlp = MlpPolicy(ob_dim=8)
    assert lstm_fused.mlp_policy_step_supported(mlp, fake_obs(L.MLP_STEP_MAX_OB))
    assert not lstm_fused.mlp_policy_step_supported(mlp, fake_obs(L.MLP_STEP_MAX_OB + 1))
    pol = CustomLSTMPolicy(ob_dim=8, n_lstm=(48, 48))
    assert lstm_fused.policy_step_supported(pol, fake_obs(8)) and lstm_fused.policy_step_supported(pol, fake_obs(48))
    assert not lstm_fused.policy_step_supported(CustomLSTMPolicy(ob_dim=8, n_lstm=(16, 16)), fake_obs(8))
    assert max(ob for ob, _ in L.F_MLP_CASES) == L.MLP_STEP_MAX_OB
