"""The LSTM kernel forms the training runs but no older test launches, on an MI355X, tensor by tensor against float64 autograd of the eager
stable-baselines definition (cases, inputs and reference: tests/lstm_forms_lib.py; tests/test_lstm_forms_reference.py checks those on the CPU).

  A  backward kernels WITHOUT an input gradient (x carries no gradient: dx == NULL at the entry point)
  B  the unfused route: irrl_lstm_seq_forward (zx) / irrl_lstm_seq_backward (dz) + the tall GEMMs of lstm_fused.py
  C  the template forms of the fused kernels that n_in selects (K = 9 / 12, split input projection or not, helper wave or not)
  D  mask edges: every step an episode start, a start at t = 0 only, at t = T-1 only, none
  E  saturated gates
  F  the policy-step kernels at observation widths other than 35
  G  the policy-step kernels at action widths other than 12: 1, 5, 15, 16 (the sampler's fourth Philox block; the thread budgets met with equality)

Bounds: per tensor max |kernel - f64| / max |f64| <= 2e-5 (f32, bf16x6) / 1e-4 (bf16x3), the project's bounds for these arithmetics at small
shapes; every test prints what it measured.  G, measured on an MI355X (worst over the 16 cases, relative to 1 + the largest entry): action 8.7e-08,
value 1.6e-07, state 9.8e-08, neglogp 1.1e-07 (bounds 2e-5 / 2e-5 / 2e-5 / 1e-4); in-kernel sampler against the Philox reference 9.6e-07 (bound
2e-3), the fourth block (slots 12 .. 15) 9.2e-07; rollout-buffer rows bit-equal.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lstm_forms_lib as L


def _dev():
    return torch.device("cuda")


def _kernel_run(case, monkeypatch, inputs=None, record=None):
    """the fused path of SBLstm.sequence for `case` -> outputs (and the C entry points it reached, when `record` is a list)"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib, lstm_fused
    from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import SBLstm
    monkeypatch.setattr(lstm_fused, "PRECISION", case.prec)
    assert SBLstm.use_fused
    args = inputs if inputs is not None else L.make_seq_inputs(case, _dev())
    with L.record_calls(_lib.load(), L.SEQ_ENTRY_POINTS) as calls:
        out = L.run_sequence(*args, case.need_dx)
        torch.cuda.synchronize()
    assert out["_fn"] == "_LstmSeqFnBackward", out["_fn"]      # the kernels ran, not the eager graph
    if record is not None:
        record += calls
    return out


def _check(case, out, ref, what, bound=None):
    errs = L.rel_errors(out, ref)
    print("\n[lstm kernels %s, %s] max |kernel - float64| / max |float64|: %s" % (what, L.case_id(case), L.fmt(errs)))
    assert set(errs) == set(L.NAMES) - (set() if case.need_dx else {"dx"})
    bound = L.BOUNDS[case.prec] if bound is None else bound
    for name, e in errs.items():
        assert e <= bound, (L.case_id(case), name, e, bound)
    return errs


def _entries(calls):
    return [name for name, _ in calls]


def _expected_entries(case, fuse_in=True, fuse_wg=True):
    if case.prec != "f32" and case.hid == 48 and case.n_in <= 48 and fuse_in and fuse_wg:
        return ["irrl_lstm_seq_forward_bf16", "irrl_lstm_seq_backward_bf16"]
    fwd = "irrl_lstm_seq_forward_x" if (case.n_in <= 48 and fuse_in) else "irrl_lstm_seq_forward"
    bwd = "irrl_lstm_seq_backward_x" if (case.n_in <= 48 and fuse_wg) else "irrl_lstm_seq_backward"
    return [fwd, bwd]


def _dx_argument(calls):
    """the dx pointer the fused backward entry point was given (None = NULL: the NEED_DX = false kernels)"""
    for name, args in calls:
        if name == "irrl_lstm_seq_backward_x":
            return args[13]
        if name == "irrl_lstm_seq_backward_bf16":
            return args[15]
    raise AssertionError("no fused backward entry point among %s" % _entries(calls))


# ---------------------------------------------------------------- A ----
@pytest.mark.parametrize("case", L.A_CASES, ids=L.case_id)
def test_backward_kernels_without_an_input_gradient_match_float64(case, monkeypatch):
    """lstm_seq_bwd_x_kernel<H, false, ...>, lstm_seq_bwd_bf16_kernel<2|3, false>: what the first layer of both stacks runs in every update."""
    calls = []
    args = L.make_seq_inputs(case, _dev())
    out = _kernel_run(case, monkeypatch, args, calls)
    assert _entries(calls) == _expected_entries(case) and _dx_argument(calls) is None
    _check(case, out, L.reference_sequence(*args, False), "no dx")


@pytest.mark.parametrize("case", L.A_RECOMPUTE_CASES, ids=L.case_id)
def test_recomputing_backward_kernel_without_an_input_gradient_matches_float64_and_the_gate_loading_one(case, monkeypatch):
    """lstm_seq_bwd_bf16_rc_kernel<false>: within the bf16x3 bound of float64, and h, state, dwx, dwh, db bit for bit what the gate-loading
    no-dx kernel gives (test_recomputing_backward_kernel_equals_the_gate_loading_one_bit_for_bit, for the <false> kernels)."""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import lstm_fused
    args = L.make_seq_inputs(case, _dev())
    outs = {}
    for recompute in (False, True):
        monkeypatch.setattr(lstm_fused, "RECOMPUTE_GATES", recompute)
        calls = []
        outs[recompute] = _kernel_run(case, monkeypatch, args, calls)
        assert _entries(calls) == _expected_entries(case) and _dx_argument(calls) is None
        gates_arg = [a for n, a in calls if n == "irrl_lstm_seq_forward_bf16"][0][11]
        assert (gates_arg is None) == recompute               # the forward kernel kept no gates: the backward one had to recompute them
    _check(case, outs[True], L.reference_sequence(*args, False), "no dx, recomputed gates")
    for name in ("h_seq", "state", "dwx", "dwh", "db"):
        assert torch.equal(outs[False][name], outs[True][name]), (name, float((outs[False][name] - outs[True][name]).abs().max()))
    assert float(outs[True]["dwx"].abs().max()) > 0


def _policy_check(pc, prec, monkeypatch, entry, n_entry):
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib, lstm_fused
    from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import SBLstm
    monkeypatch.setattr(lstm_fused, "PRECISION", prec)
    args = L.make_policy_inputs(pc, _dev())
    nlp64, val64, g64 = L.reference_policy(*args)
    assert SBLstm.use_fused
    with L.record_calls(_lib.load(), L.SEQ_ENTRY_POINTS) as calls:
        nlp, val, g = L.run_policy(*args)
        torch.cuda.synchronize()
    # four layers forward, four backward; the two first layers (observations carry no gradient) got dx == NULL
    names = _entries(calls)
    assert len(names) == 8 and names.count(entry) == n_entry, names
    nulls = [a[13] is None for n, a in calls if n == "irrl_lstm_seq_backward_x"] + [a[15] is None for n, a in calls if n == "irrl_lstm_seq_backward_bf16"]
    assert sum(nulls) == 2 and len(nulls) == (4 if pc[0][0] == 48 else 2), (names, nulls)
    errs = {k: L.rel_err(g[k], g64[k]) for k in L.POLICY_PARAM_NAMES}
    errs.update(nlp=L.rel_err(nlp, nlp64), val=L.rel_err(val, val64))
    print("\n[lstm policy %s evaluate, %s] max |kernel - float64| / max |float64| per parameter gradient: %s" % (L.case_id(pc), prec, L.fmt(errs)))
    for name in L.POLICY_PARAM_NAMES:
        assert errs[name] <= L.BOUNDS[prec], (prec, name, errs[name])
    # nlp and val as test_fused_lstm_policy_full_size_agrees_with_eager holds them
    for a, b in ((nlp64, nlp), (val64, val)):
        assert float((a - b.double()).abs().max()) / (float(a.abs().max()) + 1e-6) < 1e-4


@pytest.mark.parametrize("prec", ["bf16x3", "bf16x6", "f32"])
def test_policy_gradients_match_float64_per_parameter_tensor(prec, monkeypatch):
    """CustomLSTMPolicy.evaluate (48, 48) at T 12 x N 40, observations without a gradient: EVERY parameter's gradient on its own scale -- a
    wrong dwx of a layer whose gradients are small cannot hide behind a larger tensor of one concatenated vector."""
    _policy_check(L.POLICY_CASES[0], prec, monkeypatch, "irrl_lstm_seq_backward_x" if prec == "f32" else "irrl_lstm_seq_backward_bf16", 4)


# ---------------------------------------------------------------- B ----
@pytest.mark.parametrize("case", L.B_CASES, ids=L.case_id)
def test_unfused_route_matches_float64(case, monkeypatch):
    """n_in > 48: x wx + b as a GEMM, lstm_seq_fwd_kernel on zx, lstm_seq_bwd_kernel -> dz, then _tall_gemm_t, hprev * keep and the column
    un-permutation in Python.  (64, 256, 64, 64): T N = 16384 rows, the smallest K that takes _tall_gemm_t's split-K branch."""
    calls = []
    args = L.make_seq_inputs(case, _dev())
    out = _kernel_run(case, monkeypatch, args, calls)
    assert _entries(calls) == ["irrl_lstm_seq_forward", "irrl_lstm_seq_backward"]
    _check(case, out, L.reference_sequence(*args, case.need_dx), "unfused")


@pytest.mark.parametrize("case", L.B_SWITCH_CASES, ids=L.case_id)
def test_fusion_switches_give_the_same_layer(case, monkeypatch):
    """FUSE_INPUT_PROJECTION / FUSE_WEIGHT_GRADIENTS off, one at a time and together, at shapes the fused kernels also take: each combination
    against float64, and the two forward kernels against each other."""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import lstm_fused
    args = L.make_seq_inputs(case, _dev())
    ref = L.reference_sequence(*args, True)
    outs = {}
    for fuse_in, fuse_wg in [(True, True)] + L.B_SWITCHES:
        monkeypatch.setattr(lstm_fused, "FUSE_INPUT_PROJECTION", fuse_in)
        monkeypatch.setattr(lstm_fused, "FUSE_WEIGHT_GRADIENTS", fuse_wg)
        calls = []
        outs[(fuse_in, fuse_wg)] = _kernel_run(case, monkeypatch, args, calls)
        assert _entries(calls) == _expected_entries(case, fuse_in, fuse_wg), (fuse_in, fuse_wg, _entries(calls))
        _check(case, outs[(fuse_in, fuse_wg)], ref, "input projection %s, weight gradients %s" % ("fused" if fuse_in else "GEMM", "fused" if fuse_wg else "GEMMs"))
    for name in ("h_seq", "state"):
        e = L.rel_err(outs[(False, True)][name], outs[(True, True)][name])
        print("[lstm kernels zx forward vs fused forward, %s] %s: %.2e" % (L.case_id(case), name, e))
        assert e <= 2e-5, (name, e)
        # the backward kernel does not touch the forward outputs
        assert torch.equal(outs[(True, True)][name], outs[(True, False)][name]) and torch.equal(outs[(False, True)][name], outs[(False, False)][name])


def test_policy_with_64_unit_layers_matches_float64_per_parameter_tensor(monkeypatch):
    """n_lstm = (64, 64): the second layer of each stack has n_in = 64 and runs the unfused route inside a real policy"""
    _policy_check(L.POLICY_CASES[1], "f32", monkeypatch, "irrl_lstm_seq_backward", 2)


@pytest.mark.parametrize("tc", L.TALL_CASES, ids=L.case_id)
def test_tall_gemm_and_tall_linear_match_float64(tc):
    """_tall_gemm_t (split-K over 256 chunks from K = 16384 on, when 256 divides K; one plain GEMM otherwise) and _TallLinearFn's dw, db, dx:
    within 1e-5 of the largest entry, the bound of the fixed-order f32 sums (test_row_sum_kernel_...)."""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import lstm_fused
    K, m, n = tc
    x, w, b, wgt = L.make_tall_inputs(tc, _dev())
    ref = L.tall_reference(x, w, b, wgt)
    split = K % 256 == 0 and K >= 16384
    assert split == (K == 16384)
    bmm_calls = []
    real_bmm = torch.bmm

    def spy_bmm(*a, **k):
        bmm_calls.append(tuple(a[0].shape))
        return real_bmm(*a, **k)
    torch.bmm = spy_bmm
    try:
        direct = lstm_fused._tall_gemm_t(x, wgt)
        xx, ww, bb = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = lstm_fused.tall_linear(xx, ww, bb)
        (y * wgt).sum().backward()
    finally:
        torch.bmm = real_bmm
    assert bmm_calls == ([(256, m, K // 256)] * 2 if split else [])
    errs = {"gemm_t": L.rel_err(direct, ref["dw"]), "dw": L.rel_err(ww.grad, ref["dw"]), "db": L.rel_err(bb.grad, ref["db"]), "dx": L.rel_err(xx.grad, ref["dx"]),
            "y": L.rel_err(y.detach(), x.double() @ w.double() + b.double())}
    print("\n[tall linear K %d, m %d, n %d, %s] max |f32 - float64| / max |float64|: %s" % (K, m, n, "split-K" if split else "plain", L.fmt(errs)))
    for name, e in errs.items():
        assert e <= 1e-5, (tc, name, e)


def test_linear_layer_takes_the_tall_form_from_65536_rows_on():
    from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import SBLinear
    torch.manual_seed(65536 + 37)
    lin = SBLinear(48, 12)
    x, wgt = torch.randn(65536 + 37, 48), torch.randn(65536 + 37, 12)
    lin, x, wgt = lin.to(_dev()), x.to(_dev()), wgt.to(_dev())
    y = lin(x)
    assert type(y.grad_fn).__name__ == "_TallLinearFnBackward"
    assert type(lin(x[:65535]).grad_fn).__name__ != "_TallLinearFnBackward"
    with torch.no_grad():
        assert lin(x).grad_fn is None
    (y * wgt).sum().backward()
    ref = L.tall_reference(x, lin.w.detach(), lin.b.detach(), wgt)
    errs = {"dw": L.rel_err(lin.w.grad, ref["dw"]), "db": L.rel_err(lin.b.grad, ref["db"])}
    print("\n[SBLinear, 65573 rows] %s" % L.fmt(errs))
    assert all(e <= 1e-5 for e in errs.values()), errs


# ---------------------------------------------------------------- C ----
@pytest.mark.parametrize("case", L.C_CASES, ids=L.case_id)
def test_input_width_forms_match_float64(case, monkeypatch):
    """lstm_seq_fwd_x_kernel<H, 9 | 12, helper, split> and the backward kernels' ragged input tiles: n_in at 1, around 31 / 32 (split input
    projection from 32 on), 36 / 37 (K = 9 -> 12) and 47 (the last width without the K = 12 split)."""
    calls = []
    args = L.make_seq_inputs(case, _dev())
    out = _kernel_run(case, monkeypatch, args, calls)
    assert _entries(calls) == _expected_entries(case) and _dx_argument(calls) is not None
    n_in_arg = [a for n, a in calls if n.startswith("irrl_lstm_seq_forward")][0][4 if case.prec != "f32" else 3]
    assert n_in_arg == case.n_in
    _check(case, out, L.reference_sequence(*args, True), "n_in %d" % case.n_in)


# ---------------------------------------------------------------- D ----
@pytest.mark.parametrize("case", L.D_CASES, ids=L.case_id)
def test_mask_edges(case, monkeypatch):
    args = L.make_seq_inputs(case, _dev())
    layer, x, state, masks, wgt = args
    out = _kernel_run(case, monkeypatch, args)
    _check(case, out, L.reference_sequence(*args, True), "masks %s" % case.mask)
    if case.mask == "ones":
        assert not out["dwh"].any()               # h_{t-1} (1 - mask) is zero at every step: exactly zero, not small
    if case.mask in ("ones", "first"):
        # the state the sequence starts from is wiped before it is used: other finite values change no bit of anything
        other = torch.randn(state.shape, generator=torch.Generator().manual_seed(7)).to(state.device) * 3.0 + 1.0
        out2 = _kernel_run(case, monkeypatch, (layer, x, other, masks, wgt))
        for name in L.NAMES:
            assert torch.equal(out[name], out2[name]), (L.case_id(case), name, float((out[name] - out2[name]).abs().max()))
    else:
        assert out["dwh"].any()


# ---------------------------------------------------------------- E ----
def _finite_and_bounded(out):
    for name in L.NAMES:
        assert torch.isfinite(out[name]).all(), name
    assert float(out["h_seq"].abs().max()) <= 1.0 and float(out["state"][:, out["state"].shape[1] // 2:].abs().max()) <= 1.0


@pytest.mark.parametrize("case", L.E_CASES[:2], ids=L.case_id)
def test_saturated_gates_f32_level(case, monkeypatch):
    """wx, wh x 8, b = +-6 by unit (pre-activations up to |23|): the tails of fast_sigmoid / fast_tanh; f32 and bf16x6 within 2e-5 of float64"""
    args = L.make_seq_inputs(case, _dev())
    out = _kernel_run(case, monkeypatch, args)
    _finite_and_bounded(out)
    _check(case, out, L.reference_sequence(*args, True), "saturated x 8")


def _model_bounds(case):
    """four times the error of the float64 model of the three-product split on these inputs (CPU); the factor covers what the model leaves out,
    f32 accumulation and the order of the sums"""
    cpu = L.make_seq_inputs(case)
    ref = L.reference_sequence(*cpu, True)
    model = L.rel_errors(L.bf16x3_model_sequence(*cpu, True), ref)
    return model, {k: 4.0 * v for k, v in model.items()}


def _check_per_tensor(case, out, ref, bounds, what):
    errs = L.rel_errors(out, ref)
    print("\n[lstm kernels %s, %s] max |kernel - float64| / max |float64|: %s\n    bounds: %s" % (what, L.case_id(case), L.fmt(errs), L.fmt(bounds)))
    for name in L.NAMES:
        assert errs[name] <= bounds[name], (L.case_id(case), name, errs[name], bounds[name])


def test_saturated_gates_bf16x3_stays_within_four_times_its_float64_model(monkeypatch):
    """bf16x3 on the x 8 inputs: no number fixed in advance -- the bound is 4 x the error of a float64 model of the arithmetic (operands as
    hi = bf16(v), lo = bf16(v - hi); products hi hi + hi lo + lo hi; everything else exact) against plain float64, per tensor.
    Measured (one run): model  h 3.69e-05, state 6.99e-06, dx 2.26e-05, dwx 1.88e-05, dwh 3.65e-05, db 1.99e-05;
                        kernel h 3.70e-05, state 6.97e-06, dx 2.32e-05, dwx 1.86e-05, dwh 3.68e-05, db 2.00e-05
    -- the kernel IS the model to two digits: f32 accumulation and summation order add nothing visible at this size."""
    case = L.E_CASES[2]
    assert case.prec == "bf16x3"
    model, bounds = _model_bounds(case)
    args = L.make_seq_inputs(case, _dev())
    out = _kernel_run(case, monkeypatch, args)
    _finite_and_bounded(out)
    print("\n[lstm bf16x3 float64 model, saturated x 8] %s" % L.fmt(model))
    _check_per_tensor(case, out, L.reference_sequence(*args, True), bounds, "saturated x 8")


@pytest.mark.parametrize("case", L.E_WIDE_CASES, ids=L.case_id)
def test_deeply_saturated_gates_stay_finite_and_within_the_two_plane_model(case, monkeypatch):
    """wx, wh x 24: 12 % of the pre-activations beyond |20| (up to |58|: __expf(-z) reaches 1e25), 12 % inside |z| < 2.  The layer is badly
    conditioned here -- the eager f32 graph itself lands between 3e-6 and 1.4e-5 of float64 depending on the machine's summation order -- so no
    f32-level bound means anything.  What is asserted, per tensor: everything finite, |h| <= 1, and within 4 x the float64 model of the
    two-plane arithmetic (as in the x 8 test) for ALL three arithmetics: bf16x3 is that arithmetic, f32 and bf16x6 are finer ones and measured
    ~100 x below the bound (f32: h 5.2e-6, dwx 1.4e-5; bf16x6: h 4.8e-6, dwx 4.4e-6; bf16x3: h 2.8e-4, dwx 3.5e-4 against a model at 2.6e-4 / 3.5e-4)."""
    args = L.make_seq_inputs(case, _dev())
    out = _kernel_run(case, monkeypatch, args)
    _finite_and_bounded(out)
    _check_per_tensor(case, out, L.reference_sequence(*args, True), _model_bounds(case)[1], "saturated x 24")


# ---------------------------------------------------------------- F ----
@pytest.mark.parametrize("fc", L.F_LSTM_CASES, ids=L.case_id)
def test_lstm_policy_step_at_other_observation_widths(fc):
    """lstm_policy_step_kernel<H, 9> (ob_dim 33 .. 36: two unaligned 16-byte loads per observation row + one ragged k-step) and <H, 0> (run-time
    loop, clamped loads) against the float64 eager policy._run, tolerances of test_fused_policy_step_matches_eager_step; rollout-buffer row too."""
    hid, ob, N = fc
    dev = _dev()
    pol, obs, st, dones, noise = L.make_lstm_step_inputs(fc, dev)
    assert pol.fused_step_supported(obs)
    T = 3
    prev_rew = torch.randn(N, device=dev)
    mb_rew = torch.zeros(T, N, device=dev)
    mb = [torch.zeros(T, N, ob, device=dev), torch.zeros(T, N, 12, device=dev), torch.zeros(T, N, device=dev), torch.zeros(T, N, device=dev),
          torch.zeros(T, N, dtype=torch.bool, device=dev)]
    act, clipped, val, nlp, snew = pol.fused_step(obs, st, dones, noise=noise, rollout=dict(
        row=1, mb_obs=mb[0], mb_actions=mb[1], mb_values=mb[2], mb_neglogpacs=mb[3], mb_dones=mb[4], mb_rewards=mb_rew, prev_reward=prev_rew))
    ref = dict(zip(("action", "value", "state", "neglogp"), L.lstm_step_reference(pol, obs, st, dones, noise)))
    errs = L.step_errors({"action": act, "value": val, "state": snew, "neglogp": nlp}, ref)
    print("\n[lstm policy step hid %d, ob_dim %d, N %d] max |kernel - float64| / (1 + max |float64|): %s" % (hid, ob, N, L.fmt(errs)))
    for name, e in errs.items():
        assert e <= L.STEP_TOL[name], (fc, name, e)
    assert torch.equal(clipped, act.clamp(-1.0, 1.0))
    assert torch.equal(mb[0][1], obs) and torch.equal(mb[1][1], act) and torch.equal(mb[2][1], val) and torch.equal(mb[3][1], nlp) and torch.equal(mb[4][1], dones)
    for b in mb:
        assert not b[0].any() and not b[2].any()
    assert torch.equal(mb_rew[0], prev_rew) and not mb_rew[1:].any()
    st2 = st.clone()
    pol.fused_step(obs, st2, dones, noise=noise, states_out=st2)
    assert torch.equal(st2, snew)


@pytest.mark.parametrize("fc", L.F_MLP_CASES, ids=L.case_id)
def test_mlp_policy_step_at_other_observation_widths(fc):
    """mlp_policy_step_kernel: groups of four k with a clamped ragged end, observation rows of ob_dim words in a wave's scratch (ob_dim <= 64)"""
    ob, N = fc
    dev = _dev()
    pol, obs, dones, noise = L.make_mlp_step_inputs(fc, dev)
    assert pol.fused_step_supported(obs)
    T = 3
    mb = dict(row=2, mb_obs=torch.zeros(T, N, ob, device=dev), mb_actions=torch.zeros(T, N, 12, device=dev), mb_values=torch.zeros(T, N, device=dev),
              mb_neglogpacs=torch.zeros(T, N, device=dev), mb_dones=torch.zeros(T, N, dtype=torch.bool, device=dev),
              mb_rewards=torch.zeros(T, N, device=dev), prev_reward=torch.randn(N, device=dev))
    act, clipped, val, nlp, _ = pol.fused_step(obs, None, dones, noise=noise, rollout=mb)
    ref = dict(zip(("action", "value", "neglogp"), L.mlp_step_reference(pol, obs, noise)))
    errs = L.step_errors({"action": act, "value": val, "neglogp": nlp}, ref)
    print("\n[mlp policy step ob_dim %d, N %d] max |kernel - float64| / (1 + max |float64|): %s" % (ob, N, L.fmt(errs)))
    for name, e in errs.items():
        assert e <= L.STEP_TOL[name], (fc, name, e)
    assert torch.equal(clipped, act.clamp(-1.0, 1.0))
    assert torch.equal(mb["mb_obs"][2], obs) and torch.equal(mb["mb_actions"][2], act) and torch.equal(mb["mb_values"][2], val) and torch.equal(mb["mb_neglogpacs"][2], nlp)
    assert torch.equal(mb["mb_dones"][2], dones) and torch.equal(mb["mb_rewards"][1], mb["prev_reward"]) and not mb["mb_rewards"][2].any()
    for k in ("mb_obs", "mb_actions", "mb_values", "mb_neglogpacs", "mb_dones"):
        assert not mb[k][:2].any()


def test_mlp_policy_step_refuses_an_observation_wider_than_its_scratch():
    """65 observations do not fit a wave's scratch rows: `fused_step_supported` says no, and the entry point refuses without a launch"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import MlpPolicy
    dev = _dev()
    pol = MlpPolicy(ob_dim=L.MLP_STEP_MAX_OB + 1).to(dev)
    obs = torch.zeros(5, L.MLP_STEP_MAX_OB + 1, device=dev)
    assert not pol.fused_step_supported(obs)
    with pytest.raises(RuntimeError, match="irrl_mlp_policy_step failed"):
        pol.fused_step(obs, None, torch.zeros(5, dtype=torch.bool, device=dev))
    act, val, _, nlp = pol.step(obs, deterministic=True)          # the eager step serves such a policy
    assert act.shape == (5, 12) and torch.isfinite(act).all()


# ---------------------------------------------------------------- G ----
def _sampler_check(what, pol, act, mean64, N, A):
    """z = (action - mean64) / exp(logstd) of every env and slot against the Philox / Box-Muller reference at (seed, env + env0, step + base)"""
    import rollout_replay_lib as R
    z = (act.double().cpu() - mean64.double().cpu()) / torch.exp(pol.logstd.detach().double().cpu())
    want = R.sampler_reference(L.G_RNG_SEED, np.arange(N) + L.G_RNG_ENV0, L.G_RNG_STEP + 3, A)
    assert want.shape == (N, A) == tuple(z.shape)
    err = float(np.abs(z.numpy() - want).max())
    print("[%s] in-kernel sampler against the Philox reference, %d blocks: %.2e" % (what, (A + 3) // 4, err))
    assert err <= 2e-3, (what, err)


def _row_buffers(T, N, ob, A, dev):
    return dict(mb_obs=torch.zeros(T, N, ob, device=dev), mb_actions=torch.zeros(T, N, A, device=dev), mb_values=torch.zeros(T, N, device=dev),
                mb_neglogpacs=torch.zeros(T, N, device=dev), mb_dones=torch.zeros(T, N, dtype=torch.bool, device=dev),
                mb_rewards=torch.zeros(T, N, device=dev), prev_reward=torch.randn(N, device=dev))


def _rows_check(mb, obs, act, val, nlp, dones):
    """row 1 of the T = 3 buffers is the step, rows 0 and 2 are untouched (the reward row is one behind: row 0)"""
    assert torch.equal(mb["mb_obs"][1], obs) and torch.equal(mb["mb_actions"][1], act) and torch.equal(mb["mb_values"][1], val)
    assert torch.equal(mb["mb_neglogpacs"][1], nlp) and torch.equal(mb["mb_dones"][1], dones)
    for k in ("mb_obs", "mb_actions", "mb_values", "mb_neglogpacs", "mb_dones"):
        assert not mb[k][0].any() and not mb[k][2].any(), k
    assert torch.equal(mb["mb_rewards"][0], mb["prev_reward"]) and not mb["mb_rewards"][1:].any()


@pytest.mark.parametrize("gc", L.G_LSTM_CASES, ids=L.case_id)
def test_lstm_policy_step_at_other_action_widths(gc):
    """lstm_policy_step_kernel with act_dim 1, 5, 15, 16 (policy_heads: 16 act + 16 threads, all 256 of them at (32, 15)): given noise against
    the float64 eager step, the in-kernel sampler against the Philox reference (slots 12 .. 15: the fourth block), the rollout-buffer row"""
    hid, A, N = gc
    dev = _dev()
    pol, obs, st, dones, noise = L.make_lstm_step_inputs((hid, L.G_OB, N), dev, act=A)
    assert pol.act_dim == A and pol.fused_step_supported(obs) and 16 * A + 16 <= 8 * hid
    mb = _row_buffers(3, N, L.G_OB, A, dev)
    act, clipped, val, nlp, snew = pol.fused_step(obs, st, dones, noise=noise, rollout=dict(row=1, **mb))
    assert act.shape == (N, A) == clipped.shape
    ref = dict(zip(("action", "value", "state", "neglogp"), L.lstm_step_reference(pol, obs, st, dones, noise)))
    errs = L.step_errors({"action": act, "value": val, "state": snew, "neglogp": nlp}, ref)
    print("\n[lstm policy step hid %d, act_dim %d, N %d] max |kernel - float64| / (1 + max |float64|): %s" % (hid, A, N, L.fmt(errs)))
    for name, e in errs.items():
        assert e <= L.STEP_TOL[name], (gc, name, e)
    assert torch.equal(clipped, act.clamp(-1.0, 1.0))
    _rows_check(mb, obs, act, val, nlp, dones)
    base = torch.tensor([3], device=dev, dtype=torch.long)
    act_s, clipped_s, val_s, _, snew_s = pol.fused_step(obs, st, dones, rng=(L.G_RNG_SEED, L.G_RNG_STEP, base, L.G_RNG_ENV0))
    mean64 = L.lstm_step_reference(pol, obs, st, dones, torch.zeros_like(noise))[0]
    _sampler_check("lstm policy step hid %d, act_dim %d, N %d" % gc, pol, act_s, mean64, N, A)
    assert torch.equal(clipped_s, act_s.clamp(-1.0, 1.0)) and torch.equal(val_s, val) and torch.equal(snew_s, snew)


@pytest.mark.parametrize("gc", L.G_MLP_CASES, ids=L.case_id)
def test_mlp_policy_step_at_other_action_widths(gc):
    """mlp_policy_step_kernel with act_dim 1, 5, 15 (policy_heads_wave: 4 act + 4 lanes, the whole wave at 15)"""
    A, N = gc
    dev = _dev()
    pol, obs, dones, noise = L.make_mlp_step_inputs((L.G_OB, N), dev, act=A)
    assert pol.act_dim == A and pol.fused_step_supported(obs) and 4 * A + 4 <= 64
    mb = _row_buffers(3, N, L.G_OB, A, dev)
    act, clipped, val, nlp, _ = pol.fused_step(obs, None, dones, noise=noise, rollout=dict(row=1, **mb))
    assert act.shape == (N, A) == clipped.shape
    ref = dict(zip(("action", "value", "neglogp"), L.mlp_step_reference(pol, obs, noise)))
    errs = L.step_errors({"action": act, "value": val, "neglogp": nlp}, ref)
    print("\n[mlp policy step act_dim %d, N %d] max |kernel - float64| / (1 + max |float64|): %s" % (A, N, L.fmt(errs)))
    for name, e in errs.items():
        assert e <= L.STEP_TOL[name], (gc, name, e)
    assert torch.equal(clipped, act.clamp(-1.0, 1.0))
    _rows_check(mb, obs, act, val, nlp, dones)
    base = torch.tensor([3], device=dev, dtype=torch.long)
    act_s, clipped_s, val_s, _, _ = pol.fused_step(obs, None, dones, rng=(L.G_RNG_SEED, L.G_RNG_STEP, base, L.G_RNG_ENV0))
    mean64 = L.mlp_step_reference(pol, obs, torch.zeros_like(noise))[0]
    _sampler_check("mlp policy step act_dim %d, N %d" % gc, pol, act_s, mean64, N, A)
    assert torch.equal(clipped_s, act_s.clamp(-1.0, 1.0)) and torch.equal(val_s, val)


def test_policy_steps_refuse_an_action_width_beyond_their_thread_budget():
    """(hid 32, act 16): 16 x 16 + 16 threads are more than the workgroup's 256; MlpPolicy act 16: 4 x 16 + 4 lanes are more than a wave.
    `fused_step_supported` says no, and the entry points return 1 without a launch"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import CustomLSTMPolicy, MlpPolicy
    dev = _dev()
    hid, A = L.G_LSTM_REFUSED
    pol = CustomLSTMPolicy(ob_dim=L.G_OB, act_dim=A, n_lstm=(hid, hid)).to(dev)
    obs = torch.zeros(7, L.G_OB, device=dev)
    assert not pol.fused_step_supported(obs)
    assert CustomLSTMPolicy(ob_dim=L.G_OB, act_dim=A - 1, n_lstm=(hid, hid)).to(dev).fused_step_supported(obs)
    with pytest.raises(RuntimeError, match=r"irrl_lstm_policy_step failed \(rc=1"):
        pol.fused_step(obs, torch.zeros(7, 8 * hid, device=dev), torch.zeros(7, dtype=torch.bool, device=dev))
    mlp = MlpPolicy(ob_dim=L.G_OB, act_dim=L.G_MLP_REFUSED).to(dev)
    assert not mlp.fused_step_supported(obs)
    assert MlpPolicy(ob_dim=L.G_OB, act_dim=L.G_MLP_REFUSED - 1).to(dev).fused_step_supported(obs)
    with pytest.raises(RuntimeError, match=r"irrl_mlp_policy_step failed \(rc=1"):
        mlp.fused_step(obs, None, torch.zeros(7, dtype=torch.bool, device=dev))
    act, val, _, nlp = mlp.step(obs, deterministic=True)          # the eager step serves such a policy
    assert act.shape == (7, L.G_MLP_REFUSED) and torch.isfinite(act).all()
